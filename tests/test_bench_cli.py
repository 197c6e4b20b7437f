# bench.py command line: a plain run does only what the headline figure
# needs (roofline / CPU-baseline legs are null), --full brings the legs
# back, --dump-outputs writes what the last timed step returned.
# The GPU cases run the scaled-down "ivfpq_100k_d64" workload, each in a
# child process of its own (the command line IS what is under test).
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
SMALL = "ivfpq_100k_d64"  # n=100k, nq=2000, k=10
N, NQ, K = 100_000, 2_000, 10


def _gpu_missing():
    try:
        import torch
    except ImportError:
        return True
    return not torch.cuda.is_available()


needs_gpu = pytest.mark.skipif(_gpu_missing(), reason="needs an MI355X")


def _run(*extra):
    p = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--config", SMALL,
         # first sweep candidate (nprobe=1) is accepted: keeps the sweep and
         # the CPU-baseline leg to a second or two
         "--target-recall", "0", *extra],
        capture_output=True, text=True, cwd=REPO, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout  # ONE JSON result line
    return json.loads(lines[0])


def _check_headline(res, steps, warmup):
    assert res["unit"] == "queries/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and "QPS at recall@10" in res["metric"]
    assert res["steps"] == steps and res["warmup"] == warmup
    assert res["ms_per_step"] > 0
    # value and ms_per_step are two views of the same timed region
    assert res["value"] * res["ms_per_step"] / 1000.0 == pytest.approx(NQ, rel=1e-9)
    assert res["config"]["workload"] == SMALL
    assert res["config"]["nprobe"] == 1
    # (the scaled-down workload is full-rank, where PQ recall saturates
    # well below the 0.95 target, so only the range is checked here)
    assert 0.0 <= res["config"]["recall_at_10"] <= 1.0


def test_help_lists_new_options():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True,
                       text=True, cwd=REPO, timeout=60)
    assert p.returncode == 0
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench") / "dump"
    res = _run("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    return res, out


@pytest.mark.gpu
@needs_gpu
def test_dump_is_identical_from_run_to_run(plain_run, tmp_path):
    # same arguments -> same inputs, same index, same outputs, bit for bit
    _, first = plain_run
    again = tmp_path / "dump"
    _run("--steps", "2", "--warmup", "0", "--dump-outputs", str(again))
    for name in ("distances.npy", "ids.npy"):
        assert np.array_equal(np.load(first / name), np.load(again / name)), name


@pytest.mark.gpu
@needs_gpu
def test_plain_run_is_lean_and_dumps_outputs(plain_run):
    res, out = plain_run
    _check_headline(res, 3, 1)
    assert res["roofline"] is None and res["cpu_baseline"] is None
    assert sorted(os.listdir(out)) == ["distances.npy", "ids.npy"]
    D = np.load(out / "distances.npy")
    ids = np.load(out / "ids.npy")
    assert D.dtype == np.float32 and ids.dtype == np.float64
    assert D.shape == (NQ, K) and ids.shape == (NQ, K)
    assert np.isfinite(D).all()
    assert (np.diff(D, axis=1) >= 0).all()  # L2: best first
    assert (ids == np.floor(ids)).all() and (ids >= 0).all() and (ids < N).all()
    # no id twice within one query's top-k
    assert all(len(set(row)) == K for row in ids[:200])


@pytest.mark.gpu
@needs_gpu
def test_full_run_keeps_the_extra_legs():
    res = _run("--steps", "2", "--warmup", "1", "--full")
    _check_headline(res, 2, 1)
    roof = res["roofline"]
    assert roof["kernel"] == "k_scan_pq" and roof["unit"] == "GB/s"
    assert roof["achieved"] > 0 and roof["scan_ms"] > 0
    cpu = res["cpu_baseline"]
    assert cpu["unit"] == "QPS" and cpu["value"] > 0 and cpu["kind"] == "port"
