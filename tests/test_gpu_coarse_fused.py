# Fused coarse select (k_gemm_bf16_256_topk + k_coarse_reduce_rk) against
# the two-pass path (k_gemm_bf16_256 + k_topk_rows_rk) and against fp64.
#
# Every case goes through HipEngine.coarse() on an ivf_flat engine with
# coarse_bf16=1 and set_trained centroids, once with DFANN_COARSE_FUSED
# unset (fused where the dispatch allows it) and once with
# DFANN_COARSE_FUSED=0 (two-pass), in the same process. The two results
# must be bitwise equal: both paths apply gemm_key() to the same MFMA
# accumulators and select by the same (key, list id) order. The fused
# result must also pass the fp64 checks of
# test_gpu_dispatch_parity._check_coarse, restated here.
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributed_faiss_amd.hip_engine import HipEngine  # noqa: E402
from gpu_support import assert_bitwise, bf16_round  # noqa: E402

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
NORTH_STAR = 1e-4  # the project's relative bound
KNOB = "DFANN_COARSE_FUSED"


def _both_paths(cent, q, metric, nprobe):
    """(probes, keys) with the knob unset, then with the knob at 0."""
    nlist, d = cent.shape
    spec = {"type": "ivf_flat", "dim": d, "metric": metric, "nlist": nlist,
            "nprobe": 1, "seed": 1, "coarse_bf16": 1}
    eng = HipEngine(spec=spec)
    eng.set_trained(cent)
    saved = os.environ.pop(KNOB, None)
    try:
        fused = eng.coarse(q, nprobe)
        os.environ[KNOB] = "0"
        two_pass = eng.coarse(q, nprobe)
    finally:
        os.environ.pop(KNOB, None)
        if saved is not None:
            os.environ[KNOB] = saved
    return fused, two_pass


def _assert_bitwise_equal(fused, two_pass):
    """(probes, keys) pairs: ids equal, keys equal as bits."""
    assert_bitwise(fused[1], fused[0], two_pass[1], two_pass[0])


def _assert_fp64(cent, q, metric, probes, keys):
    nq, nprobe = probes.shape
    nlist = cent.shape[0]
    # fp64 reference over the operands the GEMM consumed; the centroid
    # norms come from the fp32 centroids
    qr = bf16_round(q).astype(np.float64)
    cr = bf16_round(cent).astype(np.float64)
    cn = (cent.astype(np.float64) ** 2).sum(axis=1)
    dot = qr @ cr.T
    absdot = np.abs(qr) @ np.abs(cr).T
    ref = cn[None, :] - 2.0 * dot if metric == L2 else -dot
    bound = NORTH_STAR * (cn[None, :] + 2.0 * absdot)
    rows = np.arange(nq)[:, None]
    # 1. returned keys within the bound for their list id
    assert (probes >= 0).all() and (probes < nlist).all()
    err = np.abs(keys.astype(np.float64) - ref[rows, probes])
    assert (err <= bound[rows, probes]).all(), (err / bound[rows, probes]).max()
    # 2. distinct ids
    srt = np.sort(probes, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    # 3. ascending keys, equal keys in ascending id order
    assert (keys[:, 1:] >= keys[:, :-1]).all()
    tie = keys[:, 1:] == keys[:, :-1]
    assert (probes[:, 1:][tie] > probes[:, :-1][tie]).all()
    # 4. nothing better was left out
    rest = np.ones((nq, nlist), bool)
    rest[rows, probes] = False
    last = keys[:, -1].astype(np.float64)[:, None]
    assert (~rest | (ref >= last - 2.0 * bound)).all()


def _random_case(nq, nlist, d):
    rng = np.random.default_rng(nq * 7919 + nlist * 31 + d)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return cent, q


SHAPES = [
    # one M-panel, eight N-tiles, one K tile: the minimum that engages
    pytest.param(256, 2048, 64, 1, id="nq256-nlist2048-d64-nprobe1"),
    pytest.param(256, 2048, 64, 2, id="nq256-nlist2048-d64-nprobe2"),
    pytest.param(256, 2048, 64, 3, id="nq256-nlist2048-d64-nprobe3"),
    pytest.param(256, 2048, 64, 16, id="nq256-nlist2048-d64-nprobe16"),
    # tails in M, N and K
    pytest.param(300, 2100, 72, 2, id="nq300-nlist2100-d72-nprobe2-tails"),
    pytest.param(300, 2100, 72, 10, id="nq300-nlist2100-d72-nprobe10-tails"),
    # last tile holds 2 valid columns (< nprobe): pads must not surface;
    # a one-row M tail
    pytest.param(257, 2050, 64, 8, id="nq257-nlist2050-d64-nprobe8-pads"),
    pytest.param(257, 2050, 64, 16, id="nq257-nlist2050-d64-nprobe16-pads"),
    # the headline K depth
    pytest.param(257, 2304, 768, 2, id="nq257-nlist2304-d768-nprobe2"),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq,nlist,d,nprobe", SHAPES)
def test_fused_equals_two_pass_and_fp64(nq, nlist, d, nprobe, metric):
    cent, q = _random_case(nq, nlist, d)
    fused, two_pass = _both_paths(cent, q, metric, nprobe)
    assert fused[0].shape == (nq, nprobe)
    _assert_bitwise_equal(fused, two_pass)
    _assert_fp64(cent, q, metric, *fused)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nprobe", [2, 16])
def test_ties_ascending_list_id(nprobe, metric):
    """64 distinct centroid rows repeated to nlist = 2048: every key occurs
    32 times, 4 times in each 256-column tile and in all 8 tiles."""
    nq, nlist, d = 256, 2048, 64
    rng = np.random.default_rng(64)
    base = rng.standard_normal((64, d)).astype(np.float32)
    cent = np.ascontiguousarray(base[np.arange(nlist) % 64])
    q = rng.standard_normal((nq, d)).astype(np.float32)
    fused, two_pass = _both_paths(cent, q, metric, nprobe)
    _assert_bitwise_equal(fused, two_pass)
    probes, keys = fused
    # the best key's 32 copies fill the result: one key, and its copies in
    # ascending list id, i.e. b, b + 64, b + 128, ...
    assert (keys == keys[:, :1]).all()
    assert (probes == probes[:, :1] + 64 * np.arange(nprobe)[None, :]).all()
    assert (probes[:, 0] < 64).all()
    _assert_fp64(cent, q, metric, probes, keys)


@pytest.mark.parametrize("metric", METRICS)
def test_nprobe17_stays_two_pass(metric):
    """nprobe = 17 is past the register-select bound: the dispatch keeps
    the two-pass path whatever the knob says."""
    cent, q = _random_case(256, 2048, 64)
    fused, two_pass = _both_paths(cent, q, metric, 17)
    _assert_bitwise_equal(fused, two_pass)
    _assert_fp64(cent, q, metric, *fused)
