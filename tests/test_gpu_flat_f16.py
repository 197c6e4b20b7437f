# Flat fp16 store (spec "flat_store": "fp16"): k_flat_f16
# with the fused select (k <= 16) and with the store epilogue (k > 16).
#
# Reference: numpy float64 over x.astype(float16) and q.astype(float16) —
# the rounding of rows and queries is the contract, the reference shares it.
# Bound of candidate u (DESIGN.md §4 tier, as test_gpu_dispatch_parity applies
# it to GEMM keys): b_u = 1e-4 * (|q|^2 + |x_u|^2 + 2 sum|q_t x_ut|) + 1e-4,
# the two norm terms dropped under IP. A rank is DECIDED when the fp64 gap to
# the neighbour on either side exceeds the two candidates' bounds together:
# both values may move by their own bound, so nothing less separates them.
# Every rank of every case below is decided (asserted on the CPU, from the
# data and the reference alone — the seeds were picked for it), so every
# returned id is compared.
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

IP, L2 = 0, 1
FLT_MAX = np.float32(3.4028235e38)
KNOB = "DFANN_FLAT_SPLITS"

# d: one 16-byte group / a padded row / exactly one K block / a K tail in the
# second block / the headline width. N: one row, the 256-row tile's edges,
# three tiles with a ragged last. nq = 300: three ragged query tiles. k: the
# three fused instantiations, the first two-pass k, and k > N on both paths.
# (d, N, nq, k, metric, seed)
CASES = [
    (8, 1, 300, 10, L2, 0),
    (8, 256, 300, 1, IP, 1),
    (20, 255, 1, 10, L2, 0),
    (20, 257, 1, 16, IP, 0),
    (20, 700, 1, 40, L2, 2),
    (64, 700, 1, 10, IP, 1),
    (64, 256, 1, 17, L2, 0),
    (64, 1, 1, 17, L2, 0),
    (100, 257, 300, 1, L2, 16),
    (100, 256, 1, 16, L2, 0),
    (768, 700, 1, 10, L2, 3),
    (768, 255, 1, 1, IP, 0),
]
FILTER_CASE = (20, 700, 1, 10, L2, 2)


@functools.lru_cache(maxsize=None)
def _data(d, n, nq, seed):
    """Seeded Gaussian rows and queries (draws: x, then q)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    return x, q


@functools.lru_cache(maxsize=None)
def _reference(d, n, nq, seed, metric):
    """fp64 distances (nq, n) in faiss sign, and the bound of each."""
    x, q = _data(d, n, nq, seed)
    xh = x.astype(np.float16).astype(np.float64)
    qh = q.astype(np.float16).astype(np.float64)
    dot = qh @ xh.T
    mag = 2.0 * (np.abs(qh) @ np.abs(xh).T)
    if metric == IP:
        return dot, 1e-4 * mag + 1e-4
    qn, xn = (qh * qh).sum(1)[:, None], (xh * xh).sum(1)[None, :]
    return qn + xn - 2.0 * dot, 1e-4 * (qn + xn + mag) + 1e-4


def _ranking(case, k, keep=None):
    """(ids, decided) of the first min(k, live) fp64 ranks, ties by id, over
    the rows with keep true (all rows without it)."""
    d, n, nq, _, metric, seed = case
    D64, bound = _reference(d, n, nq, seed, metric)
    key = -D64 if metric == IP else D64.copy()
    if keep is not None:
        key[:, ~keep] = np.inf
    live = n if keep is None else int(keep.sum())
    order = np.argsort(key, axis=1, kind="stable")[:, :live]
    ks = np.take_along_axis(key, order, 1)
    bs = np.take_along_axis(bound, order, 1)
    apart = (ks[:, 1:] - ks[:, :-1]) > (bs[:, 1:] + bs[:, :-1])
    edge = np.ones((nq, 1), bool)
    decided = np.concatenate([edge, apart], 1) & np.concatenate([apart, edge], 1)
    nv = min(k, live)
    return order[:, :nv], decided[:, :nv]


torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from distributed_faiss_amd.hip_engine import HipEngine, HipProvider  # noqa: E402
from gpu_support import assert_bitwise  # noqa: E402


def _engine(x, metric):
    """A flat fp16 engine over x; its rows are round_up(d, 8) halves."""
    eng = HipEngine(spec={"type": "flat", "dim": x.shape[1], "metric": metric,
                          "flat_store": "fp16"})
    eng.lib.dfann_code_stride.argtypes = [ctypes.c_void_p]
    assert eng.lib.dfann_code_stride(eng.h) == 2 * ((x.shape[1] + 7) & ~7)
    eng.add(x)
    return eng


def _assert_against_fp64(case, D, I, k, keep=None):
    d, n, nq, _, metric, seed = case
    D64, bound = _reference(d, n, nq, seed, metric)
    ref_ids, decided = _ranking(case, k, keep)
    nv = ref_ids.shape[1]
    assert D.shape == (nq, k) and I.shape == (nq, k)
    # the k tail past the live rows: I = -1, D = +-FLT_MAX
    assert (I[:, nv:] == -1).all()
    assert (D[:, nv:] == (-FLT_MAX if metric == IP else FLT_MAX)).all()
    ids, dist = I[:, :nv], D[:, :nv].astype(np.float64)
    assert (ids >= 0).all() and (ids < n).all()
    err = np.abs(dist - np.take_along_axis(D64, ids, 1))
    print(f"{case}: max err / bound = "
          f"{(err / np.take_along_axis(bound, ids, 1)).max():.3g}")
    assert (err <= np.take_along_axis(bound, ids, 1)).all()
    step = np.diff(dist, axis=1)
    assert ((step <= 0) if metric == IP else (step >= 0)).all()
    assert decided.all()
    np.testing.assert_array_equal(ids, ref_ids)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_search_against_fp64_and_across_splits(case, monkeypatch):
    d, n, nq, k, metric, seed = case
    x, q = _data(d, n, nq, seed)
    eng = _engine(x, metric)
    assert eng.ntotal == n
    monkeypatch.delenv(KNOB, raising=False)
    D, I = eng.search(q, k)
    _assert_against_fp64(case, D, I, k)
    for splits in ("1", "3"):
        monkeypatch.setenv(KNOB, splits)
        Ds, Is = eng.search(q, k)
        assert_bitwise(Ds, Is, D, I)


@pytest.mark.parametrize("metric", [IP, L2])
def test_bitwise_properties(metric, monkeypatch, tmp_path):
    """Three ragged query tiles over three database tiles: the first 16 of
    k = 17 (store epilogue) are the k = 16 results (fused), whatever the
    split; reconstruction returns the stored halves; save -> load changes
    nothing."""
    d, n, nq = 100, 700, 300
    x, q = _data(d, n, nq, 7)
    eng = _engine(x, metric)
    monkeypatch.delenv(KNOB, raising=False)
    D16, I16 = eng.search(q, 16)
    D17, I17 = eng.search(q, 17)
    assert_bitwise(D17[:, :16], I17[:, :16], D16, I16)
    for splits in ("1", "3"):
        monkeypatch.setenv(KNOB, splits)
        assert_bitwise(*eng.search(q, 16), D16, I16)
    monkeypatch.delenv(KNOB)
    Dr, Ir, R = eng.search_and_reconstruct(q[:5], 4)
    assert_bitwise(Dr, Ir, D16[:5, :4], I16[:5, :4])
    np.testing.assert_array_equal(
        R, x.astype(np.float16).astype(np.float32)[Ir])
    path = str(tmp_path / "flat_f16.dfann")
    eng.save(path)
    back = HipProvider().load(path)
    assert back.spec["flat_store"] == "fp16" and back.ntotal == n
    assert_bitwise(*back.search(q, 16), D16, I16)
    assert_bitwise(*back.search(q, 17), D17, I17)


def test_duplicate_rows_tie_in_ascending_id_order():
    d, n, nq, k = 20, 350, 300, 16
    x, q = _data(d, n, nq, 11)
    D, I = _engine(np.concatenate([x, x]), L2).search(q, k)
    np.testing.assert_array_equal(D[:, 0::2].view(np.uint32),
                                  D[:, 1::2].view(np.uint32))
    tied = D[:, 1:] == D[:, :-1]
    assert (I[:, 1:] > I[:, :-1])[tied].all()
    np.testing.assert_array_equal(np.sort(I[:, 0::2] % n, axis=1),
                                  np.sort(I[:, 1::2] % n, axis=1))


def test_filter_then_removal():
    d, n, nq, k, metric, seed = FILTER_CASE
    x, q = _data(d, n, nq, seed)
    eng = _engine(x, metric)
    ids = np.arange(n)
    allow = ids % 3 == 0
    D, I = eng.search_filtered(q, k, allow)
    _assert_against_fp64(FILTER_CASE, D, I, k, keep=allow)
    assert eng.remove_ids(ids[ids % 3 == 1]) == (ids % 3 == 1).sum()
    D, I = eng.search(q, k)
    _assert_against_fp64(FILTER_CASE, D, I, k, keep=ids % 3 != 1)


def test_create_refuses_bad_flat_store():
    with pytest.raises(RuntimeError, match="flat_store"):
        HipEngine(spec={"type": "flat", "dim": 8, "metric": IP,
                        "flat_store": "bf16"})
    with pytest.raises(RuntimeError, match="flat_store"):
        HipEngine(spec={"type": "ivf_flat", "dim": 8, "metric": IP,
                        "nlist": 4, "flat_store": "fp16"})
