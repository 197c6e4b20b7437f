# Grouped (list-major) MFMA scan of ivfpq lists with 8-bit codes: spec
# "scan_group_pq", DESIGN.md §6p (the bound is derived there), k_scan_pq_grp.
# Reference: numpy float64 over the stored codes, decoded through the injected
# fp32 codebooks; none of the kernel's scaling or rounding is replayed. Bound,
# with b the decoded codewords: L2, w = q - c, 1.001 2^-10 (X + V) + 1e-4 (W +
# X + V) + tau, X = 2 sum|w b|, V = sum b^2, W = sum w^2; IP 1.001 2^-10 X' +
# 1e-4 (|q.c| + X') + tau, X' = sum|q b|; tau = 1e-4 s^2 for inputs scaled by s.
# Centroids, queries and codebooks are standard normal, rows cent[l] + decode
# of uniform random codes, N = 20011 over 8 lists of SIZES (at d = 24 some
# rows land in another list than l; that no length is k * 128 is asserted on
# the engine's lists). No planted near-duplicates: they would encode to
# identical codes and tie. The id check is therefore completeness, which
# holds for the reference on any input: a probed row that was not returned
# has key64 + bound >= the returned k-th key.
# Shapes (d, m): (24, 12) dsub 2, one partial K block, row pad; (32, 8) dsub 4;
# (96, 8) dsub 12, a K block ends inside a sub-quantizer; (136, 17) dsub 8, a
# K-block tail, odd m; (776, 97) 13 K blocks, the A tile not resident in LDS.
# s = 2^-17: unscaled fp16 operands would be subnormal.
import functools
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
from gpu_support import (IP, L2, assert_bitwise, decode_rows, engine_with,  # noqa: E402
                         ivf_spec, labels)

SIZES = [2501, 2417, 2583, 2499, 2610, 2390, 2523, 2488]  # none k * 128
N, NLIST, NQ, NPROBE = sum(SIZES), len(SIZES), 300, 4
FLT_MAX = np.float32(3.4028235e38)
KNOB = "DFANN_SCAN_GROUP_PQ"
TINY = 2.0 ** -17


def _spec(metric, d, m, nlist=NLIST, **kw):
    return ivf_spec("ivfpq", d, metric, nlist, m=m, nbits=8, slab_mb=1,
                    nprobe=NPROBE, **kw)


@functools.lru_cache(maxsize=None)
def _data(d, m, s):
    """Centroids, codebooks, rows, queries, all times s (a power of two)."""
    rng = np.random.default_rng(100 + d)
    cent = rng.standard_normal((NLIST, d), dtype=np.float32)
    q = rng.standard_normal((NQ, d), dtype=np.float32)
    cb = rng.standard_normal((m, 256, d // m), dtype=np.float32)
    x = cent[labels(rng, SIZES)] + decode_rows(
        cb, rng.integers(0, 256, (N, m)))
    return tuple(np.float32(s) * a for a in (cent, cb, x, q))


def _reference(metric, s, q, c, cb, off, codes, probes):
    """fp64 (NQ, N) distances, bounds and probed mask by CSR position."""
    q, c, cb = (a.astype(np.float64) for a in (q, c, cb))
    D64, bound = np.empty((NQ, N)), np.empty((NQ, N))
    probed = np.zeros((NQ, N), bool)
    for l in range(NLIST):
        sl = slice(off[l], off[l + 1])
        b = decode_rows(cb, codes[sl, :cb.shape[0]].astype(np.int64))
        if metric == IP:
            X = np.abs(q) @ np.abs(b).T
            D64[:, sl] = (q @ c[l])[:, None] + q @ b.T
            bound[:, sl] = 1.001 * 2.0 ** -10 * X + 1e-4 * (
                np.abs(q @ c[l])[:, None] + X)
        else:
            w = q - c[l]
            X = 2.0 * (np.abs(w) @ np.abs(b).T)
            W, V = (w * w).sum(1)[:, None], (b * b).sum(1)[None, :]
            D64[:, sl] = W - 2.0 * (w @ b.T) + V
            bound[:, sl] = 1.001 * 2.0 ** -10 * (X + V) + 1e-4 * (W + X + V)
        probed[:, sl] = (probes == l).any(1)[:, None]
    return D64, bound + 1e-4 * s * s, probed


@functools.lru_cache(maxsize=None)
def _case(metric, d, m, s=1.0):
    cent, cb, x, q = _data(d, m, s)
    eng = engine_with(_spec(metric, d, m, scan_group_pq=1), cent, cb=cb, xb=x)
    off, ids, codes = eng.get_lists()
    assert (np.diff(off) % 128 != 0).all()
    probes, _ = eng.coarse(q, NPROBE)
    assert np.bincount(probes.ravel(), minlength=NLIST).max() > 128
    return (eng, q, ids) + _reference(metric, s, q, eng.get_centroids(), cb,
                                      off, codes, probes)


def _check(case, metric, D, I, k, keep=None):
    """Ids valid, probed and distinct; distances within the bound at the
    returned ids; no probed row outside the rounding band was left out."""
    _, _, ids, D64, bound, probed = case
    key = np.where(probed, -D64 if metric == IP else D64, np.inf)
    if keep is not None:
        key[:, ~keep[ids]] = np.inf
    assert (I >= 0).all()
    assert (np.diff(np.sort(I, 1), axis=1) > 0).all()
    pos = np.argsort(ids)[I]  # ids are a permutation of 0..N-1
    assert np.isfinite(np.take_along_axis(key, pos, 1)).all()
    err = np.abs(D.astype(np.float64) - np.take_along_axis(D64, pos, 1))
    rel = err / np.take_along_axis(bound, pos, 1)
    print(f"metric={metric} k={k}: max err / bound = {rel.max():.3g}")
    assert (rel <= 1.0).all()
    out = np.ones(key.shape, bool)
    np.put_along_axis(out, pos, False, 1)
    kth = (-D if metric == IP else D)[:, k - 1].astype(np.float64)
    assert not (out & (key + bound < kth[:, None])).any()


@pytest.mark.parametrize("d,m,k,s", [
    (24, 12, 1, 1.0), (32, 8, 10, 1.0), (96, 8, 10, 1.0), (136, 17, 16, 1.0),
    (136, 17, 10, TINY), (776, 97, 10, 1.0)])
@pytest.mark.parametrize("metric", [L2, IP])
def test_against_fp64(metric, d, m, k, s):
    case = _case(metric, d, m, s)
    _check(case, metric, *case[0].search(case[1], k), k)


@pytest.mark.parametrize("metric", [L2, IP])
def test_independence_and_fallbacks(metric, monkeypatch):
    """Batch = reversed batch = single queries, runs repeat; k = 17, range
    search and the knob at 0 give what a scan_group_pq: 0 index gives, the
    knob unset does not (that scan is fp32-exact: the grouped kernel ran)."""
    eng, q = _case(metric, 136, 17)[:2]
    D, I = eng.search(q, 10)
    assert_bitwise(*eng.search(q, 10), D, I)
    Dr, Ir = eng.search(q[::-1], 10)
    assert_bitwise(Dr[::-1], Ir[::-1], D, I)
    for i in (0, 151, NQ - 1):
        assert_bitwise(*eng.search(q[i:i + 1], 10), D[i:i + 1], I[i:i + 1])
    cent, cb, x = _data(136, 17, 1.0)[:3]
    base = engine_with(_spec(metric, 136, 17), cent, cb=cb, xb=x)
    radius = float(np.median(D[:, 0]))
    assert_bitwise(*eng.search(q, 17), *base.search(q, 17))
    for got, ref in zip(eng.range_search(q, radius), base.range_search(q, radius)):
        np.testing.assert_array_equal(got.view(np.uint8), ref.view(np.uint8))
    Db, Ib = base.search(q, 10)
    assert (D.view(np.uint32) != Db.view(np.uint32)).any()
    monkeypatch.setenv(KNOB, "0")
    assert_bitwise(*eng.search(q, 10), Db, Ib)


@pytest.mark.parametrize("metric", [L2, IP])
def test_filtered(metric):
    """~12 % allowed; then nothing."""
    case = _case(metric, 136, 17)
    eng, q = case[:2]
    allow = np.random.default_rng(5).random(N) < 0.12
    _check(case, metric, *eng.search_filtered(q, 5, allow), 5, keep=allow)
    D, I = eng.search_filtered(q, 10, np.zeros(N, bool))
    assert (I == -1).all()
    assert (D == (-FLT_MAX if metric == IP else FLT_MAX)).all()


def test_nan_query_row():
    eng, q = _case(L2, 136, 17)[:2]
    qn, qz = q[:40].copy(), q[:40].copy()
    qn[7], qz[7] = np.nan, 0.0
    Dn, In = eng.search(qn, 10)
    Dz, Iz = eng.search(qz, 10)
    assert (In[7] == -1).all() and (Dn[7] == FLT_MAX).all()
    rest = np.arange(40) != 7
    assert_bitwise(Dn[rest], In[rest], Dz[rest], Iz[rest])


def test_preassigned_edge_cases(monkeypatch):
    """Probe rows with -1, nlist, an empty list and one list twice: pads
    where the pair-major scan pads, the duplicate's hits twice; nq = 1."""
    d, m, k = 24, 12, 10
    rng = np.random.default_rng(9)
    cent = rng.standard_normal((6, d), dtype=np.float32)
    cent[4:] = [[40.0], [-40.0]]
    cb = 0.3 * rng.standard_normal((m, 256, d // m), dtype=np.float32)
    x = rng.standard_normal((603, d), dtype=np.float32) * 0.3
    x += cent[np.r_[np.arange(600) % 4, [4, 4, 4]]]
    eng = engine_with(_spec(L2, d, m, nlist=6, scan_group_pq=1), cent, cb=cb,
                      xb=x)
    assert list(np.diff(eng.get_lists()[0])) == [150] * 4 + [3, 0]
    q = x[[0, 1, 2, 600]]
    probes = np.array([[-1, 6, 5, 0, 0], [1, 1, -1, 5, 6], [5, 6, -1, -1, 5],
                       [4, 6, 4, 5, -1]], np.int32)
    keys = np.zeros(probes.shape, np.float32)
    D, I = eng.search_preassigned(q, probes, keys, k)
    for i in range(4):
        assert_bitwise(*eng.search_preassigned(q[i:i + 1], probes[i:i + 1],
                                               keys[i:i + 1], k),
                       D[i:i + 1], I[i:i + 1])
    monkeypatch.setenv(KNOB, "0")
    Ip = eng.search_preassigned(q, probes, keys, k)[1]
    np.testing.assert_array_equal(I == -1, Ip == -1)
    assert (I[2] == -1).all() and (I[3, :6] >= 600).all() and (I[3, 6:] == -1).all()
    np.testing.assert_array_equal(I[[0, 1, 3], 0:6:2], I[[0, 1, 3], 1:6:2])
    assert (D[I == -1] == FLT_MAX).all()


@pytest.mark.parametrize("spec", [
    _spec(L2, 16, 4, scan_group_pq=2),
    ivf_spec("ivfsq", 16, L2, NLIST, sq_type="fp16", scan_group_pq=1),
    ivf_spec("ivfsq", 16, L2, NLIST, sq_type="8bit", scan_group_pq=1),
    ivf_spec("ivf_flat", 16, L2, NLIST, scan_group_pq=1),
    {"type": "flat", "dim": 16, "metric": IP, "scan_group_pq": 1},
    dict(_spec(L2, 16, 4, scan_group_pq=1), nbits=4),
    _spec(L2, 15, 5, scan_group_pq=1),
    _spec(L2, 16, 4, scan_group_pq=1, pq_precomputed=1),
], ids=["value-2", "ivfsq-fp16", "ivfsq-8bit", "ivf_flat", "flat", "nbits-4",
        "odd-dsub", "pq_precomputed"])
def test_create_refuses(spec):
    with pytest.raises(RuntimeError, match="scan_group_pq"):
        HipEngine(spec=spec)
