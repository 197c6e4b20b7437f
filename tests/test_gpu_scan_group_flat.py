# Grouped (list-major) MFMA scan of fp32 ivf_flat lists: spec
# "scan_group_flat", DESIGN.md §6q (the bound is derived there),
# k_scan_flat_grp. Reference: numpy float64 over the stored rows (get_lists)
# and, for L2, a = fp32(q - c) and r = fp32(x - c), one float32 subtraction
# each; IP takes q and x as they are, key -dot. Bound of a candidate: L2
# 2^-14 X + 1e-4 (W + X + V) + tau, X = 2 sum|a r|, W = sum a^2, V = sum r^2;
# IP (2^-14 + 1e-4) X' + tau, X' = sum|q x|; tau = 1e-4 s^2 for inputs scaled
# by s. Data, planted neighbours and list shapes are test_gpu_scan_group.py's
# (17 rows a query at stepped distances, four or more bounds apart; _check
# asserts from inputs and reference alone that at most 1 % of the queries have
# an undecided k boundary). d (K blocks of 32 dimensions): 20 row pad (stride
# 80), one partial block; 40 a tail of 8; 136 five blocks with a tail; 392
# thirteen, the A tile not resident in LDS. slab_mb = 1 is 8192 .. 512 rows a
# slab, so lists cross slab boundaries.
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
from gpu_support import IP, L2, assert_bitwise, engine_with, ivf_spec  # noqa: E402

N, NLIST, NQ, NPROBE, NPLANT = 20011, 8, 300, 4, 17
FLT_MAX = np.float32(3.4028235e38)
KNOB = "DFANN_SCAN_GROUP_FLAT"
TINY = 2.0 ** -17


def _spec(metric, d, nlist=NLIST, **kw):
    return ivf_spec("ivf_flat", d, metric, nlist, slab_mb=1, nprobe=NPROBE, **kw)


@functools.lru_cache(maxsize=None)
def _data(metric, d, s=1.0):
    """Centroids, rows, queries, all times s (a power of two), and the (NQ,
    NPLANT) ids of the planted rows (draws: cent, q, x, [e,] the ids)."""
    rng = np.random.default_rng(100 + d)
    cent = rng.standard_normal((NLIST, d), dtype=np.float32)
    q = rng.standard_normal((NQ, d), dtype=np.float32)
    x = 3.0 * rng.standard_normal((N, d), dtype=np.float32)
    j = np.arange(NPLANT, dtype=np.float32)
    if metric == IP:
        plant = q[:, None, :] * (6.0 - 0.1 * j)[None, :, None]
    else:
        e = rng.standard_normal((NQ, NPLANT, d), dtype=np.float32)
        e /= np.linalg.norm(e, axis=2, keepdims=True)
        plant = q[:, None, :] + e * np.sqrt(d * (0.02 + 0.005 * j))[None, :, None]
    where = rng.choice(N, NQ * NPLANT, replace=False)
    x[where] = plant.reshape(-1, d)
    return tuple(np.float32(s) * a for a in (cent, x, q)) + (
        where.reshape(NQ, NPLANT),)


def _reference(metric, s, q, c, off, rows, probes):
    """fp64 (NQ, N) distances, bounds and probed mask by CSR position."""
    D64, bound = np.empty((NQ, N)), np.empty((NQ, N))
    probed = np.zeros((NQ, N), bool)
    for l in range(len(c)):
        sl = slice(off[l], off[l + 1])
        if metric == IP:
            a, r = q.astype(np.float64), rows[sl].astype(np.float64)
            D64[:, sl] = a @ r.T
            bound[:, sl] = (2.0 ** -14 + 1e-4) * (np.abs(a) @ np.abs(r).T)
        else:
            a, r = ((v - c[l]).astype(np.float64) for v in (q, rows[sl]))
            X = 2.0 * (np.abs(a) @ np.abs(r).T)
            W, V = (a * a).sum(1)[:, None], (r * r).sum(1)[None, :]
            D64[:, sl] = W - 2.0 * (a @ r.T) + V
            bound[:, sl] = 2.0 ** -14 * X + 1e-4 * (W + X + V)
        probed[:, sl] = (probes == l).any(1)[:, None]
    return D64, bound + 1e-4 * s * s, probed


@functools.lru_cache(maxsize=None)
def _case(metric, d, s=1.0):
    cent, x, q, _ = _data(metric, d, s)
    eng = engine_with(_spec(metric, d, scan_group_flat=1), cent, xb=x)
    off, ids, codes = eng.get_lists()
    assert (np.diff(off) % 128 != 0).all()
    probes, _ = eng.coarse(q, NPROBE)
    assert np.bincount(probes.ravel(), minlength=NLIST).max() > 128
    rows = np.ascontiguousarray(codes[:, :4 * d]).view(np.float32)
    return (eng, q, ids) + _reference(metric, s, q, eng.get_centroids(), off,
                                      rows, probes)


def _check(case, metric, D, I, k, keep=None):
    """Distances within the bound at the returned ids; id sets equal to the
    fp64 top-k wherever its boundary gap exceeds the two bounds; at most 1 %
    of the queries excepted (a property of inputs and reference alone)."""
    _, _, ids, D64, bound, probed = case
    key = np.where(probed, -D64 if metric == IP else D64, np.inf)
    if keep is not None:
        key[:, ~keep[ids]] = np.inf
    order = np.argsort(key, axis=1, kind="stable")[:, :k + 1]
    ks, bs = (np.take_along_axis(m, order, 1) for m in (key, bound))
    decided = ks[:, k] - ks[:, k - 1] > bs[:, k] + bs[:, k - 1]
    assert (~decided).mean() <= 0.01
    assert np.isfinite(ks[:, :k]).all() and (I >= 0).all()
    pos = np.argsort(ids)[I]  # ids are a permutation of 0..N-1
    assert np.isfinite(np.take_along_axis(key, pos, 1)).all()
    err = np.abs(D.astype(np.float64) - np.take_along_axis(D64, pos, 1))
    rel = err / np.take_along_axis(bound, pos, 1)
    print(f"metric={metric} k={k}: max err / bound = {rel.max():.3g}, "
          f"undecided = {(~decided).sum()}")
    assert (rel <= 1.0).all()
    np.testing.assert_array_equal(np.sort(I[decided], 1),
                                  np.sort(ids[order[decided, :k]], 1))


@pytest.mark.parametrize("d,k,s", [(d, k, 1.0) for d in (20, 40, 136)
                                   for k in (1, 10, 16)]
                         + [(392, 10, 1.0), (136, 10, TINY)])
@pytest.mark.parametrize("metric", [L2, IP])
def test_against_fp64(metric, d, k, s):
    case = _case(metric, d, s)
    _check(case, metric, *case[0].search(case[1], k), k)


@pytest.mark.parametrize("metric", [L2, IP])
def test_independence_and_fallbacks(metric, monkeypatch):
    """Batch = reversed batch = single queries, runs repeat; k = 17, range
    search and the knob at 0 give what a scan_group_flat: 0 index gives, the
    knob unset does not (the grouped kernel ran)."""
    eng, q = _case(metric, 40)[:2]
    D, I = eng.search(q, 10)
    assert_bitwise(*eng.search(q, 10), D, I)
    Dr, Ir = eng.search(q[::-1], 10)
    assert_bitwise(Dr[::-1], Ir[::-1], D, I)
    for i in (0, 151, NQ - 1):
        assert_bitwise(*eng.search(q[i:i + 1], 10), D[i:i + 1], I[i:i + 1])
    cent, x = _data(metric, 40)[:2]
    base = engine_with(_spec(metric, 40), cent, xb=x)
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
    """~12 % allowed: 4 % of all rows and every third planted row (six a
    query, k = 5); then nothing allowed."""
    case = _case(metric, 40)
    eng, q = case[:2]
    allow = np.random.default_rng(5).random(N) < 0.04
    allow[_data(metric, 40)[3][:, ::3]] = True
    _check(case, metric, *eng.search_filtered(q, 5, allow), 5, keep=allow)
    D, I = eng.search_filtered(q, 10, np.zeros(N, bool))
    assert (I == -1).all()
    assert (D == (-FLT_MAX if metric == IP else FLT_MAX)).all()


def test_nan_query_row():
    eng, q = _case(L2, 40)[:2]
    qn, qz = q[:40].copy(), q[:40].copy()
    qn[7], qz[7] = np.nan, 0.0
    Dn, In = eng.search(qn, 10)
    Dz, Iz = eng.search(qz, 10)
    assert (In[7] == -1).all() and (Dn[7] == FLT_MAX).all()
    rest = np.arange(40) != 7
    assert_bitwise(Dn[rest], In[rest], Dz[rest], Iz[rest])


def test_preassigned_edge_cases(monkeypatch):
    """Lists 0-3 hold 150 rows each, list 4 three rows, list 5 none. Probe
    rows with -1, nlist, the empty list and one list twice: pads where the
    pair-major scan pads, the duplicate's hits twice; nq = 1."""
    d, k = 20, 10
    rng = np.random.default_rng(9)
    cent = rng.standard_normal((6, d), dtype=np.float32)
    cent[4:] = [[40.0], [-40.0]]
    x = rng.standard_normal((603, d), dtype=np.float32) * 0.3
    x += cent[np.r_[np.arange(600) % 4, [4, 4, 4]]]
    eng = engine_with(_spec(L2, d, nlist=6, scan_group_flat=1), cent, xb=x)
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
    _spec(L2, 16, scan_group_flat=2),
    ivf_spec("ivfsq", 16, L2, NLIST, sq_type="fp16", scan_group_flat=1),
    ivf_spec("ivfpq", 16, L2, NLIST, m=4, scan_group_flat=1),
    {"type": "flat", "dim": 16, "metric": IP, "scan_group_flat": 1},
], ids=["value-2", "ivfsq", "ivfpq", "flat"])
def test_create_refuses(spec):
    with pytest.raises(RuntimeError, match="scan_group_flat"):
        HipEngine(spec=spec)
