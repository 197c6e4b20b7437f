# Grouped (list-major) MFMA scan of ivfsq fp16 lists: spec "scan_group",
# DESIGN.md §6n, k_scan_sqf_grp.
#
# Reference: numpy float64 over the operands the kernel multiplies — the stored
# fp16 rows (get_lists) and fp16(q - c) (L2; one fp32 subtraction, then the
# rounding) or fp16(q) (IP, plus the coarse key's q . c) — for the probes of
# `coarse`. Bound of a candidate, as tests/test_gpu_flat_f16.py:
# 1e-4 * (|a|^2 + |x|^2 + 2 sum|a_t x_t|) + 1e-4, the norms dropped under IP.
#
# Among ~10^4 Gaussian candidates a query's neighbouring ranks are closer
# than that bound, so the data plants them: every query gets 17 rows at
# stepped distances (L2: q + e sqrt(d (0.02 + 0.005 j)), e a unit vector; IP:
# (6 - 0.1 j) q) in front of a background of 3 N(0, 1) rows. The steps are
# four or more bounds wide; _check asserts, from inputs and reference alone,
# that at most 1 % of the queries have an undecided k boundary.
#
# Shapes (GS_TQ = 64 pair rows, GS_TN = 128 list rows, GS_K = 64 halves):
# N = 20011 over 8 lists is 1000-4500 rows a list, none a multiple of the row
# tile (asserted); slab_mb = 1 is 8192 / 2048 / 1024 rows a slab at d = 20 /
# 72 / 192, so lists cross slab boundaries; 300 x 4 pairs over 8 lists is ~150
# a list, three query tiles with a ragged last (asserted: one above 128). d =
# 20: 24-half rows (row pad, one partial K block); 72: a K-block tail; 192:
# three K blocks.
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
KNOB = "DFANN_SCAN_GROUP"


def _spec(metric, d, nlist=NLIST, **kw):
    return ivf_spec("ivfsq", d, metric, nlist, sq_type="fp16", slab_mb=1,
                    nprobe=NPROBE, **kw)


@functools.lru_cache(maxsize=None)
def _data(metric, d):
    """Centroids, rows, queries, and the (NQ, NPLANT) ids of the planted rows
    (draws: cent, q, x, [e,] the planted ids)."""
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
    return cent, x, q, where.reshape(NQ, NPLANT)


@functools.lru_cache(maxsize=None)
def _case(metric, d):
    """Engine, queries, and the fp64 (NQ, N) distances and bounds by CSR
    position, +inf key outside the probed lists."""
    cent, x, q, _ = _data(metric, d)
    eng = engine_with(_spec(metric, d, scan_group=1), cent, xb=x)
    off, ids, codes = eng.get_lists()
    assert (np.diff(off) % 128 != 0).all()
    rows = codes.view(np.float16)[:, :d].astype(np.float64)
    probes, keys = eng.coarse(q, NPROBE)
    assert np.bincount(probes.ravel(), minlength=NLIST).max() > 128
    D64 = np.empty((NQ, N))
    bound = np.empty((NQ, N))
    probed = np.zeros((NQ, N), bool)
    c = eng.get_centroids()
    for l in range(NLIST):
        xs = rows[off[l]:off[l + 1]]
        a = (q if metric == IP else q - c[l]).astype(np.float16).astype(np.float64)
        dot, mag = a @ xs.T, 2.0 * (np.abs(a) @ np.abs(xs).T)
        sl = slice(off[l], off[l + 1])
        if metric == IP:
            bias = np.zeros(NQ)  # q . c of the coarse key, where l is probed
            hit = probes == l
            bias[hit.any(1)] = -keys[hit].astype(np.float64)
            D64[:, sl], bound[:, sl] = bias[:, None] + dot, 1e-4 * mag + 1e-4
        else:
            an, xn = (a * a).sum(1)[:, None], (xs * xs).sum(1)[None, :]
            D64[:, sl] = an + xn - 2.0 * dot
            bound[:, sl] = 1e-4 * (an + xn + mag) + 1e-4
        probed[:, sl] = (probes == l).any(1)[:, None]
    return eng, q, ids, D64, bound, probed


def _check(metric, d, D, I, k, keep=None):
    """Distances within the bound at the returned ids; id sets equal to the
    fp64 top-k wherever its boundary gap exceeds the two bounds; at most 1 %
    of the queries excepted (a property of inputs and reference alone)."""
    _, _, ids, D64, bound, probed = _case(metric, d)
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
    print(f"metric={metric} d={d} k={k}: max err / bound = {rel.max():.3g}, "
          f"undecided = {(~decided).sum()}")
    assert (rel <= 1.0).all()
    np.testing.assert_array_equal(np.sort(I[decided], 1),
                                  np.sort(ids[order[decided, :k]], 1))


@pytest.mark.parametrize("d", [20, 72, 192])
@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("metric", [L2, IP])
def test_against_fp64(metric, k, d):
    eng, q = _case(metric, d)[:2]
    _check(metric, d, *eng.search(q, k), k)


@pytest.mark.parametrize("metric", [L2, IP])
def test_independence_and_fallbacks(metric, monkeypatch):
    """Rows of a batch are those of the reversed batch and of each query
    alone; runs repeat; k = 17, range search and DFANN_SCAN_GROUP=0 give what
    a scan_group: 0 index gives."""
    eng, q = _case(metric, 72)[:2]
    D, I = eng.search(q, 10)
    assert_bitwise(*eng.search(q, 10), D, I)
    Dr, Ir = eng.search(q[::-1], 10)
    assert_bitwise(Dr[::-1], Ir[::-1], D, I)
    for i in (0, 151, NQ - 1):
        assert_bitwise(*eng.search(q[i:i + 1], 10), D[i:i + 1], I[i:i + 1])
    cent, x = _data(metric, 72)[:2]
    base = engine_with(_spec(metric, 72), cent, xb=x)
    radius = float(np.median(D[:, 0]))
    assert_bitwise(*eng.search(q, 17), *base.search(q, 17))
    for got, ref in zip(eng.range_search(q, radius), base.range_search(q, radius)):
        np.testing.assert_array_equal(got.view(np.uint8), ref.view(np.uint8))
    monkeypatch.setenv(KNOB, "0")
    assert_bitwise(*eng.search(q, 10), *base.search(q, 10))


@pytest.mark.parametrize("metric", [L2, IP])
def test_filtered(metric):
    """~12 % allowed: 4 % of all rows and every third planted row (six a
    query, k = 5); then nothing allowed."""
    eng, q = _case(metric, 72)[:2]
    allow = np.random.default_rng(5).random(N) < 0.04
    allow[_data(metric, 72)[3][:, ::3]] = True
    _check(metric, 72, *eng.search_filtered(q, 5, allow), 5, keep=allow)
    D, I = eng.search_filtered(q, 10, np.zeros(N, bool))
    assert (I == -1).all()
    assert (D == (-FLT_MAX if metric == IP else FLT_MAX)).all()


def test_nan_query_row():
    eng, q = _case(L2, 72)[:2]
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
    pair-major scan pads, the duplicate's hits twice; list 3 is probed by no
    query; nq = 1."""
    d, k = 20, 10
    rng = np.random.default_rng(9)
    cent = rng.standard_normal((6, d), dtype=np.float32)
    cent[4:] = [[40.0], [-40.0]]
    x = rng.standard_normal((603, d), dtype=np.float32) * 0.3
    x += cent[np.r_[np.arange(600) % 4, [4, 4, 4]]]
    eng = engine_with(_spec(L2, d, nlist=6, scan_group=1), cent, xb=x)
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
    _spec(L2, 16, scan_group=2),
    dict(_spec(L2, 16, scan_group=1), sq_type="8bit"),
    dict(_spec(L2, 16, scan_group=1), type="ivfpq", m=4),
    dict(_spec(L2, 16, scan_group=1), type="ivf_flat"),
    {"type": "flat", "dim": 16, "metric": IP, "scan_group": 1},
], ids=lambda s: f"{s['type']}-{s.get('sq_type')}-{s['scan_group']}")
def test_create_refuses(spec):
    with pytest.raises(RuntimeError, match="scan_group"):
        HipEngine(spec=spec)
