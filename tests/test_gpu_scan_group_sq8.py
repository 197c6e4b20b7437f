# Grouped (list-major) MFMA scan of ivfsq 8-bit lists: spec "scan_group_sq8",
# DESIGN.md §6o (the bound is derived there), k_scan_sq8_grp.
# Reference: numpy float64 over the stored codes, decoded plainly, x^ = cent +
# vmin + (c + 0.5) vdiff / 255; none of the kernel's scaling or rounding is
# replayed. Bound, with s = vdiff / 255, b = c - 128, mid = vmin + 128.5 s,
# w = q - cent - mid: L2 2^-11 X + 1e-4 (W + X + V) + 1e-4, X = 2 sum|w s b|;
# IP 2^-11 X' + 1e-4 (|q.c| + sum|q mid| + X') + 1e-4, X' = sum|q s b|.
# Data and shapes as tests/test_gpu_scan_group.py, planted rows at L2 q + e
# sqrt(d (0.05 + 0.03 j)), IP (6 - 0.1 j) q. Ranges +-h f_t, f_t = 0.5 *
# 4^U(0,1), h = 14 (L2) / 30 (IP): scales differ up to 4x between dimensions
# and rows clamp to codes 0 and 255 (asserted). d = 20: 32-byte stride, row
# pad, one partial K block of 128 codes; 136: a K-block tail; 264: three K
# blocks; 776: seven, the A tile no longer resident in LDS.
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
KNOB = "DFANN_SCAN_GROUP_SQ8"


def _spec(metric, d, nlist=NLIST, **kw):
    return ivf_spec("ivfsq", d, metric, nlist, sq_type="8bit", slab_mb=1,
                    nprobe=NPROBE, **kw)


def _ranges(metric, d):
    f = 0.5 * 4.0 ** np.random.default_rng(7 + d).random(d)
    h = (30.0 if metric == IP else 14.0) * f
    return dict(vmin=(-h).astype(np.float32), vdiff=(2 * h).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _data(metric, d):
    """Centroids, rows, queries, (NQ, NPLANT) ids of the planted rows."""
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
        plant = q[:, None, :] + e * np.sqrt(d * (0.05 + 0.03 * j))[None, :, None]
    where = rng.choice(N, NQ * NPLANT, replace=False)
    x[where] = plant.reshape(-1, d)
    return cent, x, q, where.reshape(NQ, NPLANT)


def _reference(metric, d, q, c, off, codes, probes):
    """fp64 (NQ, N) distances, bounds and probed mask by CSR position."""
    r = {k: v.astype(np.float64) for k, v in _ranges(metric, d).items()}
    s = r["vdiff"] / 255.0
    mid = r["vmin"] + 128.5 * s
    q, c = q.astype(np.float64), c.astype(np.float64)
    D64, bound = np.empty((NQ, N)), np.empty((NQ, N))
    probed = np.zeros((NQ, N), bool)
    for l in range(NLIST):
        sl = slice(off[l], off[l + 1])
        cd = codes[sl, :d].astype(np.float64)
        xhat = c[l] + r["vmin"] + (cd + 0.5) * s
        sb = np.abs(s * (cd - 128.0))
        if metric == IP:
            X = np.abs(q) @ sb.T
            D64[:, sl] = q @ xhat.T
            bound[:, sl] = 2.0 ** -11 * X + 1e-4 * (
                np.abs(q @ c[l]) + np.abs(q * mid).sum(1))[:, None] + 1e-4 * X
        else:
            w = q - c[l] - mid
            X = 2.0 * (np.abs(w) @ sb.T)
            D64[:, sl] = ((q * q).sum(1)[:, None] + (xhat * xhat).sum(1)[None, :]
                          - 2.0 * (q @ xhat.T))
            bound[:, sl] = 2.0 ** -11 * X + 1e-4 * (
                (w * w).sum(1)[:, None] + X + (sb * sb).sum(1)[None, :])
        probed[:, sl] = (probes == l).any(1)[:, None]
    return D64, bound + 1e-4, probed


@functools.lru_cache(maxsize=None)
def _case(metric, d):
    cent, x, q, _ = _data(metric, d)
    eng = engine_with(_spec(metric, d, scan_group_sq8=1), cent, xb=x,
                      **_ranges(metric, d))
    off, ids, codes = eng.get_lists()
    assert (np.diff(off) % 128 != 0).all()
    assert ((codes[:, :d] == 0).any() and (codes[:, :d] == 255).any())
    probes, _ = eng.coarse(q, NPROBE)
    assert np.bincount(probes.ravel(), minlength=NLIST).max() > 128
    return (eng, q, ids) + _reference(metric, d, q, eng.get_centroids(), off,
                                      codes, probes)


def _check(metric, d, D, I, k, keep=None):
    """Distances within the bound at the returned ids; id sets equal to the
    fp64 top-k where its boundary gap exceeds the two bounds; at most 1 % of
    the queries undecided (a property of inputs and reference alone)."""
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


@pytest.mark.parametrize("d,k", [(136, 1), (136, 10), (136, 16), (264, 10),
                                 (20, 1), (776, 10)])
@pytest.mark.parametrize("metric", [L2, IP])
def test_against_fp64(metric, d, k):
    eng, q = _case(metric, d)[:2]
    _check(metric, d, *eng.search(q, k), k)


@pytest.mark.parametrize("metric", [L2, IP])
def test_independence_and_fallbacks(metric, monkeypatch):
    """Batch = reversed batch = single queries, runs repeat; k = 17, range
    search and the knob at 0 give what a scan_group_sq8: 0 index gives."""
    eng, q = _case(metric, 136)[:2]
    D, I = eng.search(q, 10)
    assert_bitwise(*eng.search(q, 10), D, I)
    Dr, Ir = eng.search(q[::-1], 10)
    assert_bitwise(Dr[::-1], Ir[::-1], D, I)
    for i in (0, 151, NQ - 1):
        assert_bitwise(*eng.search(q[i:i + 1], 10), D[i:i + 1], I[i:i + 1])
    cent, x = _data(metric, 136)[:2]
    base = engine_with(_spec(metric, 136), cent, xb=x, **_ranges(metric, 136))
    radius = float(np.median(D[:, 0]))
    assert_bitwise(*eng.search(q, 17), *base.search(q, 17))
    for got, ref in zip(eng.range_search(q, radius), base.range_search(q, radius)):
        np.testing.assert_array_equal(got.view(np.uint8), ref.view(np.uint8))
    monkeypatch.setenv(KNOB, "0")
    assert_bitwise(*eng.search(q, 10), *base.search(q, 10))


@pytest.mark.parametrize("metric", [L2, IP])
def test_filtered(metric):
    """~12 % allowed, every third planted row among them; then nothing."""
    eng, q = _case(metric, 136)[:2]
    allow = np.random.default_rng(5).random(N) < 0.04
    allow[_data(metric, 136)[3][:, ::3]] = True
    _check(metric, 136, *eng.search_filtered(q, 5, allow), 5, keep=allow)
    D, I = eng.search_filtered(q, 10, np.zeros(N, bool))
    assert (I == -1).all()
    assert (D == (-FLT_MAX if metric == IP else FLT_MAX)).all()


def test_nan_query_row():
    eng, q = _case(L2, 136)[:2]
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
    d, k = 20, 10
    rng = np.random.default_rng(9)
    cent = rng.standard_normal((6, d), dtype=np.float32)
    cent[4:] = [[40.0], [-40.0]]
    x = rng.standard_normal((603, d), dtype=np.float32) * 0.3
    x += cent[np.r_[np.arange(600) % 4, [4, 4, 4]]]
    eng = engine_with(_spec(L2, d, nlist=6, scan_group_sq8=1), cent, xb=x,
                      **_ranges(L2, d))
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
    _spec(L2, 16, scan_group_sq8=2),
    dict(_spec(L2, 16, scan_group_sq8=1), sq_type="fp16"),
    dict(_spec(L2, 16, scan_group_sq8=1), sq_type="4bit"),
    dict(_spec(L2, 16, scan_group_sq8=1), sq_type="6bit"),
    dict(_spec(L2, 16, scan_group_sq8=1), type="ivfpq", m=4),
    dict(_spec(L2, 16, scan_group_sq8=1), type="ivf_flat"),
    {"type": "flat", "dim": 16, "metric": IP, "scan_group_sq8": 1},
], ids=lambda s: f"{s['type']}-{s.get('sq_type')}-{s['scan_group_sq8']}")
def test_create_refuses(spec):
    with pytest.raises(RuntimeError, match="scan_group_sq8"):
        HipEngine(spec=spec)
