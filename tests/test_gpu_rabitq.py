# IVF-RaBitQ on the GPU against a float64 restatement of its
# formulas over the engine's own stored bytes (get_lists) and the injected
# centroids, in the tolerance tier of DESIGN.md §4 (bounds in _ref, _check).
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

from distributed_faiss_amd.hip_engine import HipEngine, HipProvider  # noqa: E402
from gpu_support import (  # noqa: E402
    IP, L2, assert_bitwise, engine_with, ivf_spec, labels, queries)
from oracle.opq import ortho_dev, polar_svd  # noqa: E402

METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
# partial byte, partial nibble, straight-line groups, guarded groups, headline
DIMS = [20, 30, 128, 136, 768]
LIST_SIZES = [0, 1, 3, 4, 5, 8, 9, 63, 64, 65, 257, 515]
NLIST, NROWS, NQ = len(LIST_SIZES), sum(LIST_SIZES), 8


def _fb(d):
    return ((d + 7) // 8 + 3) & ~3


def _spec(d, metric, **kw):
    return ivf_spec("ivfrabitq", d, metric, NLIST, **kw)


ROWS_AS_QUERIES = [7, 300, 800, 990]


@functools.lru_cache(maxsize=None)
def _case(d, metric, signs=False, **kw):
    """Centroids of one norm on a 1/64 grid; rows c + N(0, 1), or with `signs`
    c +- a, a in {0.5, 1, 2} per row (r = x - c exact; the last four queries
    are then stored rows). Two shuffled adds."""
    rng = np.random.default_rng(9000 + d)
    g = rng.standard_normal((NLIST, d))
    cent = (np.round(g / np.linalg.norm(g, axis=1, keepdims=True)
                     * 20 * np.sqrt(d) * 64) / 64).astype(np.float32)
    lbl = labels(rng, LIST_SIZES)
    r = rng.standard_normal((NROWS, d))
    if signs:
        r = np.sign(r) * rng.choice([0.5, 1.0, 2.0], (NROWS, 1))
    xb = (cent[lbl] + r).astype(np.float32)
    q = queries(rng, cent, NQ, metric)
    if signs:
        q[4:] = xb[ROWS_AS_QUERIES]
    eng = engine_with(_spec(d, metric, **kw), cent, xb=xb, split=700)
    c = {"d": d, "metric": metric, "cent": cent, "xb": xb, "q": q, "eng": eng}
    c["off"], c["ids"], c["rows"] = eng.get_lists()
    np.testing.assert_array_equal(np.diff(c["off"]), LIST_SIZES)
    return c


@functools.lru_cache(maxsize=None)
def _ref(d, metric, signs=False):
    """(value, bound), (NQ, ntotal) float64 by id; L2 distance / dot product."""
    c = _case(d, metric, signs)
    fb, rows = _fb(d), c["rows"]
    s = 2.0 * np.unpackbits(rows[:, :fb], axis=1, bitorder="little")[:, :d] - 1
    n2 = rows[:, fb:fb + 4].copy().view(np.float32)[:, 0].astype(np.float64)
    f = rows[:, fb + 4:fb + 8].copy().view(np.float32)[:, 0].astype(np.float64)
    cl = c["cent"][np.repeat(np.arange(NLIST), LIST_SIZES)]
    val, bound = np.empty((2, NQ, NROWS))
    for i, q in enumerate(c["q"]):
        if metric == L2:
            v = (q[None, :] - cl).astype(np.float64)  # fp32 subtraction first
            qn2, av = (v * v).sum(1), np.abs(v).sum(1)
            val[i, c["ids"]] = n2 + qn2 - 2 * f * (s * v).sum(1)
            bound[i, c["ids"]] = 1e-4 * (n2 + qn2 + 2 * np.abs(f) * av) + 1e-4
        else:
            q64, c64 = q.astype(np.float64), cl.astype(np.float64)
            val[i, c["ids"]] = c64 @ q64 + f * (s @ q64)
            bound[i, c["ids"]] = 1e-4 * (np.abs(c64) @ np.abs(q64)
                                         + np.abs(f) * np.abs(q64).sum()) + 1e-4
    return val, bound


def _check(metric, D, I, k, val, bound, cand=None):
    sign = -1.0 if metric == IP else 1.0
    cand = np.ones(val.shape[1], bool) if cand is None else cand
    for i in range(D.shape[0]):
        n = min(k, int(cand.sum()))
        ids = I[i, :n]
        assert (I[i, n:] == -1).all() and len(set(ids)) == n and cand[ids].all()
        assert (np.abs(D[i, :n] - val[i, ids]) <= bound[i, ids]).all()
        assert (np.diff(sign * D[i, :n]) >= 0).all()
        kth = np.sort(sign * val[i, cand])[n - 1]
        assert (sign * val[i, ids] <= kth + 2 * bound[i].max()).all()


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_scan(d, metric, k):
    c = _case(d, metric)
    probes, keys = c["eng"].coarse(c["q"], NLIST)
    D, I = c["eng"].search_preassigned(c["q"], probes, keys, k)
    _check(metric, D, I, k, *_ref(d, metric))


@pytest.mark.parametrize("d", DIMS)
def test_encode(d):
    c = _case(d, L2)
    fb, rows = _fb(d), c["rows"]
    assert rows.shape[1] == (fb + 8 + 15) // 16 * 16
    r = c["xb"][c["ids"]] - c["cent"][np.repeat(np.arange(NLIST), LIST_SIZES)]
    bits = np.zeros((NROWS, fb), np.uint8)
    bits[:, :(d + 7) // 8] = np.packbits(r > 0, axis=1, bitorder="little")
    np.testing.assert_array_equal(rows[:, :fb], bits)
    r64 = r.astype(np.float64)
    n2, n1 = (r64 * r64).sum(1), np.abs(r64).sum(1)
    tail = rows[:, fb:fb + 8].copy().view(np.float32)
    np.testing.assert_allclose(tail[:, 0], n2, rtol=1e-5)
    np.testing.assert_allclose(tail[:, 1], n2 / n1, rtol=1e-5)
    assert not rows[:, fb + 8:].any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [30, 136])
def test_known_answers(d, metric):
    """|r_i| all equal: the estimate is exact, D is the true fp64 value."""
    c, (_est, bound) = _case(d, metric, True), _ref(d, metric, True)
    x64, q64 = c["xb"].astype(np.float64), c["q"].astype(np.float64)
    true = (((q64[:, None] - x64[None]) ** 2).sum(2) if metric == L2
            else q64 @ x64.T)
    D, I = c["eng"].search(c["q"], 10)
    _check(metric, D, I, 10, true, bound)
    if metric == L2:
        np.testing.assert_array_equal(I[4:, 0], ROWS_AS_QUERIES)
        assert (np.abs(D[4:, 0]) <= bound[np.arange(4, 8), I[4:, 0]]).all()


@pytest.mark.parametrize("metric", METRICS)
def test_filtered_removed_range(metric, tmp_path):
    c, (val, bound) = _case(136, metric), _ref(136, metric)
    rng = np.random.default_rng(5)
    allow = rng.random(NROWS) < 0.5
    D, I = c["eng"].search_filtered(c["q"], 40, allow)
    _check(metric, D, I, 40, val, bound, allow)
    probes, keys = c["eng"].coarse(c["q"], NLIST)
    assert_bitwise(*c["eng"].search(c["q"], 10),
                   *c["eng"].search_preassigned(c["q"], probes, keys, 10))
    sign = -1.0 if metric == IP else 1.0
    radius = float(np.median(val))
    lims, Dr, Ir = c["eng"].range_search(c["q"], radius)
    for i in range(NQ):
        ids, key = Ir[lims[i]:lims[i + 1]], sign * val[i]
        assert len(set(ids)) == len(ids)
        assert (np.abs(Dr[lims[i]:lims[i + 1]] - val[i, ids]) <= bound[i, ids]).all()
        assert (key[ids] < sign * radius + bound[i, ids]).all()
        assert np.isin(np.flatnonzero(key < sign * radius - bound[i]), ids).all()
    c["eng"].save(str(tmp_path / "rbq.dfann"))
    eng = HipProvider().load(str(tmp_path / "rbq.dfann"))
    np.testing.assert_array_equal(eng.get_lists()[2], c["rows"])
    assert_bitwise(*eng.search(c["q"], 40), *c["eng"].search(c["q"], 40))
    gone = rng.random(NROWS) < 0.3
    assert eng.remove_ids(gone) == gone.sum()
    D, I = eng.search(c["q"], 40)
    _check(metric, D, I, 40, val, bound, ~gone)


@pytest.mark.parametrize("metric", METRICS)
def test_reconstruct_and_refine(metric):
    c, d = _case(136, metric), 136
    D, I, R = c["eng"].search_and_reconstruct(c["q"], 10)
    fb, pos = _fb(d), np.argsort(c["ids"])[I]
    rows = c["rows"][pos]
    s = 2.0 * np.unpackbits(rows[..., :fb], axis=-1, bitorder="little")[..., :d] - 1
    tail = rows[..., fb:fb + 8].copy().view(np.float32).astype(np.float64)
    a = tail[..., 0] / (tail[..., 1] * d)
    cl = c["cent"][np.searchsorted(c["off"], pos, side="right") - 1]
    np.testing.assert_allclose(R, cl + s * a[..., None], rtol=1e-5, atol=1e-5)
    rf = _case(136, metric, refine="fp32", k_factor=4.0)
    D, I = rf["eng"].search(c["q"], 10)
    x64, q64 = c["xb"].astype(np.float64), c["q"].astype(np.float64)
    val = (((q64[:, None] - x64[None]) ** 2).sum(2) if metric == L2
           else q64 @ x64.T)
    mag = ((q64 * q64).sum(1)[:, None] + (x64 * x64).sum(1)[None]
           if metric == L2 else np.abs(q64) @ np.abs(x64.T))
    got, tol = np.take_along_axis(val, I, 1), np.take_along_axis(mag, I, 1)
    assert (np.abs(D - got) <= 1e-4 * tol + 1e-4).all()
    assert (np.diff(D, axis=1) * (-1 if metric == IP else 1) >= 0).all()
    assert all(len(set(row)) == 10 for row in I)


def test_rr_is_a_plain_index_behind_the_transform():
    d, c = 136, _case(136, L2)
    eng = HipEngine(spec=_spec(d, L2, rr=1))
    with pytest.raises(RuntimeError, match="transform first"):
        eng.set_trained(c["cent"])
    eng.train(c["xb"])
    A = eng.get_transform()
    ref = polar_svd(np.random.default_rng(1).standard_normal((d, d)))
    assert A.shape == (d, d) and ortho_dev(A) <= 8 * ortho_dev(ref.astype(np.float32))
    eng.add(c["xb"])
    plain = engine_with(_spec(d, L2), eng.get_centroids(),
                        xb=eng.apply_transform(c["xb"]))
    for a, b in zip(eng.get_lists(), plain.get_lists()):
        np.testing.assert_array_equal(a, b)
    assert_bitwise(*eng.search(c["q"], 10),
                   *plain.search(eng.apply_transform(c["q"]), 10))


@pytest.mark.parametrize("bad, key", [
    ({"type": "ivfrabitq", "dim": 2049}, "dim"),
    ({"type": "ivfpq", "m": 8, "rr": 1}, "rr"),
    ({"type": "ivfrabitq", "nbits": 4}, "nbits"),
    ({"type": "ivfrabitq", "opq": 1}, "opq"),
])
def test_create_refusals(bad, key):
    with pytest.raises(RuntimeError, match=key):
        HipEngine(spec=dict(_spec(64, L2), **bad))
    assert HipEngine(spec=_spec(2048, L2)).d == 2048
