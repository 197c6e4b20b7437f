# Large k: 512 < k <= k_max = 2048 through k_select_seg,
# from each of its four sources, against references that do not pass
# through it: the range search at the all-admitting radius sorted by numpy
# (IVF, bitwise), float64 numpy (flat, tolerance tier of §4) and a numpy
# stable sort (merge_topk, bitwise).
import ctypes
import functools

import numpy as np
import pytest
import torch

from distributed_faiss_amd.hip_engine import (HipEngine, _DevView,
                                              merge_topk_dev)
from gpu_support import IP, L2, assert_bitwise

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.402823466e+38)
DIM, N, NLIST, NPROBE, NQ = 32, 4400, 8, 4, 5
RNG = np.random.default_rng(7)
XB = RNG.standard_normal((N, DIM), dtype=np.float32)
Q = RNG.standard_normal((NQ, DIM), dtype=np.float32)
ALLOW = RNG.random(N) < 0.6
KINDS = {
    "ivf_flat": {"type": "ivf_flat"},
    "ivfpq8": {"type": "ivfpq", "m": 8, "nbits": 8},
    "ivfpq4": {"type": "ivfpq", "m": 8, "nbits": 4},
    "ivfsq8": {"type": "ivfsq", "sq_type": "8bit"},
    "ivfsq16": {"type": "ivfsq", "sq_type": "fp16"},
}


def _radius(metric):
    return float(-FLT_MAX if metric == IP else FLT_MAX)


@functools.lru_cache(maxsize=None)
def _ivf(kind, metric):
    eng = HipEngine(spec=dict(KINDS[kind], dim=DIM, metric=metric, nlist=NLIST,
                              nprobe=NPROBE, seed=1234, k_max=2048))
    eng.train(XB)
    eng.add(XB)
    return (eng,) + tuple(eng.coarse(Q, NPROBE))


def _topk_of_range(rng_out, metric, k):
    """(lims, D, I) of a range search -> (nq, k) D / I in the engine's order:
    numpy lexsort on (minimize-key, id), cut at k, faiss pads."""
    lims, Dr, Ir = rng_out
    nq = lims.shape[0] - 1
    D = np.full((nq, k), -FLT_MAX if metric == IP else FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        d, ids = Dr[lims[i]:lims[i + 1]], Ir[lims[i]:lims[i + 1]]
        o = np.lexsort((ids, -d if metric == IP else d))[:k]
        D[i, :o.size], I[i, :o.size] = d[o], ids[o]
    return D, I


@functools.lru_cache(maxsize=None)
def _ivf_ref(kind, metric, filtered):
    eng, probes, keys = _ivf(kind, metric)
    allow = ALLOW if filtered else None
    return (eng.range_search_preassigned(Q, probes, keys, _radius(metric), allow),
            _ivf_search(kind, metric, filtered, 512))


def _ivf_search(kind, metric, filtered, k):
    eng, probes, keys = _ivf(kind, metric)
    if filtered:
        return eng.search_preassigned_filtered(Q, probes, keys, k, ALLOW)
    return eng.search_preassigned(Q, probes, keys, k)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("k", [513, 1024, 2048])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_ivf_equals_sorted_range(kind, metric, k, filtered):
    rng_out, (D5, I5) = _ivf_ref(kind, metric, filtered)
    D, I = _ivf_search(kind, metric, filtered, k)
    assert_bitwise(D, I, *_topk_of_range(rng_out, metric, k))
    assert_bitwise(D[:, :512], I[:, :512], D5, I5)


def test_range_result_survives_large_k_search():
    """range_D / range_I stay the caller's until the next RANGE call: read
    through the pointers the range call returned, after a large-k search."""
    eng, _, _ = _ivf("ivfpq8", L2)
    qt = torch.as_tensor(Q).cuda()
    lims = torch.empty(NQ + 1, dtype=torch.int64, device="cuda")
    total, Dp, Ip = ctypes.c_int64(0), ctypes.c_void_p(), ctypes.c_void_p()
    assert eng.lib.dfann_range_search(
        eng.h, NQ, ctypes.c_void_p(qt.data_ptr()), ctypes.c_float(40.0), None, 0,
        ctypes.c_void_p(lims.data_ptr()), ctypes.byref(total), ctypes.byref(Dp),
        ctypes.byref(Ip), eng._stream(torch)) == 0
    n = total.value
    assert n > 0
    view = lambda: (torch.as_tensor(_DevView(Dp.value, n, "<f4"), device="cuda"),
                    torch.as_tensor(_DevView(Ip.value, n, "<i8"), device="cuda"))
    before = [t.clone() for t in view()]
    eng.search(Q, 1024)
    for a, b in zip(before, view()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# flat: tolerance tier (1e-4 |ref| + 1e-4) against float64
# ---------------------------------------------------------------------------


def _check_flat(D, I, X, q, live, metric, store):
    if store == "fp16":
        X, q = X.astype(np.float16), q.astype(np.float16)
    X64, q64 = X.astype(np.float64), q.astype(np.float64)
    ref = (q64 @ X64.T if metric == IP else
           ((q64[:, None, :] - X64[None, :, :]) ** 2).sum(-1))
    tol = 1e-4 * np.abs(ref) + 1e-4
    sign = -1.0 if metric == IP else 1.0
    for i in range(q.shape[0]):
        ids = I[i]
        assert (ids >= 0).all() and np.unique(ids).size == ids.size
        assert live[ids].all()
        assert (np.abs(D[i] - ref[i, ids]) <= tol[i, ids]).all()
        assert (np.diff(sign * D[i]) >= 0).all()
        rest = live.copy()
        rest[ids] = False
        assert (sign * ref[i, rest] + tol[i, rest] >= sign * D[i, -1]).all()


@pytest.mark.parametrize("variant", ["plain", "chunks", "removed"])
@pytest.mark.parametrize("k", [513, 2048])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("store", ["fp32", "fp16"])
def test_flat(store, metric, k, variant):
    spec = {"type": "flat", "dim": DIM, "metric": metric, "flat_store": store,
            "k_max": 2048}
    if variant == "chunks":
        spec["ws_mb"] = 1  # database chunks of 4096 rows: two of them
    eng = HipEngine(spec=spec)
    eng.add(XB)
    live = np.ones(N, bool)
    if variant == "removed":
        live[::7] = False
        assert eng.remove_ids(~live) == (~live).sum()
    D, I = eng.search(Q, k)
    assert_bitwise(D[:, :512], I[:, :512], *eng.search(Q, 512))
    _check_flat(D, I, XB, Q, live, metric, store)


# ---------------------------------------------------------------------------
# where the kernel can go wrong
# ---------------------------------------------------------------------------


def _flat(X, metric):
    eng = HipEngine(spec={"type": "flat", "dim": DIM, "metric": metric,
                          "k_max": 2048})
    eng.add(X)
    return eng


def _few(n, k):
    D, I = _flat(XB[:n], L2).search(Q, k)
    m = min(n, k)
    assert (np.sort(I[:, :m], axis=1) == np.arange(m)).all()
    assert (I[:, m:] == -1).all() and (D[:, m:] == FLT_MAX).all()
    assert (np.diff(D[:, :m], axis=1) >= 0).all()


def _triples(k=1024):
    n = 700
    D, I = _flat(np.tile(XB[:n], (3, 1)), L2).search(Q, k)
    for i in range(NQ):
        run = np.diff(D[i]) == 0
        assert (np.diff(I[i])[run] > 0).all()      # ids ascend inside a run
        assert run.sum() >= 2 * (k // 3) - 2       # the copies do tie
        got = set(I[i].tolist())                   # cut at the smallest ids
        assert all(r - n in got for r in I[i] if r >= n)


def _zero_ip(k=1024):
    D, I = _flat(XB, IP).search(np.zeros((NQ, DIM), np.float32), k)
    assert (I == np.arange(k)).all() and (D == 0).all()


def _preassigned(pick, k=1024):
    """The lists pick(lists by ascending size) for every query, searched at
    k and as the sorted range reference."""
    eng, _, _ = _ivf("ivf_flat", L2)
    by_size = np.argsort(np.diff(eng.get_lists()[0]), kind="stable")
    probes = np.tile(pick(by_size), (NQ, 1)).astype(np.int32)
    keys = np.zeros(probes.shape, np.float32)
    ref = eng.range_search_preassigned(Q, probes, keys, _radius(L2))
    assert (np.diff(ref[0]) > k).all()
    return (ref[0],) + tuple(eng.search_preassigned(Q, probes, keys, k)) \
        + _topk_of_range(ref, L2, k)


def _twice():
    _, D, I, Dr, Ir = _preassigned(lambda o: o[[-1, -1, -2, -3]])
    assert_bitwise(D, I, Dr, Ir)
    assert (np.diff(I, axis=1) == 0).any()  # both copies of a row returned


def _capacity(nlists):
    """The 7 smallest lists stay under the 4096 candidates the kernel keeps
    in LDS, all 8 (4400 rows) are swept from memory."""
    lims, D, I, Dr, Ir = _preassigned(lambda o: o[:nlists])
    assert ((np.diff(lims) > 4096) == (nlists == 8)).all()
    assert_bitwise(D, I, Dr, Ir)


def _nan_row(k=1024):
    eng, _, _ = _ivf("ivf_flat", IP)
    q = Q.copy()
    q[2] = np.nan
    D, I = eng.search(q, k)
    Dg, Ig = eng.search(Q, k)
    assert (I[2] == -1).all() and (D[2] == -FLT_MAX).all()
    keep = [0, 1, 3, 4]
    assert_bitwise(D[keep], I[keep], Dg[keep], Ig[keep])


def _budget(k=1024):
    """A candidate buffer of 3600 entries holds one query's ~2200: the batch
    of 5 is split down to single queries; a query whose lists (all 8: 4400
    rows) alone exceed the budget is refused."""
    eng, probes, keys = _ivf("ivfsq8", L2)
    small = HipEngine(spec=dict(eng.spec, range_max_results=3600))
    small.set_trained(eng.get_centroids(), None, *eng.get_sq_params())
    small.add(XB)
    assert_bitwise(*small.search_preassigned(Q, probes, keys, k),
                   *eng.search_preassigned(Q, probes, keys, k))
    allp = np.tile(np.arange(NLIST, dtype=np.int32), (NQ, 1))
    with pytest.raises(RuntimeError, match="k_max.*range_max_results = 3600"):
        small.search_preassigned(Q, allp, np.zeros(allp.shape, np.float32), k)


@pytest.mark.parametrize("case", [
    lambda: _few(600, 1024), lambda: _few(1024, 1024), _triples, _zero_ip,
    _twice, lambda: _capacity(7), lambda: _capacity(8), _nan_row, _budget,
], ids=["few", "exactly_k", "triples", "zero_ip", "list_twice", "lds_resident",
        "swept", "nan_row", "budget"])
def test_edges(case):
    case()


# ---------------------------------------------------------------------------
# merge_topk (source 4) and the spec key
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("k", [513, 2048])
@pytest.mark.parametrize("S", [2, 3])
def test_merge_topk(S, k, maximize):
    rng = np.random.default_rng(S * k)
    # few distinct values: ties across and inside shards; padded tails
    Dall = np.sort(rng.integers(-40, 40, (S, NQ, k)).astype(np.float32), axis=2)
    if maximize:
        Dall = Dall[:, :, ::-1].copy()
    Dall[:, :, k - 100:] = -FLT_MAX if maximize else FLT_MAX
    Iall = np.zeros((S, NQ, k), np.int64)
    Dout, Iout = merge_topk_dev(torch.as_tensor(Dall).cuda(),
                                torch.as_tensor(Iall).cuda(), k, maximize)
    key = (-Dall if maximize else Dall).transpose(1, 0, 2).reshape(NQ, S * k)
    o = np.argsort(key, axis=1, kind="stable")[:, :k]   # slot order = s*k + j
    slot = (o // k * NQ + np.arange(NQ)[:, None]) * k + o % k
    assert_bitwise(Dout.cpu().numpy(), Iout.cpu().numpy(),
                   np.take_along_axis(key, o, 1), slot)


@pytest.mark.parametrize("extra,k,msg", [
    ({"k_max": 511}, None, "k_max=511"),
    ({"k_max": 2049}, None, "k_max=2049"),
    ({"k_max": 1024, "refine": "fp32", "type": "ivfsq"}, None, "k_max.*refine"),
    ({"k_max": 1024, "type": "hnswsq", "metric": L2, "m": 8}, None,
     "k_max.*hnswsq"),
    ({"k_max": 2048}, 2049, "k > 2048 unsupported"),
    ({}, 513, "k > 512 unsupported"),
])
def test_spec(extra, k, msg):
    spec = dict({"type": "flat", "dim": DIM, "metric": IP, "nlist": NLIST}, **extra)
    with pytest.raises(RuntimeError, match=msg):
        eng = HipEngine(spec=spec)
        assert k is not None
        eng.add(XB[:100])
        eng.search(Q, k)
