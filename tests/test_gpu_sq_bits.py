# 4- and 6-bit scalar quantizers (spec "sq_type": "4bit" | "6bit";
# DESIGN.md §6h) on the GPU, against the CPU oracle (oracle.OracleIVFSQ at
# qtype "4bit" / "6bit"). Trained artifacts are injected with set_trained and
# the restatement scans the lists the engine dumps (get_lists), so the
# coarse GEMM's tolerance tier cannot move a row between lists: every
# comparison in this file is bitwise.
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
from gpu_support import assert_bitwise, engine_with  # noqa: E402
from oracle import (  # noqa: E402
    from_engine_artifacts,
    pack_sq,
    range_from_scans,
    ranking,
    scan_lists,
    sq_code_bytes,
    sq_stride,
)
from oracle.refine import (  # noqa: E402
    refine_ref,
)

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
BITS = [pytest.param(4, id="sq4"), pytest.param(6, id="sq6")]
NLIST, NQ, NPROBE, K = 16, 32, 4, 10
# the smallest dimensions that reach each code path of the scan
DIMS = [
    pytest.param(128, id="d128-one_chunk-8_full_lanes"),
    pytest.param(40, id="d40-lanes_0_to_2-sq6_chunk_past_stride"),
    pytest.param(7, id="d7-odd-trailing_nibble-partial_group"),
    pytest.param(200, id="d200-two_chunks-ragged_tail"),
    pytest.param(768, id="d768-six_chunks_per_lane"),
]


def _spec(d, metric, bits, **kw):
    return dict({"type": "ivfsq", "dim": d, "metric": metric, "nlist": NLIST,
                 "nprobe": NPROBE, "seed": 1234, "sq_type": f"{bits}bit"}, **kw)


@functools.lru_cache(maxsize=None)
def _data(d, metric):
    """Rows around 16 centroids (some of them twins), queries likewise, and
    per-dimension ranges from the residuals to the fp64-nearest centroid."""
    n = 2000 if d == 768 else 4000
    rng = np.random.default_rng(9000 + 10 * d + metric)
    cent = (rng.standard_normal((NLIST, d)) * 2.0).astype(np.float32)
    xb = (cent[rng.integers(0, NLIST, n)]
          + rng.standard_normal((n, d))).astype(np.float32)
    # a tenth of the rows are twins (same bytes, other id): exact distance
    # ties, inside and across the top-k
    xb[n - n // 20:] = xb[:n // 20]
    q = (cent[rng.integers(0, NLIST, NQ)]
         + 0.7 * rng.standard_normal((NQ, d))).astype(np.float32)
    x64, c64 = xb.astype(np.float64), cent.astype(np.float64)
    dots = x64 @ c64.T
    key = -dots if metric == IP else (c64 ** 2).sum(-1)[None, :] - 2.0 * dots
    r = xb - cent[key.argmin(axis=1)]
    vmin = r.min(axis=0).astype(np.float32)
    vdiff = (r.max(axis=0) - vmin).astype(np.float32)
    assert (vdiff > 0).all()
    for a in (cent, xb, q, vmin, vdiff):
        a.setflags(write=False)
    return cent, xb, q, vmin, vdiff


def _engine(d, metric, bits, **kw):
    cent, xb, _q, vmin, vdiff = _data(d, metric)
    return engine_with(_spec(d, metric, bits, **kw), cent, None, vmin, vdiff,
                       xb, split=xb.shape[0] // 2 + 37)


def _oracle(d, metric, bits, eng):
    cent, _xb, _q, vmin, vdiff = _data(d, metric)
    return from_engine_artifacts(_spec(d, metric, bits), cent, vmin=vmin,
                                 vdiff=vdiff, lists=eng.get_lists())


@functools.lru_cache(maxsize=None)
def _case(d, metric, bits):
    """Engine, restatement over the engine's own lists, the engine's coarse
    probes, and the restatement's scan of every probed list (computed once,
    shared read-only by every test of the case)."""
    eng = _engine(d, metric, bits)
    orc = _oracle(d, metric, bits, eng)
    q = _data(d, metric)[2]
    probes, keys = eng.coarse(q, NPROBE)
    scans = scan_lists(orc, q, probes, keys)
    rank = ranking(scans, metric)
    for dd, ii in rank:
        assert dd.shape[0] >= 64  # every query has far more than k rows
        dd.setflags(write=False)
        ii.setflags(write=False)
    return {"eng": eng, "orc": orc, "q": q, "probes": probes, "keys": keys,
            "scans": scans, "rank": rank, "n": _data(d, metric)[1].shape[0]}


def _expect_topk(case, k, allow=None):
    D = np.empty((NQ, k), np.float32)
    I = np.empty((NQ, k), np.int64)
    for i, (dd, ii) in enumerate(case["rank"]):
        if allow is not None:
            keep = allow[ii]
            dd, ii = dd[keep], ii[keep]
        assert dd.shape[0] >= k
        D[i], I[i] = dd[:k], ii[:k]
    return D, I


# ---------------------------------------------------------------------------
# 1. scan
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("d", DIMS)
def test_scan_bitexact(d, bits, metric):
    case = _case(d, metric, bits)
    D, I = case["eng"].search_preassigned(case["q"], case["probes"],
                                          case["keys"], K)
    assert_bitwise(D, I, *_expect_topk(case, K))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
def test_selection_switch(bits, metric):
    # k = 16 is the last register-selection k, 17 the first LDS-selection k
    case = _case(128, metric, bits)
    for k in (16, 17, 1):
        D, I = case["eng"].search_preassigned(case["q"], case["probes"],
                                              case["keys"], k)
        assert_bitwise(D, I, *_expect_topk(case, k))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
def test_search_equals_preassigned(bits, metric):
    case = _case(40, metric, bits)
    for k in (K, 17):
        D, I = case["eng"].search(case["q"], k)
        assert_bitwise(D, I, *_expect_topk(case, k))


def test_results_carry_exact_ties():
    # twin rows give equal sums: the (distance, ascending id) rule is
    # exercised inside the top-k, not satisfied vacuously
    case = _case(7, L2, 4)
    D, I = case["eng"].search_preassigned(case["q"], case["probes"],
                                          case["keys"], 17)
    ties = D[:, 1:] == D[:, :-1]
    assert ties.sum() > 0
    assert (I[:, 1:][ties] > I[:, :-1][ties]).all()


# ---------------------------------------------------------------------------
# 2. stored bytes
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("d", [7, 40, 128])
def test_stored_rows_are_the_restatements_encode(d, bits, metric):
    case = _case(d, metric, bits)
    cent, xb = _data(d, metric)[:2]
    off, ids, codes = case["eng"].get_lists()
    n = case["n"]
    assert off[-1] == n and np.array_equal(np.sort(ids), np.arange(n))
    assert codes.shape == (n, sq_stride(d, bits))
    lst = np.repeat(np.arange(NLIST), np.diff(off))
    resid = xb[ids] - cent[lst]  # fp32, the engine's own subtraction
    want = pack_sq(case["orc"]._encode_resid(resid), bits)
    cb = sq_code_bytes(d, bits)
    assert want.shape == (n, cb)
    np.testing.assert_array_equal(codes[:, :cb], want)
    # every bit past d * bits is zero: the tail of the last code byte and
    # the pad bytes up to the stride
    assert not codes[:, cb:].any()
    tail = 8 * cb - d * bits
    if tail:
        assert (codes[:, cb - 1] >> (8 - tail) == 0).all()
    # not vacuous: the codes span the whole range, both ends included
    used = np.unique(case["orc"]._encode_resid(resid))
    assert used[0] == 0 and used[-1] == (1 << bits) - 1
    assert used.size > (1 << bits) // 2


# ---------------------------------------------------------------------------
# 3. filtered search, range search
# ---------------------------------------------------------------------------


def _allow10(case):
    return np.random.default_rng(5).uniform(size=case["n"]) < 0.1


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("d", [40, 200])
def test_filtered_bitexact(d, bits, metric):
    case = _case(d, metric, bits)
    allow = _allow10(case)
    assert 0.07 * case["n"] < allow.sum() < 0.13 * case["n"]
    for k in (K, 17):
        D, I = case["eng"].search_preassigned_filtered(
            case["q"], case["probes"], case["keys"], k, allow)
        assert_bitwise(D, I, *_expect_topk(case, k, allow))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
def test_filtered_single_bit(bits, metric):
    case = _case(128, metric, bits)
    # the best row of query 0: probed by it, so it is that query's only hit
    dd, ii = case["rank"][0]
    allow = np.zeros(case["n"], bool)
    allow[ii[0]] = True
    D, I = case["eng"].search_preassigned_filtered(
        case["q"], case["probes"], case["keys"], K, allow)
    assert I[0, 0] == ii[0] and (I[0, 1:] == -1).all()
    assert D[0, 0].view(np.uint32) == dd[0].view(np.uint32)
    for i in range(NQ):  # every other query: that row if probed, else none
        probed = ii[0] in case["rank"][i][1]
        assert (I[i] >= 0).sum() == int(probed)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("d", [40, 200])
def test_range_search_bitexact(d, bits, metric):
    case = _case(d, metric, bits)
    kth = np.array([dd[K - 1] for dd, _ii in case["rank"]])
    radius = float(np.float32(np.median(kth)))
    for allow in (None, _allow10(case)):
        lims_o, Do, Io = range_from_scans(case["scans"], metric, radius, allow)
        assert 0 < lims_o[-1] < 100 * NQ
        lims, D, I = case["eng"].range_search_preassigned(
            case["q"], case["probes"], case["keys"], radius, allow)
        np.testing.assert_array_equal(lims, lims_o)
        assert_bitwise(D, I, Do, Io)
    # the distances are bitwise those `search` gives the same rows
    Ds, Is = case["eng"].search_preassigned(case["q"], case["probes"],
                                            case["keys"], 17)
    lims, D, I = case["eng"].range_search_preassigned(
        case["q"], case["probes"], case["keys"], radius)
    seen = 0
    for i in range(NQ):
        got = dict(zip(I[lims[i]:lims[i + 1]].tolist(),
                       D[lims[i]:lims[i + 1]].view(np.uint32).tolist()))
        for dv, iv in zip(Ds[i].view(np.uint32).tolist(), Is[i].tolist()):
            if iv in got:
                assert got[iv] == dv
                seen += 1
    assert seen > NQ


# ---------------------------------------------------------------------------
# 4. reconstruct, refine on top
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("d", [7, 128])
def test_reconstruct_bitexact(d, bits):
    case = _case(d, L2, bits)
    D, I, R = case["eng"].search_and_reconstruct(case["q"], K)
    assert (I >= 0).all()
    assert_bitwise(D, I, *_expect_topk(case, K))
    # centroid + (vmin + (c + 0.5) * scale), scale = vdiff / Q in fp32
    np.testing.assert_array_equal(
        R.view(np.uint32), case["orc"].decode_ids(I).view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", BITS)
def test_refine_on_top_bitexact(bits, metric):
    d, kf = 40, 4
    case = _case(d, metric, bits)
    eng = _engine(d, metric, bits, refine="fp32", k_factor=kf)
    D, I = eng.search(case["q"], K)
    _Do, Io = _expect_topk(case, K * kf)  # the base stage runs at k' = 40
    Dr, Ir = refine_ref(case["q"], _data(d, metric)[1], Io, K, metric)
    assert_bitwise(D, I, Dr, Ir)


# ---------------------------------------------------------------------------
# 5. persistence
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
def test_save_load_round_trip(bits, tmp_path):
    d = 40
    case = _case(d, L2, bits)
    eng = case["eng"]
    p1, p2 = str(tmp_path / "a.dfann"), str(tmp_path / "b.dfann")
    eng.save(p1)
    eng.save(p2)
    with open(p1, "rb") as f1, open(p2, "rb") as f2:
        assert f1.read() == f2.read()
    eng2 = HipProvider().load(p1)
    assert eng2.spec["sq_type"] == f"{bits}bit" and eng2.ntotal == case["n"]
    for a, b in zip(eng2.get_lists(), eng.get_lists()):
        np.testing.assert_array_equal(a, b)
    vmin, vdiff = _data(d, L2)[3:]
    for got, want in zip(eng2.get_sq_params(), (vmin, vdiff)):
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    for got, want in zip(eng.get_sq_params(), (vmin, vdiff)):
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    for k in (K, 17):
        D, I = eng2.search_preassigned(case["q"], case["probes"],
                                       case["keys"], k)
        assert_bitwise(D, I, *_expect_topk(case, k))
    R2 = eng2.search_and_reconstruct(case["q"], K)[2]
    R1 = eng.search_and_reconstruct(case["q"], K)[2]
    np.testing.assert_array_equal(R2.view(np.uint32), R1.view(np.uint32))


# ---------------------------------------------------------------------------
# 6. training
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _trained_engines():
    """SQ8, SQ6 and SQ4 engines trained on one Gaussian set with one seed,
    the set added to each."""
    n, d = 3000, 24
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, d), dtype=np.float32)
    engs = {}
    for bits in (8, 6, 4):
        eng = HipEngine(spec={"type": "ivfsq", "dim": d, "metric": L2,
                              "nlist": 8, "nprobe": 8, "seed": 99,
                              "sq_type": f"{bits}bit"})
        eng.train(x)
        eng.add(x)
        engs[bits] = eng
    return x, engs


@pytest.mark.parametrize("bits", BITS)
def test_trained_ranges_equal_sq8s(bits):
    x, engs = _trained_engines()
    np.testing.assert_array_equal(engs[bits].get_centroids(),
                                  engs[8].get_centroids())
    vmin8, vdiff8 = engs[8].get_sq_params()
    vmin, vdiff = engs[bits].get_sq_params()
    np.testing.assert_array_equal(vmin.view(np.uint32), vmin8.view(np.uint32))
    np.testing.assert_array_equal(vdiff.view(np.uint32), vdiff8.view(np.uint32))
    assert (vdiff > 0).all()
    # scale = vdiff / Q in fp32: the restatement, given the engine's ranges
    # and lists, reconstructs and scans to the same bits
    eng = engs[bits]
    orc = from_engine_artifacts(eng.spec, eng.get_centroids(), vmin=vmin,
                                vdiff=vdiff, lists=eng.get_lists())
    q = x[:16]
    D, I, R = eng.search_and_reconstruct(q, K)
    np.testing.assert_array_equal(R.view(np.uint32),
                                  orc.decode_ids(I).view(np.uint32))
    probes, keys = eng.coarse(q, 8)
    Do, Io = orc.search_preassigned(q, probes, keys, K)
    assert_bitwise(D, I, Do, Io)


def test_reconstruction_error_orders_by_width():
    # each row against itself: the error of the returned row's decode
    # follows the step size vdiff / Q (same ranges at all three widths)
    x, engs = _trained_engines()
    q = x[:512]
    mse = {}
    for bits, eng in engs.items():
        _D, I, R = eng.search_and_reconstruct(q, 1)
        assert (I >= 0).all()
        err = R[:, 0, :].astype(np.float64) - x[I[:, 0]].astype(np.float64)
        mse[bits] = float((err ** 2).mean())
    print("reconstruction mse", mse)
    assert mse[4] > mse[6] > mse[8] > 0.0
