# Range search on the GPU against the numpy restatement
# oracle/range.py: (lims, D, I) of every row of the probed lists whose
# distance passes the strict radius test, in probe-slot then arrival-id
# order.
#
#  * bit-exact tier (np.array_equal on lims, D and I): PQ8 in-kernel / GLUT
#    f32 / GLUT f16, the 512-thread block, a partial code word, PQ4, SQ8,
#    SQfp16 — with, per query, radii taken from the oracle's full ranking;
#  * tolerance tier (IVF-Flat, PQ8 pq_precomputed): the radius sits in a gap
#    of the fp64 ranking, ids exact, distances within 1e-4 |ref| + 1e-4.
#    The seeds below were checked on the CPU: every one of the 8 queries of
#    every tolerance case has such a gap (the test fails if one has none);
#  * filters, the top-k prefix property, duplicate probes, scan_fan, OPQ,
#    determinism, errors, Index / IndexClient.
#
# Layout: the 12 lists of tests/test_gpu_dispatch_parity.py, resized to hold
# lists shorter than a block's wave count (0, 1, 3, 7), the 4-row and 8-row
# tails (7, 8, 9), the wave boundary (63, 64, 65) and more than one
# iteration of a 512-thread block (515); rows arrive shuffled in two adds.
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from gpu_support import (  # noqa: E402
    codeword_rows,
    decode_rows,
    engine_with,
    ivf_spec,
    labels,
    queries,
    wait_trained,
)

from distributed_faiss_amd.client import IndexClient  # noqa: E402
from distributed_faiss_amd.hip_engine import HipEngine, HipProvider  # noqa: E402
from distributed_faiss_amd.index_cfg import IndexCfg  # noqa: E402
from distributed_faiss_amd.server import IndexServer  # noqa: E402
from oracle import (  # noqa: E402
    from_engine_artifacts,
    range_from_scans,
    range_search_ref,
    ranking,
    scan_lists,
)
from oracle.opq import signed_selection  # noqa: E402

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
FLT_MAX = np.float32(3.4028235e38)

LIST_SIZES = [0, 1, 3, 7, 8, 9, 63, 64, 65, 127, 257, 515]
NLIST = len(LIST_SIZES)
NROWS = sum(LIST_SIZES)  # 1119
SPLIT = 700
NQ = 8
RANK = 30
CODEWORD_GAP = 0.05


def _labels(rng):
    return labels(rng, LIST_SIZES)


def _queries(rng, cent, d, metric):
    return queries(rng, cent, NQ, metric)


def _spec(typ, d, metric, **kw):
    return ivf_spec(typ, d, metric, NLIST, **kw)


# ---------------------------------------------------------------------------
# cases: data + oracle, built once per key; the oracle's per-list scans
# (radius-independent) are computed once per case and shared
# ---------------------------------------------------------------------------

_CASES = {}


def _pq_case(m, dsub, metric, nbits=8, f16=False, small=False):
    """small: centroids of spread 1.5 and codewords of spread 0.1 instead
    of 20 (5 under f16) and 1 — the pq_precomputed case, see there."""
    ksub = 1 << nbits
    d = m * dsub
    rng = np.random.default_rng(7000 + 1000 * m + dsub + nbits)
    cent = (rng.standard_normal((NLIST, d))
            * (1.5 if small else 5.0 if f16 else 20.0)).astype(np.float32)
    cb = (rng.standard_normal((m, ksub, dsub))
          * (0.1 if small else 1.0)).astype(np.float32)
    lbl = _labels(rng)
    # a quarter of each list repeats another row's codes: exact ties
    cw = codeword_rows(rng, cb, lbl,
                       CODEWORD_GAP * (0.1 if small else 1.0), 8)
    xb = (cent[lbl] + decode_rows(cb, cw) + (1e-4 if small else 1e-3)
          * rng.standard_normal((NROWS, d))).astype(np.float32)
    q = _queries(rng, cent, d, metric)
    spec = _spec("ivfpq", d, metric, m=m, nbits=nbits,
                 pq_lut_f16=1 if f16 else 0)
    orc = from_engine_artifacts(spec, cent, cb)
    orc.add(xb)
    # CPU condition: the oracle encoded the intended codewords
    np.testing.assert_array_equal(
        np.concatenate(orc.list_codes),
        np.concatenate([cw[lbl == l] for l in range(NLIST)]).astype(np.uint8))
    return {"spec": spec, "cent": cent, "cb": cb, "xb": xb, "q": q,
            "orc": orc, "metric": metric}


def _sq_case(d, metric, sq8):
    rng = np.random.default_rng(8000 + d + (1 if sq8 else 0))
    cent = (rng.standard_normal((NLIST, d)) * 20.0).astype(np.float32)
    lbl = _labels(rng)
    vmin = vdiff = None
    if sq8:
        vmin = rng.uniform(-3.0, -1.0, d).astype(np.float32)
        vdiff = rng.uniform(2.0, 6.0, d).astype(np.float32)
        c = rng.integers(0, 256, (NROWS, d))
        jit = rng.uniform(-0.1, 0.1, (NROWS, d))
        resid = vmin + (c + 0.5 + jit) * (vdiff.astype(np.float64) / 255)
    else:
        resid = (10.0 ** rng.uniform(-3.0, 1.0, (NROWS, d))
                 * rng.choice([-1.0, 1.0], (NROWS, d)))
    xb = (cent[lbl] + resid).astype(np.float32)
    q = _queries(rng, cent, d, metric)
    spec = _spec("ivfsq", d, metric, sq_type="8bit" if sq8 else "fp16")
    orc = from_engine_artifacts(spec, cent, vmin=vmin, vdiff=vdiff)
    orc.add(xb)
    if sq8:  # CPU condition: the oracle's codes are the intended ones
        want = np.concatenate([c[lbl == l] for l in range(NLIST)])
        np.testing.assert_array_equal(np.concatenate(orc.list_codes),
                                      want.astype(np.uint8))
    return {"spec": spec, "cent": cent, "cb": None, "vmin": vmin,
            "vdiff": vdiff, "xb": xb, "q": q, "orc": orc, "metric": metric}


def _flat_case(d, metric):
    rng = np.random.default_rng(FLAT_SEED + d)
    cent = (rng.standard_normal((NLIST, d)) * 1.5).astype(np.float32)
    lbl = _labels(rng)
    xb = (cent[lbl] + 0.5 * rng.standard_normal((NROWS, d))).astype(np.float32)
    q = _queries(rng, cent, d, L2)
    spec = _spec("ivf_flat", d, metric)
    orc = from_engine_artifacts(spec, cent)
    orc.add(xb)
    return {"spec": spec, "cent": cent, "cb": None, "xb": xb, "q": q,
            "orc": orc, "metric": metric}


FLAT_SEED = 9000


def _case(kind, *args):
    key = (kind,) + args
    if key not in _CASES:
        build = {"pq": _pq_case, "sq": _sq_case, "flat": _flat_case}[kind]
        c = build(*args)
        np.testing.assert_array_equal([len(i) for i in c["orc"].list_ids],
                                      LIST_SIZES)
        c["ref"] = None
        _CASES[key] = c
    return _CASES[key]


def _engine(case, **knobs):
    return engine_with(dict(case["spec"], **knobs), case["cent"], case["cb"],
                       case.get("vmin"), case.get("vdiff"), case["xb"], SPLIT)


def _ref(case, eng):
    """(probes, keys, scans, ranking): the engine's coarse output, which
    must not change between engines of a case, and the oracle's scans of
    it, computed once and left unchanged."""
    probes, keys = eng.coarse(case["q"], NLIST)
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    if case["ref"] is None:
        scans = scan_lists(case["orc"], case["q"], probes, keys)
        case["ref"] = (probes.copy(), keys.copy(), scans,
                       ranking(scans, case["metric"]))
    np.testing.assert_array_equal(case["ref"][0], probes)
    np.testing.assert_array_equal(case["ref"][1], keys)
    return case["ref"]


def _assert_same(got, want):
    for g, w, name in zip(got, want, ("lims", "D", "I")):
        assert g.dtype == w.dtype, name
        assert np.array_equal(g.view(np.uint32) if name == "D" else g,
                              w.view(np.uint32) if name == "D" else w), name


def _mid_radius(vals, rank=RANK):
    """Midpoint between two distinct neighbouring values at rank ~ `rank`
    of a best-first ranking."""
    j = rank
    while vals[j] == vals[j + 1]:
        j += 1
    return np.float32((np.float64(vals[j]) + np.float64(vals[j + 1])) / 2)


def _check_radii(eng, case):
    metric = case["metric"]
    probes, keys, scans, rank = _ref(case, eng)
    q = case["q"]

    def run(r):
        return eng.range_search_preassigned(q, probes, keys, r)

    for i in range(NQ):
        vals, ids = rank[i]
        # 1. a midpoint radius
        r = _mid_radius(vals)
        _assert_same(run(r), range_from_scans(scans, metric, r))
        # 2. exactly the rank-30 value: that row and its ties are dropped
        r = vals[RANK]
        lims, D, I = run(r)
        _assert_same((lims, D, I),
                     range_from_scans(scans, metric, r))
        better = (vals < r) if metric == L2 else (vals > r)
        assert lims[i + 1] - lims[i] == better.sum() <= RANK
        assert ids[RANK] not in I[lims[i]:lims[i + 1]]
    # 3. excluding radius: nothing passes
    top = max(float(v[0][0]) for v in rank)
    r = np.float32(0.0) if metric == L2 else np.nextafter(
        np.float32(top), np.float32(np.inf))
    lims, D, I = run(r)
    assert np.array_equal(lims, np.zeros(NQ + 1, np.int64))
    assert D.shape == (0,) and I.shape == (0,)
    assert D.dtype == np.float32 and I.dtype == np.int64
    # 4. including radius: every row of the probed lists
    r = FLT_MAX if metric == L2 else -FLT_MAX
    lims, D, I = run(r)
    _assert_same((lims, D, I), range_from_scans(scans, metric, r))
    assert np.array_equal(np.diff(lims), np.full(NQ, NROWS))


# ---------------------------------------------------------------------------
# bit-exact tier
# ---------------------------------------------------------------------------

PQ_CASES = [
    pytest.param(16, 8, 8, {"pq_lut_global": 0}, id="pq8-m16-dsub8-inkernel"),
    pytest.param(16, 8, 8, {"pq_lut_global": 1}, id="pq8-m16-dsub8-glut_f32"),
    pytest.param(16, 8, 8, {"pq_lut_f16": 1}, id="pq8-m16-dsub8-glut_f16"),
    # ws_mb 1: two queries per LUT chunk, four chunks per pass
    pytest.param(32, 4, 8, {"pq_lut_global": 1, "ws_mb": 1},
                 id="pq8-m32-dsub4-glut_f32-4_lut_chunks"),
    pytest.param(64, 2, 8, {"pq_lut_global": 0}, id="pq8-m64-dsub2-block512"),
    pytest.param(20, 3, 8, {}, id="pq8-m20-dsub3-partial_word"),
    pytest.param(16, 4, 4, {}, id="pq4-m16"),
    pytest.param(7, 3, 4, {}, id="pq4-m7-odd"),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m,dsub,nbits,knobs", PQ_CASES)
def test_pq_range_bitexact(m, dsub, nbits, knobs, metric):
    case = _case("pq", m, dsub, metric, nbits, bool(knobs.get("pq_lut_f16")))
    _check_radii(_engine(case, **knobs), case)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [20, 128, 200])
def test_sq8_range_bitexact(d, metric):
    case = _case("sq", d, metric, True)
    _check_radii(_engine(case), case)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [20, 128])
def test_sqfp16_range_bitexact(d, metric):
    case = _case("sq", d, metric, False)
    _check_radii(_engine(case), case)


# ---------------------------------------------------------------------------
# tolerance tier: the radius sits in a gap of the fp64 ranking
# ---------------------------------------------------------------------------

GAP_REL = 1e-3


def _gap_radius(ref):
    """Midpoint of the first gap of the fp64 best-first ranking between
    ranks 5 and 60 that is at least GAP_REL relative; None if there is
    none."""
    for j in range(5, 60):
        a, b = ref[j], ref[j + 1]
        if abs(b - a) >= GAP_REL * max(abs(a), abs(b)):
            return (a + b) / 2
    return None


def _check_tolerance(eng, case, ref_of_id):
    """ref_of_id: (NQ, NROWS) fp64 reference value of every arrival id."""
    metric = case["metric"]
    probes, keys = eng.coarse(case["q"], NLIST)
    lists = case["orc"].list_ids
    for i in range(NQ):
        ref = ref_of_id[i]
        order = np.argsort(ref if metric == L2 else -ref, kind="stable")
        r = _gap_radius(ref[order])
        assert r is not None, f"query {i}: no {GAP_REL} gap in ranks 5..60"
        lims, D, I = eng.range_search_preassigned(
            case["q"], probes, keys, np.float32(r))
        hit = ref < r if metric == L2 else ref > r
        want = np.concatenate([lists[int(l)][hit[lists[int(l)]]]
                               for l in probes[i]])
        got = I[lims[i]:lims[i + 1]]
        assert 5 < want.size <= 60
        assert np.array_equal(got, want), i
        err = np.abs(D[lims[i]:lims[i + 1]].astype(np.float64) - ref[got])
        assert (err <= 1e-4 * np.abs(ref[got]) + 1e-4).all(), (i, err.max())


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [20, 100])
def test_ivfflat_range_tolerance(d, metric):
    case = _case("flat", d, metric)
    q64, x64 = case["q"].astype(np.float64), case["xb"].astype(np.float64)
    if metric == L2:
        ref = ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
    else:
        ref = q64 @ x64.T
    _check_tolerance(_engine(case), case, ref)


def test_pq_precomputed_range_tolerance():
    # The precomputed-table form ||q||^2 + (|c|^2 - 2 q.c) + sum(term2 -
    # 2 term3) cancels terms of magnitude ||q||^2 + ||c||^2, so its error
    # is ~ eps * that magnitude whatever the scan does (the faiss caveat;
    # tests/test_gpu_parity.py keeps ||c|| moderate for the same reason).
    # With spread-20 centroids that is 2^-24 * 1e5 ~ 1e-2 on distances of
    # ~ 150, above the tier's bound; this case keeps the magnitudes at
    # ~ 600, i.e. an error ~ 1e-4 against a bound of ~ 1e-2.
    m, dsub = 16, 8
    case = _case("pq", m, dsub, L2, 8, False, True)
    orc = case["orc"]
    ref = np.empty((NQ, NROWS))
    cb64 = case["cb"].astype(np.float64)
    for l in range(NLIST):
        codes = orc.list_codes[l]
        if codes.shape[0] == 0:
            continue
        dec = np.concatenate([cb64[j][codes[:, j]] for j in range(m)], axis=1)
        y = case["cent"][l].astype(np.float64) + dec
        ref[:, orc.list_ids[l]] = (
            (case["q"].astype(np.float64)[:, None, :] - y[None]) ** 2).sum(-1)
    _check_tolerance(_engine(case, pq_precomputed=1), case, ref)


# ---------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------


def _allow(name, orc):
    """bool mask over ids padded to whole words with the bits >= ntotal SET
    (they must be ignored): the masks of tests/test_gpu_filtered.py."""
    ids = np.arange(NROWS)
    if name == "NONE":
        a = np.zeros(NROWS, bool)
    elif name == "MOD3":
        a = ids % 3 != 0
    else:  # NOLIST
        a = np.ones(NROWS, bool)
        a[orc.list_ids[9]] = False
    out = np.ones((NROWS + 31) // 32 * 32, bool)
    out[:NROWS] = a
    assert out.shape[0] > NROWS
    return out


@pytest.mark.parametrize("filt", ["MOD3", "NONE", "NOLIST"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["pq8", "sq8"])
def test_filtered_range_bitexact(kind, metric, filt):
    case = (_case("pq", 16, 8, metric, 8, False) if kind == "pq8"
            else _case("sq", 128, metric, True))
    eng = _engine(case)
    probes, keys, scans, rank = _ref(case, eng)
    allow = _allow(filt, case["orc"])
    for r in (_mid_radius(rank[0][0], 200),
              FLT_MAX if metric == L2 else -FLT_MAX):
        want = range_from_scans(scans, metric, r, allow[:NROWS])
        _assert_same(eng.range_search_preassigned(
            case["q"], probes, keys, r, allow), want)
        if filt == "NONE":
            assert want[0][-1] == 0
        else:
            assert 0 < want[0][-1] <= range_from_scans(
                scans, metric, r)[0][-1]
    # under the including radius the mask alone decides: it does bite
    if filt != "NONE":
        assert want[0][-1] == NQ * int(allow[:NROWS].sum()) < NQ * NROWS
    # the coarse-selecting entry probes the same lists (nprobe = nlist)
    _assert_same(eng.range_search(case["q"], r, allow), want)


# ---------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["pq8", "sq8"])
def test_prefix_is_the_topk(kind, metric):
    # the best min(k, n_i) rows of a range result are search's top-k, bitwise
    case = (_case("pq", 16, 8, metric, 8, False) if kind == "pq8"
            else _case("sq", 128, metric, True))
    eng = _engine(case)
    probes, keys, _scans, rank = _ref(case, eng)
    k = 10
    Dk, Ik = eng.search_preassigned(case["q"], probes, keys, k)
    for i in range(NQ):
        r = _mid_radius(rank[i][0])
        lims, D, I = eng.range_search_preassigned(case["q"], probes, keys, r)
        d, ids = D[lims[i]:lims[i + 1]], I[lims[i]:lims[i + 1]]
        order = np.lexsort((ids, d if metric == L2 else -d))[:k]
        n = order.size
        assert n == min(k, d.size) and n > 0
        assert np.array_equal(ids[order], Ik[i, :n])
        assert np.array_equal(d[order].view(np.uint32),
                              Dk[i, :n].view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
def test_duplicate_probe_list_contributes_twice(metric):
    case = _case("pq", 16, 8, metric, 8, False)
    eng = _engine(case)
    probes, keys, _scans, rank = _ref(case, eng)
    # slots: the 515-row list, the 65-row list, the 515-row list again
    pr = np.stack([[11, 8, 11]] * NQ).astype(np.int32)
    ke = np.stack([[keys[i, int(np.flatnonzero(probes[i] == l)[0])]
                    for l in (11, 8, 11)] for i in range(NQ)]
                  ).astype(np.float32)
    r = FLT_MAX if metric == L2 else -FLT_MAX
    lims, D, I = eng.range_search_preassigned(case["q"], pr, ke, r)
    _assert_same((lims, D, I),
                 range_search_ref(case["orc"], case["q"], pr, ke, r))
    assert np.array_equal(np.diff(lims), np.full(NQ, 515 + 65 + 515))
    for i in range(NQ):
        seg = slice(lims[i], lims[i + 1])
        assert np.array_equal(I[seg][:515], I[seg][580:])
        assert np.array_equal(D[seg][:515].view(np.uint32),
                              D[seg][580:].view(np.uint32))
        assert (np.diff(I[seg][:515]) > 0).all()


@pytest.mark.parametrize("metric", METRICS)
def test_scan_fan_is_ignored_in_range_mode(metric):
    case = _case("sq", 128, metric, True)
    e1, e4 = _engine(case, scan_fan=1), _engine(case, scan_fan=4)
    probes, keys, scans, rank = _ref(case, e1)
    for r in (_mid_radius(rank[0][0], 200),
              FLT_MAX if metric == L2 else -FLT_MAX):
        a = e1.range_search_preassigned(case["q"], probes, keys, r)
        _assert_same(e4.range_search_preassigned(case["q"], probes, keys, r), a)
        _assert_same(a, range_from_scans(scans, metric, r))


@pytest.mark.parametrize("metric", METRICS)
def test_opq_is_the_plain_engine_behind_the_transform(metric):
    d_in, m, dsub = 48, 8, 4
    d_out = m * dsub
    case = _case("pq", m, dsub, metric, 8, False)  # data at d_out
    rng = np.random.default_rng(77)
    A = signed_selection(d_in, d_out, rng)
    # rows whose transform is exactly the case's: x = A^T y (+ junk in the
    # dropped columns)
    junk = rng.standard_normal((NROWS + NQ, d_in)).astype(np.float32)
    junk[:, np.abs(A).sum(0) > 0] = 0
    xb = case["xb"] @ A + junk[:NROWS]
    q = case["q"] @ A + junk[NROWS:]
    eng = HipEngine(spec=dict(case["spec"], dim=d_in, opq=1, opq_dim=d_out))
    eng.set_transform(A)
    eng.set_trained(case["cent"], case["cb"])
    eng.add(xb[:SPLIT])
    eng.add(xb[SPLIT:])
    np.testing.assert_array_equal(eng.apply_transform(q), case["q"])
    plain = _engine(case)
    probes, keys, scans, rank = _ref(case, plain)
    po, ko = eng.coarse(q, NLIST)
    np.testing.assert_array_equal(po, probes)
    np.testing.assert_array_equal(ko, keys)
    for r in (_mid_radius(rank[0][0], 100),
              FLT_MAX if metric == L2 else -FLT_MAX):
        want = plain.range_search_preassigned(case["q"], probes, keys, r)
        _assert_same(eng.range_search_preassigned(q, probes, keys, r), want)
        _assert_same(eng.range_search(q, r), plain.range_search(case["q"], r))
        _assert_same(want, range_from_scans(scans, metric, r))


@pytest.mark.parametrize("metric", METRICS)
def test_deterministic_and_follows_adds(metric):
    case = _case("sq", 20, metric, True)
    eng = HipEngine(spec=case["spec"])
    eng.set_trained(case["cent"], None, case["vmin"], case["vdiff"])
    eng.add(case["xb"][:SPLIT])
    orc = from_engine_artifacts(case["spec"], case["cent"],
                                vmin=case["vmin"], vdiff=case["vdiff"])
    orc.add(case["xb"][:SPLIT])
    probes, keys = eng.coarse(case["q"], NLIST)
    r = _mid_radius(_ref(case, _engine(case))[3][0][0], 100)
    a = eng.range_search_preassigned(case["q"], probes, keys, r)
    b = eng.range_search_preassigned(case["q"], probes, keys, r)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    _assert_same(a, range_search_ref(orc, case["q"], probes, keys, r))
    eng.add(case["xb"][SPLIT:])
    orc.add(case["xb"][SPLIT:])
    c = eng.range_search_preassigned(case["q"], probes, keys, r)
    _assert_same(c, range_search_ref(orc, case["q"], probes, keys, r))
    assert c[0][-1] > a[0][-1]
    # NaN radius: empty
    lims, D, I = eng.range_search(case["q"], float("nan"))
    assert not lims.any() and D.size == 0 and I.size == 0
    # no queries
    lims, D, I = eng.range_search(case["q"][:0], r)
    assert lims.tolist() == [0] and D.size == 0


# ---------------------------------------------------------------------------
# errors: each names its cause and leaves the handle usable
# ---------------------------------------------------------------------------


def test_errors():
    case = _case("sq", 20, L2, True)
    q = case["q"]
    d = 20
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((400, d)).astype(np.float32)

    flat = HipEngine(spec={"type": "flat", "dim": d, "metric": L2})
    flat.train(xb)
    flat.add(xb)
    with pytest.raises(RuntimeError, match="range search unsupported for flat"):
        flat.range_search(q, 1.0)
    assert flat.search(q, 3)[1].shape == (NQ, 3)

    hn = HipEngine(spec={"type": "hnswsq", "dim": d, "metric": L2, "m": 8,
                         "ef_construction": 40, "nprobe": 16, "seed": 1})
    hn.train(xb)
    hn.add(xb)
    with pytest.raises(RuntimeError, match="range search unsupported for hnswsq"):
        hn.range_search(q, 1.0)
    assert hn.search(q, 3)[1].shape == (NQ, 3)

    rf = HipEngine(spec=dict(case["spec"], refine="fp32"))
    rf.set_trained(case["cent"], None, case["vmin"], case["vdiff"])
    rf.add(case["xb"])
    with pytest.raises(RuntimeError, match="range search unsupported with refine"):
        rf.range_search(q, 1.0)
    assert rf.search(q, 3)[1].shape == (NQ, 3)

    un = HipEngine(spec=case["spec"])
    with pytest.raises(RuntimeError, match="range search on untrained index"):
        un.range_search(q, 1.0)
    un.set_trained(case["cent"], None, case["vmin"], case["vdiff"])
    lims, D, I = un.range_search(q, 1.0)  # trained, ntotal == 0
    assert not lims.any() and lims.shape == (NQ + 1,) and D.size == 0

    small = _engine(case, range_max_results=100)
    with pytest.raises(RuntimeError,
                       match=rf"{NQ * NROWS} results exceed range_max_results = 100"):
        small.range_search(q, float(FLT_MAX))
    probes, keys, scans, rank = _ref(case, small)
    r = _mid_radius(rank[0][0], 5)
    want = range_from_scans(scans, L2, r)
    assert 0 < want[0][-1] <= 100
    _assert_same(small.range_search(q, r), want)

    with pytest.raises(RuntimeError, match="allow bitmap covers"):
        small.range_search(q, r, np.ones(NROWS - 1, bool))
    _assert_same(small.range_search(q, r, np.ones(NROWS, bool)), want)


# ---------------------------------------------------------------------------
# Index / IndexClient over two in-process shards
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_index_and_client_two_shards(tmp_path, metric):
    d, n = 32, 1200
    rng = np.random.default_rng(11)
    cent = rng.standard_normal((8, d)) * 4
    xb = (cent[rng.integers(0, 8, 2 * n)]
          + 0.3 * rng.standard_normal((2 * n, d))).astype(np.float32)
    q = xb[::97][:6] + 0.01 * rng.standard_normal((6, d)).astype(np.float32)
    cfg = IndexCfg(faiss_factory="IVF8,SQ8", dim=d, metric=metric, nprobe=8,
                   train_num=n)
    servers = []
    for s in range(2):
        srv = IndexServer(s, str(tmp_path / f"s{s}"), provider=HipProvider())
        srv.create_index("x", cfg)
        meta = [("doc", s, i % 4) for i in range(n)]
        srv.add_index_data("x", xb[s * n:(s + 1) * n], meta,
                           train_async_if_triggered=False)
        wait_trained(srv._get_index("x"))
        servers.append(srv)
    client = IndexClient(servers=servers, distributed=False)
    client.cfg = cfg
    # a radius with a few dozen hits per query, from the first shard's top-k
    D0, _I0 = servers[0]._get_index("x").engine.search(q, 30)
    radius = float(np.median(D0[:, -1]))
    for fp, fv in ((None, None), (2, 1)):
        parts = [srv.range_search("x", q, radius, fp, fv) for srv in servers]
        lims, scores, meta = client.range_search(q, radius, "x", fp, fv)
        assert lims[0] == 0 and lims[-1] == len(scores) == len(meta) > 0
        for i in range(6):
            want_s = np.concatenate(
                [p[1][p[0][i]:p[0][i + 1]] for p in parts])
            want_m = sum((p[3][p[0][i]:p[0][i + 1]] for p in parts), [])
            assert np.array_equal(scores[lims[i]:lims[i + 1]], want_s)
            assert meta[lims[i]:lims[i + 1]] == want_m
        if metric == "dot":
            assert (scores > radius).all()  # true dot products, un-negated
        else:
            assert (scores < radius).all()
        if fp is not None:
            assert all(m[2] != 1 for m in meta)
        # Index level: scores / ids / meta against the engine
        idx = servers[0]._get_index("x")
        li, sc, ids, me = idx.range_search(q, radius, fp, fv)
        allow = None if fp is None else np.array(
            [m[2] != 1 for m in idx.id_to_metadata[:n]])
        _assert_same((li, sc, ids), idx.engine.range_search(q, radius, allow))
        assert me == [idx.id_to_metadata[j] for j in ids]
