# Non-finite input and invalid probes: a NaN / Inf in a
# query, a probe outside [0, nlist) from a caller, a non-finite or
# unassignable row in train / add. The engine must answer with pads or an
# error and must never index memory by a probe or an assignment it did not
# check.
#
# Clauses (include/dfann.h, "Hostile input"):
#   S1 a probe outside [0, nlist) is an empty slot, its key is never read;
#   S2 a query row holding a NaN returns pads (range search: no hits);
#   S3 a +-Inf row without NaN returns a well-formed result;
#   S4 the finite rows of a batch return bitwise what they return when
#      every bad row of the batch is replaced by a zero row;
#   S5 host argument checks of search_preassigned;
#   A1 train refuses a non-finite training set and stays untrained;
#   A2 add refuses a chunk with an unassignable row, all or nothing.
#
# Layout: the 12 lists of tests/test_gpu_dispatch_parity.py (empty and
# single-row lists, the 4-row, 8-row and wave tails, more than one pass of
# a 512-thread block), nprobe = nlist, artifacts injected with set_trained.
#
# References for the finite rows, called per query:
#  * bit-exact tier (PQ8 in its three LUT modes, PQ4, OPQ+PQ8, SQ fp16 / 8 /
#    6 / 4): the CPU oracle over the inverted lists the engine dumped, so the
#    comparison is about the scan alone (encode parity has its own suites);
#  * tolerance tier (flat, IVF-Flat, PQ8 + refine fp32): fp64 distances of
#    the returned ids within 1e-4 of the magnitude sum, and the k-th
#    returned distance no worse than the true k-th best by that bound;
#  * hnswsq: the engine on the zero-substituted batch (S4) only; its clean
#    behaviour is pinned bit for bit by tests/test_gpu_hnsw_build.py.
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

from distributed_faiss_amd.hip_engine import HipEngine  # noqa: E402
from oracle import (  # noqa: E402
    from_engine_artifacts,
    range_from_scans,
    scan_lists,
)

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
FLT_MAX = np.float32(3.4028235e38)
NORTH_STAR = 1e-4

LIST_SIZES = [0, 1, 2, 3, 5, 63, 64, 65, 127, 129, 257, 515]
NLIST = len(LIST_SIZES)
NROWS = sum(LIST_SIZES)  # 1231
LONG_LIST = 11
SPLIT = 700
D = 32
NQ = 8
K_REG, K_LDS = 10, 40  # register selection / LDS selection
KS = [pytest.param(K_REG, id="k10-reg"), pytest.param(K_LDS, id="k40-lds")]

# the 8 queries: finite, NaN at dim 0, finite, NaN at dim d-1, +Inf, -Inf,
# Inf and NaN mixed, finite
NAN_ROWS = [1, 3, 6]
INF_ROWS = [4, 5]
FINITE_ROWS = [0, 2, 7]
INVALID_PROBES = [-1, NLIST, np.iinfo(np.int32).min, np.iinfo(np.int32).max]


def _bad_queries(q):
    d = q.shape[1]
    qb = q.copy()
    qb[1, 0] = np.nan
    qb[3, d - 1] = np.nan
    qb[4, 2] = np.inf
    qb[5, 5] = -np.inf
    qb[6, 1] = np.inf
    qb[6, 7] = np.nan
    # CPU precondition: the bad rows are exactly the intended ones
    assert np.flatnonzero(np.isnan(qb).any(1)).tolist() == NAN_ROWS
    assert np.flatnonzero(np.isinf(qb).any(1)
                          & ~np.isnan(qb).any(1)).tolist() == INF_ROWS
    assert np.flatnonzero(np.isfinite(qb).all(1)).tolist() == FINITE_ROWS
    return qb


def _zeroed(qb):
    qz = qb.copy()
    qz[~np.isfinite(qb).all(1)] = 0.0
    return qz


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), what


def _pad_d(metric):
    return FLT_MAX if metric == L2 else -FLT_MAX


def _assert_pads(D_, I_, metric, what=""):
    assert (I_ == -1).all(), what
    assert (D_ == _pad_d(metric)).all(), what


def _assert_well_formed(D_, I_, ntotal, metric, what=""):
    """S3: valid ids first and distinct, pads last, no NaN, monotone."""
    for d, i in zip(D_, I_):
        assert not np.isnan(d).any(), what
        nv = int((i >= 0).sum())
        assert (i[:nv] >= 0).all() and (i[:nv] < ntotal).all(), what
        assert np.unique(i[:nv]).size == nv, what
        assert (i[nv:] == -1).all() and (d[nv:] == _pad_d(metric)).all(), what
        if metric == L2:
            assert (d[1:] >= d[:-1]).all(), what
        else:
            assert (d[1:] <= d[:-1]).all(), what


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

# name -> (type, spec knobs, tier); tier "exact" compares with the oracle
KINDS = {
    "flat": ("flat", {}, "fp64"),
    "ivf_flat": ("ivf_flat", {}, "fp64"),
    "pq8-inkernel": ("ivfpq", {"m": 8, "pq_lut_global": 0}, "exact"),
    "pq8-glut_f32": ("ivfpq", {"m": 8, "pq_lut_global": 1}, "exact"),
    "pq8-glut_f16": ("ivfpq", {"m": 8, "pq_lut_f16": 1}, "exact"),
    "pq4": ("ivfpq", {"m": 8, "nbits": 4}, "exact"),
    "sqfp16": ("ivfsq", {"sq_type": "fp16"}, "exact"),
    "sq8": ("ivfsq", {"sq_type": "8bit"}, "exact"),
    "sq6": ("ivfsq", {"sq_type": "6bit"}, "exact"),
    "sq6-d20": ("ivfsq", {"sq_type": "6bit"}, "exact"),  # partial byte group
    "sq4": ("ivfsq", {"sq_type": "4bit"}, "exact"),
    "hnswsq": ("hnswsq", {"m": 16, "ef_construction": 64, "nprobe": 64,
                          "seed": 11}, "self"),
    "opq-pq8": ("ivfpq", {"m": 8, "opq": 1, "pq_lut_global": 0}, "exact"),
    "pq8-refine_fp32": ("ivfpq", {"m": 8, "refine": "fp32", "k_factor": 2.0},
                        "fp64"),
}
IVF_KINDS = [k for k, v in KINDS.items() if v[0] not in ("flat", "hnswsq")]
EXACT_KINDS = [k for k, v in KINDS.items() if v[2] == "exact"]
_CASES = {}


def _case(kind, metric):
    key = (kind, metric)
    if key in _CASES:
        return _CASES[key]
    typ, knobs, tier = KINDS[kind]
    d = 20 if kind.endswith("d20") else D
    rng = np.random.default_rng(4200 + 17 * sorted(KINDS).index(kind) + metric)
    f16 = bool(knobs.get("pq_lut_f16"))
    cent = (rng.standard_normal((NLIST, d))
            * (5.0 if f16 else 20.0)).astype(np.float32)
    lbl = np.repeat(np.arange(NLIST), LIST_SIZES)
    rng.shuffle(lbl)
    y = (cent[lbl] + rng.standard_normal((NROWS, d))).astype(np.float32)
    qy = (cent[rng.integers(0, NLIST, NQ)]
          + 0.7 * rng.standard_normal((NQ, d))).astype(np.float32)
    c = {"kind": kind, "typ": typ, "tier": tier, "metric": metric, "d": d,
         "cent": cent, "lbl": lbl, "cb": None, "vmin": None, "vdiff": None,
         "A": None}
    c["spec"] = dict({"type": typ, "dim": d, "metric": metric, "nlist": NLIST,
                      "nprobe": NLIST, "seed": 1234}, **knobs)
    if typ == "hnswsq":
        del c["spec"]["nlist"]
    if typ == "ivfpq":
        m = knobs["m"]
        c["cb"] = rng.standard_normal(
            (m, 1 << knobs.get("nbits", 8), d // m)).astype(np.float32)
    if typ == "ivfsq" and knobs["sq_type"] != "fp16":
        c["vmin"] = rng.uniform(-4.5, -3.5, d).astype(np.float32)
        c["vdiff"] = rng.uniform(7.0, 9.0, d).astype(np.float32)
    if knobs.get("opq"):
        # y = A x with A orthonormal: the lists are laid out in y space
        A = np.linalg.qr(rng.standard_normal((d, d)))[0].astype(np.float32)
        c["A"] = A
        c["xb"] = (y.astype(np.float64) @ A.astype(np.float64)).astype(
            np.float32)
        c["q"] = (qy.astype(np.float64) @ A.astype(np.float64)).astype(
            np.float32)
    else:
        c["xb"], c["q"] = y, qy
    # CPU precondition: every row's nearest centroid (fp64, by the metric)
    # is its label with a margin, so the engine's lists are LIST_SIZES
    if typ not in ("flat", "hnswsq"):
        y64, c64 = y.astype(np.float64), cent.astype(np.float64)
        ip = y64 @ c64.T
        key_ = -ip if metric == IP else (c64 ** 2).sum(1)[None] - 2 * ip
        srt = np.sort(key_, axis=1)
        assert (np.argmin(key_, axis=1) == lbl).all()
        assert ((srt[:, 1] - srt[:, 0]) > 1e-3 * np.abs(srt[:, 0])).all()
    c["qb"] = _bad_queries(c["q"])
    c["qz"] = _zeroed(c["qb"])
    _CASES[key] = c
    return c


def _new_engine(c, **knobs):
    eng = HipEngine(spec=dict(c["spec"], **knobs))
    if c["A"] is not None:
        eng.set_transform(c["A"])
    return eng


def _set_trained(c, eng):
    if c["typ"] == "hnswsq":
        eng.train(c["xb"])
    elif c["typ"] != "flat":
        eng.set_trained(c["cent"], c["cb"], c["vmin"], c["vdiff"])
    return eng


def _engine(c, **knobs):
    eng = _set_trained(c, _new_engine(c, **knobs))
    eng.add(c["xb"][:SPLIT])
    eng.add(c["xb"][SPLIT:])
    if c["typ"] not in ("flat", "hnswsq"):
        np.testing.assert_array_equal(np.diff(eng.get_lists()[0]), LIST_SIZES)
    return eng


def _oracle(c, eng):
    """Oracle of an exact-tier case over the ENGINE's inverted lists."""
    if "orc" not in c:
        c["orc"] = from_engine_artifacts(
            c["spec"], c["cent"], c["cb"], c["vmin"], c["vdiff"],
            lists=eng.get_lists())
    return c["orc"]


def _oracle_q(c, eng, q):
    """The oracle works in the inner space of an OPQ index."""
    return eng.apply_transform(q) if c["A"] is not None else q


def _scans(c, eng, q, probes, keys, rows):
    """Per row in `rows`: the oracle's scan of every SURVIVING slot, in slot
    order (the oracle is called per query; an invalid slot is left out and
    its key is never looked at)."""
    orc = _oracle(c, eng)
    qo = _oracle_q(c, eng, q)
    out = {}
    for i in rows:
        slots = [s for s in range(probes.shape[1])
                 if 0 <= int(probes[i, s]) < NLIST]
        out[i] = scan_lists(
            orc, qo[i:i + 1], probes[i:i + 1, slots], keys[i:i + 1, slots])[0]
    return out


def _topk_of(scan_row, metric, k, allow=None):
    d = np.concatenate([r[0] for r in scan_row] + [np.empty(0, np.float32)])
    i = np.concatenate([r[1] for r in scan_row] + [np.empty(0, np.int64)])
    if allow is not None:
        keep = allow[i]
        d, i = d[keep], i[keep]
    key = d if metric == L2 else -d
    order = np.lexsort((i, key))[:k]
    Do = np.full(k, _pad_d(metric), np.float32)
    Io = np.full(k, -1, np.int64)
    Do[:order.size], Io[:order.size] = d[order], i[order]
    return Do, Io


def _fp64_check(c, q, D_, I_, rows, allow=None):
    """Tolerance tier: distances of the returned ids against fp64, and the
    k-th returned against the true k-th best."""
    x64 = c["xb"].astype(np.float64)
    for i in rows:
        q64 = q[i].astype(np.float64)
        if c["metric"] == L2:
            ref = ((q64[None] - x64) ** 2).sum(1)
            mag = ((np.abs(q64)[None] + np.abs(x64)) ** 2).sum(1)
        else:
            ref = x64 @ q64
            mag = np.abs(x64) @ np.abs(q64)
        tol = NORTH_STAR * mag + 1e-6
        ids = I_[i]
        assert (ids >= 0).all()
        assert (np.abs(D_[i].astype(np.float64) - ref[ids]) <= tol[ids]).all()
        if c["typ"] not in ("flat", "ivf_flat"):
            continue  # an approximate base stage: no claim on the ranking
        pool = ref if allow is None else ref[allow[:NROWS]]
        best = np.sort(pool if c["metric"] == L2 else -pool)[ids.size - 1]
        got = ref[ids[-1]] if c["metric"] == L2 else -ref[ids[-1]]
        assert got <= best + 2 * tol.max()


def _check_batch(c, eng, got_bad, got_zero, k, what, ref=None):
    """S2 + S3 + S4 of one entry; ref(i) -> (D, I) of finite row i."""
    metric = c["metric"]
    (Db, Ib), (Dz, Iz) = got_bad, got_zero
    for i in FINITE_ROWS:
        # CPU-side precondition of S4: the finite rows have k real results
        assert (Iz[i] >= 0).all(), what
        _same(Db[i], Dz[i], f"{what}: S4 D row {i}")
        _same(Ib[i], Iz[i], f"{what}: S4 I row {i}")
        if ref is not None:
            Dr, Ir = ref(i)
            assert (Ir >= 0).all(), what  # CPU: k non-pad reference results
            _same(Ib[i], Ir, f"{what}: oracle I row {i}")
            _same(Db[i], Dr, f"{what}: oracle D row {i}")
    _assert_pads(Db[NAN_ROWS], Ib[NAN_ROWS], metric, f"{what}: S2")
    _assert_well_formed(Db[INF_ROWS], Ib[INF_ROWS], eng.ntotal, metric,
                        f"{what}: S3")


# ---------------------------------------------------------------------------
# S2 / S3 / S4 over every search entry and index type
# ---------------------------------------------------------------------------

SEARCH_CASES = [
    pytest.param(kind, metric, id=f"{kind}-{'ip' if metric == IP else 'l2'}")
    for kind in KINDS for metric in (IP, L2)
    if not (kind == "hnswsq" and metric == IP)]  # hnswsq is L2 only


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind,metric", SEARCH_CASES)
def test_nonfinite_queries_every_entry(kind, metric, k):
    c = _case(kind, metric)
    eng = _engine(c)
    qb, qz = c["qb"], c["qz"]
    ivf = kind in IVF_KINDS
    tier = c["tier"]
    allow3 = np.arange(NROWS) % 3 != 0  # MOD3
    allow1 = np.ones(NROWS, bool)

    probes = keys = scans = None
    if ivf:
        # dfann_coarse: a NaN row has no fillable slot
        probes, keys = eng.coarse(qz, NLIST)
        assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
        pb, kb = eng.coarse(qb, NLIST)
        assert (pb[NAN_ROWS] == -1).all()
        assert (kb[NAN_ROWS] == FLT_MAX).all()
        _same(pb[FINITE_ROWS], probes[FINITE_ROWS], "coarse probes")
        _same(kb[FINITE_ROWS], keys[FINITE_ROWS], "coarse keys")
        for i in INF_ROWS:
            v = pb[i][pb[i] != -1]
            assert ((v >= 0) & (v < NLIST)).all()
            assert np.unique(v).size == v.size
            assert not np.isnan(kb[i]).any()
        if tier == "exact":
            scans = _scans(c, eng, qz, probes, keys, FINITE_ROWS)

    def ref_topk(allow=None):
        if tier == "exact":
            return lambda i: _topk_of(scans[i], metric, k, allow)
        return None

    # search
    got_b, got_z = eng.search(qb, k), eng.search(qz, k)
    _check_batch(c, eng, got_b, got_z, k, "search", ref_topk())
    if tier == "fp64":
        _fp64_check(c, qb, got_b[0], got_b[1], FINITE_ROWS)

    # search_and_reconstruct: pads reconstruct to zero rows
    Db, Ib, Rb = eng.search_and_reconstruct(qb, k)
    Dz, Iz, Rz = eng.search_and_reconstruct(qz, k)
    _check_batch(c, eng, (Db, Ib), (Dz, Iz), k, "reconstruct", ref_topk())
    assert (Rb[NAN_ROWS] == 0).all()
    _same(Rb[FINITE_ROWS], Rz[FINITE_ROWS], "reconstruct rows")
    assert (Rb[Ib == -1] == 0).all()

    if kind != "hnswsq":
        # filtered: all-ones bitmap and MOD3
        for name, allow in (("ones", allow1), ("mod3", allow3)):
            got_b = eng.search_filtered(qb, k, allow)
            got_z = eng.search_filtered(qz, k, allow)
            _check_batch(c, eng, got_b, got_z, k, f"filtered-{name}",
                         ref_topk(allow))
            assert allow[got_b[1][got_b[1] >= 0]].all()
            if tier == "fp64":
                _fp64_check(c, qb, got_b[0], got_b[1], FINITE_ROWS, allow)

    if not ivf:
        return
    # preassigned with VALID probes: the NaN rows still return pads
    got_b = eng.search_preassigned(qb, probes, keys, k)
    got_z = eng.search_preassigned(qz, probes, keys, k)
    _check_batch(c, eng, got_b, got_z, k, "preassigned", ref_topk())
    got_b = eng.search_preassigned_filtered(qb, probes, keys, k, allow3)
    got_z = eng.search_preassigned_filtered(qz, probes, keys, k, allow3)
    _check_batch(c, eng, got_b, got_z, k, "preassigned-filtered",
                 ref_topk(allow3))

    if "refine" in c["spec"]:
        return
    # range search: a NaN row has no hit; the radius of the second pass is
    # the k-th value of finite row 0 (so that row has hits at both radii)
    incl = FLT_MAX if metric == L2 else -FLT_MAX
    for radius in (incl, Dz[0, k - 1]):
        for run in (lambda q: eng.range_search(q, radius),
                    lambda q: eng.range_search_preassigned(q, probes, keys,
                                                           radius)):
            lb, Drb, Irb = run(qb)
            lz, Drz, Irz = run(qz)
            assert not np.isnan(Drb).any()
            assert ((Irb >= 0) & (Irb < NROWS)).all()
            for i in NAN_ROWS:
                assert lb[i + 1] == lb[i]
            for i in FINITE_ROWS:
                if radius == incl:
                    assert lz[i + 1] - lz[i] == NROWS
                elif i == 0:
                    assert 1 <= lz[i + 1] - lz[i] < k
                _same(Drb[lb[i]:lb[i + 1]], Drz[lz[i]:lz[i + 1]], "range D")
                _same(Irb[lb[i]:lb[i + 1]], Irz[lz[i]:lz[i + 1]], "range I")
                if tier == "exact":
                    _, Dr, Ir = range_from_scans(
                        [scans[i]], metric, radius)
                    _same(Drb[lb[i]:lb[i + 1]], Dr, "range oracle D")
                    _same(Irb[lb[i]:lb[i + 1]], Ir, "range oracle I")


# ---------------------------------------------------------------------------
# S1: caller-supplied probes outside [0, nlist)
# ---------------------------------------------------------------------------

PROBE_KINDS = ["ivf_flat"] + [k for k in EXACT_KINDS]


def _probe_patterns(probes):
    """first slot, last slot, all slots of query 2, the slot of the long
    list; the four invalid values rotate over queries and patterns."""
    out = {}
    for pi, name in enumerate(("first", "last", "query2", "long_list")):
        p = probes.copy()
        for i in range(NQ):
            bad = INVALID_PROBES[(i + pi) % 4]
            if name == "first":
                p[i, 0] = bad
            elif name == "last":
                p[i, -1] = bad
            elif name == "query2":
                if i == 2:
                    p[i, :] = [INVALID_PROBES[s % 4] for s in range(NLIST)]
            else:
                p[i, probes[i] == LONG_LIST] = bad
        out[name] = p
    return out


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", PROBE_KINDS)
def test_invalid_probes_are_empty_slots(kind, metric):
    c = _case(kind, metric)
    eng = _engine(c)
    q = c["q"]
    exact = c["tier"] == "exact"
    probes, keys = eng.coarse(q, NLIST)
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    allow1 = np.ones(NROWS, bool)
    allow3 = np.arange(NROWS) % 3 != 0
    incl = FLT_MAX if metric == L2 else -FLT_MAX
    mid = eng.search_preassigned(q, probes, keys, K_LDS)[0][:, K_LDS - 1]
    # list 0 is empty: an invalid slot must behave exactly like a probe of it
    assert LIST_SIZES[0] == 0
    for name, p in _probe_patterns(probes).items():
        invalid = (p < 0) | (p >= NLIST)
        assert invalid.any()
        kb = keys.copy()
        kb[invalid] = np.nan  # S1: the key of an invalid slot is never read
        pe = np.where(invalid, 0, p).astype(np.int32)
        scans = _scans(c, eng, q, p, keys, range(NQ)) if exact else None
        for k in (K_REG, K_LDS):
            runs = {
                "pre": (lambda P, K_: eng.search_preassigned(q, P, K_, k),
                        None),
                "pre-ones": (lambda P, K_: eng.search_preassigned_filtered(
                    q, P, K_, k, allow1), allow1),
                "pre-mod3": (lambda P, K_: eng.search_preassigned_filtered(
                    q, P, K_, k, allow3), allow3),
            }
            for rn, (run, allow) in runs.items():
                what = f"{name}-{rn}-k{k}"
                Dg, Ig = run(p, kb)
                De, Ie = run(pe, keys)
                _same(Dg, De, what + " vs empty list D")
                _same(Ig, Ie, what + " vs empty list I")
                assert not np.isnan(Dg).any(), what
                if name == "query2":
                    _assert_pads(Dg[2], Ig[2], metric, what)
                if exact:
                    for i in range(NQ):
                        Dr, Ir = _topk_of(scans[i], metric, k, allow)
                        _same(Ig[i], Ir, f"{what} oracle I row {i}")
                        _same(Dg[i], Dr, f"{what} oracle D row {i}")
        # range: both passes; slot order survives a subset of the slots
        for rname, r in (("incl", incl), ("mid", mid[0])):
            for allow in (None, allow3):
                what = f"{name}-range-{rname}"
                lg, Dg, Ig = eng.range_search_preassigned(q, p, kb, r, allow)
                le, De, Ie = eng.range_search_preassigned(q, pe, keys, r,
                                                          allow)
                _same(lg, le, what + " lims")
                _same(Dg, De, what + " D")
                _same(Ig, Ie, what + " I")
                assert not np.isnan(Dg).any(), what
                if name == "query2":
                    assert lg[3] == lg[2], what
                if exact:
                    lr, Dr, Ir = range_from_scans(
                        [scans[i] for i in range(NQ)], metric, r, allow)
                    _same(lg, lr, what + " oracle lims")
                    _same(Dg, Dr, what + " oracle D")
                    _same(Ig, Ir, what + " oracle I")


def test_invalid_probes_with_timing_enabled():
    # the timing path sums the probed list lengths on the host
    c = _case("sq8", L2)
    eng = _engine(c)
    q = c["q"]
    probes, keys = eng.coarse(q, NLIST)
    p = _probe_patterns(probes)["first"]
    want = eng.search_preassigned(q, p, keys, K_REG)
    eng.set_timing(True)
    got = eng.search_preassigned(q, p, keys, K_REG)
    eng.set_timing(False)
    _same(got[0], want[0])
    _same(got[1], want[1])


# ---------------------------------------------------------------------------
# fused coarse path (k_gemm_bf16_256_topk + k_coarse_reduce_rk)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", METRICS)
def test_fused_coarse_nan_rows(metric):
    # the smallest shape coarse_fused_ok admits: nlist 2048, nq 256, d 64,
    # coarse_bf16, nprobe on the register path
    nlist, nq, d, nprobe, n = 2048, 256, 64, 8, 300
    rng = np.random.default_rng(77 + metric)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    xb = (cent[rng.integers(0, nlist, n)]
          + 0.1 * rng.standard_normal((n, d))).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    qb = q.copy()
    nan_rows = [0, 1, 100, 255]
    qb[0, 0] = qb[1, d - 1] = qb[100, 17] = qb[255, :] = np.nan
    qz = _zeroed(qb)
    fin = np.flatnonzero(np.isfinite(qb).all(1))
    assert fin.size == nq - len(nan_rows)
    eng = HipEngine(spec={"type": "ivf_flat", "dim": d, "metric": metric,
                          "nlist": nlist, "nprobe": nprobe, "seed": 1,
                          "coarse_bf16": 1})
    eng.set_trained(cent)
    eng.add(xb)
    pz, kz = eng.coarse(qz, nprobe)
    pb, kb = eng.coarse(qb, nprobe)
    assert ((pz >= 0) & (pz < nlist)).all()
    assert (pb[nan_rows] == -1).all()
    assert (kb[nan_rows] == FLT_MAX).all()
    _same(pb[fin], pz[fin], "fused coarse probes")
    _same(kb[fin], kz[fin], "fused coarse keys")
    for k in (K_REG, K_LDS):
        Db, Ib = eng.search(qb, k)
        Dz, Iz = eng.search(qz, k)
        _assert_pads(Db[nan_rows], Ib[nan_rows], metric)
        _same(Db[fin], Dz[fin], "fused search D")
        _same(Ib[fin], Iz[fin], "fused search I")
    # below nq 256 the two-pass path runs, with LDS selection at nprobe 40
    pz, kz = eng.coarse(qz[:8], 40)
    pb, kb = eng.coarse(qb[:8], 40)
    assert (pb[:2] == -1).all() and (kb[:2] == FLT_MAX).all()
    _same(pb[2:], pz[2:], "two-pass coarse probes")
    _same(kb[2:], kz[2:], "two-pass coarse keys")


# ---------------------------------------------------------------------------
# S5: host argument checks
# ---------------------------------------------------------------------------


def test_preassigned_argument_checks():
    c = _case("ivf_flat", L2)
    eng = _engine(c)
    q = c["q"]
    probes, keys = eng.coarse(q, NLIST)
    allow = np.ones(NROWS, bool)
    for run in (lambda q_, p, k_, k: eng.search_preassigned(q_, p, k_, k),
                lambda q_, p, k_, k: eng.search_preassigned_filtered(
                    q_, p, k_, k, allow)):
        for k in (0, 513):
            with pytest.raises(RuntimeError, match=rf"\bk\b.*k = {k}\b"):
                run(q, probes, keys, k)
        for nprobe in (0, 513):
            p = np.zeros((NQ, nprobe), np.int32)
            with pytest.raises(RuntimeError,
                               match=rf"nprobe.*nprobe = {nprobe}\b"):
                run(q, p, np.zeros((NQ, nprobe), np.float32), 10)
        Dn, In = run(q[:0], probes[:0], keys[:0], 10)
        assert Dn.shape == (0, 10) and In.shape == (0, 10)
        D512, I512 = run(q, probes, keys, 512)
        assert D512.shape == (NQ, 512) and (I512[:, :K_LDS] >= 0).all()


# ---------------------------------------------------------------------------
# A2: add
# ---------------------------------------------------------------------------

POSITIONS = [pytest.param(0, id="first"),
             pytest.param((NROWS - SPLIT) // 2, id="middle"),
             pytest.param(NROWS - SPLIT - 1, id="last")]
ADD_KINDS = ["ivf_flat", "pq8-refine_fp32", "sq6", "opq-pq8"]


def _state(c, eng):
    st = {"ntotal": eng.ntotal, "trained": eng.is_trained,
          "search": eng.search(c["q"], K_REG)}
    if c["typ"] == "hnswsq":
        st["graph"] = eng.hnsw_dump()
    elif c["typ"] != "flat":
        st["lists"] = eng.get_lists()
    if "refine" in c["spec"]:
        st["rows"] = eng.get_refine_rows()
    return st


def _assert_state(a, b, what):
    assert a["ntotal"] == b["ntotal"] and a["trained"] == b["trained"], what
    for x, y in zip(a["search"], b["search"]):
        _same(x, y, what + " search")
    for x, y in zip(a.get("lists", ()), b.get("lists", ())):
        _same(x, y, what + " lists")
    if "rows" in a:
        _same(a["rows"], b["rows"], what + " refine rows")
    if "graph" in a:
        assert a["graph"].keys() == b["graph"].keys()
        for key_, v in a["graph"].items():
            if isinstance(v, np.ndarray):
                _same(v, b["graph"][key_], f"{what} graph {key_}")
            else:
                assert v == b["graph"][key_], f"{what} graph {key_}"


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ADD_KINDS)
def test_add_refuses_nan_row(kind, metric, pos):
    c = _case(kind, metric)
    eng = _set_trained(c, _new_engine(c))
    eng.add(c["xb"][:SPLIT])
    before = _state(c, eng)
    bad = c["xb"][SPLIT:].copy()
    bad[pos, (3 * pos) % c["d"]] = np.nan
    if pos == 0:
        bad[7, 1] = np.nan  # the error names the FIRST such row
    with pytest.raises(RuntimeError,
                       match=rf"add: row {pos} of the batch has no nearest"):
        eng.add(bad)
    _assert_state(_state(c, eng), before, "after the refused add")
    # a clean retry equals an engine that never saw the bad batch
    eng.add(c["xb"][SPLIT:])
    _assert_state(_state(c, eng), _state(c, _engine(c)), "after the retry")


def test_add_stores_an_inf_row_that_gets_a_list():
    # L2 key |c|^2 - 2 x.c of a row with +Inf at dim t: -inf wherever
    # c[t] > 0, +inf elsewhere; the lowest such list wins the tie. As in
    # faiss the row is stored; it can never be returned (its distance to a
    # finite query is +inf) and the other rows are not affected.
    c = _case("ivf_flat", L2)
    t = 4
    pos_lists = np.flatnonzero(c["cent"][:, t] > 0)
    assert pos_lists.size > 0
    eng = _engine(c)
    clean = eng.search(c["q"], K_LDS)
    row = c["xb"][:1].copy()
    row[0, t] = np.inf
    eng.add(row)
    assert eng.ntotal == NROWS + 1
    off, ids, _codes = eng.get_lists()
    want = np.array(LIST_SIZES)
    want[pos_lists[0]] += 1
    np.testing.assert_array_equal(np.diff(off), want)
    assert ids[off[pos_lists[0] + 1] - 1] == NROWS
    got = eng.search(c["q"], K_LDS)
    _same(got[0], clean[0])
    _same(got[1], clean[1])


def test_add_of_a_1e30_row_is_assigned_or_refused_never_unchecked():
    # A finite 1e30 keeps every fp32 key |c|^2 - 2 x.c finite (|c[t]| ~ 20),
    # so the row IS assignable: to the list with the largest c[t], by a
    # margin far above fp32 rounding. The contract is "a list or an
    # error"; with this data it must be that list.
    c = _case("ivf_flat", L2)
    t = 9
    order = np.argsort(c["cent"][:, t])
    best, second = order[-1], order[-2]
    assert c["cent"][best, t] - c["cent"][second, t] > 1e-3 * 20.0
    eng = _engine(c)
    row = np.zeros((1, c["d"]), np.float32)
    row[0, t] = 1e30
    eng.add(row)
    assert eng.ntotal == NROWS + 1
    off, ids, _codes = eng.get_lists()
    want = np.array(LIST_SIZES)
    want[best] += 1
    np.testing.assert_array_equal(np.diff(off), want)
    assert ids[off[best + 1] - 1] == NROWS
    D_, I_ = eng.search(c["q"], K_LDS)
    _assert_well_formed(D_, I_, NROWS + 1, L2)
    assert (I_ != NROWS).all()


@pytest.mark.parametrize("value,cls", [(np.nan, "NaN"), (np.inf, "Inf"),
                                       (-np.inf, "Inf")])
@pytest.mark.parametrize("pos", POSITIONS)
def test_hnswsq_add_refuses_nonfinite_batch(pos, value, cls):
    c = _case("hnswsq", L2)
    eng = _set_trained(c, _new_engine(c))
    eng.add(c["xb"][:SPLIT])
    before = _state(c, eng)
    bad = c["xb"][SPLIT:].copy()
    bad[pos, 5] = value
    with pytest.raises(RuntimeError,
                       match=rf"add: the batch holds a non-finite value "
                             rf"\({cls}\)"):
        eng.add(bad)
    _assert_state(_state(c, eng), before, "after the refused add")
    if pos == 0 and cls == "NaN":
        eng.add(c["xb"][SPLIT:])
        _assert_state(_state(c, eng), _state(c, _engine(c)),
                      "after the retry")


def test_flat_accepts_a_nan_row_and_never_returns_it():
    c = _case("flat", L2)
    eng = _engine(c)
    clean = eng.search(c["q"], K_LDS)
    row = c["xb"][:1].copy()
    row[0, 0] = np.nan
    eng.add(row)
    assert eng.ntotal == NROWS + 1
    got = eng.search(c["q"], K_LDS)
    _same(got[0], clean[0])
    _same(got[1], clean[1])


# ---------------------------------------------------------------------------
# A1: train
# ---------------------------------------------------------------------------

TRAIN_KINDS = ["ivf_flat", "pq8-inkernel", "sq8", "sq4", "sqfp16", "opq-pq8",
               "hnswsq"]
TRAIN_BAD = [pytest.param(np.nan, "NaN", 0, id="nan-first"),
             pytest.param(np.inf, "Inf", NROWS // 2, id="inf-middle"),
             pytest.param(np.nan, "NaN", NROWS - 1, id="nan-last")]


def _artifacts(c, eng):
    out = {}
    if c["typ"] != "hnswsq":
        out["centroids"] = eng.get_centroids()
    if c["typ"] == "ivfpq":
        out["codebooks"] = eng.get_codebooks()
    if c["typ"] == "hnswsq" or c["spec"].get("sq_type", "fp16") != "fp16":
        out["vmin"], out["vdiff"] = eng.get_sq_params()
    if c["A"] is not None:
        out["A"] = eng.get_transform()
    return out


@pytest.mark.parametrize("value,cls,pos", TRAIN_BAD)
@pytest.mark.parametrize("kind", TRAIN_KINDS)
def test_train_refuses_nonfinite_set(kind, value, cls, pos):
    c = _case(kind, L2)
    spec = dict(c["spec"], opq_niter=2) if c["A"] is not None else c["spec"]
    eng = HipEngine(spec=spec)
    bad = c["xb"].copy()
    bad[pos, (5 * pos) % c["d"]] = value
    with pytest.raises(RuntimeError,
                       match=rf"train: .*non-finite value \({cls}\)"):
        eng.train(bad)
    assert not eng.is_trained
    with pytest.raises(RuntimeError, match="untrained"):
        eng.add(c["xb"][:10])
    assert eng.ntotal == 0
    # a good train afterwards gives bitwise the artifacts of a fresh index
    eng.train(c["xb"])
    assert eng.is_trained
    fresh = HipEngine(spec=spec)
    fresh.train(c["xb"])
    a, b = _artifacts(c, eng), _artifacts(c, fresh)
    assert a.keys() == b.keys() and a
    for key_ in a:
        _same(a[key_], b[key_], key_)


def test_flat_train_accepts_anything():
    c = _case("flat", L2)
    eng = HipEngine(spec=c["spec"])
    bad = c["xb"].copy()
    bad[3, 3] = np.nan
    eng.train(bad)
    assert eng.is_trained


def test_train_on_1e30_rows_ends_trained_or_in_an_error():
    # Finite rows of magnitude 1e30: a centroid that averages one has a
    # component ~1e27 and so an infinite fp32 norm, and every key against it
    # is inf or NaN; once the empty-cluster split has copied such a centroid
    # over the others no row has a nearest centroid any more. Whatever the
    # draw, the outcome is an error naming train (the index stays untrained
    # and trains cleanly afterwards) or a trained index whose searches are
    # well-formed, never an assignment of -1 used as an index.
    c = _case("sq8", L2)
    bad = c["xb"].copy()
    bad[[0, NROWS // 2, NROWS - 1], 3] = 1e30
    eng = HipEngine(spec=c["spec"])
    try:
        eng.train(bad)
    except RuntimeError as e:
        assert "train: " in str(e) and "no nearest centroid" in str(e), str(e)
        assert not eng.is_trained
        eng.train(c["xb"])
        fresh = HipEngine(spec=c["spec"])
        fresh.train(c["xb"])
        a, b = _artifacts(c, eng), _artifacts(c, fresh)
        for key_ in a:
            _same(a[key_], b[key_], key_)
        return
    assert eng.is_trained
    eng.add(c["xb"])
    assert eng.ntotal == NROWS
    off, ids, _codes = eng.get_lists()
    assert off[-1] == NROWS and np.array_equal(np.sort(ids), np.arange(NROWS))
    D_, I_ = eng.search(c["q"], K_LDS)
    _assert_well_formed(D_, I_, NROWS, L2)
