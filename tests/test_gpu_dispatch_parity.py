# GPU parity at the dispatch points the other suites never reach.
#
# scan_and_merge (csrc/dfann.hip) picks kernel, LUT mode and block size
# from m, dsub, d, k and the spec knobs; k_pq_lut has seven dsub bodies;
# gemm_keys_b picks one of four GEMMs from the tails of M, N and K. Each
# parametrization id below names the dispatch point it pins, so a failure
# maps to one instantiation.
#
#  * bit-exact tier (assert_array_equal on D and I against the oracle):
#    PQ in three LUT modes (in-kernel, f32 HBM LUT, fp16 HBM LUT), SQ8,
#    SQfp16 — plus byte equality of the finalized inverted lists;
#  * tolerance tier (fp64 reference, 1e-4 of the magnitude sum): IVF-Flat
#    scan, coarse GEMM + select (fp32 and bf16), trained centroids;
#  * exact: dfann_merge_topk against a numpy lexsort;
#  * more than one 64 MB slab and more than one persistence chunk.
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

from distributed_faiss_amd.hip_engine import (  # noqa: E402
    HipEngine,
    HipProvider,
    merge_topk_dev,
)
from gpu_support import (  # noqa: E402
    assert_lists_equal,
    bf16_round,
    codeword_rows,
    decode_rows,
    engine_with,
    ivf_spec,
    labels,
    queries,
)
from oracle import (  # noqa: E402
    from_engine_artifacts,
    kmeans,
    make_oracle_engine,
    partial_shuffle_indices,
)

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
FLT_MAX = np.float32(3.4028235e38)
NORTH_STAR = 1e-4  # the project's relative bound

# ---------------------------------------------------------------------------
# shared builder: 12 lists covering empty / single-row lists and the 4-row,
# 8-row and wave tails; rows arrive shuffled, in two add calls
# ---------------------------------------------------------------------------

LIST_SIZES = [0, 1, 2, 3, 5, 63, 64, 65, 127, 129, 257, 515]
NLIST = len(LIST_SIZES)
NROWS = sum(LIST_SIZES)  # 1231
NQ = 8
K_REG, K_LDS = 10, 40  # register selection / LDS selection


def _labels(rng):
    lbl = labels(rng, LIST_SIZES)
    assert lbl.shape[0] == NROWS
    return lbl


def _centroids(rng, d, spread):
    return (rng.standard_normal((NLIST, d)) * spread).astype(np.float32)


def _queries(rng, cent, d, metric):
    return queries(rng, cent, NQ, metric)


def _spec(typ, d, metric, **kw):
    return ivf_spec(typ, d, metric, NLIST, **kw)


def _engine(spec, xb, cent, cb=None, vmin=None, vdiff=None):
    return engine_with(spec, cent, cb, vmin, vdiff, xb, split=700)


def _oracle(spec, xb, cent, cb=None, vmin=None, vdiff=None):
    orc = from_engine_artifacts(spec, cent, cb, vmin, vdiff)
    orc.add(xb)
    orc.nprobe = NLIST
    return orc


def _assert_lists_equal(eng, orc, lbl):
    assert_lists_equal(eng, orc, LIST_SIZES, lbl)


class _OracleResults:
    """Oracle top-K_LDS per case, computed once and shared by the tests of
    the case (the k=10/16/17 results are its prefixes: one lexsort order).
    Keyed on the probes and keys the engine handed out, which must not
    change between engines of one case."""

    def __init__(self):
        self.store = {}

    def get(self, key, orc, q, probes, keys):
        hit = self.store.get(key)
        if hit is not None:
            np.testing.assert_array_equal(hit[0], probes)
            np.testing.assert_array_equal(hit[1], keys)
            return hit[2], hit[3]
        Do, Io = orc.search_preassigned(q, probes, keys, K_LDS)
        assert (Io >= 0).all()  # every query probes all 1231 rows
        self.store[key] = (probes.copy(), keys.copy(), Do, Io)
        return Do, Io


_RESULTS = _OracleResults()
_CASES = {}


def _cached(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def _assert_bitexact(eng, key, orc, q, ks):
    probes, keys = eng.coarse(q, NLIST)
    # every query probes every list, the empty one included
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    Do, Io = _RESULTS.get(key, orc, q, probes, keys)
    for k in ks:
        D, I = eng.search_preassigned(q, probes, keys, k)
        np.testing.assert_array_equal(I, Io[:, :k])
        np.testing.assert_array_equal(D, Do[:, :k])  # BITWISE


# ---------------------------------------------------------------------------
# B. PQ: (m, dsub) x metric x LUT mode
# ---------------------------------------------------------------------------

PQ_SHAPES = [
    pytest.param(16, 8, id="m16-dsub8-bench_cfg2"),
    pytest.param(64, 12, id="m64-dsub12-headline"),
    pytest.param(20, 3, id="m20-dsub3-partial_word-odd_dsub"),
    pytest.param(96, 2, id="m96-dsub2-second_64_code_pass"),
    pytest.param(16, 24, id="m16-dsub24-runtime_dsub_lut-6xfloat4"),
    pytest.param(8, 40, id="m8-dsub40-scalar_lut_loop"),
    pytest.param(32, 6, id="m32-dsub6-lut_width6"),
    pytest.param(16, 16, id="m16-dsub16-lut_width16"),
]
PQ_MODES = [
    pytest.param("inkernel", id="inkernel"),
    pytest.param("glut_f32", id="glut_f32"),
    pytest.param("glut_f16", id="glut_f16"),
]
_MODE_KNOBS = {
    "inkernel": {"pq_lut_global": 0},
    "glut_f32": {"pq_lut_global": 1},
    "glut_f16": {"pq_lut_f16": 1},
}
CODEWORD_GAP = 0.05  # data uses codewords at least this far from any other
HALF_MAX_HALVED = 32752.0  # half of fp16's largest finite value
HALF_MIN_NORMAL = 2.0 ** -14


def _pq_case(m, dsub, metric, f16):
    """Centroid + exact codeword + 1e-3 noise, so that the GEMM-decomposed
    engine encode and the sequential oracle encode pick the same codes:
    the own codeword is ~1e-3*sqrt(dsub) away, every other one at least
    CODEWORD_GAP - that."""
    d = m * dsub
    rng = np.random.default_rng(1000 * m + dsub)
    # spread 5 keeps every LUT entry inside half range (20 reaches 4e4 at
    # dsub=24); the exact modes keep the suite's usual 20
    cent = _centroids(rng, d, 5.0 if f16 else 20.0)
    cb = rng.standard_normal((m, 256, dsub)).astype(np.float32)
    lbl = _labels(rng)
    # a quarter of each list repeats the codes of another row of that list:
    # exact distance ties in every mode, inside and across the top-k
    cw = codeword_rows(rng, cb, lbl, CODEWORD_GAP, 64)
    xb = (cent[lbl] + decode_rows(cb, cw)
          + 1e-3 * rng.standard_normal((NROWS, d))).astype(np.float32)
    q = _queries(rng, cent, d, metric)
    spec = _spec("ivfpq", d, metric, m=m, pq_lut_f16=1 if f16 else 0)
    orc = _oracle(spec, xb, cent, cb)
    # CPU condition: the oracle encoded the intended codewords
    np.testing.assert_array_equal(
        np.concatenate(orc.list_codes),
        np.concatenate([cw[lbl == l] for l in range(NLIST)]).astype(np.uint8))
    # LUT statistics, gathered while the oracle builds them
    stats = {"max": 0.0, "subnormal": 0, "entries": 0}
    inner = orc.build_lut

    def tracked(qi, li):
        lut, bias = inner(qi, li)
        a = np.abs(lut)
        stats["max"] = max(stats["max"], float(a.max()))
        stats["subnormal"] += int(((a > 0) & (a < HALF_MIN_NORMAL)).sum())
        stats["entries"] += a.size
        return lut, bias

    orc.build_lut = tracked
    return {"spec": spec, "cent": cent, "cb": cb, "xb": xb, "q": q,
            "lbl": lbl, "orc": orc, "stats": stats}


def _run_pq(m, dsub, metric, mode, ks):
    f16 = mode == "glut_f16"
    key = ("pq", m, dsub, metric, f16)
    case = _cached(key, lambda: _pq_case(m, dsub, metric, f16))
    spec = dict(case["spec"], **_MODE_KNOBS[mode])
    eng = _engine(spec, case["xb"], case["cent"], case["cb"])
    _assert_lists_equal(eng, case["orc"], case["lbl"])
    _assert_bitexact(eng, key, case["orc"], case["q"], ks)
    st = case["stats"]
    assert st["entries"] == NQ * (NLIST - 1) * m * 256  # empty list: no LUT
    if f16:
        # condition of the bitwise definition: no entry near half overflow
        # (half-subnormal entries are allowed: gradual underflow is part
        # of the definition)
        assert st["max"] <= HALF_MAX_HALVED, st


@pytest.mark.parametrize("mode", PQ_MODES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m,dsub", PQ_SHAPES)
def test_pq_scan_dispatch_bitexact(m, dsub, metric, mode):
    _run_pq(m, dsub, metric, mode, (K_REG, K_LDS))


@pytest.mark.parametrize("mode", PQ_MODES)
@pytest.mark.parametrize("metric", METRICS)
def test_pq_selection_switch_k16_k17(metric, mode):
    # k=16 is the last register-selection k, k=17 the first LDS-selection k
    _run_pq(16, 8, metric, mode, (16, 17))


def test_pq_f16_half_subnormal_entries_exercised():
    # gradual underflow is part of the f16 definition: this case's tables
    # hold half-subnormal entries (IP entries q_j . cb near zero), and the
    # engine still equals the oracle bit for bit
    m, dsub = 96, 2
    _run_pq(m, dsub, IP, "glut_f16", (K_REG, K_LDS))
    st = _CASES[("pq", m, dsub, IP, True)]["stats"]
    assert st["subnormal"] > 0, st


def test_pq_f16_results_carry_exact_ties():
    # repeated codes and colliding half-rounded sums: the (distance,
    # ascending id) rule is exercised by the cases above, not just
    # satisfied vacuously
    key = ("pq", 16, 8, L2, True)
    case = _cached(key, lambda: _pq_case(16, 8, L2, True))
    eng = _engine(dict(case["spec"]), case["xb"], case["cent"], case["cb"])
    probes, keys = eng.coarse(case["q"], NLIST)
    Do, Io = _RESULTS.get(key, case["orc"], case["q"], probes, keys)
    D, I = eng.search_preassigned(case["q"], probes, keys, K_LDS)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D, Do)
    ties = D[:, 1:] == D[:, :-1]
    assert ties.sum() > 0
    assert (I[:, 1:][ties] > I[:, :-1][ties]).all()


# ---------------------------------------------------------------------------
# B. SQ8: per-dimension ranges, all 256 codes, both clamps
# ---------------------------------------------------------------------------

SQ8_DIMS = [
    pytest.param(20, id="d20-two_lanes"),
    pytest.param(100, id="d100-partial_last_lane"),
    pytest.param(128, id="d128-one_full_chunk"),
    pytest.param(200, id="d200-two_chunks"),
    pytest.param(768, id="d768-six_chunks"),
]


def _sq8_case(d, metric):
    rng = np.random.default_rng(2000 + d)
    cent = _centroids(rng, d, 20.0)
    lbl = _labels(rng)
    vmin = rng.uniform(-3.0, -1.0, d).astype(np.float32)
    vdiff = rng.uniform(2.0, 6.0, d).astype(np.float32)
    c = rng.integers(0, 256, (NROWS, d))
    jit = rng.uniform(-0.1, 0.1, (NROWS, d))
    resid = vmin + (c + 0.5 + jit) * (vdiff.astype(np.float64) / 255)
    # ~3 % of the entries leave the trained range by 0.5-2 x vdiff
    out = rng.uniform(0.0, 1.0, (NROWS, d))
    push = rng.uniform(0.5, 2.0, (NROWS, d)) * vdiff
    lo, hi = out < 0.015, out > 0.985
    resid = np.where(lo, vmin - push, resid)
    resid = np.where(hi, vmin.astype(np.float64) + vdiff + push, resid)
    want = np.where(lo, 0, np.where(hi, 255, c)).astype(np.uint8)
    assert lo.sum() > 0 and hi.sum() > 0
    assert len(np.unique(want)) == 256
    xb = (cent[lbl] + resid).astype(np.float32)
    q = _queries(rng, cent, d, metric)
    spec = _spec("ivfsq", d, metric, sq_type="8bit")
    orc = _oracle(spec, xb, cent, vmin=vmin, vdiff=vdiff)
    # CPU condition: the oracle's codes are the intended ones, clamped
    np.testing.assert_array_equal(
        np.concatenate(orc.list_codes),
        np.concatenate([want[lbl == l] for l in range(NLIST)]))
    return {"spec": spec, "cent": cent, "xb": xb, "q": q, "lbl": lbl,
            "orc": orc, "vmin": vmin, "vdiff": vdiff}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", SQ8_DIMS)
def test_sq8_scan_dispatch_bitexact(d, metric):
    key = ("sq8", d, metric)
    case = _cached(key, lambda: _sq8_case(d, metric))
    eng = _engine(case["spec"], case["xb"], case["cent"], None,
                  case["vmin"], case["vdiff"])
    _assert_lists_equal(eng, case["orc"], case["lbl"])
    _assert_bitexact(eng, key, case["orc"], case["q"], (K_REG, K_LDS))


# ---------------------------------------------------------------------------
# B. SQfp16: four decades of magnitude, both signs, exact zeros
# ---------------------------------------------------------------------------

SQF_DIMS = [
    pytest.param(20, id="d20-partial_word"),
    pytest.param(72, id="d72-second_line_one_word"),
    pytest.param(128, id="d128-two_lines"),
    pytest.param(768, id="d768-twelve_lines"),
]


def _sqf_case(d, metric):
    rng = np.random.default_rng(3000 + d)
    cent = _centroids(rng, d, 20.0)
    lbl = _labels(rng)
    mag = 10.0 ** rng.uniform(-3.0, 1.0, (NROWS, d))
    resid = mag * rng.choice([-1.0, 1.0], (NROWS, d))
    zero = rng.uniform(0.0, 1.0, (NROWS, d)) < 0.05
    resid[zero] = 0.0
    xb = (cent[lbl] + resid).astype(np.float32)
    xb[zero] = cent[lbl][zero]  # residual exactly zero
    q = _queries(rng, cent, d, metric)
    spec = _spec("ivfsq", d, metric, sq_type="fp16")
    orc = _oracle(spec, xb, cent)
    halves = np.concatenate(orc.list_codes).view(np.float16)
    assert (halves == 0).sum() >= zero.sum()
    assert (halves < 0).any() and (halves > 0).any()
    return {"spec": spec, "cent": cent, "xb": xb, "q": q, "lbl": lbl,
            "orc": orc}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", SQF_DIMS)
def test_sqfp16_scan_dispatch_bitexact(d, metric):
    key = ("sqf", d, metric)
    case = _cached(key, lambda: _sqf_case(d, metric))
    eng = _engine(case["spec"], case["xb"], case["cent"])
    _assert_lists_equal(eng, case["orc"], case["lbl"])
    _assert_bitexact(eng, key, case["orc"], case["q"], (K_REG, K_LDS))


# ---------------------------------------------------------------------------
# tolerance tier: fp64 reference over every candidate row
# ---------------------------------------------------------------------------


# share of ranks that rule 3 must decide, so that the id check bites: a
# property of the data and the fp64 reference alone (the smallest case,
# d=768 IP at k=40, decides 0.62)
DECIDED_MIN = 0.6
ATOL = 1e-4  # the suites' usual absolute floor next to the relative bound


def _assert_tolerance_tier(q, xb, D, I, metric):
    """Engine (D, I) against fp64 over ALL rows of xb (every list probed;
    ids are arrival positions). The tier's bound, as the other suites
    assert it: b_u = 1e-4 * |ref_u| + 1e-4 for candidate u. Then:
      1. every returned distance is within b of the fp64 value of its id —
         and, additionally, within 1e-4 of the sum of the magnitudes of
         its terms (sum (q-x)^2 for L2, sum |q_t x_t| for IP);
      2. ids are distinct and valid, D is ordered (ascending L2,
         descending IP);
      3. rank j holds the fp64 rank-j id wherever the fp64 gap to the
         next candidate on either side exceeds the bound, i.e. wherever
         [key-b, key+b] of that candidate meets no other candidate's;
      4. no unreturned candidate beats the last returned one by more
         than its b.
    Returns the fraction of ranks decided by 3."""
    k = D.shape[1]
    x64 = xb.astype(np.float64)
    n = xb.shape[0]
    decided = 0
    for i in range(q.shape[0]):
        q64 = q[i].astype(np.float64)
        if metric == L2:
            ref = ((q64 - x64) ** 2).sum(axis=1)
            mag, key = ref, ref
        else:
            ref = x64 @ q64
            mag, key = np.abs(x64 * q64).sum(axis=1), -ref
        b = NORTH_STAR * np.abs(ref) + ATOL
        ids = I[i]
        assert (ids >= 0).all() and (ids < n).all()
        assert len(set(ids.tolist())) == k
        got = D[i].astype(np.float64)
        gkey = got if metric == L2 else -got
        assert (gkey[1:] >= gkey[:-1]).all(), i
        err = np.abs(got - ref[ids])
        assert (err <= b[ids]).all(), (i, (err / b[ids]).max())
        assert (err <= NORTH_STAR * mag[ids]).all(), (
            i, (err / (NORTH_STAR * mag[ids])).max())
        order = np.lexsort((np.arange(n), key))
        lo, hi = (key - b)[order], (key + b)[order]
        lo_after = np.minimum.accumulate(lo[::-1])[::-1]  # min lo[j:]
        hi_before = np.maximum.accumulate(hi)             # max hi[:j+1]
        for j in range(k):
            above = hi[j] < lo_after[j + 1]
            below = j == 0 or lo[j] > hi_before[j - 1]
            if above and below:
                decided += 1
                assert ids[j] == order[j], (i, j)
        rest = np.ones(n, bool)
        rest[ids] = False
        assert (key[rest] + b[rest] >= gkey[-1]).all(), i
    return decided / (q.shape[0] * k)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", SQ8_DIMS)
def test_ivfflat_scan_dispatch_tolerance(d, metric):
    # 16-lane tree reduction: tolerance tier. Lists are still byte-exact.
    rng = np.random.default_rng(4000 + d)
    # spread 1.5 against sigma 0.5: lists stay unambiguous (centroids
    # ~2.1 sqrt(d) apart, rows 0.5 sqrt(d) from their own) and fp64 gaps
    # between neighbouring candidates stay well above the bound
    cent = _centroids(rng, d, 1.5)
    lbl = _labels(rng)
    xb = (cent[lbl] + 0.5 * rng.standard_normal((NROWS, d))).astype(np.float32)
    # plain cent[l] + 0.7 N(0,1) queries under both metrics: this scan
    # has no bias term to hide low bits under
    q = _queries(rng, cent, d, L2)
    spec = _spec("ivf_flat", d, metric)
    orc = _oracle(spec, xb, cent)
    eng = _engine(spec, xb, cent)
    _assert_lists_equal(eng, orc, lbl)
    probes, keys = eng.coarse(q, NLIST)
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    for k in (K_REG, K_LDS):
        D, I = eng.search_preassigned(q, probes, keys, k)
        decided = _assert_tolerance_tier(q, xb, D, I, metric)
        assert decided > DECIDED_MIN, decided  # the id check bites


# ---------------------------------------------------------------------------
# C. coarse GEMM + select against fp64, through dfann_coarse
# ---------------------------------------------------------------------------


def _check_coarse(nq, nlist, d, metric, nprobe, bf16):
    rng = np.random.default_rng(nq * 7919 + nlist * 31 + d)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    spec = {"type": "ivf_flat", "dim": d, "metric": metric, "nlist": nlist,
            "nprobe": 1, "seed": 1, "coarse_bf16": 1 if bf16 else 0}
    eng = HipEngine(spec=spec)
    eng.set_trained(cent)
    probes, keys = eng.coarse(q, nprobe)
    assert probes.shape == (nq, nprobe)
    # fp64 reference over the operands the GEMM consumed; the centroid
    # norms come from the fp32 centroids in both modes
    qr = (bf16_round(q) if bf16 else q).astype(np.float64)
    cr = (bf16_round(cent) if bf16 else cent).astype(np.float64)
    cn = (cent.astype(np.float64) ** 2).sum(axis=1)
    dot = qr @ cr.T
    absdot = np.abs(qr) @ np.abs(cr).T
    ref = cn[None, :] - 2.0 * dot if metric == L2 else -dot
    bound = NORTH_STAR * (cn[None, :] + 2.0 * absdot)
    rows = np.arange(nq)[:, None]
    # 1. returned keys within the bound for their list id
    assert (probes >= 0).all() and (probes < nlist).all()
    err = np.abs(keys.astype(np.float64) - ref[rows, probes])
    assert (err <= bound[rows, probes]).all(), (err / bound[rows, probes]).max()
    # 2. distinct ids
    srt = np.sort(probes, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    # 3. ascending keys, equal keys in ascending id order
    assert (keys[:, 1:] >= keys[:, :-1]).all()
    tie = keys[:, 1:] == keys[:, :-1]
    assert (probes[:, 1:][tie] > probes[:, :-1][tie]).all()
    # 4. nothing better was left out
    rest = np.ones((nq, nlist), bool)
    rest[rows, probes] = False
    last = keys[:, -1].astype(np.float64)[:, None]
    assert (~rest | (ref >= last - 2.0 * bound)).all()


COARSE_F32_SHAPES = [
    (1, 3, 5, "all_tails"),
    (33, 100, 20, ""),
    (129, 129, 130, "tails_in_M_N_K"),
    (130, 512, 100, ""),
    (257, 300, 768, ""),
]


def _coarse_f32_params():
    """Per shape nprobe = min(nlist, 512) and nprobe = 8; the id names the
    select kernel that nprobe reaches (register path up to 16). At
    nlist = 3 both give nprobe = 3 on the register path: one case."""
    out = []
    for nq, nlist, d, note in COARSE_F32_SHAPES:
        for nprobe in sorted({min(nlist, 512), min(nlist, 8)}):
            kern = "k_topk_rows_rk" if nprobe <= 16 else "k_topk_rows"
            name = f"nq{nq}-nlist{nlist}-d{d}-nprobe{nprobe}-{kern}"
            out.append(pytest.param(nq, nlist, d, nprobe,
                                    id=name + ("-" + note if note else "")))
    return out


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq,nlist,d,nprobe", _coarse_f32_params())
def test_coarse_f32_vs_fp64(nq, nlist, d, nprobe, metric):
    _check_coarse(nq, nlist, d, metric, nprobe, bf16=False)


COARSE_BF16 = [
    pytest.param(33, 100, 20, 8, id="nq33-nlist100-d20-k_gemm_bf16_nt"),
    pytest.param(33, 100, 20, 100, id="nq33-nlist100-d20-k_gemm_bf16_nt-lds"),
    pytest.param(129, 129, 136, 8, id="nq129-nlist129-d136-k_gemm_bf16_glds"),
    pytest.param(129, 129, 136, 129,
                 id="nq129-nlist129-d136-k_gemm_bf16_glds-lds"),
    pytest.param(130, 512, 96, 8, id="nq130-nlist512-d96-k_gemm_bf16_glds"),
    pytest.param(130, 512, 96, 512,
                 id="nq130-nlist512-d96-k_gemm_bf16_glds-lds"),
    pytest.param(256, 2048, 64, 512, id="nq256-nlist2048-d64-k_gemm_bf16_256"),
    pytest.param(300, 2100, 72, 512, id="nq300-nlist2100-d72-k_gemm_bf16_256"),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq,nlist,d,nprobe", COARSE_BF16)
def test_coarse_bf16_vs_fp64(nq, nlist, d, nprobe, metric):
    _check_coarse(nq, nlist, d, metric, nprobe, bf16=True)


# ---------------------------------------------------------------------------
# D. dfann_merge_topk against a numpy lexsort
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("maximize", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("k", [1, 4, 16, 17, 64, 512])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_merge_topk_vs_lexsort(S, k, nq, maximize):
    rng = np.random.default_rng(S * 100003 + k * 101 + nq * 7 + int(maximize))
    pool = rng.standard_normal(50).astype(np.float32)
    pad = -FLT_MAX if maximize else FLT_MAX
    D = np.empty((S, nq, k), np.float32)
    I = np.empty((S, nq, k), np.int64)
    for s in range(S):
        for qi in range(nq):
            # ties cross shards (50-value pool); a third of the rows end
            # in pads, some consist of nothing else
            valid = k if rng.uniform() < 0.67 else int(rng.integers(0, k + 1))
            v = np.sort(rng.choice(pool, valid))
            D[s, qi, :valid] = v[::-1] if maximize else v  # faiss order
            D[s, qi, valid:] = pad
            I[s, qi, :valid] = rng.integers(0, 1 << 40, valid)
            I[s, qi, valid:] = -1
    Dm, Im = merge_topk_dev(torch.as_tensor(D).cuda(),
                            torch.as_tensor(I).cuda(), k, maximize=maximize)
    Dm, Im = Dm.cpu().numpy(), Im.cpu().numpy()
    # key = -v for maximize (kept in the output: reference quirk 2);
    # order by (key, dense slot s*k + j); id = s*nq*k + q*k + j
    key = (-D if maximize else D).transpose(1, 0, 2).reshape(nq, S * k)
    slot = np.arange(S * k)
    for qi in range(nq):
        order = np.lexsort((slot, key[qi]))[:k]
        np.testing.assert_array_equal(Dm[qi], key[qi][order])
        np.testing.assert_array_equal(
            Im[qi], (order // k) * nq * k + qi * k + order % k)


# ---------------------------------------------------------------------------
# E. engine-trained centroids against oracle.core.kmeans
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("typ", ["ivf_flat", "ivfsq8"])
def test_trained_centroids_match_oracle_kmeans(typ):
    # 25 Lloyd steps on both sides; the assignment arithmetic differs (MFMA
    # GEMM vs numpy), so every assignment is made unambiguous: 24 blobs of
    # sigma 0.05 at spread 20, and each initial centroid alone in its blob.
    n, d, nlist, ppc, seed = 960, 20, 24, 16, 4321
    cap = nlist * ppc  # 384 < n: the strided-subsample kernel runs
    rng = np.random.default_rng(5000)
    blobs = (rng.standard_normal((nlist, d)) * 20.0).astype(np.float32)
    sel = (np.arange(cap, dtype=np.int64) * n) // cap
    init = partial_shuffle_indices(cap, nlist, seed)
    lbl = rng.integers(0, nlist, n)
    lbl[sel[init]] = np.arange(nlist)
    x = (blobs[lbl] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    stats = {}
    cent_o = kmeans(x, nlist, L2, seed, max_points_per_centroid=ppc,
                    stats=stats)
    assert stats["empty_splits"] == 0  # the split never fires
    spec = {"type": "ivf_flat" if typ == "ivf_flat" else "ivfsq", "dim": d,
            "metric": L2, "nlist": nlist, "nprobe": 1, "seed": seed,
            "max_ppc": ppc}
    if typ == "ivfsq8":
        spec["sq_type"] = "8bit"
    eng = HipEngine(spec=spec)
    eng.train(x)
    cent_e = eng.get_centroids()
    # two fp32 roundings of an essentially exact mean, plus the engine's
    # fixed-point quantum (< 2^-40 max|x|)
    bound = (2.0 * 2.0 ** -23 * np.abs(cent_o.astype(np.float64))
             + 2.0 ** -30 * float(np.abs(x).max()))
    err = np.abs(cent_e.astype(np.float64) - cent_o)
    assert (err <= bound).all(), (err / bound).max()
    if typ == "ivfsq8":
        orc = make_oracle_engine(spec)
        orc.train(x)
        np.testing.assert_array_equal(orc.centroids, cent_o)
        vmin, vdiff = eng.get_sq_params()
        cb = 2.0 * bound.max(axis=0)
        for got, want in ((vmin, orc.vmin), (vdiff, orc.vdiff)):
            tol = cb + np.spacing(np.abs(want)).astype(np.float64)
            e = np.abs(got.astype(np.float64) - want)
            assert (e <= tol).all(), (e / tol).max()


# ---------------------------------------------------------------------------
# F. more than one 64 MB slab, more than one persistence chunk
# ---------------------------------------------------------------------------


def test_two_slabs_two_persistence_chunks(tmp_path):
    # stride 3072 B: 16384 rows per slab, 21845 rows per save/load chunk;
    # 24000 rows (73.7 MB) cross both, inside list 1
    d, n, nq, k = 768, 24000, 8, 10
    rng = np.random.default_rng(6000)
    cent = (rng.standard_normal((2, d)) * 4.0).astype(np.float32)
    lbl = rng.integers(0, 2, n)
    xb = cent[lbl] + 0.5 * rng.standard_normal((n, d), dtype=np.float32)
    q = (cent[rng.integers(0, 2, nq)]
         + 0.7 * rng.standard_normal((nq, d))).astype(np.float32)
    spec = {"type": "ivf_flat", "dim": d, "metric": L2, "nlist": 2,
            "nprobe": 2, "seed": 1}
    eng = HipEngine(spec=spec)
    eng.set_trained(cent)
    eng.add(xb)
    want_ids = np.concatenate([np.flatnonzero(lbl == 0),
                               np.flatnonzero(lbl == 1)])
    assert (lbl == 0).sum() < 16384 < n  # the slab boundary lies in list 1

    def lists(e):
        off, ids, codes = e.get_lists()
        assert codes.shape == (n, 4 * d)
        return off, ids, codes

    off, ids, codes = lists(eng)
    np.testing.assert_array_equal(off, [0, (lbl == 0).sum(), n])
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(codes.view(np.uint32),
                                  xb[want_ids].view(np.uint32))
    D, I = eng.search(q, k)
    decided = _assert_tolerance_tier(q, xb, D, I, L2)
    assert decided > 0.5, decided
    p = str(tmp_path / "two_slabs.dfann")
    eng.save(p)
    eng2 = HipProvider().load(p)
    assert eng2.ntotal == n
    D2, I2 = eng2.search(q, k)
    np.testing.assert_array_equal(I2, I)
    np.testing.assert_array_equal(D2, D)
    off2, ids2, codes2 = lists(eng2)
    np.testing.assert_array_equal(off2, off)
    np.testing.assert_array_equal(ids2, ids)
    np.testing.assert_array_equal(codes2, codes)
