# 4-bit product quantization (spec "nbits": 4) on the GPU,
# against the CPU oracle (oracle.OracleIVFPQ at nbits=4).
#
#  * bit-exact tier (assert_array_equal on D and I, byte equality of the
#    packed inverted lists): plain, filtered, reconstruct, refine on top,
#    save/load — on the construction of tests/test_gpu_dispatch_parity.py
#    (helpers in tests/gpu_support.py), each shape named by the dispatch
#    point it pins;
#  * training against oracle.kmeans with 16 codewords per subspace;
#  * end to end on Gaussian data: the encode in its tolerance tier, the
#    scan bitwise on the engine's own lists;
#  * the create-time refusals.
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
    assert_lists_equal,
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
    partial_shuffle_indices,
    unpack_pq4,
)
from oracle.refine import (  # noqa: E402
    refine_ref,
)

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]

# ---------------------------------------------------------------------------
# shared builder (the dispatch-parity construction): 12 lists covering empty
# / single-row lists and the 4-row, 8-row and wave tails; rows arrive
# shuffled, in two add calls
# ---------------------------------------------------------------------------

LIST_SIZES = [0, 1, 2, 3, 5, 63, 64, 65, 127, 129, 257, 515]
NLIST = len(LIST_SIZES)
NROWS = sum(LIST_SIZES)  # 1231
NQ = 8
K_REG, K_LDS = 10, 40  # register selection / LDS selection
KSUB = 16
CODEWORD_GAP = 0.05  # data uses codewords at least this far from any other


def _spec(d, metric, m, **kw):
    return ivf_spec("ivfpq", d, metric, NLIST, m=m, **dict({"nbits": 4}, **kw))


def _engine(spec, case):
    return engine_with(spec, case["cent"], case["cb"], xb=case["xb"], split=700)


@functools.lru_cache(maxsize=None)
def _case(m, dsub, metric):
    """Centroid + exact codeword + 1e-3 noise, so that the GEMM-decomposed
    engine encode and the sequential restatement pick the same codes: the
    own codeword is ~1e-3*sqrt(dsub) away, every other one at least
    CODEWORD_GAP - that."""
    d = m * dsub
    rng = np.random.default_rng(4000 + 1000 * m + dsub)
    cent = (rng.standard_normal((NLIST, d)) * 20.0).astype(np.float32)
    cb = rng.standard_normal((m, KSUB, dsub)).astype(np.float32)
    lbl = labels(rng, LIST_SIZES)
    assert lbl.shape[0] == NROWS
    # a quarter of each list repeats the codes of another row of that list:
    # exact distance ties, inside and across the top-k
    cw = codeword_rows(rng, cb, lbl, CODEWORD_GAP, 8)
    xb = (cent[lbl] + decode_rows(cb, cw)
          + 1e-3 * rng.standard_normal((NROWS, d))).astype(np.float32)
    q = queries(rng, cent, NQ, metric)
    orc = from_engine_artifacts(_spec(d, metric, m), cent, cb)
    orc.add(xb)
    # CPU conditions: the restatement encoded the intended codewords, its
    # lists are the intended ones, and every nibble value occurs in both
    # the low and the high position
    want = np.concatenate([cw[lbl == l] for l in range(NLIST)])
    np.testing.assert_array_equal(np.concatenate(orc.list_codes), want)
    np.testing.assert_array_equal([len(i) for i in orc.list_ids], LIST_SIZES)
    np.testing.assert_array_equal(
        np.concatenate(orc.list_ids),
        np.concatenate([np.flatnonzero(lbl == l) for l in range(NLIST)]))
    assert set(np.unique(want[:, 0::2])) == set(range(KSUB))
    if m > 1:
        assert set(np.unique(want[:, 1::2])) == set(range(KSUB))
    return {"m": m, "d": d, "metric": metric, "cent": cent, "cb": cb,
            "xb": xb, "q": q, "lbl": lbl, "orc": orc, "res": {}}


def _oracle_topk(case, probes, keys, kmax):
    """The restatement's top-kmax for the case, computed once per kmax (the
    smaller k are its prefixes: one lexsort order). Keyed on the probes and
    keys the engine handed out, which must not change between engines."""
    hit = case["res"].get(kmax)
    if hit is not None:
        np.testing.assert_array_equal(hit[0], probes)
        np.testing.assert_array_equal(hit[1], keys)
        return hit[2], hit[3]
    Do, Io = case["orc"].search_preassigned(case["q"], probes, keys, kmax)
    Do.setflags(write=False)
    Io.setflags(write=False)
    case["res"][kmax] = (probes.copy(), keys.copy(), Do, Io)
    return Do, Io


def _coarse(eng, case):
    probes, keys = eng.coarse(case["q"], NLIST)
    # every query probes every list, the empty one included
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    return probes, keys


def _assert_lists_equal(eng, case):
    codes = assert_lists_equal(eng, case["orc"])
    m = case["m"]
    assert codes.shape[1] == (((m + 1) // 2 + 15) // 16) * 16  # ceil16
    assert case["orc"].packed_lists()[2].shape[1] == (m + 1) // 2
    if m % 2:  # the unused high nibble of the last code byte
        assert (codes[:, m // 2] >> 4 == 0).all()


# ---------------------------------------------------------------------------
# 1. scan, bit for bit
# ---------------------------------------------------------------------------

PQ4_SHAPES = [
    pytest.param(32, 4, id="m32-dsub4-one_word-twin_of_bench_cfg2"),
    pytest.param(64, 12, id="m64-dsub12-headline_m"),
    pytest.param(128, 6, id="m128-dsub6-four_words-unguarded-twin_of_headline"),
    pytest.param(96, 2, id="m96-dsub2-three_words"),
    pytest.param(20, 3, id="m20-dsub3-partial_word-guarded-odd_dsub"),
    pytest.param(5, 8, id="m5-dsub8-odd_m"),
    pytest.param(2, 40, id="m2-dsub40-scalar_lut_loop"),
    pytest.param(16, 24, id="m16-dsub24-6xfloat4_lut_build"),
]


def _run_scan(m, dsub, metric, ks):
    case = _case(m, dsub, metric)
    eng = _engine(_spec(case["d"], metric, m), case)
    _assert_lists_equal(eng, case)
    probes, keys = _coarse(eng, case)
    Do, Io = _oracle_topk(case, probes, keys, K_LDS)
    assert (Io >= 0).all()  # every query probes all 1231 rows
    for k in ks:
        D, I = eng.search_preassigned(case["q"], probes, keys, k)
        np.testing.assert_array_equal(I, Io[:, :k])
        np.testing.assert_array_equal(D, Do[:, :k])  # BITWISE
    return D, I


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m,dsub", PQ4_SHAPES)
def test_scan_bitexact(m, dsub, metric):
    _run_scan(m, dsub, metric, (K_REG, K_LDS))


@pytest.mark.parametrize("metric", METRICS)
def test_selection_switch_k16_k17(metric):
    # k=16 is the last register-selection k, k=17 the first LDS-selection k
    _run_scan(32, 4, metric, (16, 17))


def test_results_carry_exact_ties():
    # repeated codes give equal sums: the (distance, ascending id) rule is
    # exercised, not satisfied vacuously
    D, I = _run_scan(32, 4, L2, (K_LDS,))
    ties = D[:, 1:] == D[:, :-1]
    assert ties.sum() > 0
    assert (I[:, 1:][ties] > I[:, :-1][ties]).all()


def test_search_equals_preassigned_and_env_overrides_are_ignored(monkeypatch):
    # the 8-bit LUT-mode overrides do not reach a 4-bit index
    case = _case(32, 4, L2)
    eng = _engine(_spec(case["d"], L2, 32, pq_lut_global=-1, pq_lut_mb=1), case)
    probes, keys = _coarse(eng, case)
    Do, Io = _oracle_topk(case, probes, keys, K_LDS)
    for name in ("DFANN_PQ_LUT_GLOBAL", "DFANN_PQ_LUT_F16"):
        monkeypatch.setenv(name, "1")
    for k in (K_REG, K_LDS):
        D, I = eng.search(case["q"], k)
        np.testing.assert_array_equal(I, Io[:, :k])
        np.testing.assert_array_equal(D, Do[:, :k])


# ---------------------------------------------------------------------------
# 2. filtered
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m,dsub", [(32, 4), (20, 3)])
def test_filtered_bitexact(m, dsub, metric):
    case = _case(m, dsub, metric)
    eng = _engine(_spec(case["d"], metric, m), case)
    probes, keys = _coarse(eng, case)
    # the restatement's full ranking, masked to the allowed ids
    Dall, Iall = _oracle_topk(case, probes, keys, NROWS)
    assert (Iall >= 0).all()
    allow = np.random.default_rng(17 * m + metric).uniform(size=NROWS) < 0.3
    assert 300 < allow.sum() < 450
    keep = allow[Iall]
    for k in (K_REG, K_LDS):
        D, I = eng.search_preassigned_filtered(case["q"], probes, keys, k, allow)
        for qi in range(NQ):
            sel = np.flatnonzero(keep[qi])[:k]
            assert sel.size == k
            np.testing.assert_array_equal(I[qi], Iall[qi, sel])
            np.testing.assert_array_equal(D[qi], Dall[qi, sel])


# ---------------------------------------------------------------------------
# 3. reconstruct
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("m,dsub", [(32, 4), (5, 8)])
def test_reconstruct_bitexact(m, dsub):
    case = _case(m, dsub, L2)
    eng = _engine(_spec(case["d"], L2, m), case)
    D, I, R = eng.search_and_reconstruct(case["q"], K_REG)
    assert (I >= 0).all()
    # centroid + codeword: one fp32 add on both sides
    np.testing.assert_array_equal(R, case["orc"].decode_ids(I))


# ---------------------------------------------------------------------------
# 4. refine on top
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", METRICS)
def test_refine_on_top_bitexact(metric):
    m, dsub, k, kf = 32, 4, 10, 4
    case = _case(m, dsub, metric)
    plain = _engine(_spec(case["d"], metric, m), case)
    probes, keys = _coarse(plain, case)
    _Do, Io = _oracle_topk(case, probes, keys, K_LDS)  # k' = 40
    eng = _engine(_spec(case["d"], metric, m, refine="fp32", k_factor=kf), case)
    D, I = eng.search(case["q"], k)
    Dr, Ir = refine_ref(case["q"], case["xb"], Io[:, :k * kf], k, metric)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D.view(np.uint32), Dr.view(np.uint32))


# ---------------------------------------------------------------------------
# 5. persistence
# ---------------------------------------------------------------------------


def test_save_load_round_trip(tmp_path):
    m, dsub = 20, 3
    case = _case(m, dsub, L2)
    eng = _engine(_spec(case["d"], L2, m), case)
    probes, keys = _coarse(eng, case)
    before = [eng.search_preassigned(case["q"], probes, keys, k)
              for k in (K_REG, K_LDS)]
    lists0, cb0 = eng.get_lists(), eng.get_codebooks()
    assert cb0.shape == (m, KSUB, dsub)
    np.testing.assert_array_equal(cb0, case["cb"])
    path = str(tmp_path / "pq4.dfann")
    eng.save(path)
    eng2 = HipProvider().load(path)
    assert eng2.spec["nbits"] == 4 and eng2.ntotal == NROWS
    for a, b in zip(eng2.get_lists(), lists0):
        np.testing.assert_array_equal(a, b)
    cb2 = eng2.get_codebooks()
    assert cb2.shape == (m, KSUB, dsub)
    np.testing.assert_array_equal(cb2, cb0)
    for k, (D0, I0) in zip((K_REG, K_LDS), before):
        D, I = eng2.search_preassigned(case["q"], probes, keys, k)
        np.testing.assert_array_equal(I, I0)
        np.testing.assert_array_equal(D, D0)
    _assert_lists_equal(eng2, case)


# ---------------------------------------------------------------------------
# 6. training: 16 codewords per subspace against oracle.kmeans
# ---------------------------------------------------------------------------


def _train_layout(n, ppc, m):
    """Rows come in twins — row 40u + r in coarse blob 0 and row 40u + 20 + r
    in coarse blob 1 share one in-blob offset (base row 20u + r) — so both
    coarse centroids sit at the same offset from their blob and the
    residuals of twins coincide. Returns the first seed for which the two
    coarse initial picks fall in different coarse blobs and, per subspace,
    the 16 initial picks are 16 different base rows."""
    i = np.arange(n)
    coarse = (i // 20) % 2
    base = (i // 40) * 20 + i % 20
    cap_c, cap = 2 * ppc, KSUB * ppc
    sel_c = (np.arange(cap_c, dtype=np.int64) * n) // cap_c
    sel = (np.arange(cap, dtype=np.int64) * n) // cap
    for seed in range(4321, 4521):
        ic = partial_shuffle_indices(cap_c, 2, seed)
        if coarse[sel_c[ic[0]]] == coarse[sel_c[ic[1]]]:
            continue
        picks = [base[sel[partial_shuffle_indices(cap, KSUB, seed + 1 + j)]]
                 for j in range(m)]
        if all(np.unique(p).size == KSUB for p in picks):
            return seed, coarse, base, picks
    raise AssertionError("no seed with separated initial picks")


def test_trained_codebooks_match_oracle_kmeans():
    # 25 Lloyd steps on both sides; the assignment arithmetic differs (GEMM
    # decomposition vs numpy), so every assignment is made unambiguous: two
    # coarse blobs far apart, per subspace 16 blobs of sigma 0.05 at spread
    # 20, and each initial codeword alone in its blob.
    n, m, dsub, ppc = 640, 4, 5, 16
    d = m * dsub
    assert n > KSUB * ppc  # the strided-subsample kernel runs
    seed, coarse, base, picks = _train_layout(n, ppc, m)
    rng = np.random.default_rng(7000)
    blobs_c = np.stack([np.full(d, -400.0), np.full(d, 400.0)])
    y = np.empty((n // 2, d))
    for j in range(m):
        sub = rng.standard_normal((KSUB, dsub)) * 20.0
        lbl = rng.integers(0, KSUB, n // 2)
        lbl[picks[j]] = np.arange(KSUB)
        y[:, j * dsub:(j + 1) * dsub] = (
            sub[lbl] + 0.05 * rng.standard_normal((n // 2, dsub)))
    x = (blobs_c[coarse] + y[base]).astype(np.float32)
    spec = {"type": "ivfpq", "dim": d, "metric": L2, "nlist": 2, "nprobe": 1,
            "seed": seed, "max_ppc": ppc, "m": m, "nbits": 4}
    eng = HipEngine(spec=spec)
    eng.train(x)
    cent_e = eng.get_centroids()
    cb_e = eng.get_codebooks()
    assert cb_e.shape == (m, KSUB, dsub)
    d2 = ((x[:, None, :].astype(np.float64) - cent_e[None]) ** 2).sum(-1)
    assign = d2.argmin(axis=1)
    assert (np.sort(d2, axis=1)[:, 1] > 100.0 * d2.min(axis=1)).all()
    resid = x - cent_e[assign]  # fp32, the engine's own subtraction
    for j in (0, 1, m - 1):
        sub = np.ascontiguousarray(resid[:, j * dsub:(j + 1) * dsub])
        stats = {}
        cb_o = kmeans(sub, KSUB, L2, seed + 1 + j, max_points_per_centroid=ppc,
                      stats=stats)
        assert stats["empty_splits"] == 0  # the split never fires
        # two fp32 roundings of an essentially exact mean, plus the engine's
        # fixed-point quantum (< 2^-40 max|x|)
        bound = (2.0 * 2.0 ** -23 * np.abs(cb_o.astype(np.float64))
                 + 2.0 ** -30 * float(np.abs(sub).max()))
        err = np.abs(cb_e[j].astype(np.float64) - cb_o)
        print(f"subspace {j}: max err/bound {(err / bound).max():.3g}")
        assert (err <= bound).all(), (j, (err / bound).max())


# ---------------------------------------------------------------------------
# 7. end to end on general data, no shared artifacts
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", METRICS)
def test_end_to_end_gaussian(metric):
    n, d, nlist, m, nq = 4000, 64, 8, 16, 8
    dsub = d // m
    rng = np.random.default_rng(8000 + metric)
    xb = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    spec = {"type": "ivfpq", "dim": d, "metric": metric, "nlist": nlist,
            "nprobe": nlist, "seed": 99, "m": m, "nbits": 4}
    eng = HipEngine(spec=spec)
    eng.train(xb)
    eng.add(xb[:2500])
    eng.add(xb[2500:])
    cent, cb = eng.get_centroids(), eng.get_codebooks()
    assert cb.shape == (m, KSUB, dsub)
    off, ids, packed = eng.get_lists()
    assert off[-1] == n and np.array_equal(np.sort(ids), np.arange(n))
    codes = unpack_pq4(packed, m)
    assert codes.max() < KSUB and np.unique(codes).size == KSUB
    # encode tolerance tier: the stored codeword is a nearest one in fp64
    lst = np.repeat(np.arange(nlist), np.diff(off))
    r = xb[ids].astype(np.float64) - cent[lst].astype(np.float64)
    cb64 = cb.astype(np.float64)
    for j in range(m):
        rj = r[:, j * dsub:(j + 1) * dsub]
        dist = ((rj[:, None, :] - cb64[j][None]) ** 2).sum(-1)  # (n, 16)
        got = dist[np.arange(n), codes[:, j]]
        tol = 1e-4 * ((rj ** 2).sum(-1) + (cb64[j][codes[:, j]] ** 2).sum(-1)) \
            + 1e-4
        assert (got <= dist.min(axis=1) + tol).all(), j
    # scan: the restatement on the engine's own artifacts, bitwise
    orc = from_engine_artifacts(spec, cent, cb, lists=(off, ids, packed))
    probes, keys = eng.coarse(q, nlist)
    Do, Io = orc.search_preassigned(q, probes, keys, K_LDS)
    for k in (K_REG, K_LDS):
        D, I = eng.search_preassigned(q, probes, keys, k)
        np.testing.assert_array_equal(I, Io[:, :k])
        np.testing.assert_array_equal(D, Do[:, :k])
    D, I = eng.search(q, K_REG)
    np.testing.assert_array_equal(I, Io[:, :K_REG])


# ---------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------


def test_other_widths_are_refused():
    with pytest.raises(RuntimeError, match="4, 8"):
        HipEngine(spec=_spec(64, L2, 16, nbits=5))


@pytest.mark.parametrize("knob", ["pq_lut_f16", "pq_lut_global",
                                  "pq_precomputed"])
def test_lut_knobs_are_refused_at_4_bits(knob):
    with pytest.raises(RuntimeError, match=knob):
        HipEngine(spec=_spec(64, L2, 16, **{knob: 1}))
    # an 8-bit spec with the knob is still created
    eng = HipEngine(spec=_spec(64, L2, 16, nbits=8, **{knob: 1}))
    assert not eng.is_trained


def test_set_trained_checks_the_codebook_shape():
    eng = HipEngine(spec=_spec(64, L2, 16))
    cent = np.zeros((NLIST, 64), np.float32)
    with pytest.raises(ValueError, match="16, 16, 4"):
        eng.set_trained(cent, np.zeros((16, 256, 4), np.float32))
