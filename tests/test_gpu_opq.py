# OPQ pre-transform (spec "opq": 1) on the GPU, against the
# numpy restatement oracle/opq.py.
#
#  1. bit-exact tier: A a signed permutation / selection (y = A x exact in any
#     summation order), artifacts injected — search_preassigned and the
#     inverted lists equal the restatement bit for bit, and so does a plain
#     ivfpq engine at d_out fed the permuted data;
#  2. equivalence on a general rotation: the OPQ engine is bitwise the plain
#     d_out engine behind apply_transform — plain, filtered, preassigned and
#     with refine on top (oracle/refine.py over the ORIGINAL vectors);
#  3. transform values in the project's tolerance tier, independent of the
#     batch shape; reconstruct = A^T . decode;
#  4. training: orthonormal rows, quantization error, determinism, a
#     rank-deficient input, d_out < d_in;
#  5. persistence and the host surface (Index, IndexClient).
#
# Shapes: nq = 130 (row tile 128 + tail); (d_in, d_out, m) = (32, 32, 8),
# (40, 24, 8) (K tail against the 16- and 32-wide steps, N tail, dsub 3) and
# (32, 16, 8); 12 lists, ~1500 rows in two shuffled adds; k = 10 (register
# selection) and 40 (LDS selection).
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

from distributed_faiss_amd import Index, IndexCfg  # noqa: E402
from distributed_faiss_amd.hip_engine import HipEngine, HipProvider  # noqa: E402
from gpu_support import (  # noqa: E402
    assert_bitwise as _bitwise,
    assert_lists_equal,
    labels,
    wait_trained as _wait_trained,
)
from oracle import opq  # noqa: E402
from oracle.refine import (  # noqa: E402
    k_prime,
    refine_ref,
)

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
NBITS = [pytest.param(4, id="x4"), pytest.param(8, id="x8")]
SHAPES = [pytest.param(32, 32, 8, id="32to32-m8-rotation_only"),
          pytest.param(40, 24, 8, id="40to24-m8-k_tail-n_tail-dsub3"),
          pytest.param(32, 16, 8, id="32to16-m8-dsub2")]

LIST_SIZES = [0, 1, 2, 3, 5, 63, 64, 65, 127, 129, 385, 643]
NLIST = len(LIST_SIZES)
NROWS = sum(LIST_SIZES)  # 1487
SPLIT = 800
NQ = 130
K_REG, K_LDS = 10, 40
CODEWORD_GAP = 0.05


def _spec(d_in, d_out, m, metric, nbits, **kw):
    s = {"type": "ivfpq", "dim": d_in, "metric": metric, "nlist": NLIST,
         "nprobe": NLIST, "seed": 1234, "m": m, "nbits": nbits, "opq": 1}
    if d_out != d_in:
        s["opq_dim"] = d_out
    return dict(s, **kw)


def _plain_spec(d_out, m, metric, nbits, **kw):
    return dict({"type": "ivfpq", "dim": d_out, "metric": metric,
                 "nlist": NLIST, "nprobe": NLIST, "seed": 1234, "m": m,
                 "nbits": nbits}, **kw)


def _lift(A, y, rng):
    """x (n, d_in) float32 with A x == y exactly, for a signed selection A:
    the selected coordinates carry +-y, the others anything."""
    cols = np.abs(A).argmax(axis=1)
    sign = A[np.arange(A.shape[0]), cols]
    x = rng.standard_normal((y.shape[0], A.shape[1])).astype(np.float32)
    x[:, cols] = y * sign
    return x


# ---------------------------------------------------------------------------
# 1. bit-exact tier
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _exact_case(d_in, d_out, m, metric, nbits):
    """At d_out: centroid + an isolated codeword + 1e-3 noise (the
    GEMM-decomposed engine encode and the sequential restatement then pick
    the same codes), lifted to d_in through the signed selection."""
    ksub = 1 << nbits
    dsub = d_out // m
    rng = np.random.default_rng(7000 + 100 * d_in + d_out + nbits + metric)
    A = opq.signed_selection(d_in, d_out, rng)
    cent = (rng.standard_normal((NLIST, d_out)) * 20.0).astype(np.float32)
    cb = rng.standard_normal((m, ksub, dsub)).astype(np.float32)
    lbl = labels(rng, LIST_SIZES)
    cw = np.empty((NROWS, m), np.int64)
    for j in range(m):
        c64 = cb[j].astype(np.float64)
        gap = np.sqrt(((c64[:, None, :] - c64[None, :, :]) ** 2).sum(-1))
        np.fill_diagonal(gap, np.inf)
        iso = np.flatnonzero(gap.min(axis=1) > CODEWORD_GAP)
        assert iso.size >= 8
        cw[:, j] = rng.choice(iso, NROWS)
    dec = np.concatenate([cb[j][cw[:, j]] for j in range(m)], axis=1)
    yb = (cent[lbl] + dec
          + 1e-3 * rng.standard_normal((NROWS, d_out))).astype(np.float32)
    yq = (cent[rng.integers(0, NLIST, NQ)]
          + 0.7 * rng.standard_normal((NQ, d_out))).astype(np.float32)
    xb, q = _lift(A, yb, rng), _lift(A, yq, rng)
    orc = opq.OracleOPQ(A, NLIST, m, metric, nbits)
    orc.set_trained(cent, cb)
    # the transform is exact on this construction
    np.testing.assert_array_equal(orc.apply(xb), yb)
    np.testing.assert_array_equal(orc.apply(q), yq)
    orc.add(xb[:SPLIT])
    orc.add(xb[SPLIT:])
    np.testing.assert_array_equal(np.diff(orc.lists()[0]), LIST_SIZES)
    return {"A": A, "cent": cent, "cb": cb, "xb": xb, "q": q, "yb": yb,
            "yq": yq, "orc": orc, "res": {}}


def _assert_lists(eng, case):
    assert_lists_equal(eng, case["orc"].inner, LIST_SIZES)


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d_in,d_out,m", SHAPES)
def test_signed_permutation_bitexact(d_in, d_out, m, metric, nbits):
    case = _exact_case(d_in, d_out, m, metric, nbits)
    eng = HipEngine(spec=_spec(d_in, d_out, m, metric, nbits))
    eng.set_transform(case["A"])
    eng.set_trained(case["cent"], case["cb"])
    eng.add(case["xb"][:SPLIT])
    eng.add(case["xb"][SPLIT:])
    plain = HipEngine(spec=_plain_spec(d_out, m, metric, nbits))
    plain.set_trained(case["cent"], case["cb"])
    plain.add(case["yb"][:SPLIT])
    plain.add(case["yb"][SPLIT:])
    np.testing.assert_array_equal(eng.apply_transform(case["q"]), case["yq"])
    _assert_lists(eng, case)
    _assert_lists(plain, case)
    probes, keys = eng.coarse(case["q"], NLIST)
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    pp, pk = plain.coarse(case["yq"], NLIST)
    np.testing.assert_array_equal(pp, probes)
    np.testing.assert_array_equal(pk.view(np.uint32), keys.view(np.uint32))
    Do, Io = case["orc"].search_preassigned(case["q"], probes, keys, K_LDS)
    assert (Io >= 0).all()
    for k in (K_REG, K_LDS):
        _bitwise(*eng.search_preassigned(case["q"], probes, keys, k),
                 Do[:, :k], Io[:, :k])
        _bitwise(*plain.search_preassigned(case["yq"], probes, keys, k),
                 Do[:, :k], Io[:, :k])


# ---------------------------------------------------------------------------
# 2. equivalence on a general rotation
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _rot_case(d_in, d_out, m, metric, nbits):
    ksub = 1 << nbits
    rng = np.random.default_rng(9000 + 100 * d_in + d_out + nbits + metric)
    A = opq.random_rotation(d_in, d_out, rng)
    cent = (rng.standard_normal((NLIST, d_out)) * 2.0).astype(np.float32)
    cb = (0.5 * rng.standard_normal((m, ksub, d_out // m))).astype(np.float32)
    # rows around the centroids pulled back to d_in, plus an off-subspace
    # part that the transform drops when d_out < d_in
    lbl = rng.integers(0, NLIST, NROWS)
    xb = ((cent[lbl] + 0.6 * rng.standard_normal((NROWS, d_out))) @ A
          + 0.3 * rng.standard_normal((NROWS, d_in))).astype(np.float32)
    q = ((cent[rng.integers(0, NLIST, NQ)]
          + 0.6 * rng.standard_normal((NQ, d_out))) @ A
         + 0.3 * rng.standard_normal((NQ, d_in))).astype(np.float32)
    allow = rng.random(NROWS) < 0.3
    return {"A": A, "cent": cent, "cb": cb, "xb": xb, "q": q, "allow": allow}


def _rot_engines(d_in, d_out, m, metric, nbits, nprobe, **kw):
    c = _rot_case(d_in, d_out, m, metric, nbits)
    eng = HipEngine(spec=_spec(d_in, d_out, m, metric, nbits, nprobe=nprobe,
                               **kw))
    eng.set_transform(c["A"])
    eng.set_trained(c["cent"], c["cb"])
    plain = HipEngine(spec=_plain_spec(d_out, m, metric, nbits, nprobe=nprobe))
    plain.set_trained(c["cent"], c["cb"])
    for lo, hi in ((0, SPLIT), (SPLIT, NROWS)):
        eng.add(c["xb"][lo:hi])
        plain.add(eng.apply_transform(c["xb"][lo:hi]))
    return c, eng, plain


@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d_in,d_out,m", SHAPES)
def test_rotation_equals_plain_engine_behind_apply(d_in, d_out, m, metric,
                                                   nbits):
    c, eng, plain = _rot_engines(d_in, d_out, m, metric, nbits, 5)
    yq = eng.apply_transform(c["q"])
    # the lists: same rows, same bytes
    for a, b in zip(eng.get_lists(), plain.get_lists()):
        np.testing.assert_array_equal(a, b)
    probes, keys = eng.coarse(c["q"], 5)
    pp, pk = plain.coarse(yq, 5)
    np.testing.assert_array_equal(probes, pp)
    np.testing.assert_array_equal(keys.view(np.uint32), pk.view(np.uint32))
    for k in (K_REG, K_LDS):
        _bitwise(*eng.search(c["q"], k), *plain.search(yq, k))
        _bitwise(*eng.search_filtered(c["q"], k, c["allow"]),
                 *plain.search_filtered(yq, k, c["allow"]))
        _bitwise(*eng.search_preassigned(c["q"], probes[:, ::-1], keys[:, ::-1], k),
                 *plain.search_preassigned(yq, probes[:, ::-1], keys[:, ::-1], k))
        _bitwise(*eng.search_preassigned_filtered(c["q"], probes, keys, k,
                                                  c["allow"]),
                 *plain.search_preassigned_filtered(yq, probes, keys, k,
                                                    c["allow"]))
    D, I = eng.search(c["q"], K_REG)
    assert (I >= 0).all()


@pytest.mark.parametrize("refine", ["fp32", "fp16"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d_in,d_out,m", SHAPES)
def test_refine_on_top_reranks_the_original_vectors(d_in, d_out, m, metric,
                                                    refine):
    nbits = 8 if refine == "fp32" else 4
    c, eng, plain = _rot_engines(d_in, d_out, m, metric, nbits, 5,
                                 refine=refine, k_factor=4)
    kind, stride, rows = eng.refine_info()
    T = np.float32 if refine == "fp32" else np.float16
    # the raw store is d_in wide and holds the rows as they arrived
    assert rows == NROWS and stride == (d_in * T().itemsize + 15) // 16 * 16
    store = c["xb"].astype(T)
    got = eng.get_refine_rows()[:, :d_in * T().itemsize]
    np.testing.assert_array_equal(got, store.view(np.uint8).reshape(NROWS, -1))
    yq = eng.apply_transform(c["q"])
    for k in (K_REG, K_LDS):
        _Dc, cand = plain.search(yq, k_prime(k, 4))
        Dr, Ir = refine_ref(c["q"], store, cand, k, metric)
        _bitwise(*eng.search(c["q"], k), Dr, Ir)
    k = K_REG
    _Dc, cand = plain.search_filtered(yq, k_prime(k, 4), c["allow"])
    _bitwise(*eng.search_filtered(c["q"], k, c["allow"]),
             *refine_ref(c["q"], store, cand, k, metric))
    # reconstruct on a refine index: the stored d_in rows
    D, I, R = eng.search_and_reconstruct(c["q"], k)
    assert R.shape == (NQ, k, d_in)
    np.testing.assert_array_equal(R, store.astype(np.float32)[I])


def test_graph_capture_replays_equal_eager():
    c, eng, _plain = _rot_engines(40, 24, 8, L2, 8, 5, refine="fp32",
                                  k_factor=4)
    k = K_REG
    qt = torch.as_tensor(c["q"]).cuda()
    D = torch.empty((NQ, k), dtype=torch.float32, device="cuda")
    I = torch.empty((NQ, k), dtype=torch.int64, device="cuda")
    eng.search_dev(qt, k, D, I)  # warm-up sizes every workspace
    torch.cuda.synchronize()
    De, Ie = D.cpu().numpy(), I.cpu().numpy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.search_dev(qt, k, D, I)
    D.zero_()
    I.zero_()
    g.replay()
    torch.cuda.synchronize()
    _bitwise(D.cpu().numpy(), I.cpu().numpy(), De, Ie)


# ---------------------------------------------------------------------------
# 3. transform values
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("d_in,d_out,m", SHAPES)
def test_apply_transform_values_and_batch_independence(d_in, d_out, m):
    c, eng, plain = _rot_engines(d_in, d_out, m, L2, 8, NLIST)
    q = c["q"]
    y = eng.apply_transform(q)
    assert y.shape == (NQ, d_out) and y.dtype == np.float32
    err = np.abs(y.astype(np.float64) - opq.transform64(c["A"], q))
    assert (err <= opq.transform_bound(c["A"], q)).all(), err.max()
    # one 130-row call == 130 one-row calls == rows inside another batch
    rows = np.concatenate([eng.apply_transform(q[i:i + 1]) for i in range(NQ)])
    np.testing.assert_array_equal(rows.view(np.uint32), y.view(np.uint32))
    shifted = eng.apply_transform(np.concatenate([q[61:], q[:61]]))
    np.testing.assert_array_equal(
        np.concatenate([shifted[NQ - 61:], shifted[:NQ - 61]]).view(np.uint32),
        y.view(np.uint32))
    # reconstruct: A^T . decode, d_in wide
    k = K_REG
    D, I, R = eng.search_and_reconstruct(q, k)
    Dp, Ip, Rp = plain.search_and_reconstruct(y, k)
    _bitwise(D, I, Dp, Ip)
    assert R.shape == (NQ, k, d_in) and Rp.shape == (NQ, k, d_out)
    A64 = c["A"].astype(np.float64)
    want = Rp.astype(np.float64) @ A64
    bound = 1e-4 * (np.abs(Rp.astype(np.float64)) @ np.abs(A64)) + 1e-4
    assert (np.abs(R - want) <= bound).all()
    # ... and both batch shapes of the reconstruct agree bitwise
    D1, I1, R1 = eng.search_and_reconstruct(q[:1], k)
    _bitwise(D1, I1, D[:1], I[:1])
    np.testing.assert_array_equal(R1[0].view(np.uint32), R[0].view(np.uint32))


def test_transform_is_fp32_whatever_coarse_bf16_says():
    c, eng, _plain = _rot_engines(40, 24, 8, L2, 8, NLIST)
    eng2 = HipEngine(spec=_spec(40, 24, 8, L2, 8, coarse_bf16=1))
    eng2.set_transform(c["A"])
    np.testing.assert_array_equal(
        eng2.apply_transform(c["q"]).view(np.uint32),
        eng.apply_transform(c["q"]).view(np.uint32))


def test_transform_counts_under_gemm_timing():
    c, eng, _plain = _rot_engines(40, 24, 8, L2, 8, NLIST)
    eng.set_timing(True)
    eng.get_timing()
    eng.apply_transform(c["q"])
    t = eng.get_timing()
    assert t["gemm_flops"] == 2 * NQ * 40 * 24 and t["gemm_ms"] > 0
    eng.search(c["q"], K_REG)
    t = eng.get_timing()
    # the transform + the coarse GEMM at d_out
    assert t["gemm_flops"] == 2 * NQ * 40 * 24 + 2 * NQ * NLIST * 24
    eng.set_timing(False)


# ---------------------------------------------------------------------------
# 4. training
# ---------------------------------------------------------------------------

TRAIN_KW = dict(type="ivfpq", dim=32, metric=L2, nlist=NLIST, nprobe=4,
                seed=1234, m=8, nbits=4, opq=1, opq_niter=8)


@functools.lru_cache(maxsize=None)
def _train(zero_col=None, d_out=32):
    spec = dict(TRAIN_KW)
    if d_out != 32:
        spec["opq_dim"] = d_out
    eng = HipEngine(spec=spec)
    eng.train(opq.recipe(zero_col))
    assert eng.is_trained
    return eng, eng.get_transform()


@functools.lru_cache(maxsize=None)
def _ref_dev(zero_col=None, d_out=32, niter=2):
    """max|A A^T - I| of the SVD-polar reference rotation after its single
    rounding to float32 (the figure does not depend on niter)."""
    A = opq.opq_train(opq.recipe(zero_col), 8, 16, d_out=d_out,
                          niter=niter)
    return opq.ortho_dev(A.astype(np.float32))


def _check_orthonormal(A, x, ref_dev):
    dev = opq.ortho_dev(A)
    print(f"max|AA^T - I|: engine {dev:.3e}, fp32-rounded reference "
          f"{ref_dev:.3e}")
    # x 8: iteration round-off against a single rounding
    assert dev <= 8 * ref_dev
    if A.shape[0] == A.shape[1]:
        v = x.astype(np.float64)
        n2 = (v * v).sum(axis=1)
        a2 = ((v @ A.astype(np.float64).T) ** 2).sum(axis=1)
        assert (np.abs(a2 - n2) <= 1e-4 * n2).all()


def test_trained_rows_are_orthonormal():
    _eng, A = _train()
    assert A.shape == (32, 32) and A.dtype == np.float32
    _check_orthonormal(A, opq.recipe(), _ref_dev(niter=8))


def test_trained_rotation_halves_the_quantization_error():
    _eng, A = _train()
    xc = opq.centred(opq.recipe())
    plain = opq.pq_mse(xc, 8, 16)
    rot = opq.pq_mse(opq.transform(A, xc), 8, 16)
    Aref = opq.opq_train(opq.recipe(), 8, 16, niter=8)
    ref = opq.pq_mse(opq.transform(Aref.astype(np.float32), xc), 8, 16)
    print(f"PQ mse: plain {plain:.2f}, engine OPQ {rot:.2f} "
          f"({rot / plain:.3f}), reference OPQ {ref:.2f} ({ref / plain:.3f})")
    assert rot <= 0.5 * plain


def test_training_is_deterministic():
    _eng, A = _train()
    eng2 = HipEngine(spec=dict(TRAIN_KW))
    eng2.train(opq.recipe())
    np.testing.assert_array_equal(eng2.get_transform().view(np.uint32),
                                  A.view(np.uint32))
    # the inner index was trained on the transformed rows, equally
    np.testing.assert_array_equal(eng2.get_centroids(), _eng.get_centroids())
    np.testing.assert_array_equal(eng2.get_codebooks(), _eng.get_codebooks())


def test_training_on_rank_deficient_rows():
    x = opq.recipe(zero_col=5)
    assert not x[:, 5].any()
    _eng, A = _train(zero_col=5)
    _check_orthonormal(A, x, _ref_dev(zero_col=5))


def test_training_with_reduced_dim():
    eng, A = _train(d_out=16)
    assert A.shape == (16, 32)
    assert eng.transform_info() == (1, 32, 16)
    _check_orthonormal(A, opq.recipe(), _ref_dev(d_out=16))
    assert eng.get_centroids().shape == (NLIST, 16)
    assert eng.get_codebooks().shape == (8, 16, 2)


def test_trained_index_searches_like_plain_behind_apply():
    eng, _A = _train()
    x = opq.recipe()[:1500]
    if eng.ntotal == 0:
        eng.add(x)
    plain = HipEngine(spec={k: v for k, v in TRAIN_KW.items()
                            if not k.startswith("opq")})
    plain.set_trained(eng.get_centroids(), eng.get_codebooks())
    plain.add(eng.apply_transform(x))
    q = x[::11][:NQ]
    _bitwise(*eng.search(q, K_REG), *plain.search(eng.apply_transform(q), K_REG))


def test_injected_transform_survives_train():
    c = _rot_case(32, 16, 8, L2, 4)
    eng = HipEngine(spec=_spec(32, 16, 8, L2, 4))
    eng.set_transform(c["A"])
    eng.train(c["xb"])
    np.testing.assert_array_equal(eng.get_transform(), c["A"])
    assert eng.is_trained and eng.get_centroids().shape == (NLIST, 16)


# ---------------------------------------------------------------------------
# 5. persistence and surface
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kw", [{}, {"refine": "fp16", "k_factor": 3}],
                         ids=["plain", "refine"])
def test_save_load_round_trip(tmp_path, kw):
    c, eng, _plain = _rot_engines(40, 24, 8, IP, 4, 5, **kw)
    p = str(tmp_path / "opq.dfann")
    eng.save(p)
    e2 = HipProvider().load(p)
    assert e2.d == 40 and e2.transform_info() == (1, 40, 24)
    assert e2.ntotal == NROWS and e2.is_trained
    np.testing.assert_array_equal(e2.get_transform(), c["A"])
    np.testing.assert_array_equal(e2.get_centroids(), c["cent"])
    for k in (K_REG, K_LDS):
        _bitwise(*e2.search(c["q"], k), *eng.search(c["q"], k))
    # a loaded index keeps growing behind the same transform
    e2.add(c["xb"][:7])
    eng.add(c["xb"][:7])
    _bitwise(*e2.search(c["q"], K_REG), *eng.search(c["q"], K_REG))


def test_file_without_opq_loads_as_before(tmp_path):
    c, _eng, plain = _rot_engines(40, 24, 8, L2, 8, 5)
    p = str(tmp_path / "plain.dfann")
    plain.save(p)
    # byte layout: magic, spec, header, trained flag, ntotal, centroids,
    # codebooks, then the lists — nothing between codebooks and lists
    size = os.path.getsize(p)
    spec_len = len(plain.lib.dfann_spec_json(plain.h))
    off, ids, codes = plain.get_lists()
    assert size == (16 + spec_len + 32 + 1 + 8 + NLIST * 24 * 4
                    + 8 * 256 * 3 * 4 + (NLIST + 1) * 8 + NROWS * 8
                    + codes.size)
    e2 = HipProvider().load(p)
    assert e2.transform_info() == (0, 24, 24) and e2.d == 24
    yq = _eng.apply_transform(c["q"])
    _bitwise(*e2.search(yq, K_REG), *plain.search(yq, K_REG))
    with pytest.raises(RuntimeError, match="no opq transform"):
        e2.get_transform()


def test_surface_and_errors():
    c = _rot_case(40, 24, 8, L2, 8)
    eng = HipEngine(spec=_spec(40, 24, 8, L2, 8))
    assert eng.d == 40 and eng.d_inner == 24
    assert eng.transform_info() == (1, 40, 24)
    with pytest.raises(RuntimeError, match="transform not set"):
        eng.get_transform()
    with pytest.raises(RuntimeError, match="transform not set"):
        eng.apply_transform(c["q"])
    with pytest.raises(RuntimeError, match="dfann_set_transform"):
        eng.set_trained(c["cent"], c["cb"])
    with pytest.raises(ValueError, match="transform: expected shape"):
        eng.set_transform(c["A"].T)
    eng.set_transform(c["A"])
    np.testing.assert_array_equal(eng.get_transform(), c["A"])
    eng.set_trained(c["cent"], c["cb"])
    assert eng.get_centroids().shape == (NLIST, 24)
    assert eng.get_codebooks().shape == (8, 256, 3)
    eng.add(c["xb"][:10])
    with pytest.raises(RuntimeError, match="already holds vectors"):
        eng.set_transform(c["A"])
    with pytest.raises(ValueError, match="apply_transform"):
        eng.apply_transform(c["q"][:, :24])
    plain = HipEngine(spec=_plain_spec(24, 8, L2, 8))
    assert plain.transform_info() == (0, 24, 24)
    for call in (plain.get_transform, lambda: plain.set_transform(np.eye(24)),
                 lambda: plain.apply_transform(c["q"][:, :24])):
        with pytest.raises(RuntimeError, match="no opq transform"):
            call()
    for bad, key in (({"type": "ivfsq"}, "opq"), ({"opq_dim": 48}, "opq_dim"),
                     ({"opq_dim": 20}, "opq_dim"),
                     ({"pq_precomputed": 1}, "pq_precomputed")):
        with pytest.raises(RuntimeError, match=key):
            HipEngine(spec=dict(_spec(40, 24, 8, L2, 8), **bad))


def _clustered(seed, n=1500, d=32):
    rng = np.random.default_rng(seed)
    cent = 4.0 * rng.standard_normal((NLIST, d))
    xb = (cent[rng.integers(0, NLIST, n)]
          + rng.standard_normal((n, d))).astype(np.float32)
    q = (xb[::13][:32] + 0.01 * rng.standard_normal((32, d))).astype(np.float32)
    return xb, q


@pytest.mark.parametrize("factory,info,refine", [
    ("OPQ8_16,IVF12,PQ8", (1, 32, 16), False),
    ("OPQ8,IVF12,PQ8x4,RFlat", (1, 32, 32), True)])
def test_index_end_to_end(tmp_path, factory, info, refine):
    xb, q = _clustered(31)
    n = len(xb)
    meta = [("doc", i % 4, i) for i in range(n)]
    cfg = IndexCfg(faiss_factory=factory, dim=32, metric="l2", nprobe=NLIST,
                   train_num=n, index_storage_dir=str(tmp_path), opq_niter=3,
                   k_factor=52)
    idx = Index(cfg, provider=HipProvider())
    idx.add_batch(xb, meta, train_async_if_triggered=False)
    _wait_trained(idx, n)
    eng = idx.engine
    assert eng.transform_info() == info and eng.d == 32
    assert opq.ortho_dev(eng.get_transform()) < 1e-5
    assert idx.get_centroids().shape == (NLIST, info[2])
    scores, ids, metas, _ = idx.search_full(q, 10)
    assert [[m[2] for m in row] for row in metas] == ids.tolist()
    if refine:
        # k' = 512 exact re-ranks over the original vectors: a query 0.01
        # away from row 13 i has it first (PQ error cannot push the row out
        # of the best 512 of 1500)
        assert (ids[:, 0] == np.arange(32) * 13).all()
    else:
        plain = HipEngine(spec={k: v for k, v in eng.spec.items()
                                if not k.startswith("opq")} | {"dim": 16})
        plain.set_trained(eng.get_centroids(), eng.get_codebooks())
        plain.add(eng.apply_transform(xb))
        _bitwise(scores, ids, *plain.search(eng.apply_transform(q), 10))
    fs, fi, fm, _ = idx.search_filtered(q, 10, 1, 2)
    allow = np.array([m[1] != 2 for m in meta])
    _bitwise(fs, fi, *eng.search_filtered(q, 10, allow))
    assert all(m[1] != 2 for row in fm for m in row)
    # save -> load -> search
    assert idx.save()
    idx2 = Index.from_storage_dir(str(tmp_path), provider=HipProvider())
    assert idx2.engine.transform_info() == info
    np.testing.assert_array_equal(idx2.engine.get_transform(),
                                  eng.get_transform())
    s2, i2, m2, _ = idx2.search_full(q, 10)
    _bitwise(s2, i2, scores, ids)
    assert m2 == metas
    # return_embeddings: d_in wide rows
    _s, _m, embs = idx.search(q, 3, return_embeddings=True)
    assert np.asarray(embs).shape == (32, 3, 32)


@pytest.mark.parametrize("factory", ["OPQ8_16,IVF12,PQ8",
                                     "OPQ8,IVF12,PQ8x4,RFlat"])
def test_client_end_to_end(tmp_path, factory):
    from distributed_faiss_amd import IndexClient, IndexServer, IndexState

    xb, q = _clustered(32)
    n = len(xb)
    prov = HipProvider()
    srvs = [IndexServer(i, str(tmp_path), provider=prov) for i in range(2)]
    cli = IndexClient(servers=srvs)
    cfg = IndexCfg(faiss_factory=factory, dim=32, metric="l2", nprobe=NLIST,
                   train_num=500, opq_niter=3, k_factor=52)
    cli.create_index("o", cfg)
    for lo in range(0, n, 250):
        cli.add_index_data("o", xb[lo:lo + 250],
                           [("a" if i % 2 else "b", i)
                            for i in range(lo, lo + 250)],
                           train_async_if_triggered=False)
    cli.sync_train("o")
    import time

    for _ in range(3000):
        if (cli.get_state("o") == IndexState.TRAINED
                and cli.get_ntotal("o") == n):
            break
        time.sleep(0.01)
    assert cli.get_ntotal("o") == n
    for c in cli.get_centroids("o"):
        assert np.asarray(c).shape[0] == NLIST
    scores, metas = cli.search(q, 10, "o")
    assert scores.shape == (32, 10) and (np.diff(scores, axis=1) >= 0).all()
    assert all(m is not None for row in metas for m in row)
    if factory.endswith("RFlat"):
        # exact re-rank over each shard's rows: the near-copy comes first
        assert [row[0][1] for row in metas] == [13 * i for i in range(32)]
    fs, fm = cli.search_with_filter(q, 10, "o", filter_pos=0, filter_value="a")
    assert all(m[0] != "a" for row in fm for m in row if m is not None)
    es, em = cli.search_filtered(q, 10, "o", 0, "a")
    assert all(m is not None and m[0] != "a" for row in em for m in row)
    assert (np.diff(es, axis=1) >= 0).all()
