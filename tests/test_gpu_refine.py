# GPU: the exact re-ranking stage (refine) over IVFPQ / IVFSQ.
#
# Reference everywhere: the CPU oracle's base-stage search at k' over the
# SAME probe lists and coarse keys the engine derives (the oracle's own IP
# bias differs from the coarse GEMM's in the last bits; feeding it the
# engine's keys is what keeps the base stage bitwise, as in
# test_gpu_filtered), followed by oracle/refine.py over xb in the stored
# type. The base stages are bit-exact and the refine order is defined, so D
# and I are compared BITWISE.
#
# Data: test_gpu_filtered's bit-exact setup — d=32, nlist=8, clustered /
# codeword-exact rows, artifacts shared through set_trained, 3187 rows
# added in two batches.
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
from distributed_faiss_amd.index_cfg import IndexCfg  # noqa: E402
from oracle import make_oracle_engine  # noqa: E402
from gpu_support import assert_bitwise as _bitwise  # noqa: E402
from oracle.refine import (  # noqa: E402
    refine_ref,
)
from test_gpu_filtered import (  # noqa: E402
    _allow, _clustered, _data, _engine as _build, _masked_ref, _oracle, _pad,
    _rand, _wait_trained)

IP, L2 = 0, 1
NTOTAL, NLIST = 3187, 8
SPLIT = 1700
CFGS = [("ivfpq", None), ("ivfsq", "8bit"), ("ivfsq", "fp16")]
CFG_IDS = ["pq8", "sq8", "sqfp16"]
REFINES = ["fp32", "fp16"]
STORE_T = {"fp32": np.float32, "fp16": np.float16}
# (k, k_factor, k')
K_CASES = [(10, 1, 10), (10, 1.6, 16), (10, 1.7, 17), (10, 4, 40), (1, 1, 1),
           (40, 13, 512)]


class _Case:
    """One base index kind on one data set: the oracle, the queries and a
    cache of the oracle's base-stage candidates per (nprobe, k')."""

    def __init__(self, spec, art, xb, q):
        self.spec, self.art, self.xb, self.q = spec, art, xb, q
        self.metric = spec["metric"]
        self.orc = _oracle(spec, art, xb)
        self.plain = _build(spec, art, [xb])  # unrefined twin, coarse source
        self._coarse, self._cand, self._eng = {}, {}, {}

    def coarse(self, nprobe):
        if nprobe not in self._coarse:
            self._coarse[nprobe] = self.plain.coarse(self.q, nprobe)
        return self._coarse[nprobe]

    def cand(self, nprobe, kp):
        if (nprobe, kp) not in self._cand:
            probes, keys = self.coarse(nprobe)
            _D, I = self.orc.search_preassigned(self.q, probes, keys, kp)
            I.setflags(write=False)
            self._cand[(nprobe, kp)] = I
        return self._cand[(nprobe, kp)]

    def engine(self, refine, split=SPLIT):
        if refine not in self._eng:
            self._eng[refine] = _build(
                dict(self.spec, refine=refine), self.art,
                [self.xb[:split], self.xb[split:]])
        return self._eng[refine]

    def ref(self, refine, nprobe, kp, k):
        store = self.xb.astype(STORE_T[refine])
        return refine_ref(self.q, store, self.cand(nprobe, kp), k, self.metric)


@functools.lru_cache(maxsize=None)
def _case(typ, sq_type, metric):
    return _Case(*_data(typ, metric, sq_type))


@functools.lru_cache(maxsize=None)
def _sparse_case(typ, sq_type, metric):
    """The same rows thinned so that one list keeps 25 rows, one 5 and one
    none, with one query aimed at each: at nprobe=1 the base stage returns
    fewer than k' — and fewer than k, or zero — candidates."""
    spec, art, xb, _q = _data(typ, metric, sq_type)
    full = _oracle(spec, art, xb)
    sizes = [len(l) for l in full.list_ids]
    big = np.argsort(sizes)[::-1]
    # thin three lists that are populated in the full set
    l25, l5, l0 = (int(b) for b in big[:3])
    keep = np.ones(len(xb), bool)
    keep[np.asarray(full.list_ids[l25])[25:]] = False
    keep[np.asarray(full.list_ids[l5])[5:]] = False
    keep[np.asarray(full.list_ids[l0])] = False
    xs = np.ascontiguousarray(xb[keep])
    rng = np.random.default_rng(77)
    cent = art["cent"]
    q = np.concatenate([
        cent[[l25, l5, l0]] + 0.01 * rng.standard_normal((3, cent.shape[1])),
        xs[::301][:5]]).astype(np.float32)
    case = _Case(spec, art, xs, q)
    probes, _keys = case.coarse(1)
    assert probes[:3, 0].tolist() == [l25, l5, l0]
    assert [len(case.orc.list_ids[l]) for l in (l25, l5, l0)] == [25, 5, 0]
    return case


# ---------------------------------------------------------------------------
# pipeline parity
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_pipeline_parity(cfg, refine, metric):
    c = _case(cfg[0], cfg[1], metric)
    eng = c.engine(refine)
    assert eng.ntotal == NTOTAL
    assert eng.refine_info() == (1 if refine == "fp32" else 2,
                                 128 if refine == "fp32" else 64, NTOTAL)
    for nprobe in (NLIST, 1):
        eng.nprobe = nprobe
        for k, kf, kp in K_CASES:
            eng.k_factor = kf
            D, I = eng.search(c.q, k)
            Dr, Ir = c.ref(refine, nprobe, kp, k)
            _bitwise(D, I, Dr, Ir)
            if nprobe == NLIST:
                assert (I >= 0).all()
        # one probed list of ~400 rows < 512: the base stage padded
        assert (c.cand(1, 512) == -1).any()


def test_l2_reference_is_the_oracles_own_search():
    # for L2 no coarse key enters a distance: the candidates used above ARE
    # oracle.search(q, k')
    c = _case("ivfpq", None, L2)
    for nprobe, kp in ((NLIST, 40), (1, 512)):
        c.orc.nprobe = nprobe
        _D, I = c.orc.search(c.q, kp)
        np.testing.assert_array_equal(I, c.cand(nprobe, kp))
    c.orc.nprobe = NLIST


@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_pipeline_short_lists_carry_pads(cfg, refine, metric):
    c = _sparse_case(cfg[0], cfg[1], metric)
    eng = c.engine(refine, split=len(c.xb) // 2)
    eng.nprobe = 1
    for k, kf, kp in ((10, 1, 10), (10, 4, 40), (40, 13, 512)):
        eng.k_factor = kf
        D, I = eng.search(c.q, k)
        Dr, Ir = c.ref(refine, 1, kp, k)
        _bitwise(D, I, Dr, Ir)
        # query 0 probes 25 rows, query 1 five, query 2 an empty list
        assert (I[0] >= 0).sum() == min(k, 25)
        assert (I[1] >= 0).sum() == 5 and (I[1, 5:] == -1).all()
        assert (I[2] == -1).all() and (D[2] == _pad(metric)).all()
        assert (D[1, 5:] == _pad(metric)).all()


# ---------------------------------------------------------------------------
# the refine kernel alone, at the d that break lanes
# ---------------------------------------------------------------------------


def _wild(n, d, seed):
    """Four decades, both signs, exact zeros, one value above the fp16 max."""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.uniform(-2, 2, (n, d))
         * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32)
    x[rng.random((n, d)) < 0.05] = 0.0
    x[7, d // 2] = 70000.0
    return x


# 10 is not in the issue's list: d % 4 != 0 pads fp32 rows (strided append)
@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("d", [20, 128, 136, 200, 768, 10])
def test_refine_kernel_dims(d, refine, metric):
    n, nlist, k, kp = 600, 4, 10, 40
    xb = _wild(n, d, 40 + d)
    rng = np.random.default_rng(d)
    q = (xb[[7, 3, 100, 250, 411, 599]]
         * (1 + 0.05 * rng.standard_normal((6, d)))).astype(np.float32)
    q[:, d // 2] = np.where(q[:, d // 2] == 0, 1.0, q[:, d // 2])
    art = {"cent": (0.5 * rng.standard_normal((nlist, d))).astype(np.float32),
           "vmin": np.full(d, -100.0, np.float32),
           "vdiff": np.full(d, 200.0, np.float32)}
    spec = {"type": "ivfsq", "sq_type": "8bit", "dim": d, "metric": metric,
            "nlist": nlist, "nprobe": nlist, "seed": 9}
    eng = _build(dict(spec, refine=refine, k_factor=4), art, [xb[:333], xb[333:]])
    orc = _oracle(spec, art, xb)
    probes, keys = eng.coarse(q, nlist)
    _D, cand = orc.search_preassigned(q, probes, keys, kp)
    T = STORE_T[refine]
    with np.errstate(over="ignore"):
        store = xb.astype(T)
    if refine == "fp16":
        assert np.isinf(store[7, d // 2])
    D, I = eng.search(q, k)
    Dr, Ir = refine_ref(q, store, cand, k, metric)
    _bitwise(D, I, Dr, Ir)
    # the row holding the large value is a candidate of its own query; as
    # fp16 it is inf: last of the 40 under L2, first (dot = +inf) under IP
    assert 7 in cand[0]
    if refine == "fp16" and metric == L2:
        assert 7 not in I[0]
        assert np.isinf(refine_ref(q[:1], store, np.array([[7]]), 1, L2)[0][0, 0])
    if refine == "fp16" and metric == IP:
        assert I[0, 0] == 7 and D[0, 0] == np.inf
    # the store, byte for byte: rows in arrival order, zero pad bytes
    kind, stride, rows = eng.refine_info()
    assert rows == n and stride == (d * T().itemsize + 15) // 16 * 16
    want = np.zeros((n, stride), np.uint8)
    want[:, :d * T().itemsize] = store.view(np.uint8).reshape(n, -1)
    np.testing.assert_array_equal(eng.get_refine_rows(), want)
    np.testing.assert_array_equal(eng.get_refine_rows(330, 7), want[330:337])


# ---------------------------------------------------------------------------
# exactness end to end
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
def test_exact_when_every_row_is_a_candidate(metric):
    n, d, k = 500, 32, 10
    xb, q = _rand(n, d, 21), _rand(16, d, 22)
    cfg = IndexCfg(faiss_factory="IVF8,PQ8,RFlat", dim=d,
                   metric="l2" if metric == L2 else "dot", nprobe=8,
                   k_factor=52)
    from distributed_faiss_amd.engine_spec import resolve_engine_spec
    spec = resolve_engine_spec(cfg, n)
    assert spec["refine"] == "fp32" and spec["k_factor"] == 52.0
    eng = HipEngine(spec=spec)
    eng.train(xb)
    eng.add(xb)
    D, I = eng.search(q, k)  # k' = 512 >= n, all lists probed
    q64, x64 = q.astype(np.float64), xb.astype(np.float64)
    ref = q64 @ x64.T if metric == IP else \
        ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
    key = -ref if metric == IP else ref
    order = np.argsort(key, axis=1, kind="stable")
    tol = 1e-4 * np.abs(ref) + 1e-4
    for i in range(len(q)):
        r = ref[i, I[i]]
        assert (np.abs(D[i] - r) <= 1e-4 * np.abs(r) + 1e-4).all()
        sk = key[i, order[i]]
        for j in range(k):
            t = tol[i, order[i, j]]
            if (j == 0 or sk[j] - sk[j - 1] > 2 * t) and sk[j + 1] - sk[j] > 2 * t:
                assert I[i, j] == order[i, j]


# ---------------------------------------------------------------------------
# k_factor = 1: same candidates, new order
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_k_factor_1_keeps_the_id_set(cfg, metric):
    c = _case(cfg[0], cfg[1], metric)
    plain = _build(c.spec, c.art, [c.xb[:SPLIT], c.xb[SPLIT:]])
    eng = c.engine("fp32")
    eng.nprobe = NLIST
    eng.k_factor = 1
    for k in (10, 40):
        _D0, I0 = plain.search(c.q, k)
        _D1, I1 = eng.search(c.q, k)
        np.testing.assert_array_equal(np.sort(I0, axis=1), np.sort(I1, axis=1))


# ---------------------------------------------------------------------------
# growth across slabs
# ---------------------------------------------------------------------------


def test_growth_across_slab_boundary():
    d, nlist, k, kp = 128, 4, 10, 40
    cent, xb = _clustered(nlist, 1500, d, seed=31)
    art = {"cent": cent, "vmin": np.full(d, -2.0, np.float32),
           "vdiff": np.full(d, 4.0, np.float32)}
    spec = {"type": "ivfsq", "sq_type": "8bit", "dim": d, "metric": L2,
            "nlist": nlist, "nprobe": nlist, "seed": 5}
    q = (xb[[10, 2999, 3000, 4500, 5999]]
         + 0.01 * _rand(5, d, 32)).astype(np.float32)
    eng = _build(dict(spec, refine="fp16", k_factor=4, refine_slab_mb=1), art,
                 [xb[:3000]])
    assert eng.refine_info() == (2, 256, 3000)  # 4096 rows per 1 MB slab

    def check(n):
        orc = _oracle(spec, art, xb[:n])
        probes, keys = eng.coarse(q, nlist)
        _D, cand = orc.search_preassigned(q, probes, keys, kp)
        D, I = eng.search(q, k)
        Dr, Ir = refine_ref(q, xb[:n].astype(np.float16), cand, k, L2)
        _bitwise(D, I, Dr, Ir)
        return I

    check(3000)
    eng.add(xb[3000:])  # rows 3000..5999: crosses row 4096 into slab 2
    assert eng.refine_info() == (2, 256, 6000)
    I = check(6000)
    assert (I >= 4096).any(), "no result from the second slab"
    np.testing.assert_array_equal(
        eng.get_refine_rows(4090, 12),
        xb[4090:4102].astype(np.float16).view(np.uint8).reshape(12, -1))


# ---------------------------------------------------------------------------
# filtered / preassigned entries
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("filt", ["MOD3", "SPARSE"])
@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("cfg", CFGS[:2], ids=CFG_IDS[:2])
def test_filtered_and_preassigned_entries(cfg, metric, filt):
    c = _case(cfg[0], cfg[1], metric)
    eng = c.engine("fp16")
    eng.nprobe = NLIST
    eng.k_factor = 4
    k, kp = 10, 40
    store = c.xb.astype(np.float16)
    probes, keys = c.coarse(NLIST)
    Dfull, Ifull = c.orc.search_preassigned(c.q, probes, keys, NTOTAL)
    allow = _allow(filt, NTOTAL)
    _Dm, Im = _masked_ref(Dfull, Ifull, allow, kp, metric)
    Dr, Ir = refine_ref(c.q, store, Im, k, metric)
    if filt == "SPARSE":
        assert (Im == -1).any()  # 33 allowed rows < k'
    _bitwise(*eng.search_filtered(c.q, k, allow), Dr, Ir)
    _bitwise(*eng.search_preassigned_filtered(c.q, probes, keys, k, allow),
             Dr, Ir)
    assert allow[Ir[Ir >= 0]].all()
    Du, Iu = c.ref("fp16", NLIST, kp, k)
    _bitwise(*eng.search_preassigned(c.q, probes, keys, k), Du, Iu)


# ---------------------------------------------------------------------------
# reconstruct
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("refine", REFINES)
def test_reconstruct_returns_stored_rows(refine):
    c = _sparse_case("ivfpq", None, L2)
    eng = c.engine(refine, split=len(c.xb) // 2)
    eng.nprobe = 1
    eng.k_factor = 4
    k = 10
    D, I, R = eng.search_and_reconstruct(c.q, k)
    Dr, Ir = c.ref(refine, 1, 40, k)
    _bitwise(D, I, Dr, Ir)
    assert (I == -1).any() and (I >= 0).any()
    want = c.xb.astype(STORE_T[refine]).astype(np.float32)[np.maximum(I, 0)]
    want[I < 0] = 0.0
    np.testing.assert_array_equal(R.view(np.uint32), want.view(np.uint32))
    if refine == "fp32":  # the raw vector, not the PQ decode
        np.testing.assert_array_equal(R[I >= 0], c.xb[I[I >= 0]])


# ---------------------------------------------------------------------------
# persistence
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("refine", REFINES)
def test_save_load_add_search(refine, tmp_path):
    c = _case("ivfpq", None, L2)
    k, kp = 10, 40
    eng = _build(dict(c.spec, refine=refine, k_factor=4), c.art, [c.xb[:SPLIT]])
    D0, I0 = eng.search(c.q, k)
    rows0 = eng.get_refine_rows()
    path = str(tmp_path / "refine.dfann")
    eng.save(path)
    eng2 = HipProvider().load(path)
    assert eng2.spec["refine"] == refine and eng2.k_factor == 4.0
    assert eng2.refine_info() == eng.refine_info()
    np.testing.assert_array_equal(eng2.get_refine_rows(), rows0)
    _bitwise(*eng2.search(c.q, k), D0, I0)
    # load, then add, then search: the full index of the parity tests
    eng2.add(c.xb[SPLIT:])
    _bitwise(*eng2.search(c.q, k), *c.ref(refine, NLIST, kp, k))
    # a file cut inside the refine payload is refused with a clear message
    size = os.path.getsize(path)
    cut = str(tmp_path / "cut.dfann")
    with open(path, "rb") as f, open(cut, "wb") as g:
        g.write(f.read(size - eng.refine_info()[1] * 3 - 5))
    with pytest.raises(RuntimeError, match="truncated inside the refine payload"):
        HipProvider().load(cut)


def test_plain_index_round_trips_unchanged(tmp_path):
    c = _case("ivfpq", None, L2)
    path = str(tmp_path / "plain.dfann")
    c.plain.save(path)
    # no refine payload: the file ends with the CSR code rows
    off, _ids, codes = c.plain.get_lists()
    with open(path, "rb") as f:
        blob = f.read()
    assert blob[:8] == b"DFANN01\x00"
    assert blob.endswith(codes.tobytes())
    eng = HipProvider().load(path)
    assert eng.refine_info() == (0, 0, 0)
    _bitwise(*eng.search(c.q, 10), *c.plain.search(c.q, 10))
    with pytest.raises(RuntimeError, match="no refine stage"):
        eng.k_factor = 2


# ---------------------------------------------------------------------------
# setters
# ---------------------------------------------------------------------------


def test_set_k_factor_changes_kprime_without_rebuild():
    c = _case("ivfsq", "8bit", L2)
    eng = c.engine("fp32")
    eng.nprobe = NLIST
    for kf, kp in ((1, 10), (4, 40), (1.6, 16), (1, 10)):
        eng.k_factor = kf
        assert eng.k_factor == kf
        _bitwise(*eng.search(c.q, 10), *c.ref("fp32", NLIST, kp, 10))
    assert not np.array_equal(c.ref("fp32", NLIST, 10, 10)[1],
                              c.ref("fp32", NLIST, 40, 10)[1])
    with pytest.raises(RuntimeError, match="k_factor"):
        eng.k_factor = 0.5
    assert eng.k_factor == 1


def test_index_and_client_set_k_factor(tmp_path):
    from distributed_faiss_amd import IndexClient, IndexServer

    d = 32
    _cent, xb = _clustered(8, 400, d, seed=10)
    xb = xb[:2400]
    q = (xb[::41][:16] + 0.01 * _rand(16, d, 5)).astype(np.float32)
    srv = IndexServer(0, str(tmp_path), provider=HipProvider())
    cli = IndexClient(servers=[srv])
    cfg =IndexCfg(faiss_factory="IVF8,SQ8,Refine(SQfp16)", dim=d, metric="l2",
                   nprobe=8, train_num=2400, index_storage_dir=str(tmp_path))
    srv.create_index("r", cfg)
    srv.add_index_data("r", xb, [("doc", i) for i in range(len(xb))], False)
    idx = srv._get_index("r")
    _wait_trained(idx)
    eng = idx.engine
    assert eng.refine_info()[0] == 2 and eng.k_factor == 1.0
    plain = HipEngine(spec={k: v for k, v in eng.spec.items()
                            if k not in ("refine", "k_factor")})
    plain.set_trained(eng.get_centroids(), None, *eng.get_sq_params())
    plain.add(xb)

    def expect(kp):
        _D, cand = plain.search(q, kp)
        return refine_ref(q, xb.astype(np.float16), cand, 10, L2)

    for setter in (idx.set_k_factor,
                   lambda v: srv.set_k_factor("r", v)):
        for kf, kp in ((4, 40), (1, 10)):
            setter(kf)
            assert eng.k_factor == kf
            scores, metas, embs = srv.search("r", q, 10, True)
            Dr, Ir = expect(kp)
            np.testing.assert_array_equal(scores, Dr)
            assert [[m[1] for m in row] for row in metas] == Ir.tolist()
            # return_embeddings: the stored (fp16) vectors
            np.testing.assert_array_equal(
                np.asarray(embs, np.float32),
                xb.astype(np.float16).astype(np.float32)[Ir])
    cli.set_k_factor("r", 4)
    assert eng.k_factor == 4
    # an engine without a refine stage refuses
    cfg2 = IndexCfg(faiss_factory="IVF8,SQ8", dim=d, metric="l2", nprobe=8,
                    train_num=2400, index_storage_dir=str(tmp_path))
    srv.create_index("p", cfg2)
    srv.add_index_data("p", xb, list(range(len(xb))), False)
    _wait_trained(srv._get_index("p"))
    with pytest.raises(RuntimeError, match="no refine stage"):
        srv.set_k_factor("p", 2)


# ---------------------------------------------------------------------------
# HIP graph capture
# ---------------------------------------------------------------------------


def test_graph_capture_replays_equal_eager():
    c = _case("ivfpq", None, L2)
    eng = c.engine("fp16")
    eng.nprobe = NLIST
    eng.k_factor = 4
    k = 10
    qt = torch.as_tensor(c.q).cuda()
    D = torch.empty((len(c.q), k), dtype=torch.float32, device="cuda")
    I = torch.empty((len(c.q), k), dtype=torch.int64, device="cuda")
    eng.search_dev(qt, k, D, I)  # warm-up: every workspace is sized here
    torch.cuda.synchronize()
    De, Ie = D.cpu().numpy(), I.cpu().numpy()
    _bitwise(De, Ie, *c.ref("fp16", NLIST, 40, k))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.search_dev(qt, k, D, I)
    for _ in range(2):
        D.zero_()
        I.zero_()
        g.replay()
        torch.cuda.synchronize()
        _bitwise(D.cpu().numpy(), I.cpu().numpy(), De, Ie)
