# GPU: exact filtered search (allow-bitmap applied inside the scan kernels).
#
# Reference everywhere: the CPU oracle's FULL ranking (k = ntotal; the
# oracle has no k cap) masked to the allowed ids and truncated / padded to
# k with the engine's pad values. A filter changes no row's arithmetic, so
# the PQ / SQ8 / SQfp16 scans are compared BITWISE, like test_gpu_parity's
# bit-exact tier; IVF-Flat and flat keep their documented tolerances.
#
# Shapes: d=32, nlist=8, nprobe=8 on the clustered / codeword-exact data of
# the parity suite, cut to 3187 rows so ntotal is no multiple of 32 or 64
# and lists start mid-word. Every bitmap handed to the engine has the bits
# >= ntotal of its last word SET, to prove they are ignored.
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
from distributed_faiss_amd.index import Index  # noqa: E402
from distributed_faiss_amd.index_cfg import IndexCfg  # noqa: E402
from gpu_support import (  # noqa: E402
    clustered as _clustered,
    rand as _rand,
    wait_trained as _wait_trained,
)
from oracle import from_engine_artifacts, make_oracle_engine  # noqa: E402

IP, L2 = 0, 1
FLT_MAX = np.float32(3.4028235e38)
NTOTAL = 3187
D_, NLIST = 32, 8
FILTERS = ["ALL", "NONE", "MOD3", "SPARSE", "NOLIST"]
CFGS = [("ivfpq", None), ("ivfsq", "8bit"), ("ivfsq", "fp16")]


def _pad(metric):
    return FLT_MAX if metric == L2 else -FLT_MAX


def _data(typ, metric, sq_type=None):
    """The parity suite's bit-exact data (3200 rows), first 3187 used:
    (spec, trained-artifact kwargs, xb, q)."""
    d, nlist = D_, NLIST
    cent, xb = _clustered(nlist, 400, d, seed=10)
    spec = {"type": typ, "dim": d, "metric": metric, "nlist": nlist,
            "nprobe": nlist, "seed": 1234}
    rng = np.random.default_rng(11)
    art = {"cent": cent}
    if typ == "ivfpq":
        spec["m"] = 8
        cb = rng.standard_normal((8, 256, d // 8)).astype(np.float32)
        art["codebooks"] = cb
        lbl = rng.integers(0, nlist, xb.shape[0])
        cw = rng.integers(0, 256, (xb.shape[0], 8))
        dec = np.concatenate([cb[j][cw[:, j]] for j in range(8)], axis=1)
        xb = (cent[lbl] + dec
              + 1e-3 * rng.standard_normal(xb.shape)).astype(np.float32)
    if typ == "ivfsq":
        spec["sq_type"] = sq_type
        if sq_type == "8bit":
            art["vmin"] = np.full(d, -2.0, np.float32)
            art["vdiff"] = np.full(d, 4.0, np.float32)
    q = xb[::37][:20] + 0.01 * rng.standard_normal((20, d)).astype(np.float32)
    return spec, art, xb[:NTOTAL], q.astype(np.float32)


def _engine(spec, art, batches):
    eng = HipEngine(spec=spec)
    eng.set_trained(art["cent"], art.get("codebooks"), art.get("vmin"),
                    art.get("vdiff"))
    for b in batches:
        eng.add(b)
    return eng


def _oracle(spec, art, xb):
    orc = from_engine_artifacts(spec, art["cent"], art.get("codebooks"),
                                art.get("vmin"), art.get("vdiff"))
    orc.add(xb)
    orc.nprobe = spec["nlist"]
    return orc


@functools.lru_cache(maxsize=None)
def _setup(typ, metric, sq_type=None):
    """Engine + oracle on shared artifacts and the oracle's full ranking,
    computed once per index kind and shared (read-only) by the tests."""
    spec, art, xb, q = _data(typ, metric, sq_type)
    eng = _engine(spec, art, [xb])
    orc = _oracle(spec, art, xb)
    probes, keys = eng.coarse(q, NLIST)
    Dfull, Ifull = orc.search_preassigned(q, probes, keys, NTOTAL)
    Dfull.setflags(write=False)
    Ifull.setflags(write=False)
    return {"spec": spec, "art": art, "xb": xb, "q": q, "eng": eng,
            "orc": orc, "probes": probes, "keys": keys, "Dfull": Dfull,
            "Ifull": Ifull}


def _allow(name, ntotal, orc=None):
    """bool mask over ids, padded to whole 32-bit words with the bits
    >= ntotal SET (they must be ignored)."""
    ids = np.arange(ntotal)
    if name == "ALL":
        a = np.ones(ntotal, bool)
    elif name == "NONE":
        a = np.zeros(ntotal, bool)
    elif name == "MOD3":
        a = ids % 3 != 0
    elif name == "SPARSE":
        a = ids % 97 == 5
    elif name == "NOLIST":
        a = np.ones(ntotal, bool)
        a[np.asarray(orc.list_ids[3], dtype=np.int64)] = False
    else:
        raise KeyError(name)
    out = np.ones((ntotal + 31) // 32 * 32, bool)
    out[:ntotal] = a
    assert out.shape[0] > ntotal  # there ARE set bits past ntotal
    return out


def _masked_ref(Dfull, Ifull, allow, k, metric):
    nq = Dfull.shape[0]
    D = np.full((nq, k), _pad(metric), np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        valid = Ifull[i] >= 0
        keep = np.zeros(Ifull.shape[1], bool)
        keep[valid] = allow[Ifull[i][valid]]
        n = min(k, int(keep.sum()))
        D[i, :n] = Dfull[i][keep][:n]
        I[i, :n] = Ifull[i][keep][:n]
    return D, I


# ---------------------------------------------------------------------------
# bit-exact tier
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("cfg", CFGS)
def test_filtered_scan_bitexact(cfg, metric, k, filt):
    s = _setup(cfg[0], metric, cfg[1])
    allow = _allow(filt, NTOTAL, s["orc"])
    if filt == "NOLIST":
        assert 0 < (~allow[:NTOTAL]).sum() < NTOTAL
    D, I = s["eng"].search_preassigned_filtered(
        s["q"], s["probes"], s["keys"], k, allow)
    Dr, Ir = _masked_ref(s["Dfull"], s["Ifull"], allow, k, metric)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)  # BITWISE
    if filt == "SPARSE" and k == 50:
        n_allowed = int(allow[:NTOTAL].sum())
        assert n_allowed < k  # every list is probed: all allowed rows come back
        assert (I[:, :n_allowed] >= 0).all()
        assert (I[:, n_allowed:] == -1).all()
        assert (D[:, n_allowed:] == _pad(metric)).all()
    if filt == "NONE":
        assert (I == -1).all() and (D == _pad(metric)).all()


# (spec knobs, metric): pq_precomputed is an L2-only path
PQ_KNOBS = [({}, IP), ({}, L2), ({"pq_precomputed": 1}, L2),
            ({"pq_lut_global": 1}, IP), ({"pq_lut_global": 1}, L2),
            ({"pq_lut_f16": 1}, IP), ({"pq_lut_f16": 1}, L2)]


@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize(
    "knobs,metric", PQ_KNOBS,
    ids=[("-".join(kn) or "base") + ("-ip" if m == IP else "-l2")
         for kn, m in PQ_KNOBS])
def test_all_filter_equals_search_pq(knobs, metric, k):
    # every dispatcher path has a filtered twin that honours the spec
    spec, art, xb, q = _data("ivfpq", metric)
    eng = _engine(dict(spec, **knobs), art, [xb])
    D, I = eng.search(q, k)
    Df, If = eng.search_filtered(q, k, _allow("ALL", NTOTAL))
    np.testing.assert_array_equal(If, I)
    np.testing.assert_array_equal(Df, D)
    assert (I >= 0).all()


@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("metric", [IP, L2])
def test_all_filter_equals_search_sq8_fan(metric, k):
    spec, art, xb, q = _data("ivfsq", metric, "8bit")
    eng = _engine(dict(spec, scan_fan=4), art, [xb])
    D, I = eng.search(q, k)
    Df, If = eng.search_filtered(q, k, _allow("ALL", NTOTAL))
    np.testing.assert_array_equal(If, I)
    np.testing.assert_array_equal(Df, D)
    # and the fan path honours a real filter too
    s = _setup("ivfsq", metric, "8bit")
    allow = _allow("MOD3", NTOTAL)
    D3, I3 = eng.search_preassigned_filtered(q, s["probes"], s["keys"], k, allow)
    Dr, Ir = _masked_ref(s["Dfull"], s["Ifull"], allow, k, metric)
    np.testing.assert_array_equal(I3, Ir)
    np.testing.assert_array_equal(D3, Dr)


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("cfg", CFGS + [("ivf_flat", None)])
def test_none_filter_all_pads(cfg, metric):
    if cfg[0] == "ivf_flat":
        s = _setup_ivfflat(metric)
    else:
        s = _setup(cfg[0], metric, cfg[1])
    for k in (10, 50):
        D, I = s["eng"].search_filtered(s["q"], k, _allow("NONE", NTOTAL))
        assert (I == -1).all()
        assert (D == _pad(metric)).all()


def test_large_k_512():
    # k = 512: the Sel buffer's guard headroom under a filter
    s = _setup("ivfpq", L2)
    allow = _allow("MOD3", NTOTAL)
    D, I = s["eng"].search_preassigned_filtered(
        s["q"], s["probes"], s["keys"], 512, allow)
    Dr, Ir = _masked_ref(s["Dfull"], s["Ifull"], allow, 512, L2)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_array_equal(D, Dr)


def test_incremental_merge_translation():
    # add / search / add: the second add rebuilds cr_ids, and the bitmap
    # must be translated through the NEW id -> position map
    s = _setup("ivfpq", L2)
    eng = _engine(s["spec"], s["art"], [s["xb"][:1700]])
    eng.search(s["q"], 10)  # finalizes the first CSR image
    eng.add(s["xb"][1700:])
    assert eng.ntotal == NTOTAL
    allow = _allow("MOD3", NTOTAL)
    for k in (10, 50):
        D, I = eng.search_preassigned_filtered(
            s["q"], s["probes"], s["keys"], k, allow)
        Dr, Ir = _masked_ref(s["Dfull"], s["Ifull"], allow, k, L2)
        np.testing.assert_array_equal(I, Ir)
        np.testing.assert_array_equal(D, Dr)


@pytest.mark.parametrize("metric", [IP, L2])
def test_sq8_multichunk_rows_self_consistent(metric):
    # d = 160 > 128 takes the SQ8 scan's multi-chunk row loop, a separate
    # gating site the d=32 shapes never reach. Reference: the engine's OWN
    # unfiltered full ranking (ntotal = 499 <= the k cap of 512) masked to
    # the allowed ids — a filter changes no row's arithmetic, so bitwise.
    d, n, nlist = 160, 499, 4
    cent, xb = _clustered(nlist, 125, d, seed=61)
    xb = xb[:n]
    q = xb[::29][:12] + 0.01 * _rand(12, d, 62)
    spec = {"type": "ivfsq", "sq_type": "8bit", "dim": d, "metric": metric,
            "nlist": nlist, "nprobe": nlist, "seed": 3}
    eng = HipEngine(spec=spec)
    eng.train(xb)
    eng.add(xb)
    Dfull, Ifull = eng.search(q, n)
    assert (Ifull >= 0).all()
    for filt in ("MOD3", "SPARSE", "ALL"):
        allow = _allow(filt, n)
        for k in (10, 50):
            D, I = eng.search_filtered(q, k, allow)
            Dr, Ir = _masked_ref(Dfull, Ifull, allow, k, metric)
            np.testing.assert_array_equal(I, Ir)
            np.testing.assert_array_equal(D, Dr)


# ---------------------------------------------------------------------------
# tolerance tier: IVF-Flat (16-lane tree reduction) and flat (MFMA GEMM)
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _setup_ivfflat(metric):
    spec, art, xb, q = _data("ivf_flat", metric)
    eng = _engine(spec, art, [xb])
    orc = _oracle(spec, art, xb)
    probes, keys = eng.coarse(q, NLIST)
    Dfull, Ifull = orc.search_preassigned(q, probes, keys, NTOTAL)
    return {"eng": eng, "orc": orc, "q": q, "probes": probes, "keys": keys,
            "Dfull": Dfull, "Ifull": Ifull}


def _check_tolerance(D, I, Dr, Ir, allow, id_match):
    got = I[I >= 0]
    assert allow[got].all(), "a rejected id was returned"
    np.testing.assert_array_equal(I >= 0, Ir >= 0)  # same fill per query
    m = (I == Ir).mean()
    assert m > id_match, f"id match {m}"
    same = I == Ir
    np.testing.assert_allclose(D[same], Dr[same], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("filt", ["MOD3", "SPARSE"])
@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("metric", [IP, L2])
def test_ivfflat_filtered_tolerance(metric, k, filt):
    s = _setup_ivfflat(metric)
    allow = _allow(filt, NTOTAL)
    D, I = s["eng"].search_preassigned_filtered(
        s["q"], s["probes"], s["keys"], k, allow)
    Dr, Ir = _masked_ref(s["Dfull"], s["Ifull"], allow, k, metric)
    _check_tolerance(D, I, Dr, Ir, allow, 0.99)


FLAT_N, FLAT_D = 5003, 48


@functools.lru_cache(maxsize=None)
def _setup_flat(metric):
    # ws_mb=1 -> database chunks of 4096 + 907 rows: the chunk base offset,
    # the float4 top-k branch (4096 % 4 == 0) and the scalar one (907)
    xb, q = _rand(FLAT_N, FLAT_D, 1), _rand(20, FLAT_D, 2)
    spec = {"type": "flat", "dim": FLAT_D, "metric": metric, "ws_mb": 1}
    eng = HipEngine(spec=spec)
    eng.train(xb)
    eng.add(xb)
    orc = make_oracle_engine(spec)
    orc.add(xb)
    Dfull, Ifull = orc.search(q, FLAT_N)
    return {"eng": eng, "q": q, "Dfull": Dfull, "Ifull": Ifull}


@pytest.mark.parametrize("filt", ["MOD3", "SPARSE"])
@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("metric", [IP, L2])
def test_flat_filtered(metric, k, filt):
    s = _setup_flat(metric)
    allow = _allow(filt, FLAT_N)
    D, I = s["eng"].search_filtered(s["q"], k, allow)
    Dr, Ir = _masked_ref(s["Dfull"], s["Ifull"], allow, k, metric)
    assert (I >= 0).all()  # >= 50 allowed rows under both filters
    _check_tolerance(D, I, Dr, Ir, allow, 0.999)


@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("metric", [IP, L2])
def test_flat_all_filter_equals_search(metric, k):
    s = _setup_flat(metric)
    D, I = s["eng"].search(s["q"], k)
    Df, If = s["eng"].search_filtered(s["q"], k, _allow("ALL", FLAT_N))
    np.testing.assert_array_equal(If, I)
    np.testing.assert_array_equal(Df, D)


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------


def test_short_bitmap_is_an_error():
    s = _setup("ivfpq", L2)
    short = np.ones(NTOTAL - 1, bool)
    with pytest.raises(RuntimeError, match="bitmap"):
        s["eng"].search_filtered(s["q"], 10, short)
    with pytest.raises(RuntimeError, match="bitmap"):
        s["eng"].search_preassigned_filtered(
            s["q"], s["probes"], s["keys"], 10, short)
    with pytest.raises(RuntimeError, match="bitmap"):
        _setup_flat(L2)["eng"].search_filtered(
            _setup_flat(L2)["q"], 10, np.ones(FLAT_N - 1, bool))
    with pytest.raises(RuntimeError, match="k > 512"):
        s["eng"].search_filtered(s["q"], 513, _allow("ALL", NTOTAL))


def test_hnswsq_is_unsupported():
    d = 16
    xb = _rand(300, d, 3)
    eng = HipEngine(spec={"type": "hnswsq", "dim": d, "metric": L2, "m": 8,
                          "ef_construction": 40, "nprobe": 16, "seed": 1})
    eng.train(xb)
    eng.add(xb)
    with pytest.raises(RuntimeError, match="unsupported"):
        eng.search_filtered(xb[:4], 5, np.ones(300, bool))


# ---------------------------------------------------------------------------
# Index.search_filtered through the product provider
# ---------------------------------------------------------------------------


def test_index_search_filtered_hip_provider(tmp_path):
    d, n1, n2 = 32, 2000, 700
    _cent, xb = _clustered(8, 400, d, seed=10)
    xb = xb[:n1 + n2]
    q = xb[::41][:16] + 0.01 * _rand(16, d, 5)
    cfg = IndexCfg(faiss_factory="IVF8,Flat", dim=d, metric="l2", nprobe=8,
                   train_num=n1, index_storage_dir=str(tmp_path))
    idx = Index(cfg, provider=HipProvider())
    meta = [("doc", i % 4) for i in range(n1 + n2)]
    idx.add_batch(xb[:n1], meta[:n1], train_async_if_triggered=False)
    _wait_trained(idx)
    assert idx.engine.ntotal == n1

    def check(ntotal):
        top_k = 10
        scores, ids, metas, embs = idx.search_filtered(q, top_k, 1, 2)
        assert embs is None
        assert scores.shape == (16, top_k) and ids.shape == (16, top_k)
        for row in metas:
            assert len(row) == top_k
            for m in row:
                # all lists are probed and 3/4 of the rows are allowed
                assert m is not None
                assert m[1] != 2
        allow = np.array([m[1] != 2 for m in meta[:ntotal]])
        Dr, Ir = idx.engine.search_filtered(q, top_k, allow)
        np.testing.assert_array_equal(ids, Ir)
        np.testing.assert_array_equal(scores, Dr)
        assert [[meta[j] for j in r] for r in ids] == metas

    check(n1)
    assert len(idx._filter_cache) == 1
    idx.add_batch(xb[n1:], meta[n1:])
    _wait_trained(idx)
    assert idx.engine.ntotal == n1 + n2
    check(n1 + n2)  # cached bitmap extended by the new tail
    assert len(idx._filter_cache) == 1
    (entry,) = idx._filter_cache.values()
    assert entry["n"] == n1 + n2
    # rows of the second batch are reachable under the filter
    _s, ids, _m, _e = idx.search_filtered(xb[n1 + 1:n1 + 2], 5, 1, 2)
    assert (ids >= n1).any()
