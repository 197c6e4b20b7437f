# Refine stage, the parts that need no GPU: factory strings and builder
# keys, the numpy restatement of the refine kernel (oracle/refine.py)
# against a float64 brute force and against a hand-coded scalar lane order,
# spec validation in dfann_create, and set_k_factor through the TCP proxy.
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_faiss_amd.engine_spec import (  # noqa: E402
    ENGINE_PERF_KNOBS, REFINE_KEYS, resolve_engine_spec)
from distributed_faiss_amd.index_cfg import IndexCfg  # noqa: E402
from oracle.refine import (  # noqa: E402
    IP, L2, FLT_MAX, k_prime, refine_distances, refine_ref)

SO = os.path.join(REPO, "distributed_faiss_amd", "libdfann.so")


# ---------------------------------------------------------------------------
# factory strings / builders
# ---------------------------------------------------------------------------


def test_factory_pq_rflat():
    cfg = IndexCfg(faiss_factory="IVF64,PQ8,RFlat", dim=32, metric="l2")
    spec = resolve_engine_spec(cfg, 10000)
    assert spec["type"] == "ivfpq" and spec["nlist"] == 64 and spec["m"] == 8
    assert spec["refine"] == "fp32"
    assert "k_factor" not in spec  # engine default 1.0


def test_factory_sq8_refine_sqfp16_with_centroids():
    cfg = IndexCfg(faiss_factory="IVF{centroids},SQ8,Refine(SQfp16)", dim=32,
                   metric="dot", centroids=48, k_factor=4)
    spec = resolve_engine_spec(cfg, 10000)
    assert spec["type"] == "ivfsq" and spec["sq_type"] == "8bit"
    assert spec["nlist"] == 48 and spec["metric"] == 0
    assert spec["refine"] == "fp16" and spec["k_factor"] == 4.0


def test_factory_sqfp16_rflat():
    cfg = IndexCfg(faiss_factory="IVF8,SQfp16,RFlat", dim=32, metric="l2")
    spec = resolve_engine_spec(cfg, 10000)
    assert spec["type"] == "ivfsq" and spec["sq_type"] == "fp16"
    assert spec["nlist"] == 8 and spec["refine"] == "fp32"


@pytest.mark.parametrize("s", ["IVF8,Flat,RFlat", "IVF8,PQ8,Refine(PQ4)",
                               "IVF8,Flat,Refine(SQfp16)", "IVF8,PQ8,RFlat,RFlat"])
def test_factory_unsupported_refine(s):
    cfg = IndexCfg(faiss_factory=s, dim=32, metric="l2")
    with pytest.raises(NotImplementedError, match="RFlat"):
        resolve_engine_spec(cfg, 10000)


def test_factory_plain_strings_unchanged():
    for s, typ in [("IVF8,Flat", "ivf_flat"), ("IVF8,PQ4", "ivfpq"),
                   ("IVF8,SQ8", "ivfsq"), ("IVF8,SQfp16", "ivfsq")]:
        spec = resolve_engine_spec(
            IndexCfg(faiss_factory=s, dim=32, metric="l2", k_factor=3), 1000)
        assert spec["type"] == typ
        assert "refine" not in spec and "k_factor" not in spec


def test_builder_extra_passes_through():
    cfg = IndexCfg(index_builder_type="knnlm", dim=64, centroids=16,
                   metric="l2", code_size=8, refine="fp16", k_factor=2.5)
    spec = resolve_engine_spec(cfg, 1000)
    assert spec["type"] == "ivfpq" and spec["m"] == 8
    assert spec["refine"] == "fp16" and spec["k_factor"] == 2.5
    cfg = IndexCfg(index_builder_type="ivfsq", dim=64, centroids=16,
                   metric="dot", refine="fp32")
    spec = resolve_engine_spec(cfg, 1000)
    assert spec["type"] == "ivfsq" and spec["refine"] == "fp32"
    assert "k_factor" not in spec
    # builders that cannot refine do not forward the key
    cfg = IndexCfg(index_builder_type="ivf_simple", dim=64, centroids=16,
                   refine="fp32", k_factor=2)
    spec = resolve_engine_spec(cfg, 1000)
    assert "refine" not in spec and "k_factor" not in spec
    # they change results: kept apart from the perf knobs
    assert not set(REFINE_KEYS) & set(ENGINE_PERF_KNOBS)


def test_k_prime_rule():
    assert k_prime(10, 1) == 10
    assert k_prime(10, 1.6) == 16   # 10 * float32(1.6) = 16.0000002
    assert k_prime(10, 1.7) == 17
    assert k_prime(10, 4) == 40
    assert k_prime(1, 1) == 1
    assert k_prime(40, 13) == 512   # silent clamp
    assert k_prime(10, 1.61) == 17


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------


def _brute64(q, X, metric):
    q64, X64 = q.astype(np.float64), X.astype(np.float64)
    if metric == IP:
        return q64 @ X64.T
    return ((q64[:, None, :] - X64[None, :, :]) ** 2).sum(-1)


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("store_t", [np.float32, np.float16])
@pytest.mark.parametrize("d", [20, 128, 136, 200, 768])
def test_refine_ref_vs_float64(d, store_t, metric):
    rng = np.random.default_rng(d)
    n, nq, kp, k = 300, 7, 40, 10
    store = rng.standard_normal((n, d)).astype(np.float32).astype(store_t)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    cand = np.stack([rng.choice(n, kp, replace=False) for _ in range(nq)])
    cand[2, 30:] = -1          # base pads
    cand[5, 4:] = -1           # fewer than k valid: output pads
    D, I = refine_ref(q, store, cand, k, metric)
    ref = _brute64(q, store, metric)
    for i in range(nq):
        ids = cand[i][cand[i] >= 0]
        keys = -ref[i, ids] if metric == IP else ref[i, ids]
        order = ids[np.lexsort((ids, keys))][:k]
        nv = len(order)
        assert (I[i, nv:] == -1).all()
        assert (D[i, nv:] == (FLT_MAX if metric == L2 else -FLT_MAX)).all()
        r = ref[i, I[i, :nv]]
        np.testing.assert_array_less(np.abs(D[i, :nv] - r),
                                     1e-4 * np.abs(r) + 1e-4)
        # same ids wherever the float64 gap exceeds the tolerance
        sk = np.sort(keys)
        for j in range(nv):
            gap_lo = j == 0 or sk[j] - sk[j - 1] > 2e-4 * abs(sk[j]) + 2e-4
            gap_hi = j + 1 >= len(sk) or \
                sk[j + 1] - sk[j] > 2e-4 * abs(sk[j]) + 2e-4
            if gap_lo and gap_hi:
                assert I[i, j] == order[j]
    assert (I[5, 4:] == -1).all() and (I[5, :4] >= 0).all()


def _scalar_lane_order(q, x, metric):
    """The kernel's order written out as plain scalar loops."""
    d = len(q)
    part = [np.float32(0)] * 16
    for g in range(16):
        t0 = 8 * g
        while t0 < d:
            for t in range(t0, min(t0 + 8, d)):
                if metric == IP:
                    term = np.float32(q[t]) * np.float32(x[t])
                else:
                    df = np.float32(q[t]) - np.float32(x[t])
                    term = np.float32(df * df)
                part[g] = np.float32(part[g] + term)
            t0 += 128
    for s in (8, 4, 2, 1):
        part = [np.float32(part[g] + part[g ^ s]) for g in range(16)]
    assert all(p == part[0] for p in part)
    return part[0]


def _sequential(q, x, metric):
    acc = np.float32(0)
    for t in range(len(q)):
        if metric == IP:
            term = np.float32(q[t]) * np.float32(x[t])
        else:
            df = np.float32(q[t]) - np.float32(x[t])
            term = np.float32(df * df)
        acc = np.float32(acc + term)
    return acc


@pytest.mark.parametrize("metric", [IP, L2])
def test_lane_order_is_not_sequential(metric):
    # d = 136: lane 0 owns t = 0..7 AND 128..135, every other lane one
    # chunk. Magnitudes spanning 2^24 make float32 addition order-visible.
    d = 136
    rng = np.random.default_rng(5)
    mag = np.exp2(rng.integers(-12, 13, d)).astype(np.float32)
    x = (mag * rng.choice([-1.0, 1.0], d)
         * (1 + rng.random(d))).astype(np.float32)
    q = (rng.standard_normal(d) * np.exp2(rng.integers(-6, 7, d))).astype(np.float32)
    lane = _scalar_lane_order(q, x, metric)
    seq = _sequential(q, x, metric)
    assert lane != seq, "inputs too tame: the orders agree"
    got = refine_distances(q[None, :], x[None, :], metric)[0]
    assert got.dtype == np.float32
    assert got.tobytes() == np.float32(lane).tobytes()
    # and through the public entry, fp32 store
    D, I = refine_ref(q[None, :], x[None, :], np.array([[0]]), 1, metric)
    assert I[0, 0] == 0 and D[0, 0].tobytes() == np.float32(lane).tobytes()


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [20, 136, 200])
def test_refine_ref_equals_scalar_order_random(d, metric):
    rng = np.random.default_rng(100 + d)
    X = rng.standard_normal((5, d)).astype(np.float16)
    q = rng.standard_normal(d).astype(np.float32)
    got = refine_distances(q[None, :], X, metric)
    for r in range(5):
        want = _scalar_lane_order(q, X[r].astype(np.float32), metric)
        assert got[r].tobytes() == np.float32(want).tobytes()


def test_refine_ref_ties_break_on_id_and_inf_sorts_last():
    d = 16
    store = np.zeros((6, d), np.float16)
    store[3, 0] = np.float16(np.inf)      # as a value above 65504 is stored
    q = np.ones((1, d), np.float32)
    cand = np.array([[5, 3, 1, -1, 4, 0]])
    D, I = refine_ref(q, store, cand, 6, L2)
    assert I[0].tolist() == [0, 1, 4, 5, 3, -1]
    assert D[0, 0] == 16.0 and np.isinf(D[0, 4]) and D[0, 5] == FLT_MAX


# ---------------------------------------------------------------------------
# dfann_create spec validation (no device is touched)
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):
        import __graft_entry__

        __graft_entry__.build()
    lib = ctypes.CDLL(SO)
    lib.dfann_create.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.dfann_destroy.argtypes = [ctypes.c_void_p]
    lib.dfann_last_error.restype = ctypes.c_char_p
    lib.dfann_refine_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.dfann_set_k_factor.argtypes = [ctypes.c_void_p, ctypes.c_float]
    return lib


def _create(lib, js):
    h = ctypes.c_void_p()
    rc = lib.dfann_create(js.encode(), ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("js,kind,stride", [
    ('{"type": "ivfpq", "dim": 64, "metric": 1, "nlist": 8, "m": 8, '
     '"refine": "fp32", "k_factor": 1.6}', 1, 256),
    ('{"type": "ivfsq", "dim": 20, "metric": 0, "nlist": 8, '
     '"sq_type": "8bit", "refine": "fp16"}', 2, 48),
    ('{"type": "ivfsq", "dim": 10, "metric": 0, "nlist": 8, '
     '"sq_type": "fp16", "refine": "fp32", "refine_slab_mb": 1}', 1, 48),
    ('{"type": "ivfpq", "dim": 64, "metric": 1, "nlist": 8, "m": 8, '
     '"refine": ""}', 0, 0),
])
def test_create_accepts_refine_spec(lib, js, kind, stride):
    rc, h = _create(lib, js)
    assert rc == 0, lib.dfann_last_error()
    out = (ctypes.c_int64 * 3)()
    assert lib.dfann_refine_info(h, out) == 0
    assert list(out) == [kind, stride, 0]
    if kind:
        assert lib.dfann_set_k_factor(h, 4.0) == 0
        assert lib.dfann_set_k_factor(h, 0.5) != 0
    else:
        assert lib.dfann_set_k_factor(h, 4.0) != 0
        assert b"no refine stage" in lib.dfann_last_error()
    assert lib.dfann_destroy(h) == 0


@pytest.mark.parametrize("typ,extra", [
    ("flat", ""), ("ivf_flat", ', "nlist": 8'),
    ("hnswsq", ', "metric": 1, "m": 8')])
def test_create_rejects_refine_on_other_types(lib, typ, extra):
    rc, _h = _create(
        lib, '{"type": "%s", "dim": 16%s, "refine": "fp32"}' % (typ, extra))
    assert rc != 0
    msg = lib.dfann_last_error().decode()
    assert "refine" in msg and typ in msg


def test_create_rejects_bad_k_factor_and_codec(lib):
    base = '{"type": "ivfpq", "dim": 64, "metric": 1, "nlist": 8, "m": 8, %s}'
    rc, _h = _create(lib, base % '"refine": "fp32", "k_factor": 0.5')
    assert rc != 0 and b"k_factor" in lib.dfann_last_error()
    rc, _h = _create(lib, base % '"refine": "pq4"')
    assert rc != 0 and b"pq4" in lib.dfann_last_error()


# ---------------------------------------------------------------------------
# set_k_factor travels through server, client and the TCP proxy
# ---------------------------------------------------------------------------


def test_set_k_factor_over_tcp(tmp_path):
    import time

    from distributed_faiss_amd import IndexClient, IndexServer, IndexState
    from distributed_faiss_amd.rpc import TcpServer
    from oracle import OracleProvider

    srv = IndexServer(0, str(tmp_path / "0"), provider=OracleProvider())
    tcp = TcpServer(srv, port=0)
    tcp.start_background()
    try:
        lst = tmp_path / "servers.txt"
        lst.write_text(f"1\n127.0.0.1,{tcp.port}\n")
        cli = IndexClient(str(lst))
        cfg = IndexCfg(faiss_factory="IVF4,SQ8,RFlat", dim=16, metric="l2",
                       train_num=64, nprobe=4)
        cli.create_index("r", cfg)
        emb = np.random.default_rng(0).random((80, 16), dtype=np.float32)
        cli.add_index_data("r", emb, list(range(80)),
                           train_async_if_triggered=False)
        for _ in range(200):
            if cli.get_state("r") == IndexState.TRAINED:
                break
            time.sleep(0.05)
        assert cli.get_state("r") == IndexState.TRAINED
        cli.set_k_factor("r", 2.5)
        idx = srv._get_index("r")
        assert idx.engine.k_factor == 2.5
        assert idx.cfg.extra["k_factor"] == 2.5
        cli.close()
    finally:
        tcp.stop()
