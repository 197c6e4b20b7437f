# 4-bit product quantization (spec "nbits": 4), the parts
# that need no GPU: factory strings and the knnlm builder, the nibble
# packing, the CPU oracle (oracle.OracleIVFPQ at nbits=4) against a float64
# brute-force ADC, and the spec validation in dfann_create.
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_faiss_amd.engine_spec import resolve_engine_spec  # noqa: E402
from distributed_faiss_amd.index_cfg import IndexCfg  # noqa: E402
from oracle import (  # noqa: E402
    OracleIVFPQ,
    pack_pq4 as pack,
    unpack_pq4 as unpack,
)

KSUB = 16

IP, L2 = 0, 1
SO = os.path.join(REPO, "distributed_faiss_amd", "libdfann.so")


# ---------------------------------------------------------------------------
# factory strings / builder
# ---------------------------------------------------------------------------


def test_factory_pq32x4():
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory="IVF64,PQ32x4", dim=64, metric="l2"), 10000)
    assert spec["type"] == "ivfpq" and spec["nlist"] == 64
    assert spec["m"] == 32 and spec["nbits"] == 4
    assert "refine" not in spec


@pytest.mark.parametrize("tail,refine", [("RFlat", "fp32"),
                                         ("Refine(SQfp16)", "fp16")])
def test_factory_pq32x4_refine(tail, refine):
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory=f"IVF64,PQ32x4,{tail}", dim=64, metric="dot",
                 k_factor=4), 10000)
    assert spec["m"] == 32 and spec["nbits"] == 4
    assert spec["refine"] == refine and spec["k_factor"] == 4.0


def test_factory_centroids_placeholder():
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory="IVF{centroids},PQ16x4", dim=64, metric="l2",
                 centroids=48), 10000)
    assert spec["nlist"] == 48 and spec["m"] == 16 and spec["nbits"] == 4


def test_knnlm_bits_per_vector_4():
    spec = resolve_engine_spec(
        IndexCfg(index_builder_type="knnlm", dim=64, centroids=16,
                 metric="l2", code_size=32, bits_per_vector=4), 1000)
    assert spec["type"] == "ivfpq" and spec["m"] == 32 and spec["nbits"] == 4


@pytest.mark.parametrize("s", ["IVF64,PQ32x5", "IVF64,PQ32x16",
                               "IVF64,PQ32x5,RFlat"])
def test_factory_other_widths_refused(s):
    with pytest.raises(NotImplementedError, match=r"\[4, 8\]"):
        resolve_engine_spec(IndexCfg(faiss_factory=s, dim=64, metric="l2"),
                            10000)


@pytest.mark.parametrize("s", ["IVF64,PQ32", "IVF64,PQ32x8", "IVF64,PQ32,RFlat"])
def test_factory_default_width_is_8(s):
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory=s, dim=64, metric="l2"), 10000)
    assert spec["m"] == 32 and spec["nbits"] == 8


@pytest.mark.parametrize("s", ["IVF64,PQ32x", "IVF64,PQ32x4fs", "IVF64,PQx4",
                               "IVF64,SQ8x4"])
def test_factory_malformed_width_refused(s):
    with pytest.raises(NotImplementedError, match="PQmx4"):
        resolve_engine_spec(IndexCfg(faiss_factory=s, dim=64, metric="l2"),
                            10000)


# ---------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("m", [1, 2, 5, 20, 32, 33])
def test_pack_unpack_round_trip(m):
    rng = np.random.default_rng(m)
    codes = rng.integers(0, KSUB, (37, m)).astype(np.uint8)
    p = pack(codes)
    assert p.dtype == np.uint8 and p.shape == (37, (m + 1) // 2)
    np.testing.assert_array_equal(unpack(p, m), codes)
    # stride-padded rows (what the engine dumps) unpack the same
    padded = np.concatenate([p, np.full((37, 7), 0xAB, np.uint8)], axis=1)
    np.testing.assert_array_equal(unpack(padded, m), codes)


def test_low_nibble_is_the_even_subquantizer():
    p = pack(np.array([[0x3, 0xA, 0xF, 0x0, 0x7]]))
    np.testing.assert_array_equal(p, [[0xA3, 0x0F, 0x07]])
    # odd m: the last high nibble is 0
    rng = np.random.default_rng(0)
    codes = rng.integers(0, KSUB, (50, 5))
    assert (pack(codes)[:, -1] >> 4 == 0).all()
    assert (pack(codes)[:, -1] & 15 == codes[:, 4]).all()


def test_pack_refuses_wide_codes():
    with pytest.raises(AssertionError):
        pack(np.array([[16, 0]]))


# ---------------------------------------------------------------------------
# the restatement against a float64 brute-force ADC
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("m,dsub", [(8, 4), (5, 3)])
def test_restatement_matches_f64_adc(m, dsub, metric):
    d, nlist, n, nq, k = m * dsub, 4, 600, 6, 20
    rng = np.random.default_rng(100 * m + dsub + metric)
    cent = (rng.standard_normal((nlist, d)) * 3.0).astype(np.float32)
    xb = (cent[rng.integers(0, nlist, n)]
          + rng.standard_normal((n, d))).astype(np.float32)
    q = (cent[rng.integers(0, nlist, nq)]
         + rng.standard_normal((nq, d))).astype(np.float32)
    orc = OracleIVFPQ(d, nlist, m, metric, 4, seed=7)
    orc.max_ppc = 32
    orc.train(xb)
    assert orc.codebooks.shape == (m, KSUB, dsub)
    orc.add(xb)
    codes = np.concatenate(orc.list_codes)
    assert codes.max() < KSUB and orc.ntotal == n
    probes = np.tile(np.arange(nlist), (nq, 1))
    D, I = orc.search_preassigned(q, probes, None, k)
    assert (I >= 0).all()
    # fp64 distance to the decoded vectors of the returned ids
    R = orc.decode_ids(I).astype(np.float64)
    q64 = q.astype(np.float64)[:, None, :]
    ref = ((q64 - R) ** 2).sum(-1) if metric == L2 else (q64 * R).sum(-1)
    assert (np.abs(D - ref) <= 1e-4 * np.abs(ref) + 1e-4).all()
    # and the ranking is the fp64 ranking up to that tolerance: the k-th
    # returned value bounds every row left out
    allR = orc.decode_ids(np.tile(np.arange(n), (nq, 1))).astype(np.float64)
    full = (((q64 - allR) ** 2).sum(-1) if metric == L2
            else -(q64 * allR).sum(-1))
    kth = np.sort(full, axis=1)[:, k - 1]
    got = ref[:, -1] if metric == L2 else -ref[:, -1]
    assert (np.abs(got - kth) <= 1e-4 * np.abs(kth) + 1e-4).all()


def test_restatement_encode_picks_the_nearest_codeword():
    m, dsub, nlist = 6, 5, 3
    d = m * dsub
    rng = np.random.default_rng(9)
    orc = OracleIVFPQ(d, nlist, m, L2, 4)
    orc.centroids = (rng.standard_normal((nlist, d)) * 10.0).astype(np.float32)
    orc.codebooks = rng.standard_normal((m, KSUB, dsub)).astype(np.float32)
    orc.is_trained = True
    lbl = rng.integers(0, nlist, 200)
    cw = rng.integers(0, KSUB, (200, m))
    dec = np.concatenate([orc.codebooks[j][cw[:, j]] for j in range(m)], axis=1)
    x = (orc.centroids[lbl] + dec
         + 1e-3 * rng.standard_normal((200, d))).astype(np.float32)
    assign, codes = orc.encode(x)
    np.testing.assert_array_equal(assign, lbl)
    np.testing.assert_array_equal(codes, cw)


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
    lib.dfann_code_stride.argtypes = [ctypes.c_void_p]
    return lib


def _create(lib, **kw):
    import json

    spec = dict({"type": "ivfpq", "dim": 60, "metric": 1, "nlist": 8}, **kw)
    h = ctypes.c_void_p()
    rc = lib.dfann_create(json.dumps(spec).encode(), ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("m,nbits,stride", [
    (20, 4, 16), (5, 4, 16), (60, 4, 32), (2, 4, 16), (20, 8, 32),
    (60, 8, 64)])
def test_create_code_stride(lib, m, nbits, stride):
    # code_bytes = (m + 1) / 2 at 4 bits, m at 8; stride = ceil16
    rc, h = _create(lib, m=m, nbits=nbits)
    assert rc == 0, lib.dfann_last_error()
    assert lib.dfann_code_stride(h) == stride
    assert lib.dfann_destroy(h) == 0


@pytest.mark.parametrize("nbits", [5, 1, 16, 0])
def test_create_rejects_other_widths(lib, nbits):
    rc, _h = _create(lib, m=20, nbits=nbits)
    assert rc != 0
    msg = lib.dfann_last_error()
    assert b"4, 8" in msg, msg


@pytest.mark.parametrize("knob", ["pq_lut_f16", "pq_lut_global",
                                  "pq_precomputed"])
def test_create_rejects_lut_knobs_at_4_bits(lib, knob):
    rc, _h = _create(lib, m=20, nbits=4, **{knob: 1})
    assert rc != 0
    assert knob.encode() in lib.dfann_last_error()
    # the same knob on an 8-bit spec is still accepted
    rc, h = _create(lib, m=20, nbits=8, **{knob: 1})
    assert rc == 0, lib.dfann_last_error()
    assert lib.dfann_destroy(h) == 0


@pytest.mark.parametrize("kw", [{"pq_lut_global": -1}, {"pq_lut_global": 0},
                                {"pq_lut_mb": 64}])
def test_create_accepts_inert_knobs_at_4_bits(lib, kw):
    rc, h = _create(lib, m=20, nbits=4, **kw)
    assert rc == 0, lib.dfann_last_error()
    assert lib.dfann_destroy(h) == 0
