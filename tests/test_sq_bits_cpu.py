# 4- and 6-bit scalar quantizers (spec "sq_type": "4bit" | "6bit";
# DESIGN.md §6h), the parts that need no GPU: the bit-stream packing with
# hand-written known answers, the numpy restatement (oracle.OracleIVFSQ)
# against faiss's decode formula in float64, the factory strings, and the
# spec handling of dfann_create.
import ctypes
import json
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
    OracleIVFSQ,
    pack_sq as pack,
    sq_code_bytes as code_bytes,
    sq_stride as stride,
    unpack_sq as unpack,
)

IP, L2 = 0, 1
BITS = [4, 6]
SO = os.path.join(REPO, "distributed_faiss_amd", "libdfann.so")


# ---------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------


def test_pack_4bit_known_answer():
    # dim 0 low nibble, dim 1 high nibble of byte 0; dim 2 low nibble of
    # byte 1, whose high nibble stays 0
    np.testing.assert_array_equal(pack([[1, 2, 3]], 4), [[0x21, 0x03]])


def test_pack_6bit_known_answer():
    # 1 | 2 << 6 | 3 << 12 | 4 << 18 = 0x103081, little endian
    assert 1 | 2 << 6 | 3 << 12 | 4 << 18 == 0x103081
    np.testing.assert_array_equal(pack([[1, 2, 3, 4]], 6), [[0x81, 0x30, 0x10]])


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 7, 40, 128])
def test_pack_unpack_round_trip(d, bits):
    rng = np.random.default_rng(10 * d + bits)
    codes = rng.integers(0, 1 << bits, (37, d)).astype(np.uint8)
    codes[0] = (1 << bits) - 1  # every bit of a field set
    codes[1] = 0
    p = pack(codes, bits)
    assert p.dtype == np.uint8 and p.shape == (37, (d * bits + 7) // 8)
    assert p.shape[1] == code_bytes(d, bits)
    np.testing.assert_array_equal(unpack(p, d, bits), codes)
    # all-ones codes leave every bit past d * bits clear
    tail = 8 * p.shape[1] - d * bits
    assert p[0, -1] >> (8 - tail) == 0 if tail else True
    # stride-padded rows (what the engine dumps) unpack the same
    padded = np.concatenate([p, np.full((37, 7), 0xAB, np.uint8)], axis=1)
    np.testing.assert_array_equal(unpack(padded, d, bits), codes)


@pytest.mark.parametrize("bits", BITS)
def test_pack_refuses_wide_codes(bits):
    with pytest.raises(ValueError, match="out of range"):
        pack(np.array([[0, 1 << bits]]), bits)
    with pytest.raises(ValueError, match="out of range"):
        pack(np.array([[-1, 0]]), bits)


def test_six_bit_group_layout():
    # code i of group g sits at bit 6i of the 24-bit word at bytes 3g..3g+2
    codes = np.zeros((1, 8), np.int64)
    codes[0, 5] = 63  # group 1, i = 1: bits 6..11 of bytes 3..5
    p = pack(codes, 6)
    word = int(p[0, 3]) | int(p[0, 4]) << 8 | int(p[0, 5]) << 16
    assert word == 63 << 6 and not p[0, :3].any()


# ---------------------------------------------------------------------------
# the restatement against faiss's formula in float64
# ---------------------------------------------------------------------------


def _trained(d, nlist, metric, bits, rng, n=500):
    cent = (rng.standard_normal((nlist, d)) * 3.0).astype(np.float32)
    lbl = rng.integers(0, nlist, n)
    xb = (cent[lbl] + rng.standard_normal((n, d))).astype(np.float32)
    orc = OracleIVFSQ(d, nlist, metric, f"{bits}bit")
    orc.centroids = cent
    r = xb - cent[lbl]
    vmin = r.min(axis=0).astype(np.float32)
    vdiff = (r.max(axis=0) - vmin).astype(np.float32)
    orc.set_ranges(vmin, vdiff)
    orc.is_trained = True
    return orc, xb


@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("d", [7, 40, 200])
def test_restatement_matches_f64_formula(d, bits, metric):
    nlist, nq = 3, 5
    rng = np.random.default_rng(1000 * d + 10 * bits + metric)
    orc, xb = _trained(d, nlist, metric, bits, rng)
    orc.add(xb)
    q = (orc.centroids[rng.integers(0, nlist, nq)]
         + rng.standard_normal((nq, d))).astype(np.float32)
    Q = float((1 << bits) - 1)
    eps = 2.0 ** -24  # unit roundoff of fp32
    for li in range(nlist):
        codes = orc.list_codes[li].astype(np.float64)
        assert codes.shape[0] > 0 and codes.max() <= Q
        # faiss: x = vmin + ((c + 0.5) / Q) * vdiff, on the residual
        dec = (orc.vmin.astype(np.float64)
               + ((codes + 0.5) / Q) * orc.vdiff.astype(np.float64))
        c64 = orc.centroids[li].astype(np.float64)
        for i in range(nq):
            q64 = q[i].astype(np.float64)
            got, _ids = orc._scan_one(q[i], li, None)
            if metric == L2:
                terms = ((q64 - c64) - dec) ** 2
                ref = terms.sum(-1)
                # every term is a square of a difference of values bounded
                # by mag, formed by <= 6 roundings (r, u, scale, c*v, diff,
                # square): relative to mag^2 per term; then d adds
                mag = (np.abs(q64 - c64).max() + np.abs(orc.vmin).max()
                       + np.abs(orc.vdiff).max())
                bound = d * (12.0 * eps * mag * mag) + d * eps * terms.sum(-1)
            else:
                terms = q64 * dec
                ref = (q64 * c64).sum() + terms.sum(-1)
                mag = np.abs(q64).max() * (np.abs(orc.vmin).max()
                                          + np.abs(orc.vdiff).max())
                # bias (d products, d adds) + d terms of <= 5 roundings + the
                # d adds, each relative to the running magnitude
                run = np.abs(q64 * c64).sum() + np.abs(terms).sum(-1) + d * mag
                bound = (2.0 * d + 8.0) * eps * run
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bound).all(), (li, i, (err / bound).max())
            if metric == L2:  # and the bound is small against the distances
                assert (bound <= 1e-3 * ref).all()


@pytest.mark.parametrize("bits", BITS)
def test_restatement_encode_recovers_bin_centres(bits):
    d, nlist, n = 23, 3, 300
    rng = np.random.default_rng(50 + bits)
    orc, _xb = _trained(d, nlist, L2, bits, rng)
    Qi = (1 << bits) - 1
    lbl = rng.integers(0, nlist, n)
    cw = rng.integers(0, Qi + 1, (n, d))
    cw[0], cw[1] = 0, Qi
    # bin centre (c + 0.5) / Q of the range, plus noise far below the bin
    # width vdiff / Q. The top code's bin [1, 1 + 1/Q) is open-ended by the
    # clamp, so its centre is well inside it too.
    scale64 = orc.vdiff.astype(np.float64) / Qi
    resid = orc.vmin.astype(np.float64) + (cw + 0.5) * scale64
    resid += 0.05 * scale64 * rng.uniform(-1, 1, (n, d))
    codes = orc._encode_resid(resid.astype(np.float32))
    np.testing.assert_array_equal(codes, cw)
    # decode puts every component within half a step of the input
    dec = orc._decode_codes(codes).astype(np.float64)
    assert (np.abs(dec - resid) <= 0.5 * scale64 * 1.2).all()
    # out-of-range residuals clamp
    lo = orc._encode_resid((orc.vmin - 10 * orc.vdiff)[None, :])
    hi = orc._encode_resid((orc.vmin + 10 * orc.vdiff)[None, :])
    assert (lo == 0).all() and (hi == Qi).all()


def test_restatement_search_runs_through_the_oracle_merge():
    d, nlist, bits = 40, 4, 6
    rng = np.random.default_rng(3)
    orc, xb = _trained(d, nlist, L2, bits, rng)
    orc.add(xb)
    off, ids, packed = orc.packed_lists()
    assert packed.shape == (500, code_bytes(d, bits)) and off[-1] == 500
    other = OracleIVFSQ(d, nlist, L2, f"{bits}bit")
    other.centroids, other.is_trained = orc.centroids, True
    other.set_ranges(orc.vmin, orc.vdiff)
    other.load_lists(off, ids, packed)
    q = xb[:4]
    probes = np.tile(np.arange(nlist), (4, 1))
    D0, I0 = orc.search_preassigned(q, probes, None, 10)
    D1, I1 = other.search_preassigned(q, probes, None, 10)
    np.testing.assert_array_equal(I0, I1)
    np.testing.assert_array_equal(D0, D1)
    assert (I0 >= 0).all()


# ---------------------------------------------------------------------------
# factory strings
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
def test_factory_forms(bits):
    name, sq = f"SQ{bits}", f"{bits}bit"
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory=f"IVF64,{name}", dim=64, metric="l2"), 10000)
    assert spec["type"] == "ivfsq" and spec["nlist"] == 64
    assert spec["sq_type"] == sq and "refine" not in spec
    assert spec["metric"] == L2
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory=f"IVF64,{name}", dim=64, metric="dot"), 10000)
    assert spec["sq_type"] == sq and spec["metric"] == IP
    for tail, refine in (("RFlat", "fp32"), ("Refine(SQfp16)", "fp16")):
        spec = resolve_engine_spec(
            IndexCfg(faiss_factory=f"IVF64,{name},{tail}", dim=64,
                     metric="l2", k_factor=4), 10000)
        assert spec["type"] == "ivfsq" and spec["sq_type"] == sq
        assert spec["refine"] == refine and spec["k_factor"] == 4.0


@pytest.mark.parametrize("bits", BITS)
def test_factory_centroids_placeholder(bits):
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory=f"IVF{{centroids}},SQ{bits}", dim=64,
                 metric="l2", centroids=48), 10000)
    assert spec["nlist"] == 48 and spec["sq_type"] == f"{bits}bit"


@pytest.mark.parametrize("s", ["IVF8,SQ5", "IVF8,SQ4x2", "OPQ16,IVF8,SQ4",
                               "OPQ16,IVF8,SQ6", "IVF8,SQ6x2", "IVF8,SQ",
                               "IVF8,SQ4,Flat"])
def test_factory_still_refused(s):
    with pytest.raises(NotImplementedError):
        resolve_engine_spec(IndexCfg(faiss_factory=s, dim=64, metric="l2"),
                            10000)


def test_factory_error_names_the_new_forms():
    with pytest.raises(NotImplementedError, match=r"IVFn,SQ6, IVFn,SQ4"):
        resolve_engine_spec(
            IndexCfg(faiss_factory="IVF8,SQ5", dim=64, metric="l2"), 10000)


def test_existing_sq_forms_unchanged():
    for s, sq in (("IVF8,SQ8", "8bit"), ("IVF8,SQfp16", "fp16")):
        spec = resolve_engine_spec(
            IndexCfg(faiss_factory=s, dim=64, metric="l2"), 10000)
        assert spec["sq_type"] == sq
    spec = resolve_engine_spec(
        IndexCfg(index_builder_type="ivfsq", dim=64, centroids=8,
                 metric="l2"), 10000)
    assert spec["sq_type"] == "fp16"


# ---------------------------------------------------------------------------
# dfann_create (no device is touched)
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


def _create(lib, d, bits, **kw):
    spec = dict({"type": "ivfsq", "dim": d, "metric": 1, "nlist": 8,
                 "sq_type": f"{bits}bit"}, **kw)
    h = ctypes.c_void_p()
    rc = lib.dfann_create(json.dumps(spec).encode(), ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("d,bits,want", [
    (128, 4, 64), (40, 4, 32), (7, 4, 16), (128, 6, 96), (40, 6, 32),
    (22, 6, 32), (7, 6, 16), (768, 6, 576)])
def test_create_code_stride(lib, d, bits, want):
    assert stride(d, bits) == want  # the restatement's own rule
    rc, h = _create(lib, d, bits)
    assert rc == 0, lib.dfann_last_error()
    assert lib.dfann_code_stride(h) == want
    assert lib.dfann_destroy(h) == 0


def test_create_existing_strides_unchanged(lib):
    for sq, want in (("8bit", 48), ("fp16", 80)):
        spec = {"type": "ivfsq", "dim": 40, "metric": 1, "nlist": 8,
                "sq_type": sq}
        h = ctypes.c_void_p()
        assert lib.dfann_create(json.dumps(spec).encode(), ctypes.byref(h)) == 0
        assert lib.dfann_code_stride(h) == want
        assert lib.dfann_destroy(h) == 0


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("refine", ["fp32", "fp16"])
def test_create_accepts_refine(lib, bits, refine):
    rc, h = _create(lib, 40, bits, refine=refine, k_factor=4)
    assert rc == 0, lib.dfann_last_error()
    assert lib.dfann_code_stride(h) == stride(40, bits)
    assert lib.dfann_destroy(h) == 0


@pytest.mark.parametrize("bits", BITS)
def test_create_refuses_opq(lib, bits):
    rc, _h = _create(lib, 40, bits, opq=1)
    assert rc != 0
    assert b"opq" in lib.dfann_last_error()
