# OPQ pre-transform (spec "opq": 1), the parts that need no
# GPU: factory strings and the knnlm builder, every refusal, the spec
# validation in dfann_create, and the numpy restatement's own sanity
# (oracle/opq.py) on the structured training recipe.
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_faiss_amd.engine_spec import (ENGINE_PERF_KNOBS,  # noqa: E402
                                               OPQ_KEYS, resolve_engine_spec)
from distributed_faiss_amd.index_cfg import IndexCfg  # noqa: E402
from oracle import opq  # noqa: E402

SO = os.path.join(REPO, "distributed_faiss_amd", "libdfann.so")


def _factory(s, dim=64, **kw):
    return resolve_engine_spec(
        IndexCfg(faiss_factory=s, dim=dim, metric="l2", **kw), 10000)


# ---------------------------------------------------------------------------
# factory strings / builder
# ---------------------------------------------------------------------------


def test_factory_opq():
    spec = _factory("OPQ16,IVF64,PQ16")
    assert spec["type"] == "ivfpq" and spec["nlist"] == 64
    assert spec["m"] == 16 and spec["nbits"] == 8 and spec["dim"] == 64
    assert spec["opq"] == 1
    assert "opq_dim" not in spec and "opq_niter" not in spec
    assert "refine" not in spec


def test_factory_opq_reduced_dim():
    spec = _factory("OPQ64_256,IVF16384,PQ64", dim=768)
    assert spec["opq"] == 1 and spec["opq_dim"] == 256
    assert spec["dim"] == 768 and spec["m"] == 64 and spec["nlist"] == 16384


@pytest.mark.parametrize("tail,nbits", [("x4", 4), ("x8", 8), ("", 8)])
def test_factory_opq_widths(tail, nbits):
    spec = _factory(f"OPQ8_16,IVF12,PQ8{tail}", dim=32)
    assert spec["opq"] == 1 and spec["opq_dim"] == 16
    assert spec["m"] == 8 and spec["nbits"] == nbits


@pytest.mark.parametrize("tail,refine", [("RFlat", "fp32"),
                                         ("Refine(SQfp16)", "fp16")])
def test_factory_opq_refine(tail, refine):
    spec = _factory(f"OPQ8,IVF12,PQ8x4,{tail}", dim=32, k_factor=4,
                    opq_niter=5)
    assert spec["opq"] == 1 and spec["nbits"] == 4
    assert spec["refine"] == refine and spec["k_factor"] == 4.0
    assert spec["opq_niter"] == 5


def test_factory_opq_centroids_placeholder():
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory="OPQ16,IVF{centroids},PQ16", dim=64,
                 metric="dot", centroids=48), 10000)
    assert spec["nlist"] == 48 and spec["opq"] == 1 and spec["metric"] == 0


def test_factory_without_opq_is_unchanged():
    spec = _factory("IVF64,PQ16")
    assert not any(k in spec for k in OPQ_KEYS)


def test_knnlm_opq_keys():
    spec = resolve_engine_spec(
        IndexCfg(index_builder_type="knnlm", dim=64, centroids=16,
                 metric="l2", code_size=16, opq=1, opq_dim=32, opq_niter=4),
        1000)
    assert spec["type"] == "ivfpq" and spec["m"] == 16
    assert spec["opq"] == 1 and spec["opq_dim"] == 32
    assert spec["opq_niter"] == 4
    plain = resolve_engine_spec(
        IndexCfg(index_builder_type="knnlm", dim=64, centroids=16,
                 metric="l2", code_size=16, opq_dim=32), 1000)
    assert not any(k in plain for k in OPQ_KEYS)


def test_opq_keys_are_not_perf_knobs():
    # they change results, like REFINE_KEYS
    assert OPQ_KEYS == ("opq", "opq_dim", "opq_niter")
    assert not set(OPQ_KEYS) & set(ENGINE_PERF_KNOBS)
    # and other builders do not pick them up
    spec = resolve_engine_spec(
        IndexCfg(index_builder_type="ivfsq", dim=64, centroids=16,
                 metric="l2", opq=1), 1000)
    assert "opq" not in spec


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------


def test_factory_opq_m_mismatch_refused():
    with pytest.raises(NotImplementedError, match="OPQ m must equal"):
        _factory("OPQ32,IVF64,PQ16")


@pytest.mark.parametrize("s", ["OPQ16,IVF64,Flat", "OPQ16,IVF64,SQ8",
                               "OPQ16_32,IVF64,SQfp16",
                               "OPQ16,IVF64,SQ8,RFlat"])
def test_factory_opq_on_other_bases_refused(s):
    with pytest.raises(NotImplementedError, match="OPQ"):
        _factory(s)


@pytest.mark.parametrize("s", ["OPQ,IVF64,PQ16", "OPQ16_,IVF64,PQ16",
                               "OPQ16,PQ16", "OPQ16,Flat", "OPQ16",
                               "IVF64,OPQ16,PQ16", "OPQ16,OPQ16,IVF64,PQ16"])
def test_factory_opq_malformed_refused(s):
    # the message keeps the substrings earlier tests match
    with pytest.raises(NotImplementedError) as ei:
        _factory(s)
    msg = str(ei.value)
    assert "PQmx4" in msg and "RFlat" in msg and "OPQm" in msg


def test_factory_opq_other_width_refused():
    with pytest.raises(NotImplementedError, match=r"\[4, 8\]"):
        _factory("OPQ16,IVF64,PQ16x5")


# ---------------------------------------------------------------------------
# spec validation at create (no device is touched)
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
    lib.dfann_dim.argtypes = [ctypes.c_void_p]
    lib.dfann_transform_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.dfann_is_trained.argtypes = [ctypes.c_void_p]
    return lib


def _create(lib, **kw):
    spec = dict({"type": "ivfpq", "dim": 40, "metric": 1, "nlist": 8, "m": 8},
                **kw)
    h = ctypes.c_void_p()
    rc = lib.dfann_create(json.dumps(spec).encode(), ctypes.byref(h))
    return rc, h


def _info(lib, h):
    out = (ctypes.c_int64 * 3)()
    assert lib.dfann_transform_info(h, out) == 0
    return tuple(out)


@pytest.mark.parametrize("kw,d_out", [({}, 40), ({"opq_dim": 24}, 24),
                                      ({"opq_dim": 40}, 40),
                                      ({"opq_dim": 8, "nbits": 4}, 8)])
def test_create_opq_dims(lib, kw, d_out):
    rc, h = _create(lib, opq=1, **kw)
    assert rc == 0, lib.dfann_last_error()
    assert lib.dfann_dim(h) == 40  # the caller-facing dimension
    assert _info(lib, h) == (1, 40, d_out)
    assert lib.dfann_is_trained(h) == 0
    assert lib.dfann_destroy(h) == 0


def test_create_without_opq_reports_no_transform(lib):
    rc, h = _create(lib)
    assert rc == 0, lib.dfann_last_error()
    assert _info(lib, h) == (0, 40, 40)
    assert lib.dfann_destroy(h) == 0


def test_create_opq_lifts_the_dim_divisibility_to_opq_dim(lib):
    # dim = 44 is no multiple of m = 8, opq_dim = 24 is
    rc, h = _create(lib, dim=44, opq=1, opq_dim=24)
    assert rc == 0, lib.dfann_last_error()
    assert _info(lib, h) == (1, 44, 24)
    assert lib.dfann_destroy(h) == 0


@pytest.mark.parametrize("kw,key", [
    ({"type": "ivfsq", "opq": 1}, b"opq"),
    ({"type": "ivf_flat", "opq": 1}, b"opq"),
    ({"type": "flat", "opq": 1}, b"opq"),
    ({"opq": 1, "opq_dim": 48}, b"opq_dim"),       # > dim
    ({"opq": 1, "opq_dim": 20}, b"opq_dim"),       # % m != 0
    ({"dim": 44, "opq": 1}, b"opq_dim"),           # default d_out = dim
    ({"opq": 1, "pq_precomputed": 1}, b"pq_precomputed"),
    ({"opq_dim": 24}, b"opq_dim"),                 # without "opq"
])
def test_create_opq_refusals_name_the_key(lib, kw, key):
    rc, _h = _create(lib, **kw)
    assert rc != 0
    msg = lib.dfann_last_error()
    assert key in msg, msg


# ---------------------------------------------------------------------------
# the reference trainer's own sanity
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _trained():
    x = opq.recipe()
    A = opq.opq_train(x, m=8, ksub=16, niter=8)
    return x, A


def test_reference_rotation_is_orthonormal():
    _x, A = _trained()
    assert A.shape == (32, 32)
    assert opq.ortho_dev(A) < 1e-12
    # one rounding to float32: a few ulp of 1
    assert opq.ortho_dev(A.astype(np.float32)) < 8 * 2.0 ** -23


def test_reference_opq_beats_plain_pq():
    x, A = _trained()
    xc = opq.centred(x)
    plain = opq.pq_mse(xc, 8, 16)
    rot = opq.pq_mse(opq.transform(A.astype(np.float32), xc), 8, 16)
    print(f"plain PQ mse {plain:.2f}, OPQ mse {rot:.2f}, ratio {rot / plain:.3f}")
    assert rot <= 0.5 * plain


def test_reference_reduced_dim_rows_orthonormal():
    A = opq.opq_train(opq.recipe(), m=8, ksub=16, d_out=16, niter=2)
    assert A.shape == (16, 32)
    assert opq.ortho_dev(A) < 1e-12


def test_polar_svd_is_the_nearest_orthonormal():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((40, 24))
    P = opq.polar_svd(M)
    np.testing.assert_allclose(P.T @ P, np.eye(24), atol=1e-12)
    # M = P H with H symmetric positive definite
    H = P.T @ M
    np.testing.assert_allclose(H, H.T, atol=1e-10)
    assert np.linalg.eigvalsh((H + H.T) / 2).min() > 0


def test_signed_selection_is_exact():
    rng = np.random.default_rng(5)
    A = opq.signed_selection(40, 24, rng)
    assert (np.abs(A).sum(axis=1) == 1).all() and (np.abs(A).sum(axis=0) <= 1).all()
    x = rng.standard_normal((7, 40)).astype(np.float32)
    y = opq.transform(A, x)
    cols = np.abs(A).argmax(axis=1)
    np.testing.assert_array_equal(y, x[:, cols] * A[np.arange(24), cols])
