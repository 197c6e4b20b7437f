# ORACLE refine — restatement of the engine's refine stage (k_refine in
# csrc/kernels.hip), op for op in float32, so the GPU tests
# can compare D and I bitwise.
#
# Per candidate row, lane g in [0, 16) owns the 8-element chunks starting at
# t0 = 8g, 8g + 128, ...; inside a lane `part = part + term` runs in
# ascending t (t < d), no fused multiply-add; the 16 partials then meet in
# an xor butterfly with strides 8, 4, 2, 1. term = (q_t - x_t)^2 for L2 and
# q_t * x_t for IP, x_t being the STORED value (fp16 or fp32) widened to
# float32. Selection is by (key, ascending id), key = distance (L2) or -dot
# (IP), through the engine's monotone uint encoding of the key, so the
# order is total even when a key is NaN. Candidates that are -1 never
# enter; unfilled slots carry I = -1, D = +FLT_MAX (L2) / -FLT_MAX (IP).
import math

import numpy as np

IP, L2 = 0, 1
FLT_MAX = np.float32(3.4028235e38)
K_CAP = 512
LANES = 16
CHUNK = 8


def k_prime(k, k_factor):
    """The engine's k' rule: min(512, max(k, ceil(k * k_factor))), a product
    within 1e-4 above an integer counting as that integer (k_factor travels
    as float32)."""
    kf = float(np.float32(k_factor))
    return min(K_CAP, max(k, int(math.ceil(k * kf - 1e-4))))


def lane_partials(q, X, metric):
    """q (..., d) float32, X (..., d) float32 (already widened) ->
    (..., 16) float32 per-lane partial sums in the kernel's order."""
    d = q.shape[-1]
    part = np.zeros(X.shape[:-1] + (LANES,), np.float32)
    g = np.arange(LANES)
    with np.errstate(all="ignore"):
        for c0 in range(0, d, LANES * CHUNK):
            for j in range(CHUNK):
                t = c0 + CHUNK * g + j
                live = t < d
                if not live.any():
                    continue
                tl = t[live]
                qv = q[..., tl]
                xv = X[..., tl]
                if metric == IP:
                    term = qv * xv
                else:
                    df = qv - xv
                    term = df * df
                part[..., live] = part[..., live] + term.astype(np.float32)
    return part


def butterfly(part):
    """xor butterfly over the 16 lanes (strides 8, 4, 2, 1); every lane ends
    with the same bits, lane 0 is returned."""
    g = np.arange(LANES)
    with np.errstate(all="ignore"):
        for s in (8, 4, 2, 1):
            part = part + part[..., g ^ s]
    return part[..., 0]


def refine_distances(q, X, metric):
    """Exact-stage value per row: squared L2 distance or dot product."""
    q = np.ascontiguousarray(q, np.float32)
    X = np.ascontiguousarray(X).astype(np.float32)
    return butterfly(lane_partials(q, X, metric))


def _enc(key):
    u = np.ascontiguousarray(key, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def refine_ref(q, store, cand_I, k, metric):
    """q (nq, d) float32; store (n, d) float16 or float32 — the raw rows as
    the engine keeps them; cand_I (nq, k') int64 base-stage ids (-1 pads).
    Returns (D (nq, k) float32, I (nq, k) int64)."""
    q = np.ascontiguousarray(q, np.float32)
    cand_I = np.asarray(cand_I, np.int64)
    nq, kp = cand_I.shape
    assert kp <= K_CAP and k <= kp
    valid = cand_I >= 0
    X = store[np.where(valid, cand_I, 0)].astype(np.float32)  # (nq, kp, d)
    val = butterfly(lane_partials(q[:, None, :], X, metric))   # (nq, kp)
    with np.errstate(all="ignore"):
        key = (-val if metric == IP else val).astype(np.float32)
    comp = (_enc(key).astype(np.uint64) << np.uint64(32)) | \
        cand_I.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    comp = np.where(valid, comp, np.uint64(0xFFFFFFFFFFFFFFFF))
    order = np.argsort(comp, axis=1, kind="stable")[:, :k]
    D = np.take_along_axis(val.astype(np.float32), order, axis=1)
    I = np.take_along_axis(cand_I, order, axis=1)
    ok = np.take_along_axis(valid, order, axis=1)
    D = np.where(ok, D, FLT_MAX if metric == L2 else -FLT_MAX).astype(np.float32)
    I = np.where(ok, I, -1).astype(np.int64)
    return D, I
