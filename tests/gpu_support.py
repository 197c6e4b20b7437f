# Helpers shared by the GPU test files (a plain module: no fixtures, no
# hooks). Each file keeps its own constants (list sizes, query count, seeds,
# spreads, split point) and passes them in. Every helper that draws random
# numbers draws from the CALLER's generator, in a fixed order that the
# docstring states: the data of a test is a function of its seed alone.
import time

import numpy as np

from distributed_faiss_amd.hip_engine import HipEngine

IP, L2 = 0, 1


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------


def rand(n, d, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def clustered(nlist, per, d, seed=0, sep=20.0, sigma=0.05):
    """Well-separated clusters: assignment unambiguous for engine & oracle."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((nlist, d)).astype(np.float32) * sep
    lbl = rng.integers(0, nlist, nlist * per)
    x = cent[lbl] + sigma * rng.standard_normal((nlist * per, d)).astype(np.float32)
    return cent, x.astype(np.float32)


def labels(rng, list_sizes):
    """List label per row, list l holding list_sizes[l] rows, shuffled (one
    rng.shuffle)."""
    lbl = np.repeat(np.arange(len(list_sizes)), list_sizes)
    rng.shuffle(lbl)
    return lbl


def queries(rng, cent, nq, metric):
    """cent[l] + 0.7 N(0,1) (draws: integers(0, nlist, nq), then
    standard_normal((nq, d))). Under IP every other query is then made
    orthogonal to all centroids: its bias q.c is ~0, so the low bits of
    the scan's own sum reach the result instead of being rounded away
    under a bias of magnitude |c|^2 (the other half keeps the bias)."""
    nlist, d = cent.shape
    q = (cent[rng.integers(0, nlist, nq)]
         + 0.7 * rng.standard_normal((nq, d)))
    if metric == IP:
        c64 = cent.astype(np.float64)
        coef = np.linalg.lstsq(c64.T, q[::2].T, rcond=None)[0]
        q[::2] -= (c64.T @ coef).T
    return q.astype(np.float32)


def codeword_rows(rng, cb, lbl, gap, min_iso):
    """(nrows, m) int64 codeword per row and sub-quantizer, drawn (one
    rng.choice per sub-quantizer) among the codewords at least `gap` away
    from every other one of their codebook, so that the GEMM-decomposed
    engine encode and the sequential oracle encode pick the same codes. A
    quarter of each list of >= 4 rows then repeats the codes of another row
    of that list (one rng.choice per such list): exact distance ties."""
    m, nrows = cb.shape[0], lbl.shape[0]
    cw = np.empty((nrows, m), np.int64)
    for j in range(m):
        c64 = cb[j].astype(np.float64)
        dist = np.sqrt(((c64[:, None, :] - c64[None, :, :]) ** 2).sum(-1))
        np.fill_diagonal(dist, np.inf)
        iso = np.flatnonzero(dist.min(axis=1) > gap)
        assert iso.size >= min_iso
        cw[:, j] = rng.choice(iso, nrows)
    for l in range(int(lbl.max()) + 1):
        rows = np.flatnonzero(lbl == l)
        if rows.size >= 4:
            dup = rows[: rows.size // 4]
            cw[dup] = cw[rng.choice(rows[rows.size // 4:], dup.size)]
    return cw


def decode_rows(cb, cw):
    """(nrows, m * dsub): the codewords of cw, side by side."""
    return np.concatenate([cb[j][cw[:, j]] for j in range(cb.shape[0])], axis=1)


def bf16_round(a):
    """k_f32_to_bf16's integer formula: (u + 0x7FFF + lsb) >> 16."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    lsb = (u >> np.uint64(16)) & np.uint64(1)
    r = ((u + np.uint64(0x7FFF) + lsb) >> np.uint64(16)) & np.uint64(0xFFFF)
    return (r << np.uint64(16)).astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------


def ivf_spec(typ, d, metric, nlist, **kw):
    """Every list probed, the suite's seed."""
    return dict({"type": typ, "dim": d, "metric": metric, "nlist": nlist,
                 "nprobe": nlist, "seed": 1234}, **kw)


def engine_with(spec, cent, cb=None, vmin=None, vdiff=None, xb=None,
                split=None):
    """A HipEngine with injected trained artifacts; xb, if given, is added
    in one call or, with `split`, in two (arrival ids across adds)."""
    eng = HipEngine(spec=spec)
    eng.set_trained(cent, cb, vmin, vdiff)
    if xb is not None:
        for part in ([xb] if split is None else [xb[:split], xb[split:]]):
            eng.add(part)
    return eng


def wait_trained(idx, ntotal=None):
    """Poll an Index until it is TRAINED (and, with ntotal, holds that many
    rows)."""
    from distributed_faiss_amd.index_state import IndexState

    t0 = time.time()
    while time.time() - t0 < 30:
        if idx.get_state() == IndexState.TRAINED and (
                ntotal is None or idx.engine.ntotal == ntotal):
            return
        time.sleep(0.01)
    raise AssertionError("index did not reach TRAINED")


# ---------------------------------------------------------------------------
# assertions
# ---------------------------------------------------------------------------


def assert_bitwise(D, I, Dr, Ir):
    """Ids equal, distances equal as float32 BITS."""
    D, Dr = np.asarray(D), np.asarray(Dr)
    np.testing.assert_array_equal(I, Ir)
    assert D.dtype == np.float32 and Dr.dtype == np.float32
    np.testing.assert_array_equal(D.view(np.uint32), Dr.view(np.uint32))


def assert_lists_equal(eng, orc, list_sizes=None, lbl=None):
    """The engine's inverted lists (get_lists) against the oracle's
    (packed_lists): offsets, ids and every stored byte up to the row's
    code bytes. With list_sizes / lbl the oracle's own lists are first
    checked to be the intended ones. Returns the engine's rows, stride
    padding included."""
    off_o, ids_o, rows_o = orc.packed_lists()
    if list_sizes is not None:
        np.testing.assert_array_equal(np.diff(off_o), list_sizes)
    if lbl is not None:
        np.testing.assert_array_equal(
            ids_o, np.concatenate([np.flatnonzero(lbl == l)
                                   for l in range(orc.nlist)]))
    off, ids, rows = eng.get_lists()
    np.testing.assert_array_equal(off, off_o)
    np.testing.assert_array_equal(ids, ids_o)
    np.testing.assert_array_equal(rows[:, :rows_o.shape[1]], rows_o)
    return rows
