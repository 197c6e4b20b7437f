# GPU: remove_ids — rows deleted by arrival id, the inverted
# lists compacted physically, flat under tombstones.
#
# The reference for every check is code that already exists and is pinned to
# the oracle elsewhere: numpy masking of a get_lists dump taken BEFORE the
# removal, or search_filtered on a TWIN engine that got the same adds and
# never removed anything. The twin's search_filtered(allow = ~removed) and the
# removed engine's plain search differ only in which pinned kernel twin ran
# (a filter changes no row's arithmetic), so results are
# compared as float32 BITS — ivf_flat and flat included: both engines run the
# same kernels over the same row bytes, and no row's arithmetic depends on
# its position in the list.
#
# Shapes: d = 32, nlist = 8 with list sizes [0, 1, 63, 64, 65, 130, 300, 700]
# (an empty list, lists ending on and next to a 64-position word), nq = 16,
# k = 10 (register selector) and 100 (LDS selector), every list probed, ids
# spanning two adds.
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
    IP, L2, assert_bitwise, engine_with, ivf_spec, labels, queries, rand,
)

FLT_MAX = np.float32(3.4028235e38)
D_, NLIST, NQ = 32, 8, 16
SIZES = [0, 1, 63, 64, 65, 130, 300, 700]
N = sum(SIZES)  # 1323: no multiple of 32 or 64
SPLIT = 700
KINDS = {
    "ivf_flat": ("ivf_flat", {}),
    "pq8": ("ivfpq", {"m": 8}),
    "pq4": ("ivfpq", {"m": 8, "nbits": 4}),
    "opq": ("ivfpq", {"m": 8, "opq": 1}),
    "sqfp16": ("ivfsq", {"sq_type": "fp16"}),
    "sq8": ("ivfsq", {"sq_type": "8bit"}),
    "sq6": ("ivfsq", {"sq_type": "6bit"}),
    "sq4": ("ivfsq", {"sq_type": "4bit"}),
}
CODED = [k for k in KINDS if k != "ivf_flat"]
SETS = ["LIST", "ENDS", "WORD", "LISTB", "ALT", "NONE", "ALL"]


# ---------------------------------------------------------------------------
# data, engines, masks
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _base(kind, metric=L2, n_extra=0):
    """Spec, injected artifacts and rows of one index kind (read-only).
    Draws, in order: centroids, labels, row noise, codebooks, the OPQ
    matrix, the queries; then n_extra further rows (labels, noise)."""
    typ, kw = KINDS[kind]
    rng = np.random.default_rng(70)
    spec = ivf_spec(typ, D_, metric, NLIST, **kw)
    cent = (20.0 * rng.standard_normal((NLIST, D_))).astype(np.float32)
    lbl = labels(rng, SIZES)
    xb = cent[lbl] + 0.3 * rng.standard_normal((N, D_))
    cb = rng.standard_normal((8, 1 << kw.get("nbits", 8), D_ // 8))
    A = np.linalg.qr(rng.standard_normal((D_, D_)))[0]
    q = queries(rng, cent, NQ, metric)
    lbl2 = rng.integers(1, NLIST, n_extra)
    xb2 = cent[lbl2] + 0.3 * rng.standard_normal((n_extra, D_))
    art = {"cent": cent}
    if typ == "ivfpq":
        art["cb"] = cb.astype(np.float32)
    if kw.get("sq_type", "fp16") != "fp16":
        art["vmin"] = np.full(D_, -1.0, np.float32)
        art["vdiff"] = np.full(D_, 2.0, np.float32)
    if kw.get("opq"):
        # the index works on y = A x: rows and queries are built at y
        art["A"] = A.astype(np.float32)
        xb, xb2, q = xb @ A, xb2 @ A, q @ A
    out = {"spec": spec, "art": art, "xb": xb.astype(np.float32),
           "xb2": xb2.astype(np.float32), "q": np.ascontiguousarray(q, np.float32)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _engine(b, batches, **spec_kw):
    spec = dict(b["spec"], **spec_kw)
    art = b["art"]
    if "A" in art:  # the transform has to be there before the artifacts
        eng = HipEngine(spec=spec)
        eng.set_transform(art["A"])
        eng.set_trained(art["cent"], art.get("cb"), None, None)
    else:
        eng = engine_with(spec, art["cent"], art.get("cb"), art.get("vmin"),
                          art.get("vdiff"))
    for x in batches:
        eng.add(x)
    return eng


def _two_adds(b):
    return [b["xb"][:SPLIT], b["xb"][SPLIT:]]


@functools.lru_cache(maxsize=None)
def _twin(kind, metric=L2, **spec_kw):
    """The engine that never removes anything, and its lists (read-only)."""
    b = _base(kind, metric)
    eng = _engine(b, _two_adds(b), **dict(spec_kw))
    dump = eng.get_lists()
    for a in dump:
        a.setflags(write=False)
    np.testing.assert_array_equal(np.diff(dump[0]), SIZES)
    return eng, dump


def _mask(name, dump, n=N):
    """bool mask over ids of the rows to remove, from CSR positions of the
    pre-removal dump."""
    off, ids, _ = dump
    if name == "LIST":       # a whole list
        pos = np.arange(off[5], off[6])
    elif name == "ENDS":     # first and last row of a list
        pos = np.array([off[6], off[7] - 1])
    elif name == "WORD":     # a run across a 64-position word boundary
        pos = np.arange(634, 646)  # inside list 7, across position 640
        assert off[7] <= pos[0] and pos[0] // 64 != pos[-1] // 64
    elif name == "LISTB":    # a run across a list boundary
        pos = np.arange(off[7] - 3, off[7] + 3)
    elif name == "ALT":      # every other row
        pos = np.arange(0, ids.shape[0], 2)
    elif name == "NONE":
        pos = np.arange(0)
    elif name == "ALL":
        pos = np.arange(ids.shape[0])
    elif name == "MIX":      # the four local shapes together
        return (_mask("LIST", dump, n) | _mask("ENDS", dump, n)
                | _mask("WORD", dump, n) | _mask("LISTB", dump, n))
    elif name == "FEW":      # 14 rows: a removed top-10 sits in the twin's top-24
        return _mask("ENDS", dump, n) | _mask("WORD", dump, n)
    else:
        raise KeyError(name)
    m = np.zeros(n, bool)
    m[ids[pos]] = True
    return m


def _masked_dump(dump, removed):
    """The dump with the rows of removed ids deleted (numpy)."""
    off, ids, codes = dump
    keep = ~removed[ids]
    new_off = np.concatenate([[0], np.cumsum(keep)])[off]
    return new_off.astype(np.int64), ids[keep], codes[keep]


def _assert_lists(eng, ref):
    off, ids, codes = eng.get_lists()
    np.testing.assert_array_equal(off, ref[0])
    np.testing.assert_array_equal(ids, ref[1])
    np.testing.assert_array_equal(codes, ref[2])  # all stride bytes
    assert eng.nlive == ref[1].shape[0]


def _pads(D, I, metric):
    assert (I == -1).all()
    assert (D == (FLT_MAX if metric == L2 else -FLT_MAX)).all()


# ---------------------------------------------------------------------------
# 1. lists
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_lists_equal_masked_dump(kind, name):
    b = _base(kind)
    _, dump = _twin(kind)
    removed = _mask(name, dump)
    eng = _engine(b, _two_adds(b))
    eng.search(b["q"], 10)  # finalized before the removal
    assert eng.remove_ids(removed) == removed.sum()
    assert eng.ntotal == N and eng.nlive == N - removed.sum()
    _assert_lists(eng, _masked_dump(dump, removed))


@pytest.mark.parametrize("how", ["ids", "packed"])
def test_remove_while_rows_are_pending(how):
    """An add with no search before the removal: pending rows are merged in
    first and are removable. Also the two other argument forms."""
    b = _base("pq8")
    _, dump = _twin("pq8")
    removed = _mask("MIX", dump)
    eng = _engine(b, _two_adds(b))
    arg = (np.flatnonzero(removed) if how == "ids"
           else eng.pack_filter(removed))
    assert eng.remove_ids(arg) == removed.sum()
    _assert_lists(eng, _masked_dump(dump, removed))


# ---------------------------------------------------------------------------
# 2. slab window
# ---------------------------------------------------------------------------


def test_slab_window():
    """slab_mb = 1 with ivf_flat at d = 64: stride 256 B, 4096 rows per slab;
    10 000 rows in three slabs, 40 % removed, once finalized and once with
    the second add still pending."""
    d, n = 64, 10000
    rng = np.random.default_rng(71)
    cent = (20.0 * rng.standard_normal((NLIST, d))).astype(np.float32)
    lbl = rng.integers(0, NLIST, n)
    xb = (cent[lbl] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    removed = rng.random(n) < 0.4
    spec = ivf_spec("ivf_flat", d, L2, NLIST, slab_mb=1)
    twin = engine_with(spec, cent, xb=xb, split=6000)
    assert twin.get_lists()[2].shape == (n, 256)
    ref = _masked_dump(twin.get_lists(), removed)
    for finalize in (True, False):
        eng = engine_with(spec, cent, xb=xb, split=6000)
        if finalize:
            eng.get_lists()
        assert eng.remove_ids(removed) == removed.sum()
        _assert_lists(eng, ref)
    # the compacted slabs take adds like any other
    eng.add(xb[:100])
    assert eng.ntotal == n + 100 and eng.nlive == n + 100 - removed.sum()
    off, ids, _ = eng.get_lists()
    assert np.isin(np.arange(n, n + 100), ids).all()
    assert not removed[ids[ids < n]].any()


# ---------------------------------------------------------------------------
# 3. search
# ---------------------------------------------------------------------------


def _radius(twin, q, metric):
    D, _ = twin.search(q, 100)
    return float(np.median(D[:, 50]))


@pytest.mark.parametrize("name", ["MIX", "ALT"])
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_search_equals_twin_filtered(kind, metric, name):
    b = _base(kind, metric)
    twin, dump = _twin(kind, metric)
    removed = _mask(name, dump)
    allow = ~removed
    q = b["q"]
    eng = _engine(b, _two_adds(b))
    assert eng.remove_ids(removed) == removed.sum()
    for k in (10, 100):
        D, I = eng.search(q, k)
        Dt, It = twin.search_filtered(q, k, allow)
        assert not removed[I[I >= 0]].any()
        assert_bitwise(D, I, Dt, It)
    # preassigned, on the twin's probes
    probes, keys = twin.coarse(q, NLIST)
    D, I = eng.search_preassigned(q, probes, keys, 10)
    assert_bitwise(D, I, *twin.search_preassigned_filtered(
        q, probes, keys, 10, allow))
    # a further bitmap on top: the twin gets the two ANDed
    extra = np.arange(N) % 3 != 0
    for k in (10, 100):
        D, I = eng.search_filtered(q, k, extra)
        assert_bitwise(D, I, *twin.search_filtered(q, k, allow & extra))
    # range: lims, D and I
    r = _radius(twin, q, metric)
    lims, D, I = eng.range_search(q, r)
    lt, Dt, It = twin.range_search(q, r, allow)
    assert lims[-1] > 0
    np.testing.assert_array_equal(lims, lt)
    assert_bitwise(D, I, Dt, It)
    lims, D, I = eng.range_search(q, r, extra)
    lt, Dt, It = twin.range_search(q, r, allow & extra)
    np.testing.assert_array_equal(lims, lt)
    assert_bitwise(D, I, Dt, It)


@pytest.mark.parametrize("kind", list(KINDS))
def test_reconstruct_rows_equal_twin(kind):
    b = _base(kind)
    twin, dump = _twin(kind)
    removed = _mask("FEW", dump)
    eng = _engine(b, _two_adds(b))
    eng.remove_ids(removed)
    D, I, R = eng.search_and_reconstruct(b["q"], 10)
    assert (I >= 0).all() and not removed[I].any()
    # 14 rows are gone: the removed engine's top-10 is inside the twin's top-24
    _, It, Rt = twin.search_and_reconstruct(b["q"], 24)
    for i in range(NQ):
        for j in range(10):
            hit = np.flatnonzero(It[i] == I[i, j])
            assert hit.size == 1
            np.testing.assert_array_equal(R[i, j].view(np.uint32),
                                          Rt[i, hit[0]].view(np.uint32))


@pytest.mark.parametrize("codec", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["pq8", "sq8"])
def test_refine_equals_twin(kind, codec):
    """A refine index re-ranks over the compacted base stage; the twin
    re-ranks over its filtered base stage (the filter applies there only)."""
    kw = (("refine", codec), ("k_factor", 4.0))
    b = _base(kind)
    twin, dump = _twin(kind, L2, **dict(kw))
    removed = _mask("MIX", dump)
    eng = _engine(b, _two_adds(b), **dict(kw))
    assert eng.remove_ids(removed) == removed.sum()
    for k in (10, 100):
        D, I = eng.search(b["q"], k)
        assert_bitwise(D, I, *twin.search_filtered(b["q"], k, ~removed))
    # the store is indexed by arrival id: it keeps ntotal rows, holes included
    assert eng.refine_info()[2] == N
    np.testing.assert_array_equal(eng.get_refine_rows(), twin.get_refine_rows())


# ---------------------------------------------------------------------------
# 4. scan_rows: the rows are gone, not masked
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["ivf_flat", "pq8", "sq8"])
def test_scan_rows_counts_live_rows(kind):
    b = _base(kind)
    _, dump = _twin(kind)
    removed = _mask("ALT", dump)
    eng = _engine(b, _two_adds(b))
    eng.remove_ids(removed)
    eng.set_timing(True)
    eng.get_timing()
    eng.search(b["q"], 10)  # every list probed
    assert eng.get_timing()["scan_rows"] == NQ * (N - removed.sum())


# ---------------------------------------------------------------------------
# 5. ids are not reused
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["ivf_flat", "pq4", "sq6"])
def test_ids_are_not_reused(kind):
    n2 = 333
    b = _base(kind, L2, n2)
    twin = _engine(b, _two_adds(b) + [b["xb2"]])
    dump2 = twin.get_lists()
    _, dump = _twin(kind)
    m1 = np.concatenate([_mask("MIX", dump), np.zeros(n2, bool)])
    eng = _engine(b, _two_adds(b))
    assert eng.remove_ids(m1[:N]) == m1.sum()
    eng.add(b["xb2"])
    assert eng.ntotal == N + n2 and eng.nlive == N + n2 - m1.sum()
    _assert_lists(eng, _masked_dump(dump2, m1))
    if kind == "ivf_flat":  # (coded rows may tie with an older row)
        _, I = eng.search(b["xb2"][:NQ], 1)
        np.testing.assert_array_equal(I[:, 0], np.arange(N, N + NQ))
    # a second removal on top, naming old ids, new ids and ids already gone
    m2 = _mask("ALT", dump2, N + n2)
    assert eng.remove_ids(m2) == (m2 & ~m1).sum()
    _assert_lists(eng, _masked_dump(dump2, m1 | m2))
    assert eng.ntotal == N + n2


# ---------------------------------------------------------------------------
# 6. idempotence and determinism
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["ivf_flat", "pq8", "sqfp16"])
def test_idempotent_and_deterministic(kind):
    b = _base(kind)
    _, dump = _twin(kind)
    removed = _mask("MIX", dump)
    e1, e2 = _engine(b, _two_adds(b)), _engine(b, _two_adds(b))
    assert e1.remove_ids(removed) == e2.remove_ids(removed) == removed.sum()
    d1 = e1.get_lists()
    for a, c in zip(d1, e2.get_lists()):
        np.testing.assert_array_equal(a, c)
    assert e1.remove_ids(removed) == 0
    assert e1.remove_ids(np.zeros(N, bool)) == 0
    for a, c in zip(d1, e1.get_lists()):
        np.testing.assert_array_equal(a, c)
    assert e1.nlive == N - removed.sum()


def test_nothing_to_remove():
    """An index with no rows and an untrained one return 0."""
    b = _base("pq8")
    eng = _engine(b, [])
    assert eng.remove_ids(np.ones(8, bool)) == 0
    assert eng.ntotal == 0 and eng.nlive == 0
    raw = HipEngine(spec=b["spec"])
    assert not raw.is_trained
    assert raw.remove_ids(np.zeros(0, bool)) == 0


# ---------------------------------------------------------------------------
# 7. remove everything
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("kind", ["ivf_flat", "pq8", "sq4"])
def test_remove_everything(kind, metric):
    b = _base(kind, metric)
    eng = _engine(b, _two_adds(b))
    assert eng.remove_ids(np.ones(N, bool)) == N
    assert eng.nlive == 0 and eng.ntotal == N
    q = b["q"]
    for k in (10, 100):
        _pads(*eng.search(q, k), metric)
    _pads(*eng.search_filtered(q, 10, np.ones(N, bool)), metric)
    probes, keys = eng.coarse(q, NLIST)
    _pads(*eng.search_preassigned(q, probes, keys, 10), metric)
    lims, D, I = eng.range_search(q, 1e30 if metric == L2 else -1e30)
    assert (lims == 0).all() and D.size == 0 and I.size == 0
    off, ids, codes = eng.get_lists()
    assert (off == 0).all() and ids.size == 0 and codes.shape[0] == 0
    # a later add is searchable, under new ids
    eng.add(b["xb"][:50])
    assert eng.ntotal == N + 50 and eng.nlive == 50
    _, I = eng.search(b["xb"][:NQ], 1)
    assert ((I >= N) & (I < N + 50)).all()
    # (under IP a row need not be its own best match; coded rows may tie)
    if kind == "ivf_flat" and metric == L2:
        np.testing.assert_array_equal(I[:, 0], np.arange(N, N + NQ))


# ---------------------------------------------------------------------------
# 8. flat: tombstones
# ---------------------------------------------------------------------------

FLAT_N, FLAT_D = 5003, 48


@functools.lru_cache(maxsize=None)
def _flat_twin(metric):
    # ws_mb = 1: database chunks of 4096 + 907 rows
    spec = {"type": "flat", "dim": FLAT_D, "metric": metric, "ws_mb": 1}
    xb, q = rand(FLAT_N, FLAT_D, 72), rand(NQ, FLAT_D, 73)
    eng = HipEngine(spec=spec)
    eng.add(xb)
    return spec, xb, q, eng


def _flat_engine(metric):
    spec, xb, q, twin = _flat_twin(metric)
    eng = HipEngine(spec=spec)
    eng.add(xb[:3000])
    eng.add(xb[3000:])
    return eng, twin, xb, q


@pytest.mark.parametrize("metric", [IP, L2])
def test_flat(metric):
    eng, twin, xb, q = _flat_engine(metric)
    ids = np.arange(FLAT_N)
    removed = (ids % 2 == 0) | ((ids >= 4090) & (ids < 4100))
    assert eng.remove_ids(removed) == removed.sum()
    assert eng.ntotal == FLAT_N and eng.nlive == FLAT_N - removed.sum()
    extra = ids % 3 != 0
    for k in (10, 100):
        D, I = eng.search(q, k)
        assert (I >= 0).all() and not removed[I].any()
        assert_bitwise(D, I, *twin.search_filtered(q, k, ~removed))
        D, I = eng.search_filtered(q, k, extra)
        assert (I >= 0).all()
        assert_bitwise(D, I, *twin.search_filtered(q, k, ~removed & extra))
    # the same ids again: nothing; then all but 7 rows: 7 results and pads
    assert eng.remove_ids(removed) == 0
    last = np.ones(FLAT_N, bool)
    last[[33, 77, 79, 4001, 5001, 4097, 4099]] = False  # the last two are gone
    assert eng.remove_ids(last) == FLAT_N - removed.sum() - 5
    _, I = eng.search(q, 10)
    assert ((I >= 0).sum(axis=1) == 5).all()
    assert set(I[I >= 0]) == {33, 77, 79, 4001, 5001}
    # new rows are live, under new ids
    eng.add(xb[100:140])
    assert eng.ntotal == FLAT_N + 40 and eng.nlive == 45
    _, I = eng.search(xb[100:100 + NQ], 1)
    assert (I >= 0).all()
    if metric == L2:  # (under IP a row need not be its own best match)
        np.testing.assert_array_equal(I[:, 0], np.arange(FLAT_N, FLAT_N + NQ))
    # everything: pads
    assert eng.remove_ids(np.ones(FLAT_N + 40, bool)) == 45
    _pads(*eng.search(q, 10), metric)


# ---------------------------------------------------------------------------
# 9. persistence
# ---------------------------------------------------------------------------


def _magic(path):
    with open(path, "rb") as f:
        return f.read(7)


@pytest.mark.parametrize("kind", ["ivf_flat", "pq8", "opq", "sq6"])
def test_persistence_roundtrip(kind, tmp_path):
    b = _base(kind)
    _, dump = _twin(kind)
    removed = _mask("MIX", dump)
    eng = _engine(b, _two_adds(b))
    p1, p2 = str(tmp_path / "a.dfann"), str(tmp_path / "b.dfann")
    eng.save(p1)
    assert _magic(p1) == b"DFANN01"
    eng.remove_ids(removed)
    eng.save(p2)
    assert _magic(p2) == b"DFANN02"
    old = HipProvider().load(p1)
    assert old.ntotal == old.nlive == N
    for a, c in zip(old.get_lists(), dump):
        np.testing.assert_array_equal(a, c)
    got = HipProvider().load(p2)
    assert got.ntotal == N and got.nlive == N - removed.sum()
    _assert_lists(got, eng.get_lists())
    got.nprobe = eng.nprobe = NLIST
    for k in (10, 100):
        assert_bitwise(*got.search(b["q"], k), *eng.search(b["q"], k))
    D, I, R = got.search_and_reconstruct(b["q"], 10)
    De, Ie, Re = eng.search_and_reconstruct(b["q"], 10)
    assert_bitwise(D, I, De, Ie)
    np.testing.assert_array_equal(R, Re)
    # the loaded index goes on: ids from ntotal, removal again
    got.add(b["xb"][:10])
    assert got.ntotal == N + 10
    assert got.remove_ids(np.arange(N, N + 10)) == 10
    _assert_lists(got, eng.get_lists())


def test_persistence_refine_and_remove_all(tmp_path):
    kw = {"refine": "fp32", "k_factor": 4.0}
    b = _base("pq8")
    _, dump = _twin("pq8")
    removed = _mask("ALT", dump)
    eng = _engine(b, _two_adds(b), **kw)
    eng.remove_ids(removed)
    p = str(tmp_path / "r.dfann")
    eng.save(p)
    got = HipProvider().load(p)
    assert got.refine_info() == eng.refine_info() and got.refine_info()[2] == N
    assert_bitwise(*got.search(b["q"], 10), *eng.search(b["q"], 10))
    eng.remove_ids(np.ones(N, bool))
    eng.save(p)
    got = HipProvider().load(p)
    assert got.ntotal == N and got.nlive == 0
    _pads(*got.search(b["q"], 10), L2)
    got.add(b["xb"][:5])
    assert set(got.get_lists()[1]) == set(range(N, N + 5))


def test_persistence_flat(tmp_path):
    eng, twin, xb, q = _flat_engine(L2)
    p1, p2 = str(tmp_path / "a.dfann"), str(tmp_path / "b.dfann")
    eng.save(p1)
    assert _magic(p1) == b"DFANN01"
    removed = np.arange(FLAT_N) % 5 == 1
    eng.remove_ids(removed)
    eng.save(p2)
    assert _magic(p2) == b"DFANN02"
    got = HipProvider().load(p2)
    assert got.ntotal == FLAT_N and got.nlive == FLAT_N - removed.sum()
    for k in (10, 100):
        assert_bitwise(*got.search(q, k), *eng.search(q, k))
        assert_bitwise(*got.search(q, k), *twin.search_filtered(q, k, ~removed))


# ---------------------------------------------------------------------------
# 10. errors
# ---------------------------------------------------------------------------


def test_hnswsq_is_refused():
    xb = rand(300, D_, 74)
    eng = HipEngine(spec={"type": "hnswsq", "dim": D_, "metric": L2, "m": 8,
                          "ef_construction": 40, "nprobe": 32, "seed": 1234})
    eng.train(xb)
    eng.add(xb)
    before = eng.search(xb[:NQ], 5)
    with pytest.raises(RuntimeError, match="remove_ids unsupported for hnswsq"):
        eng.remove_ids(np.ones(300, bool))
    assert eng.ntotal == eng.nlive == 300
    assert_bitwise(*eng.search(xb[:NQ], 5), *before)


@pytest.mark.parametrize("kind", ["pq8", "flat"])
def test_short_bitmap_is_refused(kind):
    if kind == "flat":
        eng, _, _, q = _flat_engine(L2)
        n = FLAT_N
    else:
        b = _base(kind)
        eng, q, n = _engine(b, _two_adds(b)), b["q"], N
    before = eng.search(q, 10)
    short = eng.pack_filter(np.ones(n - 1, bool))
    with pytest.raises(RuntimeError,
                       match=f"bitmap covers {n - 1} ids but the index holds {n}"):
        eng.remove_ids(short)
    with pytest.raises(ValueError, match="id outside"):
        eng.remove_ids(np.array([0, n]))
    assert eng.ntotal == eng.nlive == n
    assert_bitwise(*eng.search(q, 10), *before)
