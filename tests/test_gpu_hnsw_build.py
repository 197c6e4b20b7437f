# hnswsq BUILD parity: the engine's graph against the CPU restatement
# (oracle/hnsw.py OracleHNSWBuild), bit for bit, and the search over it.
#
# Per case (tests/hnsw_cases.py): train the engine on the data, take its
# vmin/vdiff, build with the engine and with the oracle, compare levels,
# upslot, entry, maxlevel, nslots, the counts, the live neighbour prefixes
# and — because the oracle mimics the in-place writes — the whole rows
# (those bytes are what persistence stores). Then queries go through
# OracleHNSWSearch over the ORACLE'S OWN graph and must equal the engine's
# (D, I) bitwise: build and search pinned end to end with no shared dump.
#
# Localisation: every case also runs with hnsw_refine = 0 and the data
# added as 1 row and then chunks of at most 256, so each add is exactly
# one wave; the dumps are compared after every add and a mismatch names
# the wave and the first differing node.
#
# Every case asserts the oracle counter of the branch it is there for, so
# it cannot silently stop reaching it.
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
from hnsw_cases import (  # noqa: E402
    CASES,
    TRUNC_ENTRY,
    case_data,
    case_seed,
    clustered,
)
from oracle import OracleHNSWBuild, OracleHNSWSearch  # noqa: E402

FLT_MAX = np.float32(3.402823466e+38)


def _spec(name, refine):
    c = CASES[name]
    return {"type": "hnswsq", "dim": c["d"], "metric": 1, "m": c["M"],
            "ef_construction": c["efc"], "nprobe": 16, "seed": case_seed(name),
            "hnsw_refine": refine}


def _first_diff(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.shape[0] == 0:
        return -1
    bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
    return int(bad[0]) if bad.size else -1


def _assert_same_graph(ge, go, where):
    """engine dump ge == oracle dump go; a mismatch names `where` and the
    first differing node."""
    for k in ("M", "deg0", "efc", "nslots", "entry", "maxlevel"):
        assert int(ge[k]) == int(go[k]), f"{where}: {k} engine {ge[k]} oracle {go[k]}"
    ns = int(go["nslots"])
    for k in ("levels", "upslot", "cnt0"):
        i = _first_diff(ge[k], go[k])
        assert i < 0, f"{where}: {k}[{i}] engine {ge[k][i]} oracle {go[k][i]}"
    # with nslots == 0 the engine's cntU/nbrU dump is one unwritten row
    i = _first_diff(ge["cntU"][:ns], go["cntU"][:ns])
    assert i < 0, f"{where}: cntU[slot {i}] engine {ge['cntU'][i]} oracle {go['cntU'][i]}"
    # live prefixes
    live0 = np.arange(go["deg0"])[None, :] < go["cnt0"][:, None]
    i = _first_diff(np.where(live0, ge["nbr0"], -2), np.where(live0, go["nbr0"], -2))
    assert i < 0, (f"{where}: level-0 links of node {i}: engine "
                   f"{ge['nbr0'][i][:ge['cnt0'][i]]} oracle {go['nbr0'][i][:go['cnt0'][i]]}")
    liveU = np.arange(go["M"])[None, None, :] < go["cntU"][:ns, :, None]
    i = _first_diff(np.where(liveU, ge["nbrU"][:ns], -2),
                    np.where(liveU, go["nbrU"][:ns], -2))
    assert i < 0, (f"{where}: upper links of slot {i} (node "
                   f"{int(np.flatnonzero(go['upslot'] == i)[0]) if i >= 0 else -1}): "
                   f"engine {ge['nbrU'][i].tolist()} oracle {go['nbrU'][i].tolist()}")
    # whole rows, stale slots past the counts included
    i = _first_diff(ge["nbr0"], go["nbr0"])
    assert i < 0, f"{where}: stale level-0 slots of node {i}: engine {ge['nbr0'][i]} oracle {go['nbr0'][i]}"
    i = _first_diff(ge["nbrU"][:ns], go["nbrU"][:ns])
    assert i < 0, f"{where}: stale upper slots of slot {i}"


def _build_pair(name, refine, chunks):
    """Engine and oracle fed the same add calls; the dumps after every add."""
    c = CASES[name]
    train, add = case_data(name)
    eng = HipEngine(spec=_spec(name, refine))
    eng.train(train)
    vmin, vdiff = eng.get_sq_params()
    orc = OracleHNSWBuild(c["d"], c["M"], c["efc"], case_seed(name), vmin, vdiff,
                          refine=refine)
    dumps = []
    s = 0
    for ch in chunks:
        eng.add(add[s:s + ch])
        orc.add(add[s:s + ch])
        s += ch
        dumps.append((eng.hnsw_dump(), orc.dump()))
    assert s == c["n"] == eng.ntotal
    codes = OracleHNSWSearch.encode(add, vmin, vdiff)
    np.testing.assert_array_equal(codes, orc.codes)
    return dict(eng=eng, orc=orc, dumps=dumps, add=add, vmin=vmin, vdiff=vdiff,
                codes=codes)


@functools.lru_cache(maxsize=None)
def _full(name):
    return _build_pair(name, 1, CASES[name]["chunks"])


def _queries(name, nq=12):
    c = CASES[name]
    if c["data"] == "clustered":
        return clustered(nq, c["d"], seed=5)
    add = case_data(name)[1]
    rng = np.random.default_rng(5)
    rows = add[rng.integers(0, c["n"], nq)]
    # half exactly on stored vectors (tied distances), half next to them
    jit = rng.standard_normal(rows.shape).astype(np.float32) * np.float32(0.05)
    jit[::2] = 0
    return (rows + jit).astype(np.float32)


# the counter(s) each case is in the table for: name -> checks on
# (counters, waves, final dump)
def _check_waves_overcap(c, waves, g):
    assert waves == [1, 256, 256, 187]
    assert c["over_cap_runs"] >= 1       # 256 points link to node 0
    assert c["entry_changes"] >= 2
    assert g["maxlevel"] >= 3


def _check_second_pass_tail(c, waves, g):
    # n0 > 0 schedules: 300 onto 1, then 299 onto 301; refine per add
    assert waves == [1, 256, 44, 256, 43]
    assert c["over_cap_runs"] >= 1 and c["fast_path_runs"] >= 1
    assert c["dedup_hits"] >= 1          # refine re-proposes existing links


def _check_second_pass_lanes(c, waves, g):
    assert waves == [1, 256, 256, 87]
    assert c["shrink_rejections"] >= 1 and c["apply_shrink_rejections"] >= 1


def _check_half_lane_m2(c, waves, g):
    assert c["level_at_clamp"] >= 1 and c["level_clamped"] >= 1
    assert g["maxlevel"] == 8
    assert g["M"] == 2


def _check_duplicates(c, waves, g):
    assert c["truncated_runs"] >= 1      # the refine wave cuts a run at 1024
    assert c["dedup_hits"] >= 1
    assert g["cnt0"].max() == g["deg0"]  # a degree at the cap


def _check_const_dims(c, waves, g):
    assert c["over_cap_runs"] >= 1


def _check_two_adds(c, waves, g):
    assert waves == [1, 256, 243, 256, 44]


def _check_lattice_ties(c, waves, g):
    # ties in exact arithmetic, decided by the fp32 summation order
    assert c["over_cap_runs"] >= 1 and c["apply_shrink_rejections"] >= 1


def _check_truncation_visible(c, waves, g):
    # the cut run is the entry point's; the near rows (ids >= 1150) that
    # an uncut run would keep first are missing from its row
    assert c["truncated_runs"] >= 1
    e = int(g["entry"])
    assert e == TRUNC_ENTRY
    row = g["nbr0"][e][:g["cnt0"][e]]
    assert row.size == g["deg0"] and (row < 1150).all()


_CHECKS = {
    "waves_overcap": _check_waves_overcap,
    "second_pass_tail": _check_second_pass_tail,
    "second_pass_lanes": _check_second_pass_lanes,
    "half_lane_m2": _check_half_lane_m2,
    "duplicates": _check_duplicates,
    "const_dims": _check_const_dims,
    "two_adds": _check_two_adds,
    "lattice_ties": _check_lattice_ties,
    "truncation_visible": _check_truncation_visible,
}
assert set(_CHECKS) == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_build_equals_oracle_and_search_over_oracle_graph(name):
    b = _full(name)
    for i, (ge, go) in enumerate(b["dumps"]):
        _assert_same_graph(ge, go, f"{name}: after add #{i}")
    go = b["dumps"][-1][1]
    _CHECKS[name](b["orc"].counters, b["orc"].waves, go)
    if name == "const_dims":
        # the vdiff == 0 -> 1 guard and both clamps were really exercised
        assert (b["vdiff"][[1, 7, 19]] == 1).all()
        live = np.delete(np.arange(20), [1, 7, 19])
        assert (b["codes"][:, live] == 0).any() and (b["codes"][:, live] == 255).any()
        assert (b["codes"][5, live] == 0).all() and (b["codes"][25, live] == 255).all()
    # search: oracle over its OWN graph vs the engine, bitwise
    c = CASES[name]
    osr = OracleHNSWSearch(c["d"], go, b["vmin"], b["vdiff"], b["codes"])
    q = _queries(name)
    b["eng"].nprobe = 16
    D, I = b["eng"].search(q, 10)
    Do, Io = osr.search(q, 10, 16)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D.view(np.uint32), Do.view(np.uint32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_build_equals_oracle_wave_by_wave(name):
    # refine off, one wave per add: a mismatch names the wave
    n = CASES[name]["n"]
    chunks = [1] + [256] * ((n - 1) // 256)
    if n - sum(chunks):
        chunks.append(n - sum(chunks))
    b = _build_pair(name, 0, chunks)
    assert b["orc"].waves == chunks
    for i, (ge, go) in enumerate(b["dumps"]):
        _assert_same_graph(ge, go, f"{name}: wave #{i} (rows "
                           f"{sum(chunks[:i])}..{sum(chunks[:i + 1])})")
    if name in ("waves_overcap", "duplicates", "half_lane_m2"):
        assert b["orc"].counters["over_cap_runs"] >= 1


def test_save_load_then_add_equals_uninterrupted_build(tmp_path):
    # engine A adds 500 + 300; engine B adds 500, saves, loads, adds 300
    name = "two_adds"
    a = _full(name)
    train, add = case_data(name)
    e1 = HipEngine(spec=_spec(name, 1))
    e1.train(train)
    e1.add(add[:500])
    p = str(tmp_path / "h.dfann")
    e1.save(p)
    e2 = HipProvider().load(p)
    _assert_same_graph(e2.hnsw_dump(), a["dumps"][0][1], "loaded after 500")
    e2.add(add[500:])
    gb = e2.hnsw_dump()
    _assert_same_graph(gb, a["dumps"][1][1], "B (save/load between adds) vs oracle")
    _assert_same_graph(gb, a["dumps"][1][0], "B vs A")
    q = _queries(name)
    a["eng"].nprobe = 16
    e2.nprobe = 16
    Da, Ia = a["eng"].search(q, 10)
    Db, Ib = e2.search(q, 10)
    np.testing.assert_array_equal(Ia, Ib)
    np.testing.assert_array_equal(Da.view(np.uint32), Db.view(np.uint32))


# ---------------------------------------------------------------------------
# search-only widening: parity over the engine's dumped graph (as
# tests/test_hnsw.py), at the d / k / ef the d=32 test never reaches
# ---------------------------------------------------------------------------


def _dump_search(name):
    b = _full(name)
    ge = b["dumps"][-1][0]
    return b, OracleHNSWSearch(CASES[name]["d"], ge, b["vmin"], b["vdiff"], b["codes"])


@pytest.mark.parametrize("name", ["half_lane_m2", "waves_overcap",
                                  "second_pass_tail", "second_pass_lanes"])
def test_search_parity_over_engine_graph(name):  # d = 8, 20, 136, 200
    b, osr = _dump_search(name)
    eng = b["eng"]
    q = _queries(name, 6)
    for k in (1, 10):
        got = {}
        for ef in (1, 10, 512, 2000):
            eng.nprobe = ef
            D, I = eng.search(q, k)
            Do, Io = osr.search(q, k, ef)
            np.testing.assert_array_equal(I, Io, err_msg=f"k={k} ef={ef}")
            np.testing.assert_array_equal(D.view(np.uint32), Do.view(np.uint32),
                                          err_msg=f"k={k} ef={ef}")
            got[ef] = (D, I)
        # nprobe = 2000 behaves as 512
        np.testing.assert_array_equal(got[2000][0].view(np.uint32),
                                      got[512][0].view(np.uint32))
        np.testing.assert_array_equal(got[2000][1], got[512][1])
        if k == 10:  # ef < k behaves as ef = k
            np.testing.assert_array_equal(got[1][0].view(np.uint32),
                                          got[10][0].view(np.uint32))
            np.testing.assert_array_equal(got[1][1], got[10][1])
    assert osr.counters["sel_truncations"] >= 1
    eng.nprobe = 16


def test_search_k_past_the_reachable_count_pads_the_tail():
    b, osr = _dump_search("duplicates")
    eng = b["eng"]
    q = _queries("duplicates", 4)
    eng.nprobe = 512
    D, I = eng.search(q, 512)
    Do, Io = osr.search(q, 512, 512)
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D.view(np.uint32), Do.view(np.uint32))
    nvalid = (I >= 0).sum(axis=1)
    assert (nvalid >= 1).all() and (nvalid < 512).all()  # fewer reachable than k
    for i in range(q.shape[0]):
        assert (I[i, nvalid[i]:] == -1).all()
        assert (D[i, nvalid[i]:] == FLT_MAX).all()
        assert (I[i, :nvalid[i]] >= 0).all()
    eng.nprobe = 16


def test_search_at_degree_512_frontier_512():
    # M = 256 on identical vectors: reverse links fill level-0 rows to 512,
    # so at ef = 512 a full frontier of 512 meets a node with 512
    # neighbours: 1024 > SEL_CAP - 32, the one place where the headroom
    # of the Sel buffer is in question. (Measured with the oracle's
    # op-for-op Sel: the threshold filter of sel_try drops the tied
    # appends, so the count itself stays below 992 and sel_guard does not
    # fire here — counter sel_guard_compacts stays 0.)
    n, d = 1100, 8
    x = np.tile(np.random.default_rng(1).standard_normal((1, d)), (n, 1)
                ).astype(np.float32)
    eng = HipEngine(spec={"type": "hnswsq", "dim": d, "metric": 1, "m": 256,
                          "ef_construction": 512, "nprobe": 512, "seed": 11})
    eng.train(x)
    eng.add(x)
    vmin, vdiff = eng.get_sq_params()
    g = eng.hnsw_dump()
    codes = OracleHNSWSearch.encode(x, vmin, vdiff)
    osr = OracleHNSWSearch(d, g, vmin, vdiff, codes)
    q = (x[:2] + np.float32(0.001)).astype(np.float32)
    D, I = eng.search(q, 10)
    Do, Io = osr.search(q, 10, 512)
    # some expanded node's degree plus the frontier size exceeds 992
    assert g["cnt0"].max() == 512
    assert osr.counters["max_frontier_plus_degree"] > 1024 - 32
    np.testing.assert_array_equal(I, Io)
    np.testing.assert_array_equal(D.view(np.uint32), Do.view(np.uint32))


# ---------------------------------------------------------------------------
# create contract
# ---------------------------------------------------------------------------


def _create(**kw):
    spec = {"type": "hnswsq", "dim": 8, "metric": 1, "m": 4}
    spec.update(kw)
    return HipEngine(spec=spec)


def test_create_contract():
    with pytest.raises(RuntimeError, match="store_n < 2"):
        _create(m=1)        # 1/ln(1): no level distribution
    with pytest.raises(RuntimeError, match="store_n > 256"):
        _create(m=257)
    with pytest.raises(RuntimeError, match="requires L2"):
        _create(metric=0)
    assert _create(m=2).hnsw_info()[:2] == (2, 4)
    assert _create(m=256).hnsw_info()[:2] == (256, 512)
