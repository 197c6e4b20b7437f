# CPU coverage of the HNSW oracle (oracle/hnsw.py): the search
# restatement on a hand-built tiny graph, and the build restatement —
# batched distances against their scalar definitions, the wave schedule,
# the level draw, a build whose adjacency is derived by hand, and the
# branch counters the GPU cases rely on. (The bitwise engine parity runs
# on GPU — tests/test_hnsw.py, tests/test_gpu_hnsw_build.py; this pins
# the oracle's own semantics without hardware.)
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hnsw_cases import (  # noqa: E402
    CASES,
    TRUNC_ENTRY,
    case_data,
    case_seed,
    cpu_sq_params,
)
from oracle import OracleHNSWBuild  # noqa: E402
from oracle.core import (  # noqa: E402
    OracleHNSWSearch,
    hnsw_draw_level,
    hnsw_level_real,
    hnsw_wave_schedule,
)


def _graph_line(n, deg0=4, M=2):
    # path graph 0-1-2-...-n-1 at level 0; node 0 also at level 1 with a
    # long link to the middle
    g = {
        "levels": np.zeros(n, dtype=np.int32),
        "cnt0": np.zeros(n, dtype=np.int32),
        "nbr0": np.full((n, deg0), -1, dtype=np.int32),
        "upslot": np.full(n, -1, dtype=np.int32),
        "cntU": np.zeros((1, 8), dtype=np.int32),
        "nbrU": np.full((1, 8, M), -1, dtype=np.int32),
        "entry": 0, "maxlevel": 1, "M": M, "deg0": deg0, "nslots": 1,
        "efc": 8,
    }
    for i in range(n):
        nb = [j for j in (i - 1, i + 1) if 0 <= j < n]
        g["cnt0"][i] = len(nb)
        g["nbr0"][i, :len(nb)] = nb
    g["levels"][0] = 1
    g["upslot"][0] = 0
    g["cntU"][0, 0] = 1
    g["nbrU"][0, 0, 0] = n // 2  # level-1 long link
    return g


def test_oracle_hnsw_search_on_line_graph():
    n, d = 32, 8
    # points on a line: x_i = (i, 0, ..., 0)
    x = np.zeros((n, d), dtype=np.float32)
    x[:, 0] = np.arange(n, dtype=np.float32)
    vmin = x.min(0)
    vdiff = np.maximum(x.max(0) - x.min(0), 1.0).astype(np.float32)
    codes = OracleHNSWSearch.encode(x, vmin, vdiff)
    g = _graph_line(n)
    # node n//2 must be reachable via the level-1 long link then local walk
    orc = OracleHNSWSearch(d, g, vmin, vdiff, codes)
    q = x[20:21] + 0.1
    D, I = orc.search(q, 3, ef=8)
    assert I[0, 0] == 20  # nearest by decoded distance
    assert (np.diff(D[0]) >= 0).all()
    # with a beam too small to cross the whole line from node 0, the
    # level-1 shortcut to n//2 is what makes 20 reachable: removing it
    # must degrade the result
    g2 = {**{k: (v.copy() if hasattr(v, "copy") else v) for k, v in g.items()}}
    g2["cntU"] = np.zeros((1, 8), dtype=np.int32)
    g2["maxlevel"] = 0
    orc2 = OracleHNSWSearch(d, g2, vmin, vdiff, codes)
    D2, I2 = orc2.search(q, 3, ef=4)
    # greedy from 0 with ef=4 walks the line; it CAN still reach 20 on a
    # 1-D line, so just assert determinism + validity here
    assert (I2[0] >= 0).all()


def test_oracle_hnsw_encode_trunc():
    # encode mirrors k_sq_encode: trunc toward zero + clamp
    vmin = np.zeros(2, dtype=np.float32)
    vdiff = np.full(2, 2.0, dtype=np.float32)
    x = np.array([[0.0, 2.0], [1.0, -1.0]], dtype=np.float32)
    c = OracleHNSWSearch.encode(x, vmin, vdiff)
    assert c[0, 0] == 0 and c[0, 1] == 255
    assert c[1, 0] == 127  # 255*0.5 = 127.5 -> trunc 127
    assert c[1, 1] == 0    # clamped


# ---------------------------------------------------------------------------
# distances: the row-batched forms equal the scalar definitions bitwise
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("d", [8, 20, 136, 200])
def test_batched_distances_equal_scalar_bitwise(d):
    rng = np.random.default_rng(d)
    n = 24
    codes = rng.integers(0, 256, (n, d)).astype(np.uint8)
    codes[1] = codes[0]          # a zero code-code distance
    codes[2] = 0
    codes[3] = 255               # the largest per-dim difference
    vmin = rng.standard_normal(d).astype(np.float32)
    vdiff = (rng.random(d).astype(np.float32) * 7 + np.float32(0.01))
    o = OracleHNSWSearch(d, None, vmin, vdiff, codes)
    ids = np.arange(n)
    for qi in range(3):
        q = (vmin + vdiff * rng.random(d).astype(np.float32)).astype(np.float32)
        u = ((q - o.vmin) - np.float32(0.5) * o.scale).astype(np.float32)
        want = np.array([o._dist_q(u, i) for i in ids], dtype=np.float32)
        got = o._dist_q_rows(u, ids)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    for a in (0, 2, 3, 7):
        want = np.array([o._dist_cc(a, i) for i in ids], dtype=np.float32)
        got = o._dist_cc_rows(a, ids)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(o._cc_all(a).view(np.uint32),
                                      want.view(np.uint32))
    assert o._dist_cc(0, 1) == 0.0
    # the summation order is observable: a plain ascending sum differs
    # somewhere at d >= 136 (else this test could not tell the orders apart)
    if d >= 136:
        differs = False
        for a in range(n):
            diff = (codes[a].astype(np.float32) - codes.astype(np.float32)) * o.scale
            acc = np.zeros(n, dtype=np.float32)
            for t in range(d):
                acc = acc + diff[:, t] * diff[:, t]
            differs |= bool((acc != o._cc_all(a)).any())
        assert differs


# ---------------------------------------------------------------------------
# host arithmetic: wave schedule and level draw
# ---------------------------------------------------------------------------


def test_wave_schedule_known_answers():
    assert hnsw_wave_schedule(0, 700) == [1, 256, 256, 187]
    assert hnsw_wave_schedule(1, 300) == [256, 44]
    # w0/8 > 256: 4000 // 8 = 500, then (4500 // 8 = 562) cut by the rest
    assert hnsw_wave_schedule(4000, 1000) == [500, 500]
    assert hnsw_wave_schedule(4000, 1100) == [500, 562, 38]
    # the 4096 ceiling
    assert hnsw_wave_schedule(40000, 5000) == [4096, 904]
    # the schedule restarts at w0 = n0 on every add
    assert hnsw_wave_schedule(0, 1) == [1]
    assert hnsw_wave_schedule(500, 300) == [256, 44]


def test_level_draw_floor_and_clamp():
    lv = np.array([hnsw_draw_level(7, i, 2) for i in range(20000)])
    real = np.array([hnsw_level_real(7, i, 2) for i in range(20000)])
    assert lv.min() == 0 and lv.max() == 8
    assert (real >= 9).any()                     # the clamp actually cuts
    np.testing.assert_array_equal(lv, np.clip(np.floor(real), 0, 8).astype(int))
    assert (real >= 0).all()                     # u <= 1: never negative
    # u = ((z >> 11) + 1) * 2^-53 is in (0, 1]: the draw is finite for all z
    assert math.isfinite(real.max())


@pytest.mark.parametrize("M", [2, 4, 16])
def test_level_draw_histogram_is_geometric(M):
    n = 20000
    lv = np.array([hnsw_draw_level(1234, i, M) for i in range(n)])
    hist = np.bincount(lv, minlength=9)
    assert hist.sum() == n and hist.shape[0] == 9
    for l in range(9):
        # P(level = l) = M^-l - M^-(l+1); the clamp gathers the tail at 8
        p = float(M) ** -l - (float(M) ** -(l + 1) if l < 8 else 0.0)
        sigma = math.sqrt(n * p * (1 - p))
        # 4.5 binomial standard deviations; +1 covers expected counts << 1
        assert abs(hist[l] - n * p) <= 4.5 * sigma + 1, (l, hist[l], n * p)


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_case_level_draws_are_off_the_rounding_edge(name):
    # a libm that differs in the last bits from this one must not be able
    # to flip a level of a GPU case: no draw within 1e-9 of an integer
    c = CASES[name]
    real = np.array([hnsw_level_real(case_seed(name), i, c["M"])
                     for i in range(c["n"])])
    assert np.abs(real - np.round(real)).min() > 1e-9


# ---------------------------------------------------------------------------
# a build small enough to derive by hand
# ---------------------------------------------------------------------------


def test_hand_checked_build_on_a_line():
    # Points on a line at positions 10 12 13 14 15 16 17, stored as
    # pos + 0.5 with vmin = 0, vdiff = 255 (scale = 1): the code is pos, the
    # folded query u = x - 0.5 is pos, so dist_q and dist_cc are both the
    # exact integer (pos_a - pos_b)^2. M = 2 (insert keeps <= 2, level-0
    # rows hold 4); seed 277 puts ids 0..6 all at level 0; refine off; one
    # add per wave: [0], [1], [2], [3, 4, 5, 6].
    pos = np.array([10, 12, 13, 14, 15, 16, 17], dtype=np.float32)
    x = np.zeros((7, 2), dtype=np.float32)
    x[:, 0] = pos + np.float32(0.5)
    x[:, 1] = np.float32(0.5)
    seed = 277
    assert all(hnsw_draw_level(seed, i, 2) == 0 for i in range(7))
    b = OracleHNSWBuild(2, 2, 8, seed, np.zeros(2, np.float32),
                        np.full(2, 255, np.float32), refine=0)
    for s, e in ((0, 1), (1, 2), (2, 3), (3, 7)):
        b.add(x[s:e])
    assert b.waves == [1, 1, 1, 4]
    np.testing.assert_array_equal(b.codes[:, 0], pos.astype(np.uint8))
    g = b.dump()
    # wave [1]: 1 links 0; reverse 0 <- 1 appended (fast path).
    # wave [2] (pos 13): results 1 (d 1), 0 (d 9). Keep 1; 0 is REJECTED by
    #   the shrink test: dist_cc(0, 1) = 4 < dist_q(2, 0) = 9. Reverse
    #   1 <- 2 appended (fast path): row 1 = [0, 2].
    # wave [3..6] (pos 14..17) over the snapshot {0, 1, 2}: each keeps 2
    #   only (dist_cc(1, 2) = 1 and dist_cc(0, 2) = 9 are below its own
    #   distance to 1 and to 0): 2 rejections each. Node 2 holds [1] and
    #   receives 4 requests: 5 > 4, the OVER-CAP prune. By dist_cc(2, .):
    #   1 -> 1, 3 -> 1, 4 -> 4, 5 -> 9, 6 -> 16, ties by id. Keep 1; keep 3
    #   (dist_cc(3, 1) = 4 is not < 1); reject 4 (dist_cc(4, 3) = 1 < 4),
    #   5 (dist_cc(5, 3) = 4 < 9) and 6 (dist_cc(6, 3) = 9 < 16).
    want = [[1], [0, 2], [1, 3], [2], [2], [2], [2]]
    for i, w in enumerate(want):
        assert g["cnt0"][i] == len(w), i
        assert g["nbr0"][i].tolist() == w + [-1] * (4 - len(w)), i
    assert g["entry"] == 0 and g["maxlevel"] == 0 and g["nslots"] == 0
    c = b.counters
    assert c["fast_path_runs"] == 2
    assert c["over_cap_runs"] == 1
    assert c["shrink_rejections"] == 1 + 2 * 4
    assert c["apply_shrink_rejections"] == 3
    assert c["truncated_runs"] == 0 and c["entry_changes"] == 0
    # the oracle search over this graph: nothing links to 4, 5, 6, so from
    # entry 0 only 0..3 are reachable; for the point at pos 16 those are
    # 3 (pos 14), 2 (pos 13), 1 (pos 12)
    o = OracleHNSWSearch(2, g, b.vmin, b.vdiff, b.codes)
    D, I = o.search(x[5:6], 3, 8)
    assert I[0].tolist() == [3, 2, 1] and D[0].tolist() == [4.0, 9.0, 16.0]
    D, I = o.search(x[5:6], 6, 8)  # k past the reachable count: padded tail
    assert I[0].tolist() == [3, 2, 1, 0, -1, -1]
    assert D[0, 4] == D[0, 5] == np.float32(3.402823466e+38)


def test_over_cap_prune_leaves_stale_slots_past_the_count():
    # the prune rewrites only the first n_kept slots of a row: node 0 at
    # pos 20 first fills its 4 slots by appends (pos 10, 30, 21, 19 in
    # separate waves), then one more request forces a prune that keeps
    # fewer than 4 — the slots past the new count keep their old ids
    pos = np.array([20, 10, 30, 21, 19, 22], dtype=np.float32)
    x = np.zeros((6, 2), dtype=np.float32)
    x[:, 0] = pos + np.float32(0.5)
    x[:, 1] = np.float32(0.5)
    seed = 277
    b = OracleHNSWBuild(2, 2, 8, seed, np.zeros(2, np.float32),
                        np.full(2, 255, np.float32), refine=0)
    for i in range(5):
        b.add(x[i:i + 1])
    g = b.dump()
    assert g["cnt0"][0] == 4 and g["nbr0"][0].tolist() == [1, 2, 3, 4]
    b.add(x[5:6])  # pos 22 keeps 3 (pos 21); 3 <- 5 is an append
    g = b.dump()
    assert g["nbr0"][5, 0] == 3
    b2 = OracleHNSWBuild(2, 2, 8, seed, np.zeros(2, np.float32),
                         np.full(2, 255, np.float32), refine=0)
    # same, but the last point sits at pos 20 itself: nearest is node 0
    x2 = x.copy()
    x2[5, 0] = np.float32(20.5)
    for i in range(6):
        b2.add(x2[i:i + 1])
    g2 = b2.dump()
    # candidates of node 0 by dist_cc: 5 (0), 3 (1), 4 (1), 1 (100), 2 (100).
    # keep 5; 3: dist_cc(3, 5) = 1 is not < 1, keep; 4: dist_cc(4, 5) = 1 not
    # < 1, dist_cc(4, 3) = 4 not < 1, keep; 1: dist_cc(1, 4) = 81 < 100,
    # reject; 2: dist_cc(2, 3) = 81 < 100, reject. n_kept = 3: slot 3 is stale
    assert b2.counters["over_cap_runs"] == 1
    assert g2["cnt0"][0] == 3
    assert g2["nbr0"][0].tolist() == [5, 3, 4, 4]


# ---------------------------------------------------------------------------
# branch counters
# ---------------------------------------------------------------------------


def test_identical_vectors_reach_the_1024_truncation():
    n, d = 1100, 8
    x = np.tile(np.random.default_rng(1).standard_normal((1, d)), (n, 1)
                ).astype(np.float32)
    vmin, vdiff = cpu_sq_params(x)
    assert (vdiff == 1).all()  # every dimension constant: the 0 -> 1 guard
    b = OracleHNSWBuild(d, 4, 24, 11, vmin, vdiff)
    b.add(x)
    assert b.counters["truncated_runs"] >= 1
    assert b.counters["dedup_hits"] >= 1
    g = b.dump()
    assert g["cnt0"].max() == 8  # a degree at the level-0 cap
    # without the truncation the same run keeps other sources: the branch
    # is observable in the graph, not only in the counter
    b2 = OracleHNSWBuild(d, 4, 24, 11, vmin, vdiff)
    b2._apply_limit = 1 << 30
    b2.add(x)
    assert b2.counters["truncated_runs"] == 0


def _case_build(name, **attrs):
    c = CASES[name]
    train, add = case_data(name)
    vmin, vdiff = cpu_sq_params(train)
    b = OracleHNSWBuild(c["d"], c["M"], c["efc"], case_seed(name), vmin, vdiff)
    for k, v in attrs.items():
        setattr(b, k, v)
    s = 0
    for ch in c["chunks"]:
        b.add(add[s:s + ch])
        s += ch
    return b


def test_duplicates_case_reaches_truncation_and_level_clamp_case_its_clamp():
    b = _case_build("duplicates")
    assert b.counters["truncated_runs"] >= 1
    assert b.dump()["cnt0"].max() == 8
    c = CASES["half_lane_m2"]
    real = [hnsw_level_real(case_seed("half_lane_m2"), i, c["M"])
            for i in range(c["n"])]
    assert sum(r >= 8 for r in real) >= 1 and sum(r >= 9 for r in real) >= 1


def test_truncation_case_changes_the_graph():
    # the 1024 cut is visible in the graph: without it the entry point's
    # row starts with a near row (id >= 1150) the cut run never sees
    e = TRUNC_ENTRY
    lv = [hnsw_draw_level(case_seed("truncation_visible"), i, 4) for i in range(1200)]
    assert int(np.argmax(lv)) == e and lv.count(max(lv)) == 1
    cut = _case_build("truncation_visible")
    assert cut.counters["truncated_runs"] == 1
    g = cut.dump()
    assert g["entry"] == e and (g["nbr0"][e][:g["cnt0"][e]] < 1150).all()
    free = _case_build("truncation_visible", _apply_limit=1 << 30)
    assert free.counters["truncated_runs"] == 0
    gf = free.dump()
    assert gf["nbr0"][e, 0] >= 1150


def test_lattice_case_sees_the_dist_cc_summation_order():
    # summing the 8 lane partials in another grouping changes only the
    # rounding, and on this case that changes the graph
    class Swapped(OracleHNSWBuild):
        def _lanes_reduce(self, sq):
            rows = sq.shape[0]
            sq = sq.reshape(rows, self._npass, 8, 16)
            part = np.zeros((rows, 8), dtype=np.float32)
            for ps in range(self._npass):
                for b in range(16):
                    part = part + sq[:, ps, :, b]
            part = part[:, [0, 2, 1, 3, 4, 5, 6, 7]]
            lane = np.arange(8)
            for m in (4, 2, 1):
                part = part + part[:, lane ^ m]
            return part[:, 0]

    c = CASES["lattice_ties"]
    train, add = case_data("lattice_ties")
    vmin, vdiff = cpu_sq_params(train)
    assert (vmin == 0).all() and (vdiff == np.float32(3.3)).all()
    a = OracleHNSWBuild(c["d"], c["M"], c["efc"], case_seed("lattice_ties"), vmin, vdiff)
    b = Swapped(c["d"], c["M"], c["efc"], case_seed("lattice_ties"), vmin, vdiff)
    a.add(add)
    b.add(add)
    assert sorted(np.unique(a.codes).tolist()) == [0, 85, 170, 255]
    assert (a.dump()["nbr0"] != b.dump()["nbr0"]).any()


def test_m_below_2_is_rejected():
    with pytest.raises(ValueError):
        OracleHNSWBuild(8, 1, 10, 11, np.zeros(8, np.float32), np.ones(8, np.float32))
