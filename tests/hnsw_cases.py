# Shared inputs of the hnswsq build-parity tests: the CPU module
# (test_oracle_hnsw.py) checks on these very (seed, M, n) that no level draw
# sits on a rounding edge and that each case reaches the branch it is named
# for; the GPU module (test_gpu_hnsw_build.py) compares the engine with the
# oracle on them. Not a test module.
import numpy as np

SEED = 11  # spec "seed" (level draws) unless a case names its own


def clustered(n, d, seed=0, centers=16, sigma=0.3):
    crng = np.random.default_rng(1000 + d)
    cent = crng.standard_normal((centers, d)).astype(np.float32) * 3.0
    rng = np.random.default_rng(seed)
    lbl = rng.integers(0, centers, n)
    x = cent[lbl] + sigma * rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32)


def repeated6(n, d):
    """6 distinct vectors repeated: all-zero and tied distances. In every
    36 rows the first 31 are vector 0 and the last 5 are vectors 1..5, so
    that in the refine wave more than 1024 copies of vector 0 propose a
    link to the same lowest-id copy."""
    base = np.random.default_rng(6).standard_normal((6, d)).astype(np.float32)
    r = np.arange(n) % 36
    return base[np.where(r < 31, 0, r - 30)].copy()


def const_dims_outliers(n, d):
    """(train, add): 3 constant dimensions (vdiff == 0 -> 1 guard); 5 % of
    the added rows lie outside the trained range on every other dimension
    (codes clamp at 0 and at 255)."""
    x = clustered(n, d, seed=3)
    x[:, [1, 7, 19]] = np.float32(0.75)
    train = x.copy()
    add = x.copy()
    out = np.arange(n) % 20 == 5
    sign = np.where(np.arange(n) % 40 == 5, -1.0, 1.0).astype(np.float32)
    add[out] = add[out] + (sign[out] * np.float32(40.0))[:, None]
    add[:, [1, 7, 19]] = np.float32(0.75)
    return train, add


def lattice_ties(n, d):
    """(train, add): every code is one of 0, 85, 170, 255 and every
    dimension has the same scale 3.3/255, which is no power of two. Many
    pairs of rows then have the same code-code distance in exact
    arithmetic and differ only in the rounding of the fp32 sum, so the
    summation order of hnsw_dist_cc (lanes, butterfly) decides shrink tests
    and the (dist, id) order of the reverse-link merge."""
    rng = np.random.default_rng(9)
    c = rng.integers(0, 4, (n, d)) * 85
    add = ((c + 0.5) * (3.3 / 255)).astype(np.float32)  # mid-bin: code = c
    train = np.stack([np.zeros(d, np.float32), np.full(d, 3.3, np.float32)])
    return train, add


TRUNC_ENTRY = 1169  # the one node at the top level (5) for seed 33, M = 4


def truncation_visible(n, d):
    """The run cut at 1024 candidates loses links it would have kept.
    Node TRUNC_ENTRY sits at the origin and becomes the entry point; rows
    0..1149 lie on a half sphere of radius 4 around it (at d = 64 none of
    them is nearer to another than to the origin, so in the refine wave
    every one of them proposes a link to the entry point); rows 1150.. lie
    near (-1, 0, ...), nearer to the origin than the sphere and in the same
    last insertion wave as the origin, so they meet it only in refine —
    with the highest source ids, past the cut."""
    rng = np.random.default_rng(3)
    v = rng.standard_normal((n, d)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[:, 0] = np.abs(v[:, 0])
    x = (v * np.float32(4.0)).astype(np.float32)
    x[1150:] = (rng.standard_normal((n - 1150, d)) * 0.05).astype(np.float32)
    x[1150:, 0] -= np.float32(1.0)
    x[TRUNC_ENTRY] = 0
    return x, x


# name -> dict(d, M, efc, n, chunks (sizes of the add calls), data[, seed])
CASES = {
    "waves_overcap": dict(d=20, M=4, efc=16, n=700, chunks=[700], data="clustered"),
    "second_pass_tail": dict(d=136, M=8, efc=32, n=600, chunks=[1, 300, 299],
                             data="clustered"),
    "second_pass_lanes": dict(d=200, M=16, efc=40, n=600, chunks=[600],
                              data="clustered"),
    # seed 12: four of the 700 draws reach the level clamp (8) at M=2
    "half_lane_m2": dict(d=8, M=2, efc=12, n=700, chunks=[700], data="clustered",
                         seed=12),
    "duplicates": dict(d=8, M=4, efc=24, n=1200, chunks=[1200], data="repeated6"),
    "const_dims": dict(d=20, M=8, efc=24, n=600, chunks=[600], data="const_dims"),
    "two_adds": dict(d=20, M=8, efc=24, n=800, chunks=[500, 300], data="clustered"),
    # beyond the table: the two cases that make a wrong summation order in
    # hnsw_dist_cc and a missing 1024 cut change the graph (see the data)
    "lattice_ties": dict(d=136, M=8, efc=16, n=400, chunks=[400], data="lattice"),
    "truncation_visible": dict(d=64, M=4, efc=8, n=1200, chunks=[1200],
                               data="trunc", seed=33),
}


def case_seed(name):
    return CASES[name].get("seed", SEED)


def case_data(name):
    """(train, add) float32 arrays of a case."""
    c = CASES[name]
    if c["data"] == "clustered":
        x = clustered(c["n"], c["d"], seed=7)
        return x, x
    if c["data"] == "repeated6":
        x = repeated6(c["n"], c["d"])
        return x, x
    if c["data"] == "lattice":
        return lattice_ties(c["n"], c["d"])
    if c["data"] == "trunc":
        return truncation_visible(c["n"], c["d"])
    return const_dims_outliers(c["n"], c["d"])


def cpu_sq_params(train):
    """min/max ranges as the engine trains them (k_minmax_decode)."""
    vmin = train.min(axis=0).astype(np.float32)
    vdiff = (train.max(axis=0) - vmin).astype(np.float32)
    vdiff[vdiff == 0] = np.float32(1.0)
    return vmin, vdiff
