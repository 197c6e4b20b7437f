# Golden-fixture generator (the reference ships no
# known-answer vectors for IVF numerics, so WE freeze them from the
# oracle). Run from the repo root:  python3 tests/golden/make_golden.py
# Commits small .npz fixtures pinning oracle outputs (trained artifacts +
# search results) for fixed seeds; tests/test_golden.py replays them.
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import (  # noqa: E402
    make_oracle_engine,
    range_from_scans,
    ranking,
    scan_lists,
)

HERE = os.path.dirname(os.path.abspath(__file__))

D, N, NQ, K = 32, 2000, 16, 10

CONFIGS = {
    "flat_ip": {"type": "flat", "dim": D, "metric": 0},
    "flat_l2": {"type": "flat", "dim": D, "metric": 1},
    "ivfflat_l2": {"type": "ivf_flat", "dim": D, "metric": 1, "nlist": 8, "nprobe": 8},
    "ivfflat_ip": {"type": "ivf_flat", "dim": D, "metric": 0, "nlist": 8, "nprobe": 8},
    "ivfpq_l2": {"type": "ivfpq", "dim": D, "metric": 1, "nlist": 8, "m": 8, "nprobe": 8},
    "ivfpq_ip": {"type": "ivfpq", "dim": D, "metric": 0, "nlist": 8, "m": 8, "nprobe": 8},
    "ivfsq8_l2": {"type": "ivfsq", "dim": D, "metric": 1, "nlist": 8,
                  "sq_type": "8bit", "nprobe": 8},
    "ivfsq8_ip": {"type": "ivfsq", "dim": D, "metric": 0, "nlist": 8,
                  "sq_type": "8bit", "nprobe": 8},
    "ivfsqf_l2": {"type": "ivfsq", "dim": D, "metric": 1, "nlist": 8,
                  "sq_type": "fp16", "nprobe": 8},
    "ivfpq4_l2": {"type": "ivfpq", "dim": D, "metric": 1, "nlist": 8, "m": 8,
                  "nbits": 4, "nprobe": 8},
    "ivfpq4_ip": {"type": "ivfpq", "dim": D, "metric": 0, "nlist": 8, "m": 8,
                  "nbits": 4, "nprobe": 8},
    "ivfsq4_l2": {"type": "ivfsq", "dim": D, "metric": 1, "nlist": 8,
                  "sq_type": "4bit", "nprobe": 8},
    "ivfsq4_ip": {"type": "ivfsq", "dim": D, "metric": 0, "nlist": 8,
                  "sq_type": "4bit", "nprobe": 8},
    "ivfsq6_l2": {"type": "ivfsq", "dim": D, "metric": 1, "nlist": 8,
                  "sq_type": "6bit", "nprobe": 8},
    "ivfsq6_ip": {"type": "ivfsq", "dim": D, "metric": 0, "nlist": 8,
                  "sq_type": "6bit", "nprobe": 8},
}

# The sub-byte widths also pin the stored list bytes and a range result
# over all 8 probes: per query the radius is the midpoint between the 20th
# and the 21st value of the full ranking, so 20 rows pass.
SUB_BYTE = ("ivfpq4_", "ivfsq4_", "ivfsq6_")
RANGE_HITS = 20


def data():
    rng = np.random.default_rng(42)
    xb = rng.standard_normal((N, D), dtype=np.float32)
    q = rng.standard_normal((NQ, D), dtype=np.float32)
    return xb, q


def range_result(eng, q):
    """(lims, D, I) of the range search described at SUB_BYTE, with the
    engine's coarse keys (minimise-keys: the IP bias is -key)."""
    probes, sc = eng.coarse_topn(q, eng.nlist)
    keys = sc if eng.metric == 1 else -sc
    scans = scan_lists(eng, q, probes, keys)
    radius = [np.float32((np.float64(v[RANGE_HITS - 1]) + np.float64(v[RANGE_HITS])) / 2)
              for v, _ in ranking(scans, eng.metric)]
    return range_from_scans(scans, eng.metric, radius)


def main():
    xb, q = data()
    for name, spec in CONFIGS.items():
        eng = make_oracle_engine(dict(spec, seed=1234))
        eng.train(xb)
        eng.add(xb)
        D_, I_ = eng.search(q, K)
        out = {"D": D_, "I": I_}
        if spec["type"] != "flat":
            out["centroids"] = eng.centroids
        if spec["type"] == "ivfpq":
            out["codebooks"] = eng.codebooks
        if spec["type"] == "ivfsq" and spec.get("sq_type") != "fp16":
            out["vmin"] = eng.vmin
            out["vdiff"] = eng.vdiff
        if name.startswith(SUB_BYTE):
            out["packed"] = eng.packed_lists()[2]
            out["lims"], out["RD"], out["RI"] = range_result(eng, q)
        path = os.path.join(HERE, f"{name}.npz")
        with open(path, "wb") as f:
            np.savez(f, **out)
        print("wrote", path, "D[0,:3] =", D_[0, :3])


if __name__ == "__main__":
    main()
