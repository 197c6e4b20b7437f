# ORACLE range — restatement of range search over the IVF
# oracles of oracle/core.py.
#
# For each query and probe slot, in slot order, the oracle's own
# `_scan_one(q, list, bias)` gives the list's distances (squared L2, or the
# un-negated dot product with the engine's coarse key as bias) and arrival
# ids in CSR order; the strict radius test (L2: dist < radius, IP: dot >
# radius) and the optional allow mask pick the hits. Concatenated, that is
# (lims, D, I) in the contract's order — probe slot, then ascending arrival
# id — with the oracle's bit-exact float32 distances. A list named twice
# contributes twice. `orc` is any oracle IVF index (`lut_f16` is the
# oracle's own option).
import numpy as np

from .core import METRIC_L2


def scan_lists(orc, q, probes, keys):
    """Per query, per probe slot: (dist float32, ids int64) of that list
    (empty arrays for an empty list). Radius-independent: compute once and
    share between the radii of a case."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    out = []
    for i in range(q.shape[0]):
        row = []
        for s in range(probes.shape[1]):
            res = orc._scan_one(q[i], int(probes[i, s]),
                                np.float32(-keys[i, s]))
            if res is None:
                row.append((np.empty(0, np.float32), np.empty(0, np.int64)))
            else:
                row.append((np.asarray(res[0], np.float32),
                            np.asarray(res[1], np.int64)))
        out.append(row)
    return out


def range_from_scans(scans, metric, radius, allow=None):
    """(lims, D, I) from scan_lists output. radius: scalar or one per
    query. allow: bool mask over arrival ids, or None."""
    nq = len(scans)
    radius = np.broadcast_to(np.asarray(radius, np.float32), (nq,))
    lims = np.zeros(nq + 1, np.int64)
    Ds, Is = [], []
    for i, row in enumerate(scans):
        n = 0
        for dist, ids in row:
            hit = dist < radius[i] if metric == METRIC_L2 else dist > radius[i]
            if allow is not None:
                hit = hit & np.asarray(allow, bool)[ids]
            Ds.append(dist[hit])
            Is.append(ids[hit])
            n += int(hit.sum())
        lims[i + 1] = lims[i] + n
    D = np.concatenate(Ds) if Ds else np.empty(0, np.float32)
    I = np.concatenate(Is) if Is else np.empty(0, np.int64)
    return lims, D.astype(np.float32), I.astype(np.int64)


def range_search_ref(orc, q, probes, keys, radius, allow=None):
    return range_from_scans(scan_lists(orc, q, probes, keys), orc.metric,
                            radius, allow)


def ranking(scans, metric):
    """Per query: all probed rows' values, best first ((key, id) lexsort,
    key = dist for L2 and -dot for IP): the full ranking `search` cuts its
    top-k from."""
    out = []
    for row in scans:
        d = np.concatenate([r[0] for r in row])
        i = np.concatenate([r[1] for r in row])
        key = d if metric == METRIC_L2 else -d
        order = np.lexsort((i, key))
        out.append((d[order], i[order]))
    return out
