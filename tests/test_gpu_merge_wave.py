# Wave-per-query merges (k_merge_cand_w, k_merge_shards_w) against the
# block-per-query kernels they replace and against the references.
#
# The dispatch takes the wave kernels for k <= 16 and at most 256
# candidates per query (1, 2 or 4 per lane); DFANN_MERGE_WAVE=0 keeps
# k_merge_cand_rk / k_merge_shards_rk. Every case runs with the knob unset
# and with the knob at 0 in the same process: D and I must be bitwise
# equal, and the default result must equal the reference (numpy lexsort
# for the shard merge, the CPU oracle for the candidate merge).
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

from distributed_faiss_amd.hip_engine import merge_topk_dev  # noqa: E402
from gpu_support import (  # noqa: E402
    assert_bitwise,
    codeword_rows,
    decode_rows,
    engine_with,
    labels,
)
from oracle import from_engine_artifacts  # noqa: E402

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
FLT_MAX = np.float32(3.4028235e38)
KNOB = "DFANN_MERGE_WAVE"


def _both(run):
    """run() with the knob unset, then with the knob at 0."""
    saved = os.environ.pop(KNOB, None)
    try:
        wave = run()
        os.environ[KNOB] = "0"
        block = run()
    finally:
        os.environ.pop(KNOB, None)
        if saved is not None:
            os.environ[KNOB] = saved
    return wave, block


# ---------------------------------------------------------------------------
# shard merge: dfann_merge_topk against a numpy lexsort (data recipe of
# test_gpu_dispatch_parity.test_merge_topk_vs_lexsort)
# ---------------------------------------------------------------------------

SHARD_SHAPES = [
    pytest.param(4, 16, id="S4-k16-C64-one_per_lane_full"),
    pytest.param(5, 13, id="S5-k13-C65-two_per_lane_first"),
    pytest.param(8, 16, id="S8-k16-C128-two_per_lane_full"),
    pytest.param(43, 3, id="S43-k3-C129-four_per_lane_first"),
    pytest.param(16, 16, id="S16-k16-C256-four_per_lane_full"),
    pytest.param(257, 1, id="S257-k1-C257-block_kernel"),
]


@pytest.mark.parametrize("maximize", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("nq", [1, 3, 4, 5, 37])
@pytest.mark.parametrize("S,k", SHARD_SHAPES)
def test_shard_merge_wave_vs_block_vs_lexsort(S, k, nq, maximize):
    rng = np.random.default_rng(S * 100003 + k * 101 + nq * 7 + int(maximize))
    pool = rng.standard_normal(50).astype(np.float32)
    pad = -FLT_MAX if maximize else FLT_MAX
    D = np.empty((S, nq, k), np.float32)
    I = np.empty((S, nq, k), np.int64)
    for s in range(S):
        for qi in range(nq):
            # ties cross shards (50-value pool); a third of the rows end
            # in pads, some consist of nothing else
            valid = k if rng.uniform() < 0.67 else int(rng.integers(0, k + 1))
            v = np.sort(rng.choice(pool, valid))
            D[s, qi, :valid] = v[::-1] if maximize else v  # faiss order
            D[s, qi, valid:] = pad
            I[s, qi, :valid] = rng.integers(0, 1 << 40, valid)
            I[s, qi, valid:] = -1
    Dt, It = torch.as_tensor(D).cuda(), torch.as_tensor(I).cuda()

    def run():
        Dm, Im = merge_topk_dev(Dt, It, k, maximize=maximize)
        return Dm.cpu().numpy(), Im.cpu().numpy()

    wave, block = _both(run)
    assert_bitwise(*wave, *block)
    Dm, Im = wave
    # key = -v for maximize (kept in the output: reference quirk 2);
    # order by (key, dense slot s*k + j); id = s*nq*k + q*k + j
    key = (-D if maximize else D).transpose(1, 0, 2).reshape(nq, S * k)
    slot = np.arange(S * k)
    for qi in range(nq):
        order = np.lexsort((slot, key[qi]))[:k]
        np.testing.assert_array_equal(Dm[qi], key[qi][order])
        np.testing.assert_array_equal(
            Im[qi], (order // k) * nq * k + qi * k + order % k)


# ---------------------------------------------------------------------------
# candidate merge: search_preassigned on a small IVFPQ and a small IVF-Flat
# index, 1992 rows in 32 lists (list 0 empty, lists 1-3 hold 6 rows)
# ---------------------------------------------------------------------------

LIST_SIZES = [0, 1, 2, 3, 5, 17, 63, 64, 65, 100] + [76] * 22
NLIST = len(LIST_SIZES)
NROWS = sum(LIST_SIZES)
NQ = 7  # two blocks of four waves, the second one partial
K = 16
assert NLIST == 32 and NROWS == 1992


def _data(typ, metric):
    """(spec, cent, cb, xb, q, lbl, cw): numpy only."""
    rng = np.random.default_rng(77 + metric)
    lbl = labels(rng, LIST_SIZES)
    if typ == "ivf_flat":
        # small integers: every product and partial sum is exact in fp32,
        # so the engine's tree reduction and the oracle's sequential sum
        # agree bitwise, and equal distances occur across lists
        d = 64
        cent = rng.integers(-4, 5, (NLIST, d)).astype(np.float32)
        xb = (cent[lbl] + rng.integers(-1, 2, (NROWS, d))).astype(np.float32)
        q = (cent[rng.integers(0, NLIST, NQ)]
             + rng.integers(-1, 2, (NQ, d))).astype(np.float32)
        spec = {"type": typ, "dim": d, "metric": metric, "nlist": NLIST,
                "nprobe": NLIST, "seed": 1234}
        cb = cw = None
    else:
        # centroid + exact codeword + 1e-3 noise (the parity suite's recipe:
        # engine and oracle encode the same codes); a quarter of the rows
        # repeat another row's codes, so exact ties reach the merge
        m, dsub = 8, 4
        d = m * dsub
        cent = (rng.standard_normal((NLIST, d)) * 20.0).astype(np.float32)
        cb = rng.standard_normal((m, 256, dsub)).astype(np.float32)
        cw = codeword_rows(rng, cb, lbl, 0.05, 64)
        xb = (cent[lbl] + decode_rows(cb, cw)
              + 1e-3 * rng.standard_normal((NROWS, d))).astype(np.float32)
        q = (cent[rng.integers(0, NLIST, NQ)]
             + 0.7 * rng.standard_normal((NQ, d))).astype(np.float32)
        spec = {"type": typ, "dim": d, "metric": metric, "nlist": NLIST,
                "nprobe": NLIST, "seed": 1234, "m": m}
    return spec, cent, cb, xb, q, lbl, cw


def _build(typ, metric):
    """Engine and oracle over the same set_trained artifacts."""
    spec, cent, cb, xb, q, lbl, cw = _data(typ, metric)
    eng = engine_with(spec, cent, cb, xb=xb, split=1000)
    orc = from_engine_artifacts(spec, cent, cb)
    orc.add(xb)
    # both hold the intended lists
    np.testing.assert_array_equal([len(i) for i in orc.list_ids], LIST_SIZES)
    off, ids, _ = eng.get_lists()
    np.testing.assert_array_equal(np.diff(off), LIST_SIZES)
    np.testing.assert_array_equal(ids, np.concatenate(orc.list_ids))
    if cb is not None:
        np.testing.assert_array_equal(
            np.concatenate(orc.list_codes),
            np.concatenate([cw[lbl == l] for l in range(NLIST)]).astype(np.uint8))
    probes, keys = eng.coarse(q, NLIST)
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    return {"eng": eng, "orc": orc, "q": q, "probes": probes, "keys": keys}


_CASES = {}


def _case(typ, metric):
    if (typ, metric) not in _CASES:
        _CASES[(typ, metric)] = _build(typ, metric)
    return _CASES[(typ, metric)]


def _check(c, probes, keys, k):
    """wave == block bitwise, wave == oracle; returns the wave (D, I)."""
    wave, block = _both(
        lambda: c["eng"].search_preassigned(c["q"], probes, keys, k))
    assert_bitwise(*wave, *block)
    Do, Io = c["orc"].search_preassigned(c["q"], probes, keys, k)
    np.testing.assert_array_equal(wave[1], Io)
    np.testing.assert_array_equal(wave[0], Do)  # BITWISE
    return wave


TYPES = ["ivfpq", "ivf_flat"]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nprobe", [4, 5, 8, 9, 16, 17])
@pytest.mark.parametrize("typ", TYPES)
def test_cand_merge_k16(typ, nprobe, metric):
    # C = 64, 80, 128, 144, 256 on the wave kernel; 272 on the block kernel
    c = _case(typ, metric)
    _check(c, c["probes"][:, :nprobe], c["keys"][:, :nprobe], K)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nprobe", [1, 5, 32])
@pytest.mark.parametrize("typ", TYPES)
def test_cand_merge_k1(typ, nprobe, metric):
    c = _case(typ, metric)
    _check(c, c["probes"][:, :nprobe], c["keys"][:, :nprobe], 1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("typ", TYPES)
def test_cand_merge_same_list_twice(typ, metric):
    """Probes 0 and 1 name the same list: every row of it arrives twice as
    an exact (key, id) pair, and both copies are returned."""
    c = _case(typ, metric)
    probes = c["probes"][:, :4].copy()
    keys = c["keys"][:, :4].copy()
    probes[:, 1] = probes[:, 0]
    keys[:, 1] = keys[:, 0]
    D, I = _check(c, probes, keys, K)
    twice = 0
    for i in range(NQ):
        ids, cnt = np.unique(I[i][I[i] >= 0], return_counts=True)
        assert cnt.max() <= 2
        twice += int((cnt == 2).sum())
    assert twice > 0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("typ", TYPES)
def test_cand_merge_fewer_rows_than_k(typ, metric):
    """Lists 0-3 hold 0 + 1 + 2 + 3 rows: ranks 6.. are pads."""
    c = _case(typ, metric)
    probes = np.tile(np.arange(4, dtype=np.int32), (NQ, 1))
    col = np.argsort(c["probes"], axis=1)[:, :4]  # column of list 0..3
    keys = np.take_along_axis(c["keys"], col, axis=1)
    D, I = _check(c, probes, keys, K)
    assert (I[:, :6] >= 0).all() and (I[:, 6:] == -1).all()
    assert (D[:, 6:] == (-FLT_MAX if metric == IP else FLT_MAX)).all()
