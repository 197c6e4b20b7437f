# Pipelined IVF search (DESIGN.md §3 "Search pipeline"): the query batch cut
# into chunks that go round-robin over two stream lanes.
#
# Every case runs search_dev on ONE engine twice, with DFANN_PIPE_LANES=2
# (and a small DFANN_PIPE_CHUNK, so that there are full chunks and a ragged
# one) and with DFANN_PIPE_LANES=1, the serial path. The knobs are read per
# call. Each stage of the search is independent per query row, so the two
# results must be equal bit for bit.
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

from distributed_faiss_amd.hip_engine import HipEngine  # noqa: E402
from gpu_support import assert_bitwise  # noqa: E402

IP, L2 = 0, 1
METRICS = [pytest.param(IP, id="ip"), pytest.param(L2, id="l2")]
LANES, CHUNK = "DFANN_PIPE_LANES", "DFANN_PIPE_CHUNK"
D, NLIST, NROWS, NPROBE, K = 64, 32, 4000, 4, 10
NQ, NQ_CHUNK = 200, 64  # three full chunks and a ragged one of 8


class _knobs:
    """The two overrides set for the block, and put back after it."""

    def __init__(self, lanes, chunk=None):
        self.want = {LANES: str(lanes),
                     CHUNK: None if chunk is None else str(chunk)}

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in self.want}
        for k, v in self.want.items():
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _data(n, nq, d, seed):
    """Rows and queries around 64 shared centres, so that lists differ in
    length and a query's probed lists hold near rows."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((64, d)).astype(np.float32)
    xb = centres[rng.integers(0, 64, n)] + rng.standard_normal((n, d))
    q = centres[rng.integers(0, 64, nq)] + rng.standard_normal((nq, d))
    return xb.astype(np.float32), q.astype(np.float32)


def _trained(spec, xb):
    eng = HipEngine(spec=spec)
    eng.train(xb)
    eng.add(xb)
    return eng


def _search(eng, qt, k, lanes, chunk):
    with _knobs(lanes, chunk):
        Dt, It = eng.search_dev(qt, k)
    torch.cuda.synchronize()
    return Dt.cpu().numpy(), It.cpu().numpy()


def _assert_lanes_agree(eng, q, k=K, chunk=NQ_CHUNK):
    qt = torch.as_tensor(q).cuda()
    D2, I2 = _search(eng, qt, k, 2, chunk)
    D1, I1 = _search(eng, qt, k, 1, chunk)
    assert D1.shape == (len(q), k)
    assert (I1[:, 0] >= 0).all()  # a real result, not pads
    assert_bitwise(D2, I2, D1, I1)
    return D1, I1


def _spec(typ, metric, **kw):
    return dict({"type": typ, "dim": D, "metric": metric, "nlist": NLIST,
                 "nprobe": NPROBE, "seed": 1234}, **kw)


PQ8_F16 = dict(m=8, nbits=8, pq_lut_f16=1)  # the fp16 GLUT scan path


@pytest.fixture(scope="module")
def small():
    return _data(NROWS, 700, D, seed=11)


@pytest.fixture(scope="module")
def pq_engine(small):
    """One L2 fp16-GLUT IVFPQ engine shared by the cases that only search."""
    return _trained(_spec("ivfpq", L2, **PQ8_F16), small[0])


@pytest.mark.parametrize("metric", METRICS)
def test_pq8_fp16_lut(small, metric):
    xb, q = small
    eng = _trained(_spec("ivfpq", metric, **PQ8_F16), xb)
    _assert_lanes_agree(eng, q[:NQ])


@pytest.mark.parametrize("metric", METRICS)
def test_fused_coarse(metric):
    """nq = 600 at chunk 256: two full M tiles and a ragged 88-row chunk,
    which must go through k_gemm_bf16_256_topk like the whole batch."""
    nlist, n, nq = 2048, 20000, 600
    rng = np.random.default_rng(5)
    cent = rng.standard_normal((nlist, D)).astype(np.float32)
    xb = (cent[rng.integers(0, nlist, n)]
          + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    q = (cent[rng.integers(0, nlist, nq)]
         + 0.3 * rng.standard_normal((nq, D))).astype(np.float32)
    eng = HipEngine(spec={"type": "ivf_flat", "dim": D, "metric": metric,
                          "nlist": nlist, "nprobe": 8, "seed": 1234,
                          "coarse_bf16": 1})
    eng.set_trained(cent)
    eng.add(xb)
    _assert_lanes_agree(eng, q, chunk=256)


@pytest.mark.parametrize("spec", [
    pytest.param(_spec("ivfsq", L2, sq_type="8bit"), id="ivfsq8"),
    pytest.param(_spec("ivf_flat", IP), id="ivfflat"),
])
def test_other_ivf_types(small, spec):
    xb, q = small
    _assert_lanes_agree(_trained(spec, xb), q[:NQ])


def test_refine_around_pipelined_base(small):
    xb, q = small
    eng = _trained(_spec("ivfpq", L2, refine="fp32", k_factor=4.0, **PQ8_F16),
                   xb)
    _assert_lanes_agree(eng, q[:NQ])


def test_graph_capture(small, pq_engine):
    """A lanes=2 search captured under torch.cuda.graph: the lanes join the
    capture as parallel branches. Replays, also with another query batch in
    the static input, equal the eager serial result."""
    _, q = small
    qa, qb = q[:NQ], q[NQ:2 * NQ]
    ref_a = _assert_lanes_agree(pq_engine, qa)  # also the warm-up
    ref_b = _assert_lanes_agree(pq_engine, qb)
    q_static = torch.as_tensor(qa).cuda()
    D_static = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
    I_static = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    with _knobs(2, NQ_CHUNK):
        with torch.cuda.graph(g):
            pq_engine.search_dev(q_static, K, D_static, I_static)
    for batch, ref in ((None, ref_a), (None, ref_a), (qb, ref_b)):
        if batch is not None:
            q_static.copy_(torch.as_tensor(batch).cuda())
        D_static.zero_()
        I_static.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_bitwise(D_static.cpu().numpy(), I_static.cpu().numpy(), *ref)


def test_workspace_growth_and_second_engine(small, pq_engine):
    """nq 200, 700, 200 on one engine (the lanes' workspaces grow, then are
    reused), with the calls of a second engine in between."""
    xb, q = small
    other = _trained(_spec("ivfsq", L2, sq_type="8bit"), xb[:2000])
    for nq in (200, 700, 200):
        _assert_lanes_agree(pq_engine, q[:nq])
        _assert_lanes_agree(other, q[:nq])


def test_serial_fallback_below_one_chunk(small, pq_engine):
    _, q = small
    _assert_lanes_agree(pq_engine, q[:40])


def test_serial_fallback_timing(small, pq_engine):
    """With timing on the call stays serial, and the per-stage buckets are
    filled as they are without the knob."""
    _, q = small
    pq_engine.set_timing(True)
    try:
        pq_engine.get_timing()
        qt = torch.as_tensor(q[:NQ]).cuda()
        D2, I2 = _search(pq_engine, qt, K, 2, NQ_CHUNK)
        t = pq_engine.get_timing()
    finally:
        pq_engine.set_timing(False)
    for bucket in ("gemm_ms", "lut_ms", "scan_ms", "merge_ms"):
        assert t[bucket] > 0, (bucket, t)
    assert t["scan_launches"] == 1  # one scan over the whole batch
    D1, I1 = _search(pq_engine, qt, K, 1, NQ_CHUNK)
    assert_bitwise(D2, I2, D1, I1)


def test_serial_fallback_filtered(small, pq_engine):
    _, q = small
    allow = np.random.default_rng(3).random(NROWS) < 0.5
    with _knobs(2, NQ_CHUNK):
        D2, I2 = pq_engine.search_filtered(q[:NQ], K, allow)
    with _knobs(1):
        D1, I1 = pq_engine.search_filtered(q[:NQ], K, allow)
    assert allow[I1[I1 >= 0]].all()
    assert_bitwise(D2, I2, D1, I1)
