# PQ scan at the 16-code group boundaries of scan_row_dist.
#
# A row's codes are read in passes of 64 and summed in groups of 16. With
# m % 16 == 0 the scan takes the unguarded groups (DFANN_PROC16_PQ_FULL),
# any other m the per-code guarded ones. test_gpu_dispatch_parity section B
# pins m in {8, 16, 20, 32, 64, 96}; the shapes here add the group counts
# it lacks, built and compared exactly as there (its helpers, its 12 lists
# with the empty one, the ones shorter than a wave and the ones that are
# no multiple of the block size, bitwise against the oracle):
#   m = 48: third group present, fourth absent
#   m = 80: second 64-code pass with one group
#   m = 24, m = 72: guarded path, half a group in the first / second pass
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

import test_gpu_dispatch_parity as parity  # noqa: E402

K_REG, K_LDS = 10, 20  # register selection / LDS selection (k > 16)
assert K_LDS <= parity.K_LDS  # the shared oracle result is a top-40

GROUP_SHAPES = [
    pytest.param(48, 2, id="m48-dsub2-three_groups"),
    pytest.param(80, 2, id="m80-dsub2-second_pass_one_group"),
    pytest.param(24, 2, id="m24-dsub2-guarded_half_group"),
    pytest.param(72, 2, id="m72-dsub2-guarded_half_group_second_pass"),
]


@pytest.mark.parametrize("mode", parity.PQ_MODES)
@pytest.mark.parametrize("metric", parity.METRICS)
@pytest.mark.parametrize("m,dsub", GROUP_SHAPES)
def test_pq_scan_group_boundaries_bitexact(m, dsub, metric, mode):
    parity._run_pq(m, dsub, metric, mode, (K_REG, K_LDS))


@pytest.mark.parametrize("metric", parity.METRICS)
def test_pq_scan_three_groups_filtered(metric):
    """m = 48 through the filtered scan: the oracle's top-64 over all 1231
    rows, masked to the allowed ids, is the filtered top-k (two thirds of
    the rows are allowed, so 64 leave about 43; the test checks >= k)."""
    m, dsub = 48, 2
    key = ("pq", m, dsub, metric, False)
    case = parity._cached(key, lambda: parity._pq_case(m, dsub, metric, False))
    eng = parity._engine(dict(case["spec"]), case["xb"], case["cent"],
                         case["cb"])
    q = case["q"]
    probes, keys = eng.coarse(q, parity.NLIST)
    Do, Io = case["orc"].search_preassigned(q, probes, keys, 64)
    assert (Io >= 0).all()
    allow = np.ones((parity.NROWS + 31) // 32 * 32, bool)
    allow[:parity.NROWS] = np.arange(parity.NROWS) % 3 != 0
    for k in (K_REG, K_LDS):
        D, I = eng.search_preassigned_filtered(q, probes, keys, k, allow)
        for i in range(q.shape[0]):
            keep = allow[Io[i]]
            assert keep.sum() >= k
            np.testing.assert_array_equal(I[i], Io[i][keep][:k])
            np.testing.assert_array_equal(D[i], Do[i][keep][:k])  # BITWISE
