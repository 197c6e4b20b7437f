# Spec key "scan_group_pq" (DESIGN.md §6p): cfg.extra carries it into the
# engine spec as a perf knob, for the knnlm builder and the IVFn,PQm factory
# form.
import pytest

from distributed_faiss_amd.engine_spec import resolve_engine_spec
from distributed_faiss_amd.index_cfg import IndexCfg


@pytest.mark.parametrize("how", [
    {"index_builder_type": "knnlm"},
    {"faiss_factory": "IVF64,PQ8"},
], ids=["builder", "factory"])
def test_scan_group_pq_reaches_the_engine_spec(how):
    cfg = IndexCfg(dim=32, metric="l2", centroids=64, scan_group_pq=1, **how)
    assert cfg.extra == {"scan_group_pq": 1}
    spec = resolve_engine_spec(cfg, 10000)
    assert spec["type"] == "ivfpq" and spec["nbits"] == 8
    assert spec["scan_group_pq"] == 1
    cfg.extra = {}
    assert "scan_group_pq" not in resolve_engine_spec(cfg, 10000)
