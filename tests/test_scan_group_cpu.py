# Spec key "scan_group" (DESIGN.md §6n): cfg.extra carries it into the engine
# spec as a perf knob, for the ivfsq builder and the IVFn,SQfp16 factory form.
import pytest

from distributed_faiss_amd.engine_spec import resolve_engine_spec
from distributed_faiss_amd.index_cfg import IndexCfg


@pytest.mark.parametrize("how", [
    {"index_builder_type": "ivfsq"},
    {"faiss_factory": "IVF64,SQfp16"},
], ids=["builder", "factory"])
def test_scan_group_reaches_the_engine_spec(how):
    cfg = IndexCfg(dim=32, metric="l2", centroids=64, scan_group=1, **how)
    assert cfg.extra == {"scan_group": 1}
    spec = resolve_engine_spec(cfg, 10000)
    assert spec["type"] == "ivfsq" and spec["sq_type"] == "fp16"
    assert spec["scan_group"] == 1
    cfg.extra = {}
    assert "scan_group" not in resolve_engine_spec(cfg, 10000)
