# Spec key "scan_group_flat" (DESIGN.md §6q): cfg.extra carries it into the
# engine spec as a perf knob, for the ivf_simple builder and the IVFn,Flat
# factory form.
import pytest

from distributed_faiss_amd.engine_spec import resolve_engine_spec
from distributed_faiss_amd.index_cfg import IndexCfg


@pytest.mark.parametrize("how", [
    {"index_builder_type": "ivf_simple"},
    {"faiss_factory": "IVF64,Flat"},
], ids=["builder", "factory"])
def test_scan_group_flat_reaches_the_engine_spec(how):
    cfg = IndexCfg(dim=32, metric="l2", centroids=64, scan_group_flat=1, **how)
    assert cfg.extra == {"scan_group_flat": 1}
    spec = resolve_engine_spec(cfg, 10000)
    assert spec["type"] == "ivf_flat"
    assert spec["scan_group_flat"] == 1
    cfg.extra = {}
    assert "scan_group_flat" not in resolve_engine_spec(cfg, 10000)
