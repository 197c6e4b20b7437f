# Spec key "scan_group_sq8" (DESIGN.md §6o): cfg.extra carries it into the
# engine spec as a perf knob for the IVFn,SQ8 factory form.
from distributed_faiss_amd.engine_spec import resolve_engine_spec
from distributed_faiss_amd.index_cfg import IndexCfg


def test_scan_group_sq8_reaches_the_engine_spec():
    cfg = IndexCfg(dim=32, metric="l2", centroids=64, scan_group_sq8=1,
                   faiss_factory="IVF64,SQ8")
    assert cfg.extra == {"scan_group_sq8": 1}
    spec = resolve_engine_spec(cfg, 10000)
    assert spec["type"] == "ivfsq" and spec["sq_type"] == "8bit"
    assert spec["scan_group_sq8"] == 1
    cfg.extra = {}
    assert "scan_group_sq8" not in resolve_engine_spec(cfg, 10000)
