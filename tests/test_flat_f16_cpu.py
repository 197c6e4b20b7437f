# Flat fp16 store, the part that needs no GPU: how the
# factory string "SQfp16" and the builder key "flat_store" resolve.
import pytest

from distributed_faiss_amd.engine_spec import (ENGINE_PERF_KNOBS, FLAT_KEYS,
                                               resolve_engine_spec)
from distributed_faiss_amd.index_cfg import IndexCfg


@pytest.mark.parametrize("metric,code", [("dot", 0), ("l2", 1)])
def test_factory_sqfp16_is_flat_fp16(metric, code):
    spec = resolve_engine_spec(
        IndexCfg(faiss_factory="SQfp16", dim=24, metric=metric), 1000)
    assert spec["type"] == "flat" and spec["flat_store"] == "fp16"
    assert spec["metric"] == code and spec["dim"] == 24


@pytest.mark.parametrize("metric", ["dot", "l2"])
def test_builder_flat_store_stays_inner_product(metric):
    spec = resolve_engine_spec(
        IndexCfg(index_builder_type="flat", dim=24, metric=metric,
                 flat_store="fp16"), 1000)
    assert spec["type"] == "flat" and spec["flat_store"] == "fp16"
    assert spec["metric"] == 0
    plain = resolve_engine_spec(
        IndexCfg(index_builder_type="flat", dim=24, metric=metric), 1000)
    assert "flat_store" not in plain


def test_flat_store_changes_results_so_is_no_perf_knob():
    assert FLAT_KEYS == ("flat_store",)
    assert not set(FLAT_KEYS) & set(ENGINE_PERF_KNOBS)


def test_unsupported_factory_message_lists_sqfp16():
    with pytest.raises(NotImplementedError, match=r"Flat, SQfp16, IVFn,Flat"):
        resolve_engine_spec(
            IndexCfg(faiss_factory="SQ8", dim=24, metric="l2"), 1000)
