# Factory strings of IVF-RaBitQ: no GPU needed.
import pytest

from distributed_faiss_amd.engine_spec import resolve_engine_spec
from distributed_faiss_amd.index_cfg import IndexCfg


def _resolve(factory, **extra):
    cfg = IndexCfg(faiss_factory=factory, dim=96, metric="l2", nprobe=4,
                   **extra)
    return resolve_engine_spec(cfg, 10000)


@pytest.mark.parametrize("factory, more", [
    ("IVF8,RaBitQ", {}),
    ("RR,IVF8,RaBitQ", {"rr": 1}),
    ("IVF8,RaBitQ,RFlat", {"refine": "fp32", "k_factor": 4.0}),
    ("RR,IVF8,RaBitQ,Refine(SQfp16)", {"rr": 1, "refine": "fp16",
                                       "k_factor": 4.0}),
])
def test_factory_forms(factory, more):
    assert _resolve(factory, k_factor=4) == dict(
        {"type": "ivfrabitq", "dim": 96, "metric": 1, "nlist": 8, "nprobe": 4,
         "seed": 1234}, **more)


@pytest.mark.parametrize("factory", [
    "IVF8,RaBitQx2", "RaBitQ", "OPQ8,IVF8,RaBitQ", "RR,IVF8,PQ8"])
def test_malformed_neighbours(factory):
    with pytest.raises(NotImplementedError, match="RR,IVFn,RaBitQ"):
        _resolve(factory)
