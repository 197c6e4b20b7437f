# Engine spec resolution: IndexCfg -> engine spec dict.
#
# Restates the reference's builder table and factory-string path
# (distributed_faiss/index.py:25-100 builders, :380-401 _init_faiss_index,
# :497-508 infer_n_centroids) as a backend-neutral spec dict consumed by
# both the HIP engine (distributed_faiss_amd/hip_engine.py) and the test
# oracle. Engine spec keys:
#   type:    "flat" | "ivf_flat" | "ivfpq" | "ivfsq"
#   dim, metric (0=IP, 1=L2), nlist, m, nbits (ivfpq: 4 | 8; DESIGN.md
#   §6d), sq_type ("fp16"|"8bit"|"6bit"|"4bit"), nprobe, seed
#   refine ("fp32"|"fp16"), k_factor: exact re-ranking over ivfpq / ivfsq
#   (faiss IndexRefineFlat / IndexRefine)
#   opq (1), opq_dim, opq_niter: learned orthonormal pre-transform in front
#   of ivfpq (faiss IndexPreTransform(OPQMatrix))
#
# Behavioral quirks kept on purpose (SURVEY.md §2 quirk list):
#   * builder "flat" ALWAYS builds an inner-product flat index, ignoring
#     cfg.metric (reference index.py:94: lambda cfg: faiss.IndexFlatIP).
#   * builder "knnlm" overwrites cfg.nprobe with the fresh index's default
#     nprobe == 1 (reference index.py:47: cfg.nprobe = index.nprobe).
#   * builder "ivfsq" uses the fp16 codec, not 8-bit (reference
#     index.py:65); 8-, 6- and 4-bit SQ are reachable only via the factory
#     string (e.g. "IVF{centroids},SQ8", reference
#     tests/test_index_config.json).

import math
import re

from .index_cfg import IndexCfg, METRIC_INNER_PRODUCT

DEFAULT_SEED = 1234


def infer_n_centroids(total_data_size: int) -> int:
    # Reference index.py:497-508 verbatim thresholds (note they use 10e5
    # == 1e6 etc. — kept as written).
    if total_data_size < 10e5:
        return int(2 * math.sqrt(total_data_size))
    elif total_data_size < 10e6:
        return 65536
    elif total_data_size < 10e7:
        return 262144
    return 1048576


def _base(cfg: IndexCfg) -> dict:
    return {
        "dim": cfg.dim,
        "metric": cfg.get_metric(),
        "nprobe": int(cfg.nprobe),
        "seed": int(cfg.extra.get("seed", DEFAULT_SEED)),
    }


def _builder_spec(cfg: IndexCfg) -> dict:
    t = cfg.index_builder_type
    spec = _base(cfg)
    if t == "flat":
        # reference index.py:94 — always IP, metric ignored (quirk 3)
        spec.update(type="flat", metric=METRIC_INNER_PRODUCT)
        return spec
    if t == "ivf_simple":
        # reference index.py:36-40
        spec.update(type="ivf_flat", nlist=int(cfg.centroids))
        return spec
    if t == "knnlm":
        # reference index.py:43-48; fresh faiss IndexIVFPQ has nprobe=1 and
        # the builder writes it back into cfg.
        cfg.nprobe = 1
        spec.update(
            type="ivfpq",
            nlist=int(cfg.centroids),
            m=int(cfg.extra.get("code_size", 64)),
            nbits=int(cfg.extra.get("bits_per_vector", 8)),
            nprobe=1,
        )
        return _apply_refine(cfg, _apply_opq(cfg, spec))
    if t == "ivfsq":
        # reference index.py:63-68 — QT_fp16
        spec.update(type="ivfsq", nlist=int(cfg.centroids), sq_type="fp16")
        return _apply_refine(cfg, spec)
    if t == "hnswsq":
        # reference index.py:51-60: faiss.IndexHNSWSQ(dim, QT_8bit,
        # store_n) — L2 asserted; efSearch = cfg.nprobe at build,
        # efConstruction from cfg.extra. Deviation (documented,
        # DESIGN.md §hnsw): our engine honors later set_nprobe as
        # efSearch, where the reference's set_nprobe is a silent no-op
        # on an HNSW index (faiss_index.nprobe is not efSearch).
        assert cfg.get_metric() == 1, "hnsw is supposed to work with L2 sim space"
        spec.update(
            type="hnswsq",
            m=int(cfg.extra.get("store_n", 128)),
            ef_construction=int(cfg.extra.get("ef_construction", 100)),
        )
        return spec
    if t == "ivf_gpu":
        raise NotImplementedError(
            "index_builder_type='ivf_gpu' is out of scope (the faiss-GPU "
            "wrapper is exactly what this engine replaces, SURVEY.md §2)"
        )
    raise KeyError(f"unknown index_builder_type {t!r}")


# optional third component, PQ / SQ bases only: faiss IndexRefineFlat
# ("RFlat") and IndexRefine over an fp16 scalar quantizer ("Refine(SQfp16)")
# optional first component, PQ bases only: faiss OPQMatrix ("OPQ<m>" or
# "OPQ<m>_<d_out>")
_FACTORY_RE = re.compile(
    r"^(?:OPQ(?P<opq_m>\d+)(?:_(?P<opq_d>\d+))?,)?"
    r"IVF(\d+),(?:(Flat)|(PQ(\d+)(?:x(\d+))?|SQ8|SQ6|SQ4|SQfp16)"
    r"(?:,(RFlat|Refine\(SQfp16\)))?)$")
_FACTORY_REFINE = {"RFlat": "fp32", "Refine(SQfp16)": "fp16"}
# faiss QT_8bit / QT_6bit / QT_4bit / QT_fp16 -> engine "sq_type"
_FACTORY_SQ = {"SQ8": "8bit", "SQ6": "6bit", "SQ4": "4bit", "SQfp16": "fp16"}
# "PQ<m>x<b>": bits per sub-quantizer code; "PQ<m>" is faiss's default 8
PQ_NBITS_SUPPORTED = (4, 8)

# Refine keys of cfg.extra. NOT perf knobs: they change results.
REFINE_KEYS = ("refine", "k_factor")
# OPQ keys of cfg.extra (builder knnlm; "opq_niter" also with an OPQ factory
# string). Result-changing like REFINE_KEYS, not perf knobs.
OPQ_KEYS = ("opq", "opq_dim", "opq_niter")


def _apply_opq(cfg: IndexCfg, spec: dict) -> dict:
    """cfg.extra["opq"] (truthy), ["opq_dim"], ["opq_niter"] on the ivfpq
    builder; the engine checks m | opq_dim <= dim."""
    if cfg.extra.get("opq"):
        spec["opq"] = 1
        if "opq_dim" in cfg.extra:
            spec["opq_dim"] = int(cfg.extra["opq_dim"])
        if "opq_niter" in cfg.extra:
            spec["opq_niter"] = int(cfg.extra["opq_niter"])
    return spec


def _apply_refine(cfg: IndexCfg, spec: dict) -> dict:
    """cfg.extra["refine"] ("fp32"|"fp16", builders knnlm / ivfsq) and
    cfg.extra["k_factor"] (builders and factory strings)."""
    if cfg.extra.get("refine"):
        spec["refine"] = str(cfg.extra["refine"])
    if "k_factor" in cfg.extra and spec.get("refine"):
        spec["k_factor"] = float(cfg.extra["k_factor"])
    return spec


def _factory_spec(cfg: IndexCfg, total_data_size: int) -> dict:
    # reference index.py:380-401: centroid inference + {centroids} substitution,
    # then faiss.index_factory(dim, str, metric) — metric IS respected here.
    cfg.centroids = int(cfg.centroids)
    if cfg.centroids == 0 or cfg.infer_centroids:
        cfg.centroids = infer_n_centroids(total_data_size)
    s = cfg.faiss_factory
    if "{centroids}" in s:
        s = s.format(centroids=cfg.centroids)
    spec = _base(cfg)
    if s == "Flat":
        spec.update(type="flat")
        return spec
    mm = _FACTORY_RE.match(s)
    if not mm:
        raise NotImplementedError(
            f"factory string {s!r} not supported; supported: Flat, IVFn,Flat, "
            "IVFn,PQm, IVFn,PQmx4, IVFn,PQmx8, IVFn,SQ8, IVFn,SQ6, IVFn,SQ4, "
            "IVFn,SQfp16, "
            "the PQ / SQ forms followed by ,RFlat or ,Refine(SQfp16), and "
            "the PQ forms preceded by OPQm, or OPQm_d, (same m)"
        )
    opq_m = mm.group("opq_m")
    nlist = int(mm.group(3))
    kind = mm.group(4) or mm.group(5)
    if opq_m is not None and not kind.startswith("PQ"):
        raise NotImplementedError(
            f"factory string {s!r}: OPQ is supported in front of IVFn,PQm "
            "only, not Flat / SQ8 / SQ6 / SQ4 / SQfp16"
        )
    if kind == "Flat":
        spec.update(type="ivf_flat", nlist=nlist)
        return spec
    if kind.startswith("PQ"):
        nbits = int(mm.group(7)) if mm.group(7) else 8
        if nbits not in PQ_NBITS_SUPPORTED:
            raise NotImplementedError(
                f"factory string {s!r}: PQ with {nbits} bits per code not "
                f"supported; supported: {list(PQ_NBITS_SUPPORTED)}"
            )
        spec.update(type="ivfpq", nlist=nlist, m=int(mm.group(6)), nbits=nbits)
        if opq_m is not None:
            if int(opq_m) != spec["m"]:
                raise NotImplementedError(
                    f"factory string {s!r}: OPQ{opq_m} in front of "
                    f"PQ{spec['m']} not supported (the OPQ m must equal the "
                    "PQ m)"
                )
            spec["opq"] = 1
            if mm.group("opq_d"):
                spec["opq_dim"] = int(mm.group("opq_d"))
            if "opq_niter" in cfg.extra:
                spec["opq_niter"] = int(cfg.extra["opq_niter"])
    else:
        spec.update(type="ivfsq", nlist=nlist, sq_type=_FACTORY_SQ[kind])
    if mm.group(8):
        spec["refine"] = _FACTORY_REFINE[mm.group(8)]
        if "k_factor" in cfg.extra:
            spec["k_factor"] = float(cfg.extra["k_factor"])
    return spec


# Engine performance knobs passed through from cfg.extra (our extension:
# the reference has no equivalent — faiss knobs ride the factory string).
# Documented in INTEGRATION.md; consumed by the HIP engine
# (csrc/dfann.hip create_from_spec), ignored by the test oracle.
ENGINE_PERF_KNOBS = (
    "coarse_bf16",    # assign/coarse GEMMs on bf16 MFMA (approximate path)
    "max_ppc",        # k-means subsample cap per centroid
    "ws_mb",          # workspace chunk budget (key matrices)
    "pq_precomputed", # PQ-L2 term2/term3 tables
    "pq_lut_global",  # ADC LUTs built to HBM (GLUT scan path)
    "pq_lut_mb",      # GLUT chunk budget
    "pq_lut_f16",     # fp16 ADC tables (tolerance path)
    "scan_fan",       # list-segment fan (experiment knob)
    "range_max_results",  # range search: largest result, in hits
)


def _apply_perf_knobs(cfg: IndexCfg, spec: dict) -> dict:
    for k in ENGINE_PERF_KNOBS:
        if k in cfg.extra:
            spec[k] = cfg.extra[k]
    return spec


def resolve_engine_spec(cfg: IndexCfg, total_data_size: int) -> dict:
    """Mirror of reference Index._init_faiss_index (index.py:380-401)."""
    if cfg.index_builder_type:
        return _apply_perf_knobs(cfg, _builder_spec(cfg))
    if cfg.faiss_factory:
        return _apply_perf_knobs(cfg, _factory_spec(cfg, total_data_size))
    raise RuntimeError(
        "Either faiss_factory or valid index_builder_type should be specified "
        "to initialize index"
    )
