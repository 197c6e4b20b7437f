# ORACLE — CPU restatement of the reference hot path's arithmetic.
#
# TEST INFRASTRUCTURE ONLY. Only tests/, __graft_entry__.smoke() and
# bench.py's cpu_baseline leg may import, call or execute anything in this
# package. The product path (distributed_faiss_amd/) never imports it and
# fails loudly when the HIP engine is missing on a GPU box.
#
# What this restates: the arithmetic the reference delegates to the
# un-vendored third-party `faiss-cpu>=1.7.2` wheel (reference setup.py:32),
# at the call sites of distributed_faiss/index.py:
#   - train      (index.py:217)  k-means coarse quantizer, PQ codebooks, SQ ranges
#   - add        (index.py:425)  coarse assign + PQ/SQ encode + list append
#   - search     (index.py:257)  coarse top-nprobe + list scan + top-k
#   - search_and_reconstruct (index.py:255)
#   - reconstruct_n (index.py:350, quantizer centroids)
# and the client merge (reference client.py:29-54, 265-310).
#
# PARITY PINNING STATUS: faiss cannot be imported or built
# in this container and its sources are not vendored under /root/reference,
# so for IVF/IVFPQ/IVFSQ numerical results this oracle is PARITY UNPINNED —
# it restates faiss v1.7's documented algorithms (residual IVFPQ with
# ksub=256 ADC LUT scan; SQ fp16 and 8-bit min/max affine codec; k-means
# with fixed iteration count) and WE generate the golden vectors
# (tests/golden/, script tests/golden/make_golden.py). What IS pinned by
# the reference's own tests and is ported verbatim into tests/:
#   - the merge known-answer test (reference tests/test_integration.py:181-203)
#   - the sharded==single-flat equality invariant
#     (reference tests/test_integration.py:205-265)
#
# Deliberate deviations from faiss (documented in DESIGN.md §oracle):
#   - k-means subsampling is strided, not random (the reference's own
#     training-data order is nondeterministic — index.py:211 shuffles with
#     the unseeded global numpy RNG — so random-subsample equivalence is
#     unobservable through the reference API anyway).
#   - k-means empty-cluster handling: split the largest cluster,
#     deterministic (faiss splits a probabilistically chosen one).
#   - ties everywhere break to the lower id (faiss heap behavior for
#     within-list scans; cross-list tie order in faiss is heap-order
#     dependent and unpinned).
#
# Engine-side options restated here (the engine's own contracts, not
# faiss-cpu behaviour unless noted; each DEFINES a bit-exact tier of the
# GPU suite and is checked on the CPU against an independent formula):
#   - core.OracleIVFPQ(nbits=4|8): one class over ksub = 1 << nbits
#     (DESIGN.md §6d); pack_pq4 / unpack_pq4 give the stored 4-bit rows;
#   - core.OracleIVFSQ(qtype=fp16|8bit|6bit|4bit): one integer-codec path
#     over Q = (1 << bits) - 1; pack_sq / unpack_sq give the
#     stored 4- and 6-bit rows;
#   - every IVF oracle: packed_lists() / load_lists() exchange inverted
#     lists with an engine as stored bytes, and from_engine_artifacts()
#     builds a trained oracle from an engine's centroids, codebooks or
#     ranges and, optionally, its lists;
#   - refine.py: the exact re-ranking stage;
#   - range.py: range search over any IVF oracle's _scan_one (§6g);
#   - opq.py: the OPQ pre-transform, OracleOPQ and the OPQ trainer (§6f).
# make_oracle_engine builds the plain index of a spec and ignores the opq,
# refine and k_factor keys.
#
# fp16-LUT tier (spec "pq_lut_f16"): OracleIVFPQ rounds every
# ADC table entry to IEEE half once (numpy float16: round-to-nearest-even,
# gradual underflow), widens it back to fp32 and sums sequentially in fp32
# exactly as the exact path does; the IP bias stays fp32. This DEFINES the
# engine's fp16-LUT scan bit for bit (tests/test_gpu_dispatch_parity.py);
# it is the engine's own table approximation (faiss GpuIndexIVFPQ
# useFloat16LookupTables analogue), not a faiss-cpu behaviour.
#
# hnswsq tier (oracle/hnsw.py): BOTH sides are restated
# op-for-op. core.OracleHNSWSearch mirrors k_hnsw_search over any graph of
# the hnsw_dump layout; core.OracleHNSWBuild mirrors the build — host level
# draws and wave schedule, k_hnsw_insert over the frozen snapshot, the
# (dst, level, src)-sorted reverse-link merge of k_hnsw_apply (fast path,
# over-cap prune, truncation of a run to 1024 candidates), the entry
# update and the refine pass. The engine's graph dump and its search
# results over that graph are bitwise equal to the oracle's
# (tests/test_hnsw.py, tests/test_gpu_hnsw_build.py). The batched wave
# insertion itself is a documented deviation from faiss's sequential
# insertion (parity with faiss unpinned there by construction; graph
# quality is held by the recall property gate).

from .core import (  # noqa: F401
    METRIC_INNER_PRODUCT,
    METRIC_L2,
    splitmix64_seq,
    partial_shuffle_indices,
    kmeans,
    OracleFlat,
    OracleIVFFlat,
    OracleIVFPQ,
    OracleIVFSQ,
    pack_pq4,
    unpack_pq4,
    pack_sq,
    unpack_sq,
    sq_code_bytes,
    sq_stride,
    make_oracle_engine,
    from_engine_artifacts,
    save_oracle_engine,
    load_oracle_engine,
    OracleProvider,
    aggregate_results,
    OracleHNSWSearch,
    OracleHNSWBuild,
)
from .opq import OracleOPQ  # noqa: F401
from .range import (  # noqa: F401
    range_from_scans,
    range_search_ref,
    ranking,
    scan_lists,
)
from .refine import (  # noqa: F401
    k_prime,
    refine_distances,
    refine_ref,
)
