/* dfann — MI355X-native ANN engine, C-ABI boundary.
 *
 * This library replaces the faiss Python-module surface consumed by the
 * reference's distributed_faiss/index.py and client.py.
 * Each entry point cites the reference interface it replaces. Host
 * bindings: ctypes (distributed_faiss_amd/hip_engine.py); see
 * INTEGRATION.md for the binding a maintainer would add.
 *
 * Conventions:
 *  - all functions return 0 on success, nonzero on error;
 *    dfann_last_error() gives the message (thread-local).
 *  - pointers suffixed _dev are DEVICE (HIP) pointers — tensors already
 *    resident in HBM; pointers suffixed _host are host memory.
 *  - `stream` is a hipStream_t (pass the caller's current stream; 0 ok).
 *  - distances follow faiss conventions: L2 = squared distance
 *    (minimize), IP = dot product (maximize); unfilled result slots are
 *    I = -1 with D = +FLT_MAX (L2) / -FLT_MAX (IP).
 *  - ids are implicit arrival positions per index (reference quirk,
 *    SURVEY.md §2 item 9).
 *  - filtered search (dfann_search_filtered,
 *    dfann_search_preassigned_filtered) takes an allow-bitmap over those
 *    ids and applies it inside the scan kernels.
 *
 * Limits (engine caps; the faiss-backed reference has none of these):
 *  - k (top-k) <= 512 everywhere (dfann_search*, dfann_merge_topk):
 *    selection buffers are sized SEL_CAP=1024 with k<=512 headroom.
 *    Larger k returns an error ("k > 512 unsupported").
 *  - nprobe is clamped to min(nlist, 512). A request above 512 is
 *    honored as 512 and a one-time warning is printed to stderr (the
 *    reference would probe more lists; recall at nprobe=512 is the cap).
 *  - per-shard ntotal < 2^32: ids round-trip through u32 inside the
 *    scan/merge kernels (CSR positions and merge slots are u32), so one
 *    shard holds at most 4.29e9 vectors. The C-ABI keeps i64 ids; the
 *    1B-vector headline config is 8 shards x 125M, well inside the cap.
 *  - refine stage: the base stage is searched at
 *    k' = min(512, max(k, ceil(k * k_factor))). The clamp at 512 is SILENT:
 *    k = 40 with k_factor = 13 re-ranks 512 candidates, not 520. A product
 *    k * k_factor within 1e-4 above an integer counts as that integer
 *    (k_factor travels as float32: 10 * 1.6f re-ranks 16, not 17).
 *  - refine needs dim <= 15360 (the query is staged in LDS next to the
 *    512-entry sort buffer).
 *
 * OPQ pre-transform ("opq": 1, ivfpq only): the index is
 * faiss IndexPreTransform(OPQMatrix(dim, m, opq_dim), IndexIVFPQ). A linear
 * map y = A x, A (opq_dim, dim) fp32 row-major with orthonormal rows and no
 * bias, runs in front of an ivfpq that works entirely at opq_dim: callers
 * pass and receive dim-wide vectors (dfann_dim, dfann_search_reconstruct,
 * the refine store), while everything faiss extract_index_ivf would reach
 * lives at opq_dim — dfann_get_centroids is (nlist, opq_dim), the
 * codebooks (m, 1 << nbits, opq_dim / m). The transform always runs in
 * fp32 (whatever "coarse_bf16" says) in one kernel whose per-row result
 * does not depend on the batch it came in, and counts under gemm_ms /
 * gemm_flops. Deviations from faiss OPQMatrix::train: 16 outer iterations
 * by default ("opq_niter"; faiss 50), k-means 25 iterations on the first
 * round and 4 hot-started after (faiss 40 / 4), at most 65536 strided
 * training rows, and the polar factor by Newton-Schulz in fp64 on the GPU
 * instead of an SVD.
 *
 * Hostile input. A bad vector or probe gives pads or an
 * error, never a read or write indexed by an unchecked value:
 *  S1 a probe outside [0, nlist) (-1, nlist, INT32_MIN, INT32_MAX, ...) is an
 *     EMPTY SLOT in every scan mode, in the LUT kernels and in both range
 *     passes; the keys entry of such a slot is never read. dfann_coarse
 *     reports a slot it cannot fill (a NaN row; a list whose key is not
 *     < FLT_MAX) as probe -1 with key +FLT_MAX. Deviation: faiss asserts
 *     key < nlist; here that would cost a host sync, so the slot is skipped
 *     (as faiss search_preassigned skips -1).
 *  S2 a query row holding a NaN returns all pads (I = -1, D = +FLT_MAX for
 *     L2 / -FLT_MAX for IP) from every search entry and index type, zero
 *     rows from dfann_search_reconstruct, zero hits from range search.
 *  S3 a row holding +-Inf but no NaN returns a well-formed result: valid,
 *     distinct ids first, pads last, D never NaN and monotone in the
 *     metric's order (D may be +-Inf). Nothing more is promised.
 *  S4 the other rows of the batch are not affected: they return bitwise
 *     what they return with each bad row replaced by a zero row.
 *  S5 dfann_search_preassigned[_filtered]: k in 1..512, 1 <= nprobe <= 512,
 *     nq == 0 returns at once; the error names the argument.
 *  A1 dfann_train refuses a training set holding a NaN or Inf ("train: the
 *     training set holds a non-finite value (NaN|Inf)") before it learns
 *     anything; the index stays untrained and a later clean train gives the
 *     artifacts of a fresh index. Finite rows no centroid can be assigned to
 *     (products overflow fp32) end in a "train:" error too. flat trains
 *     nothing and accepts anything.
 *  A2 dfann_add, ivf types: rows are taken in internal chunks of
 *     max(65536, ws_mb MB / 4 dim) rows. A chunk with a row that has no
 *     nearest centroid (a NaN row; products that overflow) is refused as a
 *     whole — "add: row R of the batch has no nearest centroid", R the first
 *     such row — with nothing of it stored; chunks before it stay and
 *     ntotal counts them. Searches after a refused add return what they
 *     did before, and a later clean add gives the lists of an index that
 *     never saw the bad batch. An Inf row that does get a list is stored as
 *     it is (faiss does the same); it cannot affect other rows. hnswsq
 *     refuses any batch holding a NaN or Inf (such a node would get no links
 *     and could become the entry point). flat stores anything; a NaN row
 *     can never be returned. Deviation: faiss consumes the id of a bad row
 *     and stores nothing; here the id is not consumed.
 */
#ifndef DFANN_H
#define DFANN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dfann_index dfann_index; /* opaque */
typedef void *dfann_stream;             /* hipStream_t */

/* --- lifecycle -------------------------------------------------------- */

/* Build an index from a JSON spec {"type": "flat"|"ivf_flat"|"ivfpq"|
 * "ivfsq", "dim": int, "metric": 0|1, "nlist": int, "m": int,
 * "nbits": 4|8, "sq_type": "fp16"|"8bit"|"6bit"|"4bit", "nprobe": int,
 * "seed": int}.
 * "slab_mb" (ivf types; default 64, clamped to 1..4096): size of the slabs
 * the inverted-list codes and the pending appends live in; the list merge
 * and dfann_remove_ids work through them one slab at a time.
 * "ivfpq" codes: "nbits" (default 8) bits per sub-quantizer, 1 << nbits
 * codewords each; any other value is an error. At 8 a row is m bytes; at
 * 4 it is (m + 1) / 2 bytes, byte b = code[2b] |
 * code[2b+1] << 4 (faiss ProductQuantizer bit order; odd m leaves the last
 * high nibble 0). Rows are padded to a multiple of 16 bytes
 * (dfann_code_stride). Codebooks are (m, 1 << nbits, dim / m) fp32. At 4
 * bits only the fp32 LUT built in the scan kernel exists: "pq_lut_f16",
 * "pq_lut_global": 1 and "pq_precomputed" are errors naming the knob
 * ("pq_lut_global": -1|0 and "pq_lut_mb" are accepted, without effect).
 * "ivfsq" codes: "sq_type" (default "fp16"; a value not listed above is
 * read as "fp16"). "fp16": 2 * dim bytes per row. "8bit" / "6bit" / "4bit"
 * (faiss QT_8bit / QT_6bit / QT_4bit): B = 8 | 6 | 4 bits per
 * dimension, code = clamp((int)(Q * (r - vmin) / vdiff), 0, Q) with Q =
 * (1 << B) - 1 over per-dimension ranges of the training residuals
 * (dfann_get_sq_params / dfann_set_trained carry vmin and vdiff at all
 * three widths), decoded as vmin + (code + 0.5) * (vdiff / Q). A row is a
 * little-endian bit stream of ceil(dim * B / 8) bytes, dimension t at bit
 * B * t (faiss Codec8bit / Codec6bit / Codec4bit): at 4 bits byte t / 2
 * holds dimension t in bits 4 * (t & 1); at 6 bits dimensions 4g .. 4g+3
 * fill bytes 3g .. 3g+2, code i at bit 6i of that 24-bit little-endian
 * word. Rows are padded to a multiple of 16 bytes (dfann_code_stride);
 * every bit past dim * B, pad bytes included, is zero. "hnswsq" is always
 * 8-bit.
 * Refine stage, "ivfpq" / "ivfsq" only (faiss IndexRefineFlat /
 * IndexRefine(SQfp16)): "refine": "fp32"|"fp16" (absent or
 * "" = off) keeps every added vector raw (round16(dim * 4 or 2) bytes per
 * row) and re-ranks the base stage's k' candidates exactly; "k_factor":
 * float >= 1 (default 1.0, see Limits for k'); "refine_slab_mb": slab size
 * of the raw store (default 64). "refine" on flat / ivf_flat / hnswsq and
 * k_factor < 1 are errors.
 * OPQ, "ivfpq" only (see the header comment): "opq": 1 turns the
 * pre-transform on; "opq_dim": d_out (default dim; m must divide it and it
 * must be <= dim); "opq_niter": outer training iterations (default 16).
 * Errors naming the key: "opq" on another index type, opq_dim > dim,
 * opq_dim % m != 0, and "opq" with "pq_precomputed" (the term2 table is
 * not wired behind the transform).
 * Replaces: faiss.IndexFlatIP/IndexFlatL2 (ref index.py:28-30,94),
 * faiss.IndexIVFFlat (ref index.py:38), faiss.IndexIVFPQ (ref
 * index.py:46), faiss.IndexIVFScalarQuantizer + QT_fp16/QT_8bit (ref
 * index.py:55,64-66; QT_6bit / QT_4bit through the factory string),
 * faiss.index_factory (ref index.py:396). */
int dfann_create(const char *spec_json, dfann_index **out);
int dfann_destroy(dfann_index *h);

/* --- build path ------------------------------------------------------- */

/* Replaces faiss `Index.train` at ref index.py:217 (k-means coarse
 * quantizer; + per-subspace PQ codebooks / SQ ranges on residuals). On an
 * "opq" index it first learns the transform on the raw rows (faiss
 * OPQMatrix::train; skipped when one was injected), then trains the inner
 * index on the transformed set (faiss IndexPreTransform::train).
 * Deterministic: same rows and seed give a bitwise-identical transform.
 * Non-finite rows are refused (Hostile input, A1). */
int dfann_train(dfann_index *h, int64_t n, const float *x_dev,
                dfann_stream stream);

/* Replaces faiss `Index.add` at ref index.py:425 (coarse assign + encode
 * + inverted-list append; ids = arrival order). A chunk with an
 * unassignable row is refused whole (Hostile input, A2). */
int dfann_add(dfann_index *h, int64_t n, const float *x_dev,
              dfann_stream stream);

/* --- search path ------------------------------------------------------ */

/* Replaces faiss `Index.search` at ref index.py:257. D_dev: (nq,k) f32,
 * I_dev: (nq,k) i64. k <= 512 (see Limits above). NaN / Inf query rows:
 * Hostile input, S2 - S4. */
int dfann_search(dfann_index *h, int64_t nq, const float *q_dev, int k,
                 float *D_dev, int64_t *I_dev, dfann_stream stream);

/* Replaces faiss `Index.search_and_reconstruct` at ref index.py:255.
 * R_dev: (nq,k,d) f32 (decoded vectors; zeros at padded slots). On a
 * refine index the rows come from the raw store instead of the code
 * decode: fp32 rows exactly, fp16 rows widened. */
/* On an "opq" index the rows are dim wide: decoded at opq_dim, then
 * multiplied by A^T (faiss VectorTransform::reverse_transform of an
 * orthonormal matrix); with refine they still come from the raw store. */
int dfann_search_reconstruct(dfann_index *h, int64_t nq, const float *q_dev,
                             int k, float *D_dev, int64_t *I_dev,
                             float *R_dev, dfann_stream stream);

/* Coarse quantization only: top-nprobe list ids (i32, (nq,nprobe)) and
 * their minimize-keys (f32; L2: |c|^2-2q.c, IP: -q.c). Mirrors the
 * quantizer search half of faiss IndexIVF::search. A slot that cannot be
 * filled is probe -1 with key +FLT_MAX (Hostile input, S1). */
int dfann_coarse(dfann_index *h, int64_t nq, const float *q_dev, int nprobe,
                 int32_t *probes_dev, float *keys_dev, dfann_stream stream);

/* Search with externally supplied probe lists (+keys for the IP bias).
 * Mirrors faiss IndexIVF::search_preassigned; also the parity-test hook
 * for probe-set-independent bit-exactness.
 * k in 1..512, 1 <= nprobe <= 512, nq == 0 returns at once (S5);
 * probes_dev and keys_dev must not be NULL (as in the range entry). A probe
 * outside [0, nlist) is an empty slot and its key is not read (S1). */
int dfann_search_preassigned(dfann_index *h, int64_t nq, const float *q_dev,
                             int nprobe, const int32_t *probes_dev,
                             const float *keys_dev, int k, float *D_dev,
                             int64_t *I_dev, dfann_stream stream);

/* Exact top-k over the rows whose arrival id is set in allow_bits_dev
 * (uint32 words, bit i&31 of word i>>5; nbits >= ntotal, extra bits
 * ignored). Same conventions, caps and pads as dfann_search. Mirrors faiss
 * SearchParameters.sel = IDSelectorBitmap; replaces the over-fetch +
 * host post-filter of ref client.py:213-263. The bitmap is read during
 * the call only (stream-ordered; nothing is cached across calls).
 * Errors: nbits < ntotal; hnswsq ("filtered search unsupported for
 * hnswsq" — beam search under a filter is a different algorithm). */
int dfann_search_filtered(dfann_index *h, int64_t nq, const float *q_dev, int k,
                          const uint32_t *allow_bits_dev, int64_t nbits,
                          float *D_dev, int64_t *I_dev, dfann_stream stream);
/* dfann_search_preassigned under the same filter (same S1 / S5 rules). */
int dfann_search_preassigned_filtered(dfann_index *h, int64_t nq,
        const float *q_dev, int nprobe, const int32_t *probes_dev,
        const float *keys_dev, int k, const uint32_t *allow_bits_dev,
        int64_t nbits, float *D_dev, int64_t *I_dev, dfann_stream stream);

/* Mirrors faiss Index::remove_ids(IDSelectorBitmap). Removes every stored row
 * whose arrival id is set in remove_bits_dev (dfann_search_filtered's bitmap
 * convention; nbits >= ntotal else an error; bits at or past ntotal and bits
 * of ids already removed are ignored). *nremoved_out = rows removed by THIS
 * call. Synchronizes the stream; not graph-capturable. Deviation: faiss
 * IndexFlat renumbers the survivors and faiss IVF re-issues ids after a
 * removal; here an id is never renumbered and never issued twice.
 * After the call no entry point returns a removed id (search, preassigned,
 * filtered, range, reconstruct, refine, dfann_get_lists); dfann_ntotal is
 * unchanged and the next add issues ids from it upward; dfann_nlive drops by
 * *nremoved_out. A call that removes nothing (no bit set, ids already
 * removed, an index without rows, an untrained ivf index) returns 0 and
 * leaves the index bitwise as it was.
 * ivf_flat / ivfpq / ivfsq: rows are removed PHYSICALLY. Rows
 * still pending from an add are merged first; then the inverted lists are
 * compacted (one fresh slab, then the old slabs reused behind the read
 * window), stably — inside a list the survivors keep
 * ascending arrival id — so the offsets, ids and code bytes are the
 * pre-removal dump with the removed rows deleted, and every later search
 * reads fewer bytes. Peak memory: the codes plus one slab ("slab_mb").
 * Refine store: indexed by arrival id, it never moves; removed rows stay as
 * unreferenced holes, their memory is not reclaimed, and dfann_refine_info
 * still reports ntotal rows.
 * flat: ids are positions in the raw arena, so removal leaves tombstones: a
 * device live-bitmap over ids, allocated by the first removal, under which
 * every later search runs the filtered top-k kernels (dfann_search_filtered
 * ANDs it with the caller's bitmap). Arena memory is not reclaimed.
 * Errors: hnswsq ("remove_ids unsupported for hnswsq": unlinking a graph
 * node is a different algorithm), nbits < ntotal, a NULL bitmap. */
int dfann_remove_ids(dfann_index *h, const uint32_t *remove_bits_dev,
                     int64_t nbits, int64_t *nremoved_out, dfann_stream stream);

/* Range search. Mirrors faiss Index::range_search over an
 * IVF index: every row of the min(nprobe, nlist, 512) probed lists whose
 * distance passes the STRICT radius test — L2: dist < radius (squared L2,
 * the value dfann_search returns); IP: dot > radius (the un-negated dot
 * product dfann_search returns). Distances are bitwise dfann_search's.
 * allow_dev: optional allow-bitmap (dfann_search_filtered conventions,
 * nbits >= ntotal); NULL = unfiltered, nbits ignored.
 * lims_dev: (nq+1) i64 device, lims[0] = 0; query i owns D/I[lims[i] ..
 * lims[i+1]). *total_out = lims[nq]. *D_dev_out / *I_dev_out: engine-owned
 * device arrays of total f32 / i64 arrival ids, valid until the next range
 * call on the handle or its destruction (NULL while nothing was ever
 * returned). Order inside a query: probe slot ascending, then ascending
 * CSR position (= ascending arrival id) inside the list; not by distance.
 * Byte-identical run to run.
 * The call synchronizes the stream (once to read the total, once after the
 * fill pass to read its error word): it cannot be captured into a graph.
 * Workspace: nq * nprobe * 8 wave counts (4 B) and offsets (8 B).
 * Spec key "range_max_results" (default 1 << 27 hits, 1.6 GB of D + I): a
 * larger total is an error naming the key, the total and the limit, raised
 * before the result arrays grow. radius NaN: empty result.
 * Errors: flat, hnswsq, an index with refine (faiss IndexRefine has no
 * range search either), an untrained index, nbits < ntotal. */
int dfann_range_search(dfann_index *h, int64_t nq, const float *q_dev,
                       float radius, const uint32_t *allow_dev, int64_t nbits,
                       int64_t *lims_dev, int64_t *total_out,
                       const float **D_dev_out, const int64_t **I_dev_out,
                       dfann_stream stream);
/* The same over caller-supplied probe lists (dfann_coarse's probes and
 * keys). Mirrors faiss IndexIVF::range_search_preassigned. A list named
 * twice contributes its hits twice. 1 <= nprobe <= 512. A probe outside
 * [0, nlist) contributes nothing in either pass (Hostile input, S1). */
int dfann_range_search_preassigned(dfann_index *h, int64_t nq,
        const float *q_dev, int nprobe, const int32_t *probes_dev,
        const float *keys_dev, float radius, const uint32_t *allow_dev,
        int64_t nbits, int64_t *lims_dev, int64_t *total_out,
        const float **D_dev_out, const int64_t **I_dev_out,
        dfann_stream stream);

/* --- knobs / introspection -------------------------------------------- */

/* ref index.py:352-356. Effective nprobe is min(nprobe, nlist, 512) at
 * search time (see Limits above); values above 512 warn once. */
int dfann_set_nprobe(dfann_index *h, int nprobe);
/* Mirrors faiss IndexRefine::k_factor (the field index_factory's
 * "...,RFlat" users set through ParameterSpace "k_factor_rf"): changes k'
 * of every later search, no rebuild. Errors: index without a refine
 * stage; k_factor < 1. Not persisted by dfann_save (the spec's value is). */
int dfann_set_k_factor(dfann_index *h, float k_factor);
/* Mirrors faiss IndexRefine::refine_index (its codec, code_size and
 * ntotal): out = {kind 0 none / 1 fp32 / 2 fp16, row stride in bytes,
 * rows stored}. */
int dfann_refine_info(dfann_index *h, int64_t out[3]);
/* Mirrors faiss IndexRefine::refine_index->reconstruct_n(row0, n) without
 * the decode: rows [row0, row0+n) of the raw store to host, stride-padded
 * (pad bytes are zero). Test plumbing. */
int dfann_get_refine_rows(dfann_index *h, int64_t row0, int64_t n,
                          void *out_host);
/* ids ever issued = the first id of the next add (faiss .ntotal until a row
 * is removed; removal never lowers it) */
int64_t dfann_ntotal(dfann_index *h);
/* rows stored: ntotal minus the rows dfann_remove_ids took out */
int64_t dfann_nlive(dfann_index *h);
int dfann_nlist(dfann_index *h);                  /* faiss .nlist */
int dfann_is_trained(dfann_index *h);
int dfann_dim(dfann_index *h); /* the caller-facing dim (d_in under opq) */
/* spec json the index was created with (valid until destroy) */
const char *dfann_spec_json(dfann_index *h);

/* Coarse centroids to host, (nlist,d) f32 ((nlist, opq_dim) on an "opq"
 * index: what faiss extract_index_ivf(index)->quantizer holds). Replaces
 * quantizer.reconstruct_n(0, nlist) at ref index.py:350. Errors on flat
 * (no quantizer — the reference would AttributeError). */
int dfann_get_centroids(dfann_index *h, float *out_host);

/* --- persistence (replaces faiss read_index/write_index at ref
 *     index.py:297,460; our own file format).
 *     An index nothing was ever removed from writes magic "DFANN01", byte
 *     for byte as before; after a removal the magic is "DFANN02": nlive
 *     follows ntotal, the list sections hold nlive rows, flat appends its
 *     live bitmap, the refine store keeps ntotal rows. Both load. --------- */
int dfann_save(dfann_index *h, const char *path);
int dfann_load(const char *path, dfann_index **out);

/* --- trained-artifact exchange (parity-test plumbing: train once, load
 *     the same artifacts into oracle and engine — SURVEY.md §8c) ------- */
/* On an "opq" index the artifacts are at opq_dim and the call errors until
 * a transform is set (dfann_set_transform). */
int dfann_set_trained(dfann_index *h, const float *centroids_host,
                      const float *codebooks_host, const float *vmin_host,
                      const float *vdiff_host);
/* OPQ transform exchange. A_host: (opq_dim, dim) fp32 row-major.
 * dfann_get_transform replaces reading faiss LinearTransform::A of
 * IndexPreTransform::chain[0]; dfann_set_transform replaces assigning it
 * (with is_trained = true) — it is refused once vectors were added. Both
 * error on an index without "opq"; get also before a transform exists. */
int dfann_get_transform(dfann_index *h, float *A_host);
int dfann_set_transform(dfann_index *h, const float *A_host);
/* Mirrors faiss VectorTransform::apply: y_dev (n, opq_dim) = x_dev (n, dim)
 * through the transform — the same kernel dfann_add and every search entry
 * run, so a row's result is bitwise what the index saw. */
int dfann_apply_transform(dfann_index *h, int64_t n, const float *x_dev,
                          float *y_dev, dfann_stream stream);
/* Mirrors faiss IndexPreTransform::chain / VectorTransform::{d_in, d_out}:
 * out = {opq on 0|1, d_in, d_out}; d_in == d_out == dim without "opq". */
int dfann_transform_info(dfann_index *h, int64_t out[3]);
/* codebooks: (m, 1 << nbits, dsub) fp32 — (m,256,dsub) at nbits=8,
 * (m,16,dsub) at nbits=4 — for dfann_set_trained and dfann_get_codebooks */
int dfann_get_codebooks(dfann_index *h, float *out_host);
/* Dump the finalized inverted lists to host: off (nlist+1 i64), ids
 * (nlive i64, arrival ids in CSR order), codes (nlive * stride u8) —
 * nlive = dfann_nlive, which equals ntotal until a row is removed.
 * stride = code_bytes rounded up to 16 (ivfpq nbits=4 and ivfsq "6bit" /
 * "4bit": packed rows, see dfann_create). Used by the CPU-baseline leg of
 * bench.py to scan the SAME index content the GPU holds. */
int dfann_get_lists(dfann_index *h, int64_t *off_host, int64_t *ids_host,
                    uint8_t *codes_host);
int dfann_code_stride(dfann_index *h);
int dfann_get_sq_params(dfann_index *h, float *vmin_host,
                        float *vdiff_host); /* (d,), (d,); ivfsq "8bit" /
                                               "6bit" / "4bit" and hnswsq */

/* --- shard-merge (replaces ResultHeap + _aggregate_results' arithmetic,
 *     ref client.py:29-54,265-310; fed by the RCCL all-gather of
 *     per-shard top-k in the multi-GPU path) -------------------------- */
/* D_dev: (S,nq,k) f32 shard distances (faiss sign conventions);
 * I_dev: (S,nq,k) i64 shard ids (-1 pads). maximize: 1 for dot.
 * Output ids are GLOBAL slots s*nq*k + q*k + j into the gathered input
 * (the caller maps slots to (shard, local id) / metadata, mirroring ref
 * client.py:290,297-298). Dout is negated for maximize (ref quirk 2).
 * k <= 512 (see Limits above). */
int dfann_merge_topk(int64_t nq, int S, int k, const float *D_dev,
                     const int64_t *I_dev, int maximize, float *Dout_dev,
                     int64_t *Iout_dev, dfann_stream stream);

/* --- hnswsq (replaces faiss.IndexHNSWSQ at ref index.py:51-60) --------
 * spec: {"type": "hnswsq", "dim", "metric": 1 (L2 only — the reference
 * asserts), "m": store_n (link cap M; level-0 cap 2M), "ef_construction",
 * "nprobe" (= efSearch; honored dynamically — deviation: the
 * reference's set_nprobe is a silent no-op on HNSW), "seed"}.
 * Build is a BATCHED wave insertion over frozen snapshots with reverse
 * links applied in sorted order — deterministic given (data, seed, wave
 * schedule), but a DIFFERENT graph than faiss's sequential insertion
 * (quality gated by recall tests). Search parity is
 * pinned by the oracle restatement over the dumped graph. ------------- */

/* info: out = {M, deg0, nslots, entry, maxlevel, ef_construction} */
int dfann_hnsw_info(dfann_index *h, int64_t out[6]);
/* dump the graph to host: levels (n i32), cnt0 (n), nbr0 (n x 2M),
 * upslot (n), cntU (nslots x 8), nbrU (nslots x 8 x M) */
int dfann_hnsw_dump(dfann_index *h, int32_t *levels_host, int32_t *cnt0_host,
                    int32_t *nbr0_host, int32_t *upslot_host,
                    int32_t *cntU_host, int32_t *nbrU_host);

/* --- kernel timing for the roofline harness (bench.py) ---------------- */

typedef struct dfann_timing {
  double scan_ms;      /* ivf list-scan kernel ALONE, summed over launches */
  int64_t scan_launches;
  int64_t scan_rows;   /* codes scanned (algorithmic units) */
  int64_t scan_bytes;  /* scan_rows * packed code stride */
  double gemm_ms;      /* coarse/flat distance GEMM */
  int64_t gemm_flops;  /* 2*M*N*K summed */
  double merge_ms;
  int64_t merge_launches;
  double lut_ms;       /* ADC-table build (k_pq_lut / term3), GLUT/PRE paths */
  int64_t lut_launches;
} dfann_timing;

int dfann_set_timing(dfann_index *h, int enabled);
/* Synchronizes the recorded events, fills out, and resets accumulators. */
int dfann_get_timing(dfann_index *h, dfann_timing *out);

const char *dfann_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DFANN_H */
