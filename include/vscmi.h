/*
 * vscmi.h -- C ABI of libvscmi.so: the MI355X (gfx950) descriptor-search / candidate /
 * temporal-localisation engine that sits under the vsc.index / vsc.candidates / vcsl.vta call
 * surface of facebookresearch/vsc2022.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Every array is owned by the caller; the library frees
 *     nothing it did not allocate and hands back no memory except opaque handles that have an
 *     explicit *_destroy.
 *   - Each array argument carries a memory kind: VSC_MEM_HOST (pageable host memory, e.g. a
 *     numpy array) or VSC_MEM_DEVICE (HBM of the handle's device, e.g. a torch tensor's
 *     data_ptr).  Scalars written through pointers (counts, radii) are always host memory.
 *   - All feature matrices are fp32, C-contiguous, row-major [n][dim]; frame-row and video
 *     ordinals are int32 (row counts < 2^31).
 *   - Return value: VSC_OK (0) or a negative VSC_ERR_* code; vsc_last_error() returns a
 *     thread-local message.  The Python layer raises RuntimeError / ValueError from these,
 *     matching the reference's exception/assert convention (vsc/index.py:37-40,
 *     vsc/storage.py:49-57, vsc/baseline/localization.py:59,64).
 *   - A handle owns one HIP stream; calls on one handle are serialised by the caller, distinct
 *     handles may be used from distinct threads.  No callbacks into the caller.
 *   - Arithmetic contract: every similarity is the fp32 fma chain in ascending k
 *     (acc = fmaf(q[k], r[k], acc), acc0 = +0), produced on the matrix cores by
 *     v_mfma_f32_32x32x2_f32.  Results are bit-identical to oracle/vsc_oracle.c.
 *
 * Paths below are relative to the reference checkout (/root/reference).
 */
#ifndef VSCMI_H
#define VSCMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSC_OK 0
#define VSC_ERR_INVALID (-1)  /* bad argument */
#define VSC_ERR_HIP (-2)      /* HIP runtime failure */
#define VSC_ERR_NOMEM (-3)    /* device allocation failed */
#define VSC_ERR_CAPACITY (-4) /* caller-provided output capacity too small; *n_out holds the need */
#define VSC_ERR_OVERFLOW (-5) /* internal hit buffer overflowed (pathological score distribution) */
#define VSC_ERR_NODEVICE (-6) /* no gfx950 device */

#define VSC_MEM_HOST 0
#define VSC_MEM_DEVICE 1

/* same numeric values as faiss.METRIC_INNER_PRODUCT / faiss.METRIC_L2 (vsc/index.py:78,145) */
#define VSC_METRIC_INNER_PRODUCT 0
#define VSC_METRIC_L2 1

/* how an index stores its reference rows (vsc/index.py:75-82: the codec_str handed to faiss.index_factory) */
#define VSC_CODEC_FLAT 0   /* "Flat": fp32 rows */
#define VSC_CODEC_SQFP16 1 /* "SQfp16" (faiss IndexScalarQuantizer, QT_fp16): IEEE half floats, scored in fp32 */

#define VSC_TN_MAX_BOXES 16

typedef struct vsc_index vsc_index_t;

const char* vsc_last_error(void);
int vsc_version(void);
/* number of visible HIP devices whose arch is gfx950 (0 => the library cannot run) */
int vsc_device_count(void);

/* ---------------------------------------------------------------- flat index
 * Replaces faiss.index_factory(dim, "Flat", metric) + index.add(x) (vsc/index.py:82,94).
 * The reference set stays resident in HBM across searches; add is incremental.
 *
 * Every score the library returns is the fp32 chain acc = fmaf(q[k], r[k], acc), k ascending.  For
 * inner-product indexes the thresholded searches and the k-NN first evaluate the score matrix at reduced precision
 * on the matrix cores -- int8 (v_mfma_i32_16x16x64_i8, dims <= 1024) where hits are sparse, fp16 otherwise -- and
 * hand to that exact stage every pair whose low-precision score plus a rigorous error bound reaches the threshold;
 * the outputs are bit-identical to the all-fp32 route.
 *
 * Options.  Every switch below is an option of the handle: `vsc_index_set_option(idx, "<name>", value)` with the name in
 * lower case and without the VSC_ prefix ("i8_density", "prefilter", "knn_step", ...; "f16_kernel": 1 = ring), and the
 * environment variable of the same name supplies its initial value when a handle is created (read once, then it stays
 * with that handle):
 *   VSC_PREFILTER=0           no pre-filter (every search on the exact fp32 MFMA kernel); =2 forces it onto every
 *                             batch / every k-NN regardless of size (tests)
 *   VSC_PREFILTER_DENSITY=f   expected hit density below which a batch of the thresholded search is pre-filtered
 *                             (default 0.05)
 *   VSC_F16_KERNEL=ring       the 256x256 LDS-ring fp16 pre-filter instead of the panel-stationary one (A/B)
 *   VSC_I8=0                  no int8 image (fp16 pre-filter only); =2 forces the int8 kernel onto every
 *                             pre-filtered batch (tests)
 *   VSC_I8_DENSITY=f          expected hit density below which a pre-filtered batch runs on int8 (default 5e-4)
 *   VSC_I8_MAX_REL=f          sqrt(dim) x mean(E_r / N'_r) of the references above which the index never starts
 *                             on int8 (default 0.35: the 8-bit bound would pass too much of the matrix)
 *   VSC_I8_EXCLUDE=0          keep coordinates on which all references agree inside the int8 images
 *   VSC_I8_CENTER=0|1|2       the int8 reference image holds y - mu, mu = the mean of the rows present at the first search over
 *                             >= 1024 rows (fixed from then on); the rows' x . mu moves their thresholds (exact: x.y = x.(y - mu) + x.mu).  1 (default):
 *                             when the mean carries >= 2 % of the rows' energy (uncentred embeddings; isotropic rows are left
 *                             alone), 0 never, 2 always (tests).  Read-only options "i8_center_on", "i8_center_share"
 *   VSC_I8_SORT=0             int8 launches see their rows in batch order (default: sorted by threshold / scale)
 *   VSC_I8_GROUP=n            radius searches with per-row thresholds (excluded coordinates): inside groups of 2^n
 *                             rows of the threshold order the rows are ordered by scale (default 9; 0: off)
 *   VSC_I8P_ORDER=0           panel-major work items with stealing (default 1: slice-major)
 *   VSC_I8P_SLICE=n           col-steps of 512 reference rows per work item (default 32 slice-major)
 *   VSC_I8P_PAIR=0 / 2        never / always (dims <= 512) use work items of two 128-row panels (256 x 32 wave tiles;
 *                             default 1: where a launch is large enough)
 *   VSC_I8_SCREEN=1           fp16 screen between the int8 pre-filter and the exact stage (measured neutral: off)
 *   VSC_DEFER=0|1|2           deferred rescoring in vsc_index_global_topk: pre-filtered batches leave the exact score of
 *                             a pair uncomputed when it is proven to exceed the radius and to lie at or below a floor
 *                             under which the next re-threshold event is expected to cut; the event then drops the
 *                             pair unscored (or, where the guess was too high, scores it first).  Results, order, radius
 *                             and events are those of 0 (off).  1 (default): the batches an event is expected to follow;
 *                             2: every pre-filtered batch (tests).  VSC_DEFER_I8=0: fp16 batches only (int8 batches defer
 *                             through the fp16 screen).  VSC_DEFER_MARGIN=<m> (0.05): the floor is the score of rank
 *                             (K + 1) rows seen / rows at the expected event x (1 + m) among the kept hits.  Off in seeded
 *                             searches, with VSC_SORT_HITS=0, a caller-sized hit buffer, VSC_RESCORE_SORT=0, the k-NN and
 *                             vsc_index_range_search.  Read-only options of the last search: "deferred" (pairs),
 *                             "defer_forced" (pairs scored after all), "defer_events_ok", "defer_events_forced",
 *                             "n_rethreshold"
 *   VSC_KNN_STEP=n            query rows per launch of a k-NN threshold pass (default: 32768, doubled until rows x range
 *                             reaches VSC_KNN_STEP_WORK (64) x 32768 x 196608 or VSC_KNN_STEP_MAX (262144) rows)
 *   VSC_I8_KNN=0              k-NN threshold passes on the fp16 kernel
 *   VSC_RESCORE_SORT=0        exact stage over the waves' candidate segments as they are (default: compacted and
 *                             sorted by reference row)
 *   VSC_KNN_LEVELS=1          pre-filtered k-NN with one refinement level; VSC_KNN_SUBSET=<factor> (default 300),
 *   VSC_KNN_S0DIV=<n> (28), VSC_KNN_S0MIN=<rows> (1024), VSC_KNN_RATIO=<r> (by k), VSC_KNN_NCHUNK=<n>: sizes of its exact subset pass / levels
 *   VSC_KNN_FIRST_TILE=0      exact k-NN kernel, k > 1: insert every score of a run's first tile (default: only those that reach
 *                             a per-wave lower bound of the row's k-th largest score of that tile; A/B)
 *   VSC_DEBUG_I8 / VSC_DEBUG_SCREEN: notes on stderr when a search falls back from int8 / per screen launch
 *   VSC_TOPK_SHORTCUT=0|1|2   proven top-K route of vsc_index_global_topk (see there); VSC_TOPK_SAMPLE=<rows> (4096)
 *   density_hint=<d>          (option only) expected hit density of the batches of the next thresholded searches; > 0: the
 *                             exact / fp16 / int8 rule uses it instead of K / (rows x references) -- the sharded schedule calls the
 *                             seeded search once per batch with a generous budget K and knows the density the batch will have
 *   VSC_SORT_HITS=0           vsc_index_global_topk / _seeded (inner product) return their hits as a SET, in the kept
 *                             list's order, instead of (score desc, row asc, ref asc): the column-sharded schedule joins
 *                             a batch's hits to a list that is sorted once at the end.  min(n, K) entries come back; K
 *                             of them may be a truncated list
 * Process-wide (first use): VSC_SIM_GRID (persistent grid of the exact similarity kernel), VSC_POISON_ALLOC=1
 * (fresh device buffers filled with 0xFF). */
int vsc_index_create(int dim, int metric, int device, vsc_index_t** out);
/* The same with a codec, fixed for the life of the handle; vsc_index_create means VSC_CODEC_FLAT.
 *
 * VSC_CODEC_SQFP16.  By definition the index on rows X behaves as the Flat index on
 *     dec(X) = the rows rounded to IEEE half floats (round to nearest even, subnormals kept) and converted back:
 * every search returns the rows, references and score BITS of that Flat index -- same routes, same options, same
 * arithmetic contract (the fp32 chain over the query's fp32 values and the references' decoded values).  Rows that
 * are already half floats (descriptor files written with --store_fp16) decode to themselves: the codec loses nothing
 * on them.  The rows live once in HBM, as half floats in the layout the fp16 pre-filter reads; the packed fp32 image
 * of a Flat handle is never allocated (512-d inner product: 1556 instead of 3604 bytes per row with both pre-filter
 * images).  The store is kept whatever "prefilter" and the metric say; the int8 image, the excluded coordinates and
 * the centre are derived from the decoded values.  The exact stage of the pre-filtered routes gathers its reference
 * rows from the store; the exact kernels that stream whole rows (pre-filter off, exact k-NN subsets) run over
 * bounded ranges of rows decoded into a scratch buffer.
 * A row holding NaN, +-inf or a value beyond +-65504 makes vsc_index_add / _add_f16 fail with VSC_ERR_INVALID and
 * leaves the index as it was.
 * Read-only options of both codecs: "codec", and "ref_bytes" = bytes currently allocated for reference images of all
 * kinds (store, pre-filter images, per-row tables). */
int vsc_index_create_codec(int dim, int metric, int device, int codec, vsc_index_t** out);
int vsc_index_destroy(vsc_index_t* idx);
/* Programmatic form of the switches above (the reference's analogue: faiss.ParameterSpace().set_index_parameter(index,
 * name, value) on the object vsc/index.py:82 creates).  Options that decide which images of the reference rows are kept
 * ("prefilter" 0 <-> non-0, "i8" 0 <-> non-0, "f16_kernel", "i8_exclude", "i8_center") can only change while the index is empty:
 * VSC_ERR_INVALID otherwise, as for an unknown name or an out-of-range value.  "cand_budget": entries of the candidate
 * list a k-NN threshold pass may ask for (default 2^28; the rows per launch are halved until it fits). */
int vsc_index_set_option(vsc_index_t* idx, const char* name, double value);
int vsc_index_get_option(const vsc_index_t* idx, const char* name, double* value);
/* Run every launch and copy of this handle on the caller's HIP stream (a hipStream_t, e.g. torch's current stream) instead
 * of the handle's own non-blocking stream: work the caller queued on that stream before a call -- the kernel that
 * produced the query rows -- is then ordered before the library's reads without a device-wide synchronisation.
 * hip_stream = NULL is HIP's default stream (torch's default); own != 0 goes back to the handle's own stream (hip_stream
 * is ignored then).  Calls still return only when their results are complete.
 * Lifetime: a bound stream must stay alive while a call of this handle runs on it; between calls nothing of the handle
 * is pending on it.  When the handle leaves a caller's stream (another vsc_index_set_stream, vsc_index_destroy) the
 * library does NOT touch that stream again -- it may already be destroyed -- and drains the device instead. */
int vsc_index_set_stream(vsc_index_t* idx, void* hip_stream, int own);
int vsc_index_add(vsc_index_t* idx, const float* x, int64_t n, int x_mem);
/* Rows that are already IEEE half floats ([n][dim] uint16 bit patterns, host or device).  SQfp16 handle: they reach
 * the store without an fp32 copy on the host and without a staging buffer of fp32 size.  Flat handle: the result of
 * vsc_index_add of the upcast array. */
int vsc_index_add_f16(vsc_index_t* idx, const uint16_t* x, int64_t n, int x_mem);
/* fp32 [n][dim] of rows [i0, i0 + n) as the searches see them: the rows as added (Flat), dec of them (SQfp16).
 * (faiss index.reconstruct_n) */
int vsc_index_reconstruct(vsc_index_t* idx, int64_t i0, int64_t n, float* out, int out_mem);
int64_t vsc_index_ntotal(const vsc_index_t* idx);
int vsc_index_dim(const vsc_index_t* idx);
int vsc_index_metric(const vsc_index_t* idx);
/* Capacity (entries) of the internal kept-hit buffer used by vsc_index_global_topk; 0 restores the
 * default max(32*ntotal, 2K) + 2K.  A search that overflows it returns VSC_ERR_OVERFLOW.  With the default, a search
 * that overflows is rerun with four times the entries and the handle starts its later searches there: read-only option
 * "hit_cap_learned" (entries; 0 while no search of the handle was rerun). */
int vsc_index_set_hit_capacity(vsc_index_t* idx, int64_t cap);
/* block until all work queued on the handle's stream has finished */
int vsc_index_sync(vsc_index_t* idx);

/* Replaces faiss index.search(x, k) (vsc/index.py:174; vsc/baseline/score_normalization.py:96).
 * Per query row the k best refs ordered by (score desc, ref asc) [L2: (dist asc, ref asc)].
 * out_s[nq*k] fp32, out_j[nq*k] int64 (faiss idx_t); missing slots hold -1 and -/+FLT_MAX.
 * k <= 4096; k <= 64 runs on the MFMA kernels (fp16 pre-filter + exact stage for large problems), larger k on an
 * explicit score matrix (same fp32 chains, same order; O(k * nr) per row). */
int vsc_index_knn(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int k, float* out_s,
                  int64_t* out_j, int out_mem);

/* Replaces faiss index.range_search(x, radius) (reached through
 * faiss.contrib.exhaustive_search.range_search_max_results at vsc/index.py:147-154): all (row, ref)
 * with score > radius (IP) or dist < radius (L2), STRICT.  Rows ascending, refs ascending within a
 * row.  lims[nq+1] cumulative counts; D/I written when cap >= *n_out, else VSC_ERR_CAPACITY (*n_out
 * = required).  All outputs host memory. */
int vsc_index_range_search(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, float radius,
                           int64_t* lims, float* D, int64_t* I, int64_t cap, int64_t* n_out);

/* Replaces VideoIndex._global_threshold_knn_search (vsc/index.py:142-165): the adaptive
 * global-threshold search of range_search_max_results(exponential_query_iterator(Q), radius=-/+1e10,
 * max_results=2K, min_results=K) followed by the stable sort + truncate to K.  Reproduces the
 * reference's batch schedule (32, 64, ... rows) and strict re-thresholding, ties included.
 * Output: <= K hits ordered by (score desc, row asc, ref asc) [L2: dist asc].
 * out_* capacity `cap` (>= K suffices).  *final_radius receives the last radius.
 *
 * Optional proven route (option "topk_shortcut" / VSC_TOPK_SHORTCUT: 0 = never [default], 1 = inner-product query sets of
 * >= 65536 rows and >= 4e10 pairs, 2 = wherever it is defined [tests]).  What the reference returns is the first K of
 * {s > tau_final} in sorted order, and tau_final -- the (K+1)-th best score of the row PREFIX its last re-threshold event
 * saw -- cannot exceed s_(K+1), the (K+1)-th best score of the whole matrix; so whenever s_K > s_(K+1) the reference's
 * result IS the exact top-K, whatever its batch schedule did on the way.  The route computes that top-K without the
 * doubling batches (the schedule over a strided sample of <= "topk_sample" = 4096 rows seeds a radius just below the cut;
 * all rows then run as steady 32768-row batches from it with the budget K + 1), checks s_K > s_(K+1) on the result and
 * returns it only then; with a tie on the cut, a seed that turned out too high or an overflow it replays the schedule as
 * above.  Results are bit-identical either way (tests/test_gpu_topk_proven.py).  Off by default because the proof cannot
 * succeed at BASELINE's sizes: with 2e12 scores and K = 48 M about 70 pairs share every fp32 value at the cut (4.6e9 pairs
 * per unit of score x 1.5e-8 per ulp), a tie on the cut is certain and the schedule's own final radius decides (DESIGN.md
 * section 8).  On the proven route *final_radius is the steady run's last radius (every returned hit lies above it).
 * get_option("last_topk_route"): 0 schedule, 1 proven, 2 tried + replayed. */
int vsc_index_global_topk(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K,
                          int32_t* out_i, int32_t* out_j, float* out_s, int64_t cap, int out_mem,
                          int64_t* n_out, float* final_radius);

/* The same search for a caller that already knows a radius below the K-th best score (the query-sharded pipeline,
 * vsc2022_amd/dist.py: every rank seeds its local search with a radius agreed over a row sample -- what FAISS gives
 * the reference when an index is spread over GPUs, vsc/index.py:153): the rows run as steady 32768-row batches from
 * `radius0` (a score for inner product, a distance for L2) instead of replaying the doubling schedule from -/+1e10.
 * Returns every hit STRICTLY beyond max(radius0, the re-threshold radii) -- the re-threshold rule of
 * range_search_max_results stays active (more than 2K kept: radius <- (K+1)-th best), so a seed that is too low costs
 * time, not memory -- ordered and truncated like vsc_index_global_topk; *final_radius = the last radius: the list is
 * complete beyond it.  Fewer than K hits come back when the seed was too high: the caller falls back to the unseeded
 * search.  radius0 must be finite. */
int vsc_index_global_topk_seeded(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K, float radius0,
                                 int32_t* out_i, int32_t* out_j, float* out_s, int64_t cap, int out_mem,
                                 int64_t* n_out, float* final_radius);

/* Fused candidate generation: vsc_index_global_topk followed by vsc_pair_max without the hit list
 * leaving HBM -- the whole of CandidateGeneration.query with MaxScoreAggregation
 * (vsc/candidates.py:36-40 over vsc/index.py:96-165).  row2q[nq] / row2r[ntotal] (host) map frame
 * rows to video ordinals.  Outputs (host, capacity cap; cap >= min(K, nq*ntotal) suffices): pairs in
 * score-descending stable order.  *n_hits receives the number of frame hits found (<= K). */
int vsc_index_candidates(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K,
                         const int32_t* row2q, const int32_t* row2r, int32_t* out_q, int32_t* out_r,
                         float* out_s, int64_t cap, int64_t* n_pairs, int64_t* n_hits);

/* ------------------------------------------------------- candidate generation
 * Replaces the regroup loop of VideoIndex.search (vsc/index.py:121-140) fused with
 * MaxScoreAggregation + the stable descending sort of CandidateGeneration.query
 * (vsc/candidates.py:24-40).  hits must be in search order (as produced by
 * vsc_index_global_topk).  row2q[nq_rows] / row2r[nr_rows] map frame rows to video ordinals.
 * Output pairs in first-appearance order (== score-descending, stable): video ordinals, max score
 * and the index of the pair's first hit.  cap >= n suffices.  device selects the GPU. */
int vsc_pair_max(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n,
                 int hits_mem, const int32_t* row2q, int64_t nq_rows, const int32_t* row2r,
                 int64_t nr_rows, int maps_mem, int32_t* out_q, int32_t* out_r, float* out_s,
                 int64_t* out_first, int64_t cap, int out_mem, int64_t* n_pairs, int device);

/* The same regroup with a choice of aggregation, for hit lists in either order -- the ScoreAggregation extension point of
 * vsc/candidates.py:14-26 for the four aggregations that run on the device.  One definition for all of them, chosen so
 * that a host function and a kernel compute the same bits: for one (query video, ref video) pair with hit scores
 * s_1..s_c (fp32, FINITE: a precondition, not checked) let d be those scores as float64, sorted descending; then
 *   VSC_AGG_MAX      the largest score (fp32; a run holding both zeros yields +0.0);
 *   VSC_AGG_SUM      acc = 0.0; for v in d: acc = acc + v -- one IEEE float64 add per hit, in that order -- as float32(acc);
 *   VSC_AGG_MEAN     the same acc, float32(acc / float64(c));
 *   VSC_AGG_TOPMEAN  the same loop over the first min(top_m, c) entries of d, divided by float64(min(top_m, c)).
 * (numpy: np.cumsum(np.sort(x.astype(np.float64))[::-1])[k - 1].)  Equal scores are identical numbers and acc starts at
 * +0.0, so neither the order of ties nor the sign of a zero can change a result.
 * hits_order: 1 = the list is in search order (score descending, as vsc_index_global_topk returns it), 0 = any order,
 * e.g. the (row, rank) order of a k-NN result: the descending order of every pair's scores is then established here.
 * Output pairs in their FINAL order: first-appearance order over the hit list (the reference's dict order), stably
 * sorted by the aggregated fp32 score descending with -0.0 == +0.0 (vsc/candidates.py:38-40).  out_q / out_r video
 * ordinals, out_s the aggregated score, out_first (optional) the index of the pair's first hit in the caller's list,
 * out_count (optional) its number of hits.  cap >= n suffices; VSC_ERR_CAPACITY with *n_pairs set otherwise.  n < 2^31.
 * VSC_ERR_INVALID before any launch (and before the device is looked at) for an unknown agg or top_m < 1 with
 * VSC_AGG_TOPMEAN.  A hit row outside [0, nq_rows) x [0, nr_rows): VSC_ERR_INVALID -- checked on the host for a list in
 * host memory, by a device-side error word otherwise (the kernel skips the hit: nothing is read outside the maps).
 * Handle-less family (vsc_set_aux_stream); host or device arrays with the conventions of vsc_pair_max. */
#define VSC_AGG_MAX 0
#define VSC_AGG_SUM 1
#define VSC_AGG_MEAN 2
#define VSC_AGG_TOPMEAN 3
int vsc_pair_aggregate(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n, int hits_mem,
                       const int32_t* row2q, int64_t nq_rows, const int32_t* row2r, int64_t nr_rows, int maps_mem,
                       int hits_order, int agg, int64_t top_m, int32_t* out_q, int32_t* out_r, float* out_s,
                       int64_t* out_first, int32_t* out_count, int64_t cap, int out_mem, int64_t* n_pairs, int device);

/* vsc_index_candidates with a choice of aggregation (agg, top_m: as above) and of retrieval: K >= 0 is the global-
 * threshold search of K hits (vsc/index.py:142-165, hits in search order), K < 0 the vanilla k-NN retrieval with k = -K
 * (vsc/index.py:108-117,167-177, hits in (row, rank) order).  The hits never leave HBM.  VSC_ERR_INVALID before any
 * launch for an unknown agg, top_m < 1 with VSC_AGG_TOPMEAN and k > ntotal (an empty k-NN slot has no video).  Outputs as
 * vsc_index_candidates, pairs in the final order of vsc_pair_aggregate; cap >= min(|K| hits, nq * ntotal) suffices. */
int vsc_index_candidates_agg(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K, const int32_t* row2q,
                             const int32_t* row2r, int agg, int64_t top_m, int32_t* out_q, int32_t* out_r, float* out_s,
                             int64_t cap, int64_t* n_pairs, int64_t* n_hits);

/* The final ordering of a hit list on its own: (score desc, query row asc, reference row asc), the order in which
 * VideoIndex._global_threshold_knn_search flattens and stably sorts its hits (vsc/index.py:158-165) -- for callers that
 * assemble a hit list themselves (the sharded schedule, vsc2022_amd/engine.py: the kept hits of the column slices arrive at
 * the rank that owns their query rows in no particular order).  Arrays of n entries, host or device; out_* may not alias the
 * inputs.  max_row / max_ref: exclusive upper bounds of the row / reference numbers (<= 0: unknown, all 31 bits are
 * sorted); they only save sort passes. */
int vsc_sort_hits(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n, int hits_mem,
                  int64_t max_row, int64_t max_ref, int32_t* out_i, int32_t* out_j, float* out_s, int out_mem,
                  int device);

/* Exact order statistics over UNSORTED score lists that are spread over ranks -- the re-threshold events of
 * range_search_max_results (vsc/index.py:147-154: "more than 2K kept -> radius = the (K+1)-th best") when the kept list
 * lives on several GPUs (vsc2022_amd/dist.py:kth_best_unsorted), without sorting anything: a 4 x 8-bit radix select whose
 * per-level histograms are summed by the CALLER (one all-reduce of 256 counters per level).
 *   state   int64[4] in device memory: {key prefix found so far, its mask, 1-based rank still wanted among the keys that
 *           match the prefix, scores strictly above the prefix so far}; start with {0, 0, k, 0}.
 *   vsc_score_histogram   hist[256] (device int64) <- per-digit counts, digit = bits [shift, shift+8) of the key, over the
 *           scores whose key matches state's prefix; shift = 24, 16, 8, 0 in that order.  key = order-preserving image of
 *           score + 0.0f (-0.0 and +0.0 share a key, as they compare equal in the reference's float comparisons).
 *   vsc_score_pick        narrows state by the (summed) histogram of that level.
 * After the level with shift 0 state[0] is the key of the k-th best score of the union and state[3] the number of scores
 * strictly above it; the sum of the first level's histogram is the size of the union (k beyond it: state is meaningless).
 * Device pointers only.  On a caller's stream (vsc_set_aux_stream) both calls only ENQUEUE -- the caller's next operation on
 * that stream is ordered behind them and a whole selection runs without a host round trip --; on the library's own
 * stream they return when done. */
int vsc_score_histogram(const float* scores, int64_t n, const int64_t* state, int shift, int64_t* hist, int device);
int vsc_score_pick(const int64_t* hist, int64_t* state, int shift, int device);

/* The other half of a re-threshold event (apply_maxres inside faiss.contrib.exhaustive_search, reached at vsc/index.py:147-154:
 * "re-filter every kept batch with a strict s > radius") for a kept list the caller holds in HBM: out_* <- the (row, ref,
 * score) triples with score > radius (STRICT), in no particular order; *n_out (host) their number.  Device arrays of n entries;
 * out_* of capacity n, not aliasing the inputs. */
int vsc_filter_hits(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n, float radius, int32_t* out_i,
                    int32_t* out_j, float* out_s, int64_t* n_out, int device);

/* perm[n] (int32) <- the stable argsort of a score list, best first: equal scores (-0.0 == +0.0) keep their input order.
 * Merges the ranks' candidate lists (vsc/candidates.py:38-40 sorts with Python's stable sort; the concatenation of the
 * ranks' lists in rank order IS first-appearance order, vsc2022_amd/dist.py:merge_candidates).  Host or device arrays. */
int vsc_argsort_scores(const float* scores, int64_t n, int mem, int32_t* perm, int perm_mem, int device);

/* Per-row merge of k-NN lists from reference shards (BASELINE configs[4]; vsc2022_amd/dist.py:ref_sharded_knn): row x of
 * scores / ids holds m candidates (ids: GLOBAL reference rows, < 0 = empty slot); out_* [nq, k] <- the k best per row
 * under (score desc, id asc) -- what faiss index.search returns on the concatenated reference set (vsc/index.py:174);
 * missing slots hold -1 and -FLT_MAX.  1 <= k <= m <= 1024; device pointers. */
int vsc_merge_topk(const float* scores, const int64_t* ids, int64_t nq, int m, int k, float* out_s, int64_t* out_ids,
                   int device);

/* The stream of the entry points that own no handle on `device` (vsc_pair_max, vsc_pair_aggregate, vsc_sort_hits, vsc_score_histogram, vsc_score_pick,
 * vsc_filter_hits, vsc_argsort_scores, vsc_merge_topk, vsc_row_normalize, vsc_tn_forward_sim, vsc_align_forward_sim):
 * as vsc_index_set_stream. */
int vsc_set_aux_stream(int device, void* hip_stream, int own);

/* Replaces sklearn.preprocessing.normalize(x) (row L2; vsc/baseline/score_normalization.py:84,
 * vsc/baseline/sscd_baseline.py:129-130): out = x / max(||x||, 0 -> 1). */
int vsc_row_normalize(const float* x, int64_t n, int dim, int x_mem, float* out, int out_mem,
                      int device);

/* --------------------------------------------------- temporal localisation
 * Replaces VCSLLocalization over batches of candidates (vsc/baseline/localization.py:28-96):
 * per pair sims = q.feature @ r.feature.T + bias (localization.py:36,52-54), the VCSL
 * Temporal-Network aligner reached through model.forward_sim (localization.py:58; vcsl.vta `tn`,
 * third-party -- see DESIGN.md for the unpinned-parity note), and the MaxSim box score
 * (localization.py:88-91).
 *
 * A context keeps the query and reference descriptors of LocalizationWithMetadata.__init__
 * (localization.py:29-31) resident in HBM: qfeat[total_q_rows][dim] with q_off[n_qvid+1] row
 * offsets per query video; same for refs. */
typedef struct vsc_tn_ctx vsc_tn_ctx_t;

/* Supported ranges (anything else is VSC_ERR_INVALID): tn_top_k 1..16, tn_max_step 1..64, max_path 0..15
 * (max_path + 1 extractions fill at most the VSC_TN_MAX_BOXES = 16 boxes of a pair).  min_length, min_sim and max_iou
 * are unrestricted: a min_sim below every score admits every edge, max_iou <= 0 keeps the first box only, max_iou > 1
 * keeps every one.  Every combination in range runs for every video length; the working state of a pair grows with
 * tn_top_k^2 * tn_max_step per query frame, and pairs whose state or similarity tile do not fit the LDS of a launch
 * run from HBM with identical results. */
typedef struct vsc_tn_params {
    int32_t tn_max_step; /* 1..64; VCSL default 10; reference passes 5 (sscd_baseline.py:122,132) */
    int32_t tn_top_k;    /* 1..16; 5 */
    int32_t max_path;    /* 0..15; 10 */
    int32_t min_length;  /* VCSL default 5; reference passes 4 */
    float min_sim;       /* 0.2 */
    float max_iou;       /* 0.3 */
} vsc_tn_params;

int vsc_tn_create(const float* qfeat, const int64_t* q_off, int64_t n_qvid, const float* rfeat,
                  const int64_t* r_off, int64_t n_rvid, int dim, int feat_mem, int device,
                  vsc_tn_ctx_t** out);
/* The same with a codec for the REFERENCE rows, fixed for the life of the context; vsc_tn_create means VSC_CODEC_FLAT
 * with fp32 references in feat_mem.  The query side is fp32 (qfeat, in feat_mem) under both codecs.
 *
 * rfeat / ref_f16 / ref_mem: the reference rows [total_r_rows][dim], in ref_mem (VSC_MEM_HOST / VSC_MEM_DEVICE); fp32
 * when ref_f16 == 0, else IEEE half floats given as uint16 bit patterns, as vsc_index_add_f16 takes them.
 *
 * VSC_CODEC_SQFP16.  The contract of the index codec (vsc_index_create_codec), word for word: a context whose
 * references are the rows X behaves as the Flat context on
 *     dec(X) = the rows rounded to IEEE half floats (round to nearest even, subnormals kept) and converted back:
 * vsc_tn_localize returns that context's boxes, box counts and MaxSim score BITS, vsc_tn_similarity its matrix BITS;
 * vsc_tn_set_queries and vsc_tn_set_stream mean what they mean there.  Rows that are already half floats decode to
 * themselves.  The reference rows live once in HBM, as half floats ([rows + slack][dim padded to 64], natural order:
 * 2 bytes per padded element instead of 4); the packed fp32 image of a Flat context is never allocated, and half rows
 * reach the store in staging chunks of their own size, never as fp32.  The kernels convert the halves in registers
 * (exactly) and run the same ascending-k fp32 chain.
 * A reference row holding NaN, +-inf or a value beyond +-65504 makes the call fail with VSC_ERR_INVALID: *out is NULL
 * and nothing stays allocated.
 * VSC_CODEC_FLAT with ref_f16 != 0 is the Flat context of the upcast rows. */
int vsc_tn_create_codec(const float* qfeat, const int64_t* q_off, int64_t n_qvid, const void* rfeat, int ref_f16,
                        const int64_t* r_off, int64_t n_rvid, int dim, int feat_mem, int ref_mem, int codec,
                        int device, vsc_tn_ctx_t** out);
/* Bytes the context asked the device for to hold its reference descriptor rows (the counterpart of the index's
 * read-only "ref_bytes"): rows rounded up as the kernels need them x padded dim x 4 (Flat) or 2 (SQfp16). */
int64_t vsc_tn_ref_bytes(const vsc_tn_ctx_t* ctx);
int vsc_tn_destroy(vsc_tn_ctx_t* ctx);
/* As vsc_index_set_stream, for a localisation context. */
int vsc_tn_set_stream(vsc_tn_ctx_t* ctx, void* hip_stream, int own);
/* Replace the QUERY side of a context (a new query batch against the same, resident references: the per-query-set
 * step of vsc/baseline/sscd_baseline.py:90-176 when many query sets meet one reference set).  The reference rows
 * stay packed in HBM; only the nq query rows are uploaded and packed.  Same argument meaning as vsc_tn_create. */
int vsc_tn_set_queries(vsc_tn_ctx_t* ctx, const float* qfeat, const int64_t* q_off, int64_t n_qvid, int feat_mem);

/* One localize_all batch.  pair_q/pair_r[n_pairs] are video ordinals.  Outputs (host or device):
 *   out_nbox[n_pairs]                       number of boxes (<= VSC_TN_MAX_BOXES)
 *   out_boxes[n_pairs][VSC_TN_MAX_BOXES][4] q_lo, r_lo, q_hi, r_hi (frame indices, inclusive ends)
 *   out_boxmax[n_pairs][VSC_TN_MAX_BOXES]   max(sims[q_lo:q_hi, r_lo:r_hi]) - bias (half-open slice,
 *                                           localization.py:91); -inf for an empty slice */
int vsc_tn_localize(vsc_tn_ctx_t* ctx, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs,
                    int pairs_mem, const vsc_tn_params* params, float bias, int32_t* out_nbox,
                    int32_t* out_boxes, float* out_boxmax, int out_mem);

/* vcsl.vta.build_vta_model("TN").forward_sim([(name, sims), ...]) (vsc/baseline/localization.py:58)
 * on caller-supplied similarity matrices (host memory): pair p is the row-major lq[p] x lr[p] fp32
 * matrix at sims + sims_off[p]; sims_off[n_pairs] is the total length.  Outputs (host) as in
 * vsc_tn_localize with bias = 0. */
int vsc_tn_forward_sim(const float* sims, const int64_t* sims_off, const int32_t* lq, const int32_t* lr,
                       int64_t n_pairs, const vsc_tn_params* params, int32_t* out_nbox,
                       int32_t* out_boxes, float* out_boxmax, int device);

/* LocalizationWithMetadata.similarity / VCSLLocalization.similarity (localization.py:33-36,48-54)
 * for one pair: out[lq*lr] (host) = q.feature @ r.feature.T + bias; *lq / *lr receive the shape.
 * cap is the capacity of out in floats (VSC_ERR_CAPACITY if too small). */
int vsc_tn_similarity(vsc_tn_ctx_t* ctx, int32_t q_vid, int32_t r_vid, float bias, float* out,
                      int64_t cap, int32_t* lq, int32_t* lr);

/* ------------------------------------------------------------- DnS localisation on the device
 * VCSLLocalizationDnS (vsc/baseline/dns_baseline.py:108-163) without a matrix leaving the GPU: the fine matrix of a pair
 * (a torch model's output, or the region Chamfer similarity computed here) is blended with the coarse similarity inside
 * the Temporal-Network kernel, aligned and scored.  Everything is opt-in: a context that never sees these calls behaves
 * as before.
 *
 * Fine descriptors of a video are [L][R][D]: L the frame count of the same video in the context, 1 <= R <=
 * VSC_FINE_MAX_REGIONS regions per frame, D = fdim values per region; VSC_FINE_ATT: fp32 values, VSC_FINE_BIN: bytes
 * {0, 1} taken as 2 x - 1 in {-1, +1} (exact).  All inputs must be finite (documented, not checked).  The arithmetic,
 * every step one correctly rounded fp32 operation (the library is built with -ffp-contract=off and no fast-math):
 *   1. region matrix   G[i,a; j,b]: acc = +0; acc = fmaf(q[i,a,d], r[j,b,d], acc) for d ascending -- the engine's chain;
 *                      BIN: followed by one division by (float)D
 *   2. forward Chamfer A[i,j]: t = +0; for a = 0 .. R-1 in that order t = t + max_b G[i,a; j,b]; A = t / (float)R
 *   3. backward        B[i,j]: the same with the roles of a and b swapped (sum over b ascending of max_a): the
 *                      reference's model(ref, query).mT, from the same G
 *   4. mapping         F0 = symmetric ? (A + B) / 2.0f : A;  F = F0 / 2.0f + 0.5f
 *   5. blend           C = the coarse tile, vsc_tn_similarity's bits including + bias;
 *                      S = geometric_mean ? sqrtf(fmaxf(F, 1e-7f) * fmaxf(C, 1e-7f)) : F   (the product rounded to fp32:
 *                      numpy's np.sqrt(sim.clip(1e-7) * sim_cg.clip(1e-7)) on fp32 arrays)
 *   6. alignment       S through the Temporal Network; box score max(S[q_lo:q_hi, r_lo:r_hi]) - bias as vsc_tn_localize
 * The max of steps 2-3 is a plain fp32 maximum (G holds no -0.0: the chain starts from +0).
 *
 * The 1-bit store (VSC_FINE_BITS, vsc_tn_set_fine_bits) keeps BIN descriptors as the bits they are and computes the same
 * step 1 from integers.  With q, r in {-1, +1} every partial sum of the chain is an integer of magnitude <= D, so for
 * D <= 2^24 no step rounds and, with the values read as bits (+1 = 1, -1 = 0),
 *     acc == (float)(D - 2 popcount(q xor r))
 * exactly; the same single division by (float)D follows.  Steps 2-6 are the same code.  Results are the BITS of the
 * VSC_FINE_BIN store on the same descriptors, at 1/32 of its memory.
 *   layout   one row per (frame, region) of ceil(D / 128) 16-byte words; bit d of the row = element d, i.e. bit d % 8 of
 *            byte d / 8 -- numpy's np.packbits(x, axis=-1, bitorder="little").  The bits from D up to the end of the row
 *            are zero on BOTH sides: they xor to zero and never enter a popcount (D in the formula is the true fdim).
 *            64 zero rows of slack follow a side's last frame, as in the fp32 store.
 *   masking  packed input carries ceil(D / 8) bytes per row; the unused high bits of a row's last byte are the caller's:
 *            the library masks them, whatever they hold changes no result.
 *
 * The half-float store (VSC_FINE_F16, vsc_tn_set_fine_f16) keeps ATT descriptors as IEEE half floats, which is what the
 * DnS indexer writes for an attention student (feature.half()).  With dec(X) = (float)(half)X -- the index codec's
 * encoder: round to nearest even, subnormals kept -- a context whose descriptors X are in this store returns the BITS
 * that the VSC_FINE_ATT store returns on dec(X), in step 1 and therefore in everything downstream of it: a half
 * converts to fp32 exactly (the hardware conversion, in registers), the same values enter the same chain from +0 in
 * the same ascending order, and steps 2-6 are the same code.  Half-float inputs decode to themselves: their results
 * are those of the VSC_FINE_ATT store on the same descriptors, at half of its memory and half of the transfer.  No
 * product or sum is ever formed in half precision.
 *   layout   one row per (frame, region) of fdim halves padded with zeros to a multiple of 64, natural k order (each
 *            lane half of the kernel loads a 16-byte piece and keeps its 4 of the 8 values); 64 zero rows of slack
 *            follow a side's last frame, rows padded to a multiple of 128 as in the fp32 store: vsc_tn_fine_bytes is
 *            round_up(frames R + 64, 128) * round_up(fdim, 64) * 2 per side, exactly half of the VSC_FINE_ATT figure.
 *   refusal  a source element that is NaN, +-inf or of magnitude beyond 65504 (fp32 source), or a half holding inf or
 *            NaN (half source), is VSC_ERR_INVALID -- the index codec's rule.  The side being written is then DROPPED
 *            (the context holds no descriptors and no bytes for it), the other side is untouched, and
 *            vsc_tn_fine_similarity refuses until the side is set again: a half-written side is never readable. */
#define VSC_FINE_ATT 0
#define VSC_FINE_BIN 1
#define VSC_FINE_BITS 2 /* a context state only (vsc_tn_set_fine_bits): vsc_tn_set_fine refuses it as an unknown kind */
#define VSC_FINE_F16 3  /* a context state only, like VSC_FINE_BITS (vsc_tn_set_fine_f16): vsc_tn_set_fine refuses it */
#define VSC_FINE_MAX_REGIONS 16
/* Attach fine descriptors to a context: qfine / rfine = [total frames of that side][regions][fdim] in `mem` (host or
 * device; host sources are staged in chunks), fp32 (ATT) or bytes (BIN); the frame counts and video offsets are the
 * context's own.  Either pointer may be NULL: that side is left as it is -- unless regions, fdim or kind differ from
 * what the context holds, which drops both sides first.  vsc_tn_set_queries drops the query side, whose frames it
 * replaces.  The rows are kept as L R packed fp32 rows of fdim (padded to 64) in the engine's k-interleaved layout; BIN is
 * stored as +-1 fp32 here and as bits by vsc_tn_set_fine_bits.  VSC_ERR_INVALID for regions outside
 * 1..VSC_FINE_MAX_REGIONS, fdim < 1 or an unknown kind. */
int vsc_tn_set_fine(vsc_tn_ctx_t* ctx, const void* qfine, const void* rfine, int regions, int fdim, int kind, int mem);
/* Attach BIN descriptors to a context as bits (the VSC_FINE_BITS store above).  packed = 0: the input of VSC_FINE_BIN,
 * bytes {0, 1}, [frames][regions][fdim]; packed = 1: already packed, [frames][regions][ceil(fdim / 8)] bytes as
 * np.packbits(x, axis=-1, bitorder="little") makes them (tail bits masked here).  `mem`, a NULL side, changed regions /
 * fdim, and vsc_tn_set_queries as for vsc_tn_set_fine; going from an ATT / BIN store to this one or back drops both
 * sides first.  vsc_tn_fine_similarity then runs the popcount kernel; every other call is unchanged.  VSC_ERR_INVALID for
 * regions outside 1..VSC_FINE_MAX_REGIONS, fdim outside 1..2^24 (the bound of the identity), packed outside {0, 1} or no
 * context. */
int vsc_tn_set_fine_bits(vsc_tn_ctx_t* ctx, const void* qfine, const void* rfine, int regions, int fdim, int packed, int mem);
/* Attach ATT descriptors to a context as half floats (the VSC_FINE_F16 store above).  src_f16 = 0: the input of
 * VSC_FINE_ATT, fp32 [frames][regions][fdim], rounded here; src_f16 = 1: IEEE halves of the same shape, taken as they
 * are (no fp32 copy of them exists at any time).  `mem`, a NULL side, changed regions / fdim, and vsc_tn_set_queries as
 * for vsc_tn_set_fine; going from an ATT / BIN / BITS store to this one or back drops both sides first.
 * vsc_tn_fine_similarity then runs the region Chamfer kernel on half rows; every other call is unchanged.
 * VSC_ERR_INVALID for regions outside 1..VSC_FINE_MAX_REGIONS, fdim < 1, src_f16 outside {0, 1} or no context (judged
 * before the context is read), and for a source element a half cannot hold (see "refusal" above: that side is dropped). */
int vsc_tn_set_fine_f16(vsc_tn_ctx_t* ctx, const void* qfine, const void* rfine, int regions, int fdim, int src_f16, int mem);
/* Bytes the context asked the device for to hold the fine descriptor rows of both sides (cf. vsc_tn_ref_bytes); the
 * packed bytes for a VSC_FINE_BITS store, the half-float bytes for a VSC_FINE_F16 store. */
int64_t vsc_tn_fine_bytes(const vsc_tn_ctx_t* ctx);
/* Stage 1: F (steps 1-4) of every pair of the list, row-major lq x lr, at out + out_off[p]; out_off[n_pairs] lies where
 * `out` does (out_mem), cap is the capacity of `out` in floats.  VSC_ERR_CAPACITY with nothing written when a pair does
 * not fit; VSC_ERR_INVALID when a side that has frames has no fine descriptors, or for a pair ordinal outside the
 * context's videos (checked on the host copy of the list and again by the kernel, which skips the tile and raises an
 * error word: nothing is read out of range).  One launch over (pair, tile) work items, of the kernel of the context's
 * store (fp32 or half-float rows on the matrix cores, or bit rows by popcount); stream and synchronisation as vsc_tn_localize. */
int vsc_tn_fine_similarity(vsc_tn_ctx_t* ctx, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                           int symmetric, float* out, const int64_t* out_off, int64_t cap, int out_mem);
/* Stage 2: steps 5-6 for one localize_all batch.  `fine` is a slab of F matrices (stage 1's output or a torch model's),
 * pair p row-major lq x lr at fine + fine_off[p]; fine and fine_off[n_pairs] lie in fine_mem.  A host slab is copied down
 * once, up to the last cell a pair covers.  Without geometric_mean the fine matrices are aligned as they are and no
 * descriptor is read.  Outputs, stream and synchronisation as vsc_tn_localize; the box table feeds vsc_tn_match_rows
 * unchanged.  Both reference codecs: only the coarse side has one. */
int vsc_tn_localize_fine(vsc_tn_ctx_t* ctx, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                         const float* fine, const int64_t* fine_off, int fine_mem, int geometric_mean,
                         const vsc_tn_params* params, float bias, int32_t* out_nbox, int32_t* out_boxes, float* out_boxmax,
                         int out_mem);
/* S (step 5) of one pair on the host: `fine` = its F matrix (lq x lr floats in fine_mem); out, cap, lq, lr as
 * vsc_tn_similarity. */
int vsc_tn_similarity_fine(vsc_tn_ctx_t* ctx, int32_t q_vid, int32_t r_vid, float bias, const float* fine, int fine_mem,
                           int geometric_mean, float* out, int64_t cap, int32_t* lq, int32_t* lr);

/* ------------------------------------------------------------- DTW / DP aligners
 * vcsl.vta.build_vta_model("DTW" / "DP") on the device (vsc2022_amd/vcsl/aligners.py spells both algorithms out choice
 * by choice; the boxes here are those of its host functions `dtw` / `dp` on the same fp32 matrices, integer for
 * integer).  One 64-lane workgroup per pair; the similarity tile is vsc_tn_similarity's, bit for bit; the warping-path
 * costs, path scores and run scores are float64 sums of the host's operands in the host's order, the match / alive
 * test is `s >= (float)min_sim` in fp32 (as NumPy compares an fp32 matrix with a Python float), the IoU a float64
 * quotient.  A pair's whole working state lives in LDS: pairs of more than VSC_ALIGN_MAX_CELLS = lq * lr cells are not
 * attempted (status 1) and are the caller's to align. */
#define VSC_ALIGN_DTW 1
#define VSC_ALIGN_DP 2
#define VSC_ALIGN_MAX_CELLS 9216
typedef struct vsc_align_params {
    int32_t method;      /* VSC_ALIGN_DTW / VSC_ALIGN_DP */
    int32_t discontinue; /* 0..15 */
    int32_t min_length;  /* >= 0 */
    int32_t max_path;    /* 0..VSC_TN_MAX_BOXES (DP; DTW ignores it) */
    double min_sim;
    double max_iou;
} vsc_align_params;

/* One localize_all batch through DTW / DP.  Arguments, output layout (out_nbox, out_boxes, out_boxmax), stream and
 * synchronisation as vsc_tn_localize.  out_status[n_pairs] says who finished a pair:
 *   0  done here (a pair with an empty video: no boxes)
 *   1  not attempted: lq * lr > VSC_ALIGN_MAX_CELLS
 *   2  more than VSC_TN_MAX_BOXES boxes passed the keep filter
 * out_nbox[p] = 0 whenever out_status[p] != 0.  VSC_ERR_INVALID for a discontinue outside 0..15, a max_path outside
 * 0..VSC_TN_MAX_BOXES, min_length < 0 or an unknown method. */
int vsc_tn_align(vsc_tn_ctx_t* ctx, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                 const vsc_align_params* params, float bias, int32_t* out_nbox, int32_t* out_boxes, float* out_boxmax,
                 int32_t* out_status, int out_mem);
/* The aligners' forward_sim on caller-supplied matrices (host memory, laid out as for vsc_tn_forward_sim); outputs
 * (host) as above with bias = 0. */
int vsc_align_forward_sim(const float* sims, const int64_t* sims_off, const int32_t* lq, const int32_t* lr, int64_t n_pairs,
                          const vsc_align_params* params, int32_t* out_nbox, int32_t* out_boxes, float* out_boxmax,
                          int32_t* out_status, int device);

/* ------------------------------------------------------------- match rows
 * The last step of the reference's pipeline on the device: the padded box table of a localize_all batch becomes the
 * rows of matches.csv (vsc/baseline/localization.py:66-73: query_start = ts_q[x1][0], query_end = ts_q[x2][1],
 * ref_start = ts_r[y1][0], ref_end = ts_r[y2][1]) as dense columns, in the order localize_all emits its Match rows.
 * Every output is a copy or a gather -- no arithmetic on values: the contract is exact, bit for bit.
 *
 * The per-frame [start, end] tables of both sides, float64 [total rows of that side][2] in ts_mem, copied into HBM and
 * kept with the context (float32, float64 and integer sources up to 32 bits pass through float64 exactly; 1-D
 * timestamps are handed over as (t, t) rows).  Either pointer may be NULL: that side is left as it is.
 * vsc_tn_set_queries drops the query table, whose rows it replaces. */
int vsc_tn_set_timestamps(vsc_tn_ctx_t* ctx, const double* q_ts, const double* r_ts, int ts_mem);
/* The rows of one batch.  pair_q / pair_r (pairs_mem) and nbox / boxes / boxmax (in_mem) are the arguments and outputs
 * of vsc_tn_localize or vsc_tn_align, host or device.  Row order: pair order, then box slot order.  Outputs (out_mem):
 *   out_pair[cap]      int32   index of the row's pair in this call's pair list
 *   out_box[cap][4]    int32   q_lo, r_lo, q_hi, r_hi (may be NULL)
 *   out_score[cap]     fp32    the box's boxmax value
 *   out_times[cap][4]  double  query_start, query_end, ref_start, ref_end
 * *n_rows (host) receives the number of rows the inputs describe (the sum of nbox).  cap < that: VSC_ERR_CAPACITY and
 * nothing is written.  All out_* NULL with cap == 0: VSC_OK, the count only (no timestamp table needed).
 * Pairs that vsc_tn_align did not finish (status != 0) have nbox == 0 and contribute no rows.
 *
 * The row offsets are the exclusive prefix sum of nbox, computed on the device; the row pass handles one (pair, slot)
 * per lane.  Stream and synchronisation as vsc_tn_localize: the call returns synchronised.
 * Nothing is read outside the tables, whatever the inputs hold.  Guarded: a box count outside 0..VSC_TN_MAX_BOXES, a
 * pair ordinal outside the context's videos, a corner outside [0, L) of its video, a missing timestamp table.  What
 * lies in host memory is checked on the host before anything is launched; for device memory the kernels skip the
 * offending rows and raise an error word.  Either way the call returns VSC_ERR_INVALID and the outputs are undefined.
 * The launches are accounted under class 3 of the process-wide kernel-time accounting below. */
int vsc_tn_match_rows(vsc_tn_ctx_t* ctx, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                      const int32_t* nbox, const int32_t* boxes, const float* boxmax, int in_mem, int32_t* out_pair,
                      int32_t* out_box, float* out_score, double* out_times, int64_t cap, int out_mem, int64_t* n_rows);

/* ------------------------------------------------------------- segment AP of the matching track
 * vsc/metrics.py match_metric on the device, up to its last few vector operations: ground-truth rows and prediction rows
 * -> per group of equal scores, in descending score order, the score and the four running sums the metric divides
 * (intersection with the ground truth on the query and the reference axis, covered length on both), + the ground truth's
 * length per axis.  The caller finishes with r = sqrt((iq / tq) * (ir / tr)), p = sqrt((iq / cq) * (ir / cr)),
 * ap = sum p * diff(r).  The contract is exact: every value is the float64 the host's walk computes, operation for
 * operation and in its order (ranking: stable, descending, -0.0 and 0.0 one key; per pair the coalesced interval lists of
 * `VideoPair.add_prediction`; the sums strictly in rank order) -- tests/match_metric_ref.py restates it.
 *
 * Rows carry the ordinal of their (query, ref) pair, 0 <= ordinal < n_pairs, any numbering:
 *   gt_pair[n_gt] int32, gt_times[n_gt][4] double (query_start, query_end, ref_start, ref_end), gt_first[n_gt_pairs]
 *   int32 = the ordinals of the ground truth's pairs in first-appearance order, the order their lengths are summed in
 *   (NULL: 0, 1, ..., n_gt_pairs - 1) -- all three in gt_mem;
 *   pred_pair[n_pred] int32, pred_score[n_pred] double, pred_times[n_pred][4] double in pred_mem.
 * Outputs, host memory: out_score[cap], out_sums[cap][4] (iq, ir, cq, cr at each group end), *n_groups, gt_len[2]
 * (tq, tr), stats[8] (may be NULL) = pairs evaluated from LDS, pairs evaluated from an HBM slab (more than 320 rows),
 * prediction rows, groups; then the kernel time of the sorts, the pair kernels and the ordered sums in microseconds (HIP
 * events, 0 unless vsc_aux_profile is on) and a reserved 0.  cap < the number of groups: VSC_ERR_CAPACITY, *n_groups is
 * set and nothing else is written.
 *
 * Nothing is read outside the tables, whatever the inputs hold.  Guarded on the device (an error word, VSC_ERR_INVALID,
 * outputs untouched): a pair ordinal outside [0, n_pairs), a non-finite score or time, end < start, and a pair with
 * more than VSC_METRIC_MAX_PAIR_ROWS rows (predictions + ground-truth segments).  One wave evaluates a pair and its
 * work is quadratic in the pair's rows (a counting sort of N^2 / 64 comparisons per lane and axis, then rows / 64 walks
 * over the N-entry lists, read from HBM above 320 rows): a fraction of a second at the bound by that count (estimated,
 * not measured), a minute at ten times as many -- so such a table is refused instead of holding a shared GPU.  The
 * challenge's tables have a handful of rows per pair.
 * Handle-less family: runs on the stream of vsc_set_aux_stream and returns synchronised.  The library keeps its scratch
 * for the call (about 100 bytes of HBM per prediction row of the largest call so far) with the device's context. */
#define VSC_METRIC_MAX_PAIR_ROWS 8192
int vsc_match_metric(const int32_t* gt_pair, const double* gt_times, int64_t n_gt, const int32_t* gt_first, int64_t n_gt_pairs,
                     int gt_mem, const int32_t* pred_pair, const double* pred_score, const double* pred_times, int64_t n_pred,
                     int pred_mem, int64_t n_pairs, double* out_score, double* out_sums, int64_t cap, int64_t* n_groups,
                     double* gt_len, int64_t* stats, int device);

/* ---------------------------------------------------------- instrumentation
 * Kernel-time accounting for bench.py: HIP events recorded on the handle's stream around the
 * dominant similarity kernel.  vsc_index_profile(idx, 1) enables it; vsc_index_profile_read
 * returns accumulated kernel milliseconds, launches and algorithmic flops since the last reset. */
int vsc_index_profile(vsc_index_t* idx, int enable);
int vsc_index_profile_read(vsc_index_t* idx, double* sim_ms, int64_t* sim_launches, double* sim_flops,
                           int reset);
/* Same accounting per kernel class: 0 = exact fp32 similarity kernels (what vsc_index_profile_read
 * reports), 1 = fp16 pre-filter GEMM (work = algorithmic flops 2*nq*nr*dim), 2 = exact re-scoring of
 * the pre-filter's candidates (work unused), 3 = re-threshold kernels of the search schedule (radix select +
 * compaction; work unused), 4 = final ordering of the kept hits (work = bytes of the hit triples read),
 * 5 = int8 pre-filter kernel of the sparse batches (work = 2*nq*nr*dim), 6 = the preamble of its launches (row
 * thresholds / scales, the sort of the launch's rows, quantisation of the query panels; work unused). */
int vsc_index_profile_read_class(vsc_index_t* idx, int cls, double* ms, int64_t* launches, double* work,
                                 int reset);
/* Process-wide accounting of the entry points that own no index handle, same method (HIP events on the
 * stream the kernels run on): cls 0 = vsc_pair_max (vsc/candidates.py:24-40 on device hits), cls 1 = the
 * Temporal-Network launches of vsc_tn_localize / vsc_tn_forward_sim (vcsl.vta TN.forward_sim), cls 2 = the DTW / DP
 * launches of vsc_tn_align / vsc_align_forward_sim, cls 3 = the launches of vsc_tn_match_rows.
 * bytes = algorithmic bytes of the calls (4*dim*(Lq+Lr) per pair + boxes; 12 B per hit
 * + 20 B per pair; match rows: 332 B per pair + 60 B written and 32 B gathered per row).  bench.py and scripts only. */
int vsc_aux_profile(int enable);
int vsc_aux_profile_read(int cls, double* ms, int64_t* calls, double* bytes, int reset);
/* Counters of the last thresholded search on this handle: pairs the fp16 pre-filter passed on to
 * the exact stage, and (reserved) hits. */
int vsc_index_search_stats(vsc_index_t* idx, int64_t* candidates, int64_t* hits);

/* ------------------------------------------------- frame inference
 * Epilogue of one convolution of the SSCD trunk with its BatchNorm folded in (what
 * vsc/baseline/inference_impl.py:210-239 runs through TorchScript as conv -> bn -> (+ identity) -> relu):
 * y[r, c] = act(y[r, c] + bias[c] (+ res[r, c])), bf16 device arrays [rows, cols] (NHWC activations, cols =
 * channels, a multiple of 8), fp32 bias, fp32 arithmetic with one rounding; res may be NULL; relu != 0 applies
 * max(., 0).  In place on y, on the HIP stream `hip_stream` (NULL = the default stream).  Device pointers only. */
int vsc_bias_act_bf16(void* y, const void* res, const float* bias, int64_t rows, int64_t cols, int relu,
                      void* hip_stream);
/* A 3x3 (padding 1, stride 1 or 2; taps = 9) or 1x1 (taps = 1, stride 1) convolution of that trunk as an implicit GEMM
 * on the matrix cores with the epilogue inside: out[b, ho, wo, n] = act(sum x[b, hi, wi, c] * w[n, tap, c] + bias[n]
 * (+ res[b, ho, wo, n])); x [B, H, W, C] NHWC, w [N, taps, C] (= the channels-last memory of the PyTorch weight
 * [N, C, kh, kw]), res / out [B, Ho, Wo, N] with Ho = (H - 1) / stride + 1: bf16 device arrays; bias fp32; C and N
 * multiples of 64.  fp32 accumulation, one rounding.  Same stream convention. */
int vsc_conv_bias_act_bf16(const void* x, const void* w, const float* bias, const void* res, void* out, int64_t B,
                           int64_t H, int64_t W, int64_t C, int64_t N, int taps, int stride, int relu, void* hip_stream);
/* The stem's tail in one pass: out = maxpool3x3(stride 2, padding 1)(relu(x + bias)); x [N, H, W, C], out
 * [N, (H-1)/2+1, (W-1)/2+1, C] bf16 NHWC device arrays, C a multiple of 8; bit-identical to the two separate passes. */
int vsc_pool3x3s2_bias_relu_bf16(const void* x, const float* bias, void* out, int64_t N, int64_t H, int64_t W,
                                 int64_t C, void* hip_stream);
/* A 1x1 convolution of that trunk (or a Linear layer of the ViT) with its epilogue in one kernel:
 * out[m, n] = act(sum_k a[m, k] * w[n, k] + bias[n] (+ res[m, n])); a [M, K] = NHWC activations (M = batch * H * W),
 * w [N, K] = the convolution's weight as stored (Cout x Cin), res / out [M, N]: bf16 device arrays, bias fp32;
 * fp32 accumulation on the matrix cores, one rounding.  act: 0 = none, 1 = ReLU, 2 = exact erf GELU (nn.GELU()).
 * N and K multiples of 64; res may be NULL; out must not alias a.  Same stream convention. */
int vsc_gemm_bias_act_bf16(const void* a, const void* w, const float* bias, const void* res, void* out,
                           int64_t M, int64_t N, int64_t K, int act, void* hip_stream);

/* ------------------------------------------------- DINO ViT inference (--baseline dino --fast)
 * Attention of a ViT with head dimension 64, read from the qkv Linear's output rows: qkv [B * N, 3 * C] bf16 with
 * C = 64 * heads (q of head h at columns 64 h, k at C + 64 h, v at 2 C + 64 h); out [B * N, C] = softmax(q k^T / 8) v
 * per (image, head), head h at columns 64 h.  bf16 operands on the matrix cores, fp32 scores, softmax and
 * accumulation.  1 <= N <= 1024.  Same stream convention. */
int vsc_vit_attention_bf16(const void* qkv, void* out, int64_t B, int64_t N, int64_t heads, void* hip_stream);
/* LayerNorm of the rows of x [rows, cols] bf16 -> out bf16 (may alias x): fp32 mean and biased variance,
 * (x - mean) / sqrt(var + eps) * gamma + beta with fp32 gamma / beta [cols], one rounding.  cols a multiple of 64. */
int vsc_layernorm_bf16(const void* x, const float* gamma, const float* beta, void* out, int64_t rows, int64_t cols,
                       float eps, void* hip_stream);
/* Token assembly: out [B, P + 1, C] bf16 with out[b, 0] = cls + pos[0] and out[b, 1 + p] = patch[b * P + p] +
 * pos[1 + p]; patch [B * P, C] bf16 (the patch-embedding GEMM's output), cls [C] and pos [P + 1, C] fp32.
 * C a multiple of 8. */
int vsc_vit_tokens_bf16(const void* patch, const float* cls, const float* pos, void* out, int64_t B, int64_t P,
                        int64_t C, void* hip_stream);
/* The copy-detection head of DINO (eval_copy_detection): y = LayerNorm(x) of every token of x [B, N, C] bf16 (fp32
 * gamma / beta, eps), out [B, 2 C] fp32 = y[b, 0] (CLS) followed by (mean over tokens 1 .. N-1 of
 * max(y, 1e-6)^4)^(1/4).  N >= 2, C a multiple of 64 and <= 1024. */
int vsc_vit_cdpool_bf16(const void* x, const float* gamma, const float* beta, float* out, int64_t B, int64_t N,
                        int64_t C, float eps, void* hip_stream);

/* ------------------------------------------------- DnS L3-iMAC region descriptors (--baseline dns --fast)
 * Region max-pool of an NHWC bf16 activation with the channel L2 normalisation in the same kernel: x [B, H, W, C] bf16
 * (a stage output of the trunk as it stands in memory), grid gh = (H - win) / stride + 1, gw likewise (no padding,
 * floor); m[c] = max over dy, dx < win of x[b, gy * stride + dy, gx * stride + dx, c], over signed values (bf16 widens
 * to fp32 exactly, so the maximum is exact), and
 *     out[(b * gh * gw + gy * gw + gx) * out_row + out_col + c] = m[c] / max(sqrt(sum_c m[c]^2), eps)
 * with the sum (in no fixed order), root and division in fp32.  out is fp32 with rows of out_row floats; columns outside
 * [out_col, out_col + C) of a row are not written, so the taps of a network fill column slices of one buffer.
 * C a multiple of 8 and <= 4096; win, stride >= 1; H, W >= win; out_row >= out_col + C; eps >= 0; x 16-byte aligned;
 * anything else, or a NULL pointer with B > 0, is VSC_ERR_INVALID before any device call.  B = 0 is a no-op.  Inputs
 * must be finite and zero or of magnitude within [2^-50, 2^50] (not checked): the squares and their sum then stay
 * inside fp32's normal range.  Device pointers only; same stream convention as the kernels above. */
int vsc_region_pool_l2_bf16(const void* x, float* out, int64_t B, int64_t H, int64_t W, int64_t C, int win, int stride,
                            int64_t out_row, int64_t out_col, float eps, void* hip_stream);
/* In place x[r, :] /= max(||x[r, :]||_2, eps) on an fp32 device matrix [rows, cols]: torch's F.normalize, which clamps
 * the norm from below -- not sklearn's normalisation, which leaves zero rows alone and is what the host-or-device
 * row normaliser of the search API implements.  rows >= 0 (0: no-op), cols >= 1, eps >= 0. */
int vsc_rows_l2norm_f32(float* x, int64_t rows, int64_t cols, float eps, void* hip_stream);

/* ------------------------------------------------- frame transform of the inference CLI (--packed_batch)
 * What the reference does to a decoded frame on the host (vsc/baseline/inference_impl.py:39-69: PIL image ->
 * torchvision Resize / CenterCrop / ToTensor / Normalize), reproduced bit for bit for n uint8 RGB frames of DIFFERENT
 * source sizes and one common output shape.  Per frame i: dense HWC source [src_h, src_w, 3] at src + src_off[i] ->
 * resize to (dst_h, dst_w) -> window [top, top + out_h) x [left, left + out_w) -> value -> out.
 *
 * Resize = PIL's ImagingResample, 8-bit, BILINEAR (triangle filter, support 1), PRECISION_BITS = 22.  For one axis
 * in -> out, every (int) truncating toward zero, all else in double:
 *     scale = in / out;  fs = max(scale, 1.0);  support = fs;  ksize = (int)ceil(support) * 2 + 1
 *     for xx in 0..out-1:
 *         center = (xx + 0.5) * scale
 *         xmin = max((int)(center - support + 0.5), 0)
 *         xmax = min((int)(center + support + 0.5), in) - xmin                     (number of taps, <= ksize)
 *         w[x] = max(0, 1 - |(x + xmin - center + 0.5) * (1.0 / fs)|)
 *         ww = sum of w[x] in x order;  k[x] = w[x] / ww   (ww != 0)
 *         K[x] = k < 0 ? (int)(-0.5 + k * 2^22) : (int)(0.5 + k * 2^22)            (int32)
 *     out[xx] = clip8((sum_x in[xmin + x] * K[x] + 2^21) >> 22)      (int32 sum, arithmetic shift, clamp to 0..255)
 * The horizontal pass runs first, the vertical pass second, and the image between them is uint8: rounded and clipped
 * by the line above.  An axis with in == out is skipped: its data passes through untouched.  The int32 sum cannot
 * overflow (255 * sum K ~ 2^30).
 *
 * Value: v = ((float)level / 255.0f - mean[c]) / std[c], three correctly rounded fp32 operations in that order
 * (ToTensor, then Normalize with fp32 mean / std).  VSC_FRAME_OUT_F32_NCHW writes v to out [n, 3, out_h, out_w] float;
 * VSC_FRAME_OUT_BF16_NHWC writes v rounded to nearest even to out [n, out_h, out_w, 3] bf16 (tensor.to(bfloat16)).
 *
 * The resize target and window of a transform (short edge to 288 / 320, centre crop with Python's half-to-even round)
 * are the caller's: (dst_h, dst_w, top, left) are taken as given.  Only the rows and columns the window needs are
 * computed.  The coefficient tables are built on the host, once per distinct (in, out) pair, and kept across calls.
 * src and out are device pointers; every other array is host memory.  Limits, each VSC_ERR_INVALID with a message
 * before any device call: 0 <= n <= 2^20 (0 is a no-op); 1 <= src_h, src_w <= 8192; 1 <= dst_h, dst_w <= 4096;
 * out_h, out_w >= 1 and the window inside [0, dst) on both axes; src_off >= 0; std[c] != 0; a known out_format; no NULL
 * pointer with n > 0.  Launches on `hip_stream` of the current device (NULL = the default stream), as the kernels
 * above; calls on different streams share scratch memory and are ordered one after the other on the device. */
#define VSC_FRAME_OUT_F32_NCHW 0  /* out [n, 3, oh, ow] float */
#define VSC_FRAME_OUT_BF16_NHWC 1 /* out [n, oh, ow, 3] bf16 */
int vsc_frame_transform_u8(const uint8_t* src, const int64_t* src_off, const int32_t* src_h, const int32_t* src_w,
                           const int32_t* dst_h, const int32_t* dst_w, const int32_t* top, const int32_t* left, int64_t n,
                           int out_h, int out_w, const float* mean, const float* std, int out_format, void* out,
                           void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VSCMI_H */
