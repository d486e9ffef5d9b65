// Argument blocks and launchers of the HIP kernels (shared by the kernel translation units and
// the C-ABI layer in api.hip).
#pragma once
#include "vscmi_common.h"
#include "cand_list.h"

namespace vscmi {

// Scratch of the radix sorts (sortpairs.hip): two key and two value ping-pong buffers + the sort's own temporary.
struct SortScratch {
    DevBuf w0, w1, w2, w3, tmp;
};
// Scratch of the pair aggregation beyond the sorts' (pair_reduce.hip): the per-pair results, the final sort's ping-pong
// buffers and the control words.
struct PairAggScratch {
    DevBuf k2, v2a, v2b, rs, rfirst, rcnt, ctl;
};
// A hit list on the device: (row, ref, score) in three parallel arrays.
struct HitView { int32_t* i; int32_t* j; float* s; };
struct ConstHitView {
    const int32_t* i; const int32_t* j; const float* s;
    ConstHitView(const int32_t* i_, const int32_t* j_, const float* s_) : i(i_), j(j_), s(s_) {}
    ConstHitView(const HitView& v) : i(v.i), j(v.j), s(v.s) {}
};

struct SimThreshArgs {
    const float* Q; const float* R; int dpad; int nq; int i0; int nr; int tq; int tr;
    const float* radius; int32_t* out_i; int32_t* out_j; float* out_s;
    unsigned long long* counter; long long cap; int* overflow;
};
// fp16 pre-filter (sim_f16.hip): emits every (row, ref) whose fp16 score PLUS the tile's error bound
// exceeds *radius -- a superset of the exact hits; the exact stage (rescore.hip) then applies the exact test.
struct SimF16Args {
    const _Float16* Q; const _Float16* R;  // fp16 images [rows pad 256][dpadh], natural k order
    const float* qn; const float* rn;      // per-row upper bounds of the L2 norm (+inf: row not representable)
    int dpadh; int nq; int i0; int nr; int tq; int tr;
    float c1, c2, c3;                      // |fp16 score - exact score| <= c1*nq*nr + c2*(nq+nr) + c3
    const float* radius;
    // k-NN mode: per-row thresholds (indexed like qn; the test becomes fp16 score + bound >= row_thr[row]);
    // nullptr = thresholded search against *radius
    const float* row_thr;
    CandList list;                         // where the candidates go (cand_list.h)
};
// panel-stationary fp16 pre-filter (sim_f16p.hip; dpadh <= 512): the query side is the natural fp16 image, the
// reference side the FRAGMENT-MAJOR image written by launch_pack_half_frag (layout.hip)
constexpr int F16P_PANEL_ROWS = 128;  // query rows per LDS-resident panel
constexpr int F16P_COL_STEP = 512;    // reference columns per workgroup step (8 waves x 64); row padding of the image
constexpr int F16P_MAX_DPADH = 512;   // the panel must fit the LDS: 128 rows x dpadh x 2 B <= 128 KiB
// The fragment-major fp16 image: index of the 16-byte piece `piece` (k = 8 piece .. 8 piece + 7) of row `row`.  Rows
// are grouped in wave tiles of 64 (two 32-row MFMA blocks); per k-step of 16 a tile holds 128 pieces: block, k half,
// row inside the block -- the B operand of one v_mfma_f32_32x32x16_f16 (lane l: row l & 31, k half l >> 5) is 1 KiB
// of consecutive memory.  The writers (layout.hip, codec_f16.hip) and the codec's readers go through here; the panel
// kernel reads whole fragments by construction, and the exact stage (rescore.hip: rescore_list, f16_screen_kernel)
// spells the same index out.  (Row: the caller's own integer type -- only the tile index needs 64 bits)
template <typename Row>
__host__ __device__ __forceinline__ int64_t frag_piece(Row row, int piece, int dpadh) {
    return (int64_t)(row >> 6) * (dpadh / 16) * 128 + ((row >> 5) & 1) * 64 + (row & 31) + (piece >> 1) * 128 + (piece & 1) * 32;
}
struct SimF16PArgs {
    const _Float16* Q; const void* Rf;
    const float* qn; const float* rn;      // per-row upper bounds of the L2 norm (+inf: row not representable)
    int dpadh; int nq; int i0; int nr;
    int npanel; int nsteps; int slice;     // work split (sim_f16p_plan); items = (panel, slice of col-steps)
    int* next_slice;                       // [npanel] slices handed out so far (zeroed by the launcher)
    float c1, c2, c3;
    const float* radius; const float* row_thr;  // as in SimF16Args
    CandList list;
    // deferred rescoring (radius searches only; nullptr or *floor = +inf: off): a candidate whose exact score is PROVEN to
    // lie in (*radius, *floor] is stored with the top bit of its row set (DEFER_MARK) and goes to the deferred set
    const float* floor = nullptr;
};
// panel-stationary INT8 pre-filter (sim_i8p.hip; dims <= 1024): the query side is the launch's own int8 image with one
// scale per 128-row panel (quant_query_panels), the reference side the fragment-major int8 image + per-row meta of
// launch_quant_ref_frag (quant_i8.hip)
constexpr int I8P_MAX_DPAD8 = 1024;    // the panel must fit the LDS: 128 rows x dpad8 B <= 128 KiB
// coordinates left out of the int8 images because every reference row holds the same value there (quant_i8.hip)
constexpr int I8_MAX_EXCLUDED = 8;
struct ExcludedDims {
    int n = 0;
    int idx[I8_MAX_EXCLUDED] = {};     // logical coordinate
    float val[I8_MAX_EXCLUDED] = {};   // the references' common value
    __host__ __device__ bool holds(int k) const {
        bool h = false;
#pragma unroll
        for (int c = 0; c < I8_MAX_EXCLUDED; ++c) h |= c < n && idx[c] == k;
        return h;
    }
};
struct SimI8PArgs {
    const void* Q; const float4* pstat;   // [npanel * 128][dpad8] int8; per panel {1 / s, max E, max N, max N'}
    const void* Rf; const float4* rmeta;  // fragment-major int8 image; per reference row {1 / s, E, N, N'}
    int dpad8; int nq; int i0; int nr;
    int npanel; int nsteps; int slice;     // work split (sim_f16p_plan)
    int* next_slice;                       // [npanel + 1]: per-panel slice counters + one global item counter
    int order;                             // 0: panel-major with stealing; 1: slice-major (all panels of a slice first)
    int pair;                              // 1: work items of TWO panels, wave tiles of 256 rows x 32 columns (sim_i8p_pairs)
    float c_acc;                           // rounding of the exact fp32 chain per |q||r|
    const float* radius; const float* row_thr;  // as in SimF16Args (row_thr indexed by POSITION inside the launch)
    CandList list;
};
// top bit of a candidate's row in a list written with SimF16PArgs::floor set: the pair is deferred, not re-scored
constexpr uint32_t DEFER_MARK = 0x80000000u;
struct RescoreArgs {
    const float* Q; const float* R; int dpad;  // packed fp32 images (exact arithmetic contract)
    CandList list;  // the pre-filter launch's candidates (cand_list.h); tail_count is reset to 0 after the pass
    // the int8 kernel hands over POSITIONS inside its launch when the launch's rows were permuted (sorted by threshold
    // or by scale): row = perm_i0 + perm[position - perm_i0].  nullptr: the list holds rows
    const int32_t* perm; int perm_i0;
    unsigned long long* n_cand_total;      // statistics
    const float* radius; int32_t* out_i; int32_t* out_j; float* out_s;
    unsigned long long* counter; long long cap;  // (a full kept-hit list sets bit 0 of *list.overflow)
    const float* row_thr;  // k-NN mode: keep score >= row_thr[global row] (nullptr: score > *radius)
    // the launch searched the reference rows [j0, j0 + nr): the kernels' images were handed over from row j0 on, the
    // candidate list holds refs RELATIVE to it (cand_compact / the segment-wise exact stage add j0 back)
    int j0 = 0;
    // SQfp16 codec: the reference rows are read from the fp16 store instead of R (rsrc: 0 = R, packed fp32; 1 = Rh in
    // natural layout; 2 = Rh fragment-major) and converted in registers; the chain is the same
    const _Float16* Rh = nullptr; int dpadh = 0; int rsrc = 0;
    // the deferred set D (cand_compact: marked entries go here as (row, absolute ref) instead of the dense list);
    // d_count = its fill level, d_total = pairs deferred so far (statistics).  More than d_cap sets bit 0 of *list.overflow
    int32_t* d_i = nullptr; int32_t* d_j = nullptr; unsigned long long* d_count = nullptr; unsigned long long* d_total = nullptr;
    long long d_cap = 0;
};
// fp16 screen of the int8 route's candidates (rescore.hip): the pair list sorted by reference row in, the pairs whose
// fp16 score + error bound still reaches the threshold out
struct ScreenArgs {
    const _Float16* Qh; const float* qn;  // row-major fp16 query image, norm bounds (absolute rows)
    const _Float16* Rh; const float* rn;  // reference image: fragment-major (frag) or row-major
    int dpadh; int frag;
    float c1, c2, c3;                     // |fp16 score - exact score| <= c1 |q||r| + c2 (|q| + |r|) + c3
    const float* radius; const float* row_thr;
    const uint32_t* sj; const uint32_t* si; long long n;
    uint32_t* out_j; uint32_t* out_i; unsigned long long* n_out;
    unsigned long long* n_cand_total;     // statistics: += n
    int* overflow;
    // deferred rescoring (floor != nullptr and *floor < +inf): a pair proven to lie in (*radius, *floor] joins the
    // deferred set instead of the survivors (fields as in RescoreArgs)
    const float* floor = nullptr;
    int32_t* d_i = nullptr; int32_t* d_j = nullptr; unsigned long long* d_count = nullptr; unsigned long long* d_total = nullptr;
    long long d_cap = 0;
};
struct SimKnnArgs {
    const float* Q; const float* R; int dpad; int nq; int nr; int tq; int tr; int nchunk; int k;
    float* part_s; int32_t* part_j;
    int no_first_tile_select;  // option knn_first_tile = 0: k > 1 inserts every score of a run's first tile (A/B)
};
struct KnnMergeArgs {
    const float* part_s; const int32_t* part_j; int nq; int nchunk; int k; float* out_s; int64_t* out_j; int l2;
};
struct ScoreMatArgs { const float* Q; const float* R; int dpad; int dim; int nq; int nr; int metric; float* S; };
struct MatThreshArgs {
    const float* S; int nq; int nr; int i0; const float* radius; int32_t* out_i; int32_t* out_j; float* out_s;
    unsigned long long* counter; long long cap; int* overflow;
};
struct MatKnnArgs { const float* S; int nq; int nr; int k; float* part_s; int32_t* part_j; };
struct SelectCtl {
    unsigned long long n; unsigned long long n_tmp; float radius; int overflow; int active;
    unsigned int prefix; unsigned int prefix_mask; unsigned long long rank; unsigned int hist[256];
    unsigned long long n_rethreshold;
    unsigned long long n_cand_total;  // pre-filter candidates of the whole search (statistics)
    unsigned long long n_tail;        // fill level of the candidate list's shared tail (current batch)
    // deferred rescoring (api_search.hip, "the deferred set"): pairs proven to lie in (radius, floor] wait in D, score-less
    unsigned long long n_d;           // fill level of D
    unsigned long long n_deferred;    // pairs that ever entered D (statistics)
    float floor;                      // +inf: no floor chosen since the last event
    int need_force;                   // the last event could not be decided with D left out: the host re-scores D
    unsigned int ev_ok;               // events decided with a non-empty D left out (statistics)
    unsigned int pad_;
};
struct TnPairArgs {
    const float* qfeat; const float* rfeat; const int64_t* q_off; const int64_t* r_off; int dpad;
    const int32_t* pair_q; const int32_t* pair_r; const int32_t* work; int n_work; vsc_tn_params prm;
    float bias; int max_lq; int lds_tile_floats; float* slab; int64_t slab_floats;
    int32_t* out_nbox; int32_t* out_boxes; float* out_boxmax;
    // forward_sim mode (sims_in != nullptr): precomputed matrices, pair p at sims_in + sims_off[p]
    const float* sims_in; const int64_t* sims_off; const int32_t* sims_lq; const int32_t* sims_lr;
    // over-long videos: per-workgroup working state in HBM (state_bytes each) instead of LDS; nullptr = LDS
    char* state; int64_t state_bytes;
    // SQfp16 context: the reference rows as half floats, [rows][dpad] in natural k order, instead of rfeat (nullptr:
    // rfeat, packed fp32).  The query side is packed fp32 either way
    const _Float16* rfeat_h;
    // DnS blend (vsc_tn_localize_fine with geometric_mean; nullptr: none): the fine matrix F of pair p, row-major lq x lr at
    // fine + fine_off[p]; the tile becomes sqrtf(fmaxf(F, 1e-7f) * fmaxf(tile, 1e-7f)) before anything reads it
    const float* fine; const int64_t* fine_off;
};
struct TnSimsArgs {
    const float* qfeat; const float* rfeat; int64_t qrow0, rrow0; int lq, lr, dpad; float bias; float* out;
    const _Float16* rfeat_h;  // as in TnPairArgs
    const float* fine;        // the pair's fine matrix (lq x lr) to blend with, as in TnPairArgs; nullptr: none
};
// Region Chamfer similarity of a batch of pairs (fine_sim.hip): one work item = FQ x FR whole frames of one pair
struct FineSimArgs {
    const float* qfine; const float* rfine;  // packed fp32 rows, regions rows per frame, dpad floats each
    const int64_t* q_off; const int64_t* r_off; int64_t n_qvid, n_rvid;  // the context's frame offsets per video
    const int32_t* pair_q; const int32_t* pair_r;
    const int32_t* work; int n_work;  // [n_work][3]: pair, first query frame, first reference frame of the tile
    int regions, fdim, dpad, bin, symmetric;
    float* out; const int64_t* out_off;  // F of pair p, row-major lq x lr, at out + out_off[p]
    int* err;  // error word: bit 0 = a pair ordinal outside the context's videos (that work item is skipped)
    // VSC_FINE_F16 (launch_fine_sim's `half_rows`): the rows of both sides as half floats instead -- [rows][dpad] halves,
    // natural k order, zero padded, as launch_encode_rows(..., frag = false) writes them; qfine / rfine are not read.
    // (Last, so that the fp32 kernel finds every other field where it was.)
    const _Float16* qfine_h; const _Float16* rfine_h;
};
// The same on the 1-bit store (fine_bits.hip, VSC_FINE_BITS): FineSimArgs' fields under FineSimArgs' names, the rows as bits
struct FineBitsArgs {
    const uint4* qbits; const uint4* rbits;  // bit rows, regions rows per frame, w16 16-byte words each (zero past fdim)
    const int64_t* q_off; const int64_t* r_off; int64_t n_qvid, n_rvid;
    const int32_t* pair_q; const int32_t* pair_r;
    const int32_t* work; int n_work;
    int regions, fdim, w16, symmetric;
    float* out; const int64_t* out_off;
    int* err;
};

// DTW / DP aligners (align.hip): one candidate pair per single-wavefront workgroup, as tn_pair_kernel; the fields the
// similarity tile reads (tn_sims.h) carry TnPairArgs' names
struct AlignArgs {
    const float* qfeat; const float* rfeat; const int64_t* q_off; const int64_t* r_off; int dpad;
    const int32_t* pair_q; const int32_t* pair_r; const int32_t* work; int n_work; vsc_align_params prm;
    float bias;
    int32_t* out_nbox; int32_t* out_boxes; float* out_boxmax; int32_t* out_status;
    // forward_sim mode (sims_in != nullptr): precomputed matrices, pair p at sims_in + sims_off[p]
    const float* sims_in; const int64_t* sims_off; const int32_t* sims_lq; const int32_t* sims_lr;
    const _Float16* rfeat_h;  // as in TnPairArgs
};
// Match rows (match_rows.hip): the padded box table of a batch -> one dense row per box
struct MatchRowsArgs {
    const int32_t* pair_q; const int32_t* pair_r; int64_t n_pairs;
    const int32_t* nbox; const int32_t* boxes; const float* boxmax;  // as vsc_tn_localize / vsc_tn_align write them
    const int64_t* q_off; const int64_t* r_off; int64_t n_qvid, n_rvid;
    const double* q_ts; const double* r_ts;  // [rows][2] start, end of every frame
    int32_t* pair_off;  // [n_pairs] scratch: row offset of the pair inside its tile
    int64_t* tile_off;  // [match_rows_tiles(n_pairs)] scratch: tile sums, then their exclusive scan
    int64_t* ctl;       // [0] rows of the batch, [1] error word (bit 0 box count, bit 1 pair ordinal, bit 2 corner)
    int32_t* out_pair; int32_t* out_box; float* out_score; double* out_times;  // out_box may be nullptr
};
// Segment AP (metric.hip): the tables of vsc_match_metric in device memory -> the group-end sums in host memory
// (kept with the device context for the life of the process, as its Workspace is: ~100 B per prediction row of the largest
// call so far, 40 MB at 400 000 rows)
struct MetricScratch {
    DevBuf buf[24];
};
struct MetricIn {
    const int32_t* gt_pair; const double* gt_times; int64_t n_gt;
    const int32_t* gt_first; int64_t n_gt_pairs;  // the ground truth's pairs in first-appearance order (nullptr: 0, 1, 2, ...)
    const int32_t* pred_pair; const double* pred_score; const double* pred_times; int64_t n_pred;
    int64_t n_pairs;
};
struct MetricOut {
    double* scores; double* sums; int64_t cap;  // host: [cap], [cap][4]
    int64_t n_groups;
    double* gt_len;    // host [2]
    int64_t stats[8];  // pairs on the LDS route, pairs on the HBM route, rows, groups; microseconds of the sorts, the pair
                       // kernels and the ordered sums (0 unless vsc_aux_profile is on); 0
};
// The working state of one pair, all of it in LDS: byte offsets into the workgroup's dynamic array and their sum.  The
// kernel carves by the pair's own shape; a launch asks for the largest `total` among its pairs.
//   both: tile   the similarity matrix, fp32 [lq][lr] (not in forward_sim mode: the caller's matrix is read in place)
//         kept   the boxes that passed the keep filter, int [VSC_TN_MAX_BOXES][4]
//   DTW:  f64    three rolling anti-diagonals of D, double [min(lq, lr) + 1] each
//         runs   score (double) and box (4 x uint16) of every run of the warping path: at most (lq + lr) / 2 runs (a
//                path of lq + lr - 1 cells at most, a non-matching cell between two runs at least)
//         bytes  the traceback rule of every cell, decided when the cell is filled (0 diagonal, 1 up, 2 left: [lq][lr]),
//                then the lq + lr steps of the path at most
//   DP:   f64    S, double [lq][lr]
//         runs   the boxes in extraction order, int [VSC_TN_MAX_BOXES][4]
//         u16    the predecessor step of every cell, (a << 8) | b, 0 = none
//         bytes  dead-row and dead-column flags, [lq] + [lr]
struct AlignLayout { size_t f64, runs, tile, kept, u16, bytes, total; };
__host__ __device__ inline AlignLayout align_layout(int method, int lq, int lr, bool tile_in_lds) {
    const size_t cells = (size_t)lq * lr, edge = (size_t)lq + lr;
    const bool dtw = method == VSC_ALIGN_DTW;
    AlignLayout L;
    size_t off = 0;
    L.f64 = off;
    off += dtw ? 3 * ((size_t)(lq < lr ? lq : lr) + 1) * 8 : cells * 8;
    L.runs = off;
    off += dtw ? (edge / 2 + 1) * 16 : (size_t)VSC_TN_MAX_BOXES * 16;
    L.tile = off;
    off += tile_in_lds ? cells * 4 : 0;
    L.kept = off;
    off += (size_t)VSC_TN_MAX_BOXES * 16;
    L.u16 = off;
    off += dtw ? 0 : cells * 2;
    L.bytes = off;
    off += dtw ? cells + edge : edge;
    L.total = (off + 15) & ~(size_t)15;
    return L;
}
// The launches' LDS budget.  Every pair of at most VSC_ALIGN_MAX_CELLS cells fits: lq + lr <= cells + 1 and
// min(lq, lr) <= sqrt(cells) bound the layout above by 14 B per cell + 1 B per edge frame (DP), or 5 B per cell + 9 B per
// edge frame (DTW), + 3 KiB of fixed parts
constexpr size_t ALIGN_LDS_MAX = 150 * 1024;
static_assert(14 * (size_t)VSC_ALIGN_MAX_CELLS + (VSC_ALIGN_MAX_CELLS + 1) + 3072 <= ALIGN_LDS_MAX, "DP state of the largest pair");
static_assert(5 * (size_t)VSC_ALIGN_MAX_CELLS + 9 * (VSC_ALIGN_MAX_CELLS + 1) + 3072 <= ALIGN_LDS_MAX, "DTW state of the largest pair");
static_assert(VSC_ALIGN_MAX_CELLS < 32768, "frame indices are kept in 16 bits");

int launch_sim_thresh(const SimThreshArgs&, hipStream_t);
int launch_sim_f16(const SimF16Args&, hipStream_t);
int sim_f16_grid(int tq, int tr);
int launch_rescore(const RescoreArgs&, hipStream_t);
int launch_cand_count(const RescoreArgs&, int, unsigned long long*, hipStream_t);
int launch_cand_compact(const RescoreArgs&, int, uint32_t*, uint32_t*, unsigned long long*, hipStream_t);
int launch_rescore_dense(const RescoreArgs&, const uint32_t*, const uint32_t*, long long, hipStream_t,
                         const unsigned long long* n_dev = nullptr);
int launch_f16_screen(const ScreenArgs&, hipStream_t);
int sort_candidates_by_ref(uint32_t*, uint32_t*, uint32_t*, uint32_t*, int64_t, int64_t, DevBuf&, const uint32_t**,
                           const uint32_t**, hipStream_t);
void sim_f16p_plan(int64_t nq, int64_t nr, int* npanel, int* nsteps, int* slice, int* grid);
int launch_sim_f16p(const SimF16PArgs&, int grid, hipStream_t);
int launch_sim_i8p(const SimI8PArgs&, int grid, hipStream_t);
bool sim_i8p_pairs(int dpad8, int npanel, int nsteps, int slice, bool force);  // does a launch of this size use work items of two panels?
int launch_quant_ref_frag(const float*, int, void*, float4*, int64_t, int64_t, int, const ExcludedDims&, const float*, hipStream_t);
int launch_col_sums(const float*, int64_t, int, double*, double*, hipStream_t);
int launch_row_center(const float*, int, int, const float*, float*, float*, hipStream_t);
int launch_dim_minmax(const float*, int64_t, int, unsigned*, unsigned*, hipStream_t);
int launch_meta_looseness(const float4*, int64_t, double*, hipStream_t);
int launch_quant_query_panels(const float*, int, int, int, void*, int, float4*, const int32_t*, const float*, float*,
                              const ExcludedDims&, hipStream_t);
int launch_row_absmax(const float*, int, int, const ExcludedDims&, float*, hipStream_t);
int launch_row_bias_thresholds(const float*, int, int, const float*, const float*, const ExcludedDims&, const float*, const float*, float*,
                               hipStream_t);
int sort_rows_by_threshold(const float*, int64_t, SortScratch&, const int32_t**, hipStream_t);
int argsort_scores_desc(const float*, int64_t, SortScratch&, const int32_t**, hipStream_t);
int launch_ctl_init(SelectCtl*, float, hipStream_t);
int launch_filter_hits(ConstHitView, long long, float, HitView, unsigned long long*, hipStream_t);
int launch_score_hist(const float*, long long, const long long*, int, long long*, hipStream_t);
int launch_score_pick(const long long*, long long*, int, hipStream_t);
int launch_merge_topk(const float*, const long long*, long long, int, int, float*, long long*, hipStream_t);
int sort_rows_by_threshold_then_scale(const float*, const float*, int64_t, int, SortScratch&, const int32_t**, hipStream_t);
int launch_pack_half_frag(const float*, int64_t, int, _Float16*, float*, int64_t, int64_t, int, hipStream_t);
int launch_pack_half(const float*, int64_t, int, _Float16*, float*, int64_t, int, hipStream_t);
int launch_sim_knn(const SimKnnArgs&, hipStream_t);
int launch_knn_merge(const KnnMergeArgs&, hipStream_t);
int knn_from_hits(ConstHitView, int64_t, int64_t, int, SortScratch&, float*, int64_t*, hipStream_t);
int launch_knn_row_thr(const float*, int64_t, int, float*, int64_t, hipStream_t);
int launch_knn_seed_hits(const float*, const int64_t*, int64_t, int, HitView, unsigned long long*, hipStream_t);
int launch_score_matrix(const ScoreMatArgs&, hipStream_t);
int launch_matrix_thresh(const MatThreshArgs&, hipStream_t);
int launch_matrix_knn(const MatKnnArgs&, hipStream_t);
int set_thresh_kernel_attrs();
int enqueue_rethreshold(SelectCtl*, HitView, HitView, unsigned long long, hipStream_t);
int enqueue_rethreshold_deferred(SelectCtl*, HitView, HitView, unsigned long long, hipStream_t);
int enqueue_floor_select(SelectCtl*, const float*, unsigned long long, hipStream_t);
int launch_defer_reset(SelectCtl*, hipStream_t);
int sort_hits_topk(ConstHitView, int64_t, int64_t, int64_t, int64_t, SortScratch&, HitView, int, int64_t*, hipStream_t);
int sort_hits_rowcol(ConstHitView, int64_t, SortScratch&, HitView, int, hipStream_t);
int pair_max_device(const int32_t*, const int32_t*, const float*, int64_t, const int32_t*, const int32_t*, int64_t, int64_t,
                    SortScratch&, DevBuf&, int32_t*, int32_t*, float*, int64_t*, int64_t, int64_t*, hipStream_t);
// pair_reduce.hip: max / sum / mean / top-m mean per (query video, ref video), pairs in their final order
int pair_agg_check(const char* who, int agg, int64_t top_m);
int pair_aggregate_device(const int32_t* hi, const int32_t* hj, const float* hs, int64_t n, const int32_t* row2q, const int32_t* row2r,
                          int64_t nq_rows, int64_t nr_rows, int hits_order, int agg, int64_t top_m, SortScratch&, PairAggScratch&,
                          int32_t* out_q, int32_t* out_r, float* out_s, int64_t* out_first, int32_t* out_count, int64_t cap,
                          int64_t* n_pairs, hipStream_t);
int launch_knn_to_hits(const int64_t* ids, int64_t nq, int k, int32_t* hi, int32_t* hj, hipStream_t);
int launch_pack_rows(const float*, int64_t, int, float*, int64_t, int, hipStream_t, float kpad = 0.0f);
int launch_row_normalize(const float*, int64_t, int, float*, hipStream_t);
// dynamic LDS a tn_pair_kernel launch may ask for (working state + similarity tile): what launch_tn_pairs sets as the
// kernel's limit and what tn_run_buckets plans its LDS-tile buckets against (a workgroup has 160 KiB on gfx950)
constexpr size_t TN_LAUNCH_LDS_MAX = 158 * 1024;
size_t tn_state_bytes_host(int, int, int, int idx_bytes = 2);
int launch_tn_pairs(const TnPairArgs&, size_t, hipStream_t);
int launch_tn_sims(const TnSimsArgs&, hipStream_t);
int fine_sim_frames(int regions);  // frames per side of a work item of launch_fine_sim
int launch_fine_sim(const FineSimArgs&, hipStream_t, bool half_rows = false);
int launch_bin_to_pm1(const uint8_t*, int64_t, float*, hipStream_t);
int fine_bits_row_words(int fdim);  // 16-byte words of one bit row (fine_bits.hip)
int launch_fine_bits(const FineBitsArgs&, hipStream_t);
int launch_pack_bits(const uint8_t*, bool, int64_t, int, uint32_t*, int64_t, int, hipStream_t);
int launch_align_pairs(const AlignArgs&, size_t, hipStream_t);
int64_t match_rows_tiles(int64_t n_pairs);
int launch_match_rows_scan(const MatchRowsArgs&, hipStream_t);
int launch_match_rows_emit(const MatchRowsArgs&, hipStream_t);
int match_metric_device(const MetricIn&, MetricScratch&, MetricOut&, hipStream_t);
// SQfp16 codec (codec_f16.hip)
int launch_encode_rows(const void*, bool, int64_t, int, _Float16*, float*, int64_t, int64_t, int, bool, int*, hipStream_t);
int launch_decode_rows(const _Float16*, int, bool, int64_t, int64_t, int64_t, float*, int, bool, hipStream_t);
int launch_unpack_rows(const float*, int, int64_t, int, float*, hipStream_t);
int launch_half_to_float(const _Float16*, int64_t, float*, hipStream_t);
int launch_score_matrix_h16(const ScoreMatArgs&, const _Float16*, int, bool, hipStream_t);
int launch_hits_mark(const unsigned long long*, unsigned long long*, hipStream_t);
int launch_hits_add_offset(int32_t*, const unsigned long long*, const unsigned long long*, long long, int, hipStream_t);
int launch_knn_parts_scatter(const float*, const int32_t*, int64_t, int, int, int, int, int, float*, int32_t*, hipStream_t);


}  // namespace vscmi
