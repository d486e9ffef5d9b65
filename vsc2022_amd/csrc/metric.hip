// Segment AP of the matching track (vsc_match_metric): ground-truth rows and prediction rows, each tagged with the ordinal
// of its (query, ref) pair -> per group of equal scores, in descending score order, the four running sums the metric's
// tail needs (intersection with the ground truth and covered length, per axis) + the two ground-truth lengths.  The
// contract is exact: vsc/metrics.py match_metric's float64 operations in match_metric's order (tests/match_metric_ref.py
// restates it; -ffp-contract=off keeps every operation its own rounding).
//
// Launches:
//   seg_keys            per prediction row an order-preserving 64-bit image of score + 0.0 (-0.0 and 0.0: one key), per
//                       ground-truth row its pair ordinal; ordinals and scores are checked here;
//   radix sorts         predictions by key, descending and stable -> rank order; the ranks, stably, by pair ordinal -> every
//                       pair's rows together in rank order; ground-truth rows by pair ordinal;
//   seg_bounds          first position of every pair in the two sorted lists (binary search, one pair per lane);
//   seg_pair<false>     ONE PAIR PER WAVE, ONE PREFIX PER LANE.  The pair's P predictions (rank order, tag k = 1..P) and G
//                       ground-truth segments are staged in LDS; a segment's tag is the first k whose prediction overlaps
//                       it in area (lanes are in rank order: the first set bit of a ballot).  Per axis ONE list of all P + G
//                       items sorted by (lo, hi, index) -- rank by counting --: the predictions alone and the segments
//                       alone are subsequences of it in the same order.  All lanes walk the list in lockstep (wave-uniform
//                       broadcast reads; only the predicate `tag <= my k` differs per lane) and coalesce three times --
//                       predictions, segments, both --, adding every finished interval's hi - lo to a total that starts
//                       at 0.0.  inter_k = (covered_k + truth_k) - union_k; lane k takes lane k-1's values with one
//                       cross-lane move and writes its row's four deltas at the row's rank.  More than 64 predictions:
//                       chunks of 64 prefixes with a carry of the last lane's values.  The same list without the
//                       predictions gives the pair's ground-truth length per axis.
//   seg_pair<true>      pairs of more than MET_LDS_ITEMS items: the same code on a slab in HBM (a correctness route, not a
//                       tuned one).  The LDS launch only lists them; no pair is handed to the host.
//   seg_gather_len      the pairs' ground-truth lengths in the caller's (first-appearance) order;
//   seg_accumulate      the ORDERED sums: one workgroup, chunks of 256 rows staged in LDS, one lane per column adds them
//                       strictly in order (a tree or a Hillis-Steele scan would change the bits); group ends are flagged
//                       in parallel, their positions come from an integer scan; the running values and the score are
//                       written at each group end.
// Nothing is read or written outside the tables whatever the inputs hold: an ordinal out of range, a non-finite score or
// time and end < start raise the error word (ctl[2]) that the entry point turns into VSC_ERR_INVALID; the sort keys are
// integer images, a total order even for NaN, so that every per-pair permutation is one.  A pair of more than
// VSC_METRIC_MAX_PAIR_ROWS rows is refused the same way (error word, VSC_ERR_INVALID): see seg_pair_kernel.
//
// What bounds it (200 000 pairs, 400 000 rows, 8 000 ground-truth rows): the 64-bit sort is 8 passes x 28 B per row = 90 MB
// and the ordinal sort 3 passes x 20 B = 24 MB of traffic, tens of microseconds at HBM rate but some 60 dependent launches;
// the pair kernel reads 40 B and writes 32 B per row; the accumulate pass is 400 000 dependent double adds per column.
// Measured (profiles/match_metric.md): sorts 0.39 ms, pair kernel 0.40 ms, ordered sums 9.1 ms -- none of them tuned.
#include "api_internal.h"
#include "radix.h"

namespace vscmi {

constexpr int MET_LDS_ITEMS = 320;        // predictions + segments of a pair on the LDS route (44 B each: 14 KB per wave)
constexpr int MET_NEVER = 0x7fffffff;     // tag of a segment no prediction overlaps

struct MetricArgs {
    const int32_t* gt_pair; const double* gt_times; int64_t n_gt;
    const int32_t* pred_pair; const double* pred_score; const double* pred_times; int64_t n_pred;
    int64_t n_pairs;
    const uint32_t* rank_row;   // [n_pred] rank -> prediction row
    const uint32_t* pos_rank;   // [n_pred] position in (pair, rank) order -> rank
    const uint32_t* gpos_row;   // [n_gt] position in pair order -> ground-truth row
    const uint32_t* pstart;     // [n_pairs + 1] first position of the pair's predictions
    const uint32_t* gstart;     // [n_pairs + 1] ... of its ground-truth rows
    double* deltas;             // [n_pred][4] by rank: d inter query, d inter ref, d covered query, d covered ref
    double* gt_len;             // [n_pairs][2]
    int64_t* ctl;               // [0] pairs listed for the HBM route, [1] their items, [2] error word
    int32_t* big_pair; int64_t* big_off; int64_t big_cap;
    double* slab_t; int32_t* slab_tag; uint32_t* slab_perm; int64_t slab_items;
};

__device__ __forceinline__ void met_raise(int64_t* ctl, unsigned bit) {
    atomicOr(reinterpret_cast<unsigned int*>(ctl + 2), bit);
}

// order-preserving image of a double (larger value => larger key); x + 0.0 first: -0.0 and 0.0 share a key
__device__ __forceinline__ uint64_t d2key(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key2d(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}
__device__ __forceinline__ bool met_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN

__global__ __launch_bounds__(256) void seg_keys_kernel(MetricArgs a, uint64_t* __restrict__ key, uint32_t* __restrict__ row,
                                                       uint32_t* __restrict__ gkey, uint32_t* __restrict__ grow) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_pred) {
        const double s = a.pred_score[i];
        if (!met_finite(s)) met_raise(a.ctl, 4u);
        const int32_t p = a.pred_pair[i];
        if (p < 0 || p >= a.n_pairs) met_raise(a.ctl, 1u);
        key[i] = d2key(s);
        row[i] = (uint32_t)i;
    }
    if (i < a.n_gt) {
        const int32_t p = a.gt_pair[i];
        const bool ok = p >= 0 && p < a.n_pairs;
        if (!ok) met_raise(a.ctl, 2u);
        gkey[i] = ok ? (uint32_t)p : (uint32_t)a.n_pairs;  // (rows of no pair sort behind every pair)
        grow[i] = (uint32_t)i;
    }
}

// rank r -> (pair ordinal of its row, r): the keys of the second sort
__global__ __launch_bounds__(256) void seg_rank_pairs_kernel(MetricArgs a, const uint32_t* __restrict__ rank_row,
                                                             uint32_t* __restrict__ pkey, uint32_t* __restrict__ prank) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_pred) return;
    const uint32_t row = rank_row[r];
    const int32_t p = row < a.n_pred ? a.pred_pair[row] : -1;
    pkey[r] = (p >= 0 && p < a.n_pairs) ? (uint32_t)p : (uint32_t)a.n_pairs;
    prank[r] = (uint32_t)r;
}

__device__ __forceinline__ uint32_t met_lower_bound(const uint32_t* __restrict__ keys, int64_t n, uint32_t p) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < p) lo = mid + 1; else hi = mid;
    }
    return (uint32_t)lo;
}

__global__ __launch_bounds__(256) void seg_bounds_kernel(const uint32_t* __restrict__ pkeys, int64_t n_pred,
                                                         const uint32_t* __restrict__ gkeys, int64_t n_gt, int64_t n_pairs,
                                                         uint32_t* __restrict__ pstart, uint32_t* __restrict__ gstart) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n_pairs) return;
    pstart[p] = met_lower_bound(pkeys, n_pred, (uint32_t)p);
    gstart[p] = met_lower_bound(gkeys, n_gt, (uint32_t)p);
}

// the host's _coalesce followed by its ordered sum, one interval at a time
struct Coalescer {
    double lo = 0.0, hi = 0.0, total = 0.0;
    bool started = false;
    __device__ __forceinline__ void add(double l, double h) {
        if (started && l <= hi) {
            hi = h > hi ? h : hi;
        } else {
            if (started) total += hi - lo;
            lo = l; hi = h; started = true;
        }
    }
    __device__ __forceinline__ double end() const { return started ? total + (hi - lo) : total; }
};

template <bool HBM>
__global__ __launch_bounds__(64) void seg_pair_kernel(MetricArgs a) {
    __shared__ double s_t[HBM ? 4 : MET_LDS_ITEMS * 4];
    __shared__ int32_t s_tag[HBM ? 1 : MET_LDS_ITEMS];
    __shared__ uint32_t s_perm[HBM ? 2 : MET_LDS_ITEMS * 2];
    const int lane = threadIdx.x;
    int64_t p;
    int64_t slab_off = 0;
    if constexpr (HBM) {
        p = a.big_pair[blockIdx.x];
        slab_off = a.big_off[blockIdx.x];
        if (p < 0 || p >= a.n_pairs) return;
    } else {
        p = blockIdx.x;
    }
    const uint32_t ps = a.pstart[p], gs = a.gstart[p];
    const int64_t P64 = (int64_t)a.pstart[p + 1] - ps, G64 = (int64_t)a.gstart[p + 1] - gs;
    if (P64 < 0 || G64 < 0 || ps + P64 > a.n_pred || gs + G64 > a.n_gt) return;  // (never: the bounds are sorted)
    // one wave does a pair's work, and that work is quadratic in its rows (counting sort: N^2 / 64 comparisons per lane and
    // axis; walk: P / 64 passes over N entries, each a global load on the HBM route): beyond the documented bound the pair
    // is refused, not run
    if (P64 + G64 > VSC_METRIC_MAX_PAIR_ROWS) {
        if (lane == 0) met_raise(a.ctl, 16u);
        return;
    }
    const int P = (int)P64, G = (int)G64, N = P + G;
    double* t;
    int32_t* tag;
    uint32_t* perm;
    if constexpr (HBM) {
        if (slab_off < 0 || slab_off + N > a.slab_items) return;  // (never: the offsets were handed out from the same counts)
        t = a.slab_t + slab_off * 4;
        tag = a.slab_tag + slab_off;
        perm = a.slab_perm + slab_off * 2;
    } else {
        if (N > MET_LDS_ITEMS) {  // listed for the HBM route
            if (lane == 0) {
                const unsigned long long slot = atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl), 1ull);
                const unsigned long long off = atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl + 1), (unsigned long long)N);
                if ((int64_t)slot < a.big_cap) {
                    a.big_pair[slot] = (int32_t)p;
                    a.big_off[slot] = (int64_t)off;
                }
            }
            return;
        }
        t = s_t;
        tag = s_tag;
        perm = s_perm;
    }
    // ---- stage: predictions in rank order, then the ground-truth segments
    bool bad = false;
    for (int i = lane; i < N; i += 64) {
        const double* src;
        if (i < P) {
            const uint32_t r = a.pos_rank[ps + i];
            const uint32_t row = r < a.n_pred ? a.rank_row[r] : 0u;
            src = a.pred_times + (int64_t)(row < a.n_pred ? row : 0u) * 4;
        } else {
            const uint32_t row = a.gpos_row[gs + (i - P)];
            src = a.gt_times + (int64_t)(row < a.n_gt ? row : 0u) * 4;
        }
        const double v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
        bad |= !(met_finite(v0) && met_finite(v1) && met_finite(v2) && met_finite(v3)) || v1 < v0 || v3 < v2;
        t[i * 4 + 0] = v0; t[i * 4 + 1] = v1; t[i * 4 + 2] = v2; t[i * 4 + 3] = v3;
        tag[i] = i < P ? i + 1 : MET_NEVER;
    }
    if (bad) met_raise(a.ctl, 8u);
    __syncthreads();
    // ---- wake-up rank of every segment: the first prediction that overlaps it in area (the host's own expression)
    for (int g = 0; g < G; ++g) {
        const double g0 = t[(P + g) * 4 + 0], g1 = t[(P + g) * 4 + 1], g2 = t[(P + g) * 4 + 2], g3 = t[(P + g) * 4 + 3];
        for (int c0 = 0; c0 < P; c0 += 64) {
            const int k = c0 + lane;
            bool ov = false;
            if (k < P) {
                const double p0 = t[k * 4 + 0], p1 = t[k * 4 + 1], p2 = t[k * 4 + 2], p3 = t[k * 4 + 3];
                const double w = (g1 < p1 ? g1 : p1) - (g0 > p0 ? g0 : p0);
                const double h = (g3 < p3 ? g3 : p3) - (g2 > p2 ? g2 : p2);
                ov = fabs((w >= 0.0 ? w : 0.0) * (h >= 0.0 ? h : 0.0)) > 0.0;
            }
            const unsigned long long m = __ballot(ov);
            if (m) {
                if (lane == 0) tag[P + g] = c0 + (int)__ffsll((long long)m);  // (1-based bit = 1-based rank in the chunk)
                break;
            }
        }
    }
    // ---- the list of each axis: rank by counting over integer keys (lo, hi, index)
    for (int axis = 0; axis < 2; ++axis) {
        for (int i = lane; i < N; i += 64) {
            const uint64_t lo_i = d2key(t[i * 4 + 2 * axis]), hi_i = d2key(t[i * 4 + 2 * axis + 1]);
            int rank = 0;
            for (int j = 0; j < N; ++j) {
                const uint64_t lo_j = d2key(t[j * 4 + 2 * axis]), hi_j = d2key(t[j * 4 + 2 * axis + 1]);
                rank += (lo_j < lo_i || (lo_j == lo_i && (hi_j < hi_i || (hi_j == hi_i && j < i)))) ? 1 : 0;
            }
            perm[axis * N + rank] = (uint32_t)i;
        }
    }
    __syncthreads();
    // ---- the pair's ground-truth length per axis: all its segments, awake or not (wave-uniform)
    for (int axis = 0; axis < 2; ++axis) {
        Coalescer len;
        for (int e = 0; e < N; ++e) {
            const uint32_t i = perm[axis * N + e];
            if (i < (uint32_t)P || i >= (uint32_t)N) continue;
            len.add(t[i * 4 + 2 * axis], t[i * 4 + 2 * axis + 1]);
        }
        if (lane == 0) a.gt_len[p * 2 + axis] = len.end();
    }
    // ---- the prefixes, 64 at a time
    double carry_inter[2] = {0.0, 0.0}, carry_cov[2] = {0.0, 0.0};
    for (int c0 = 0; c0 < P; c0 += 64) {
        const int k = c0 + lane + 1;  // this lane's prefix: the state after the pair's k-th prediction
        uint32_t rank = 0;
        if (k <= P) rank = a.pos_rank[ps + k - 1];
        for (int axis = 0; axis < 2; ++axis) {
            Coalescer cov, tru, uni;
            for (int e = 0; e < N; ++e) {
                const uint32_t i = perm[axis * N + e];
                if (i >= (uint32_t)N) continue;
                const int tg = tag[i];
                if (tg > c0 + 64) continue;  // (asleep for every prefix of this chunk)
                const double lo = t[i * 4 + 2 * axis], hi = t[i * 4 + 2 * axis + 1];
                if (tg <= k) {
                    uni.add(lo, hi);
                    if (i < (uint32_t)P) cov.add(lo, hi); else tru.add(lo, hi);
                }
            }
            const double c = cov.end();
            const double inter = (c + tru.end()) - uni.end();
            double prev_inter = __shfl_up(inter, 1), prev_c = __shfl_up(c, 1);
            if (lane == 0) { prev_inter = carry_inter[axis]; prev_c = carry_cov[axis]; }
            if (k <= P && rank < a.n_pred) {
                a.deltas[(int64_t)rank * 4 + axis] = inter - prev_inter;
                a.deltas[(int64_t)rank * 4 + 2 + axis] = c - prev_c;
            }
            carry_inter[axis] = __shfl(inter, 63);
            carry_cov[axis] = __shfl(c, 63);
        }
    }
}

__global__ __launch_bounds__(256) void seg_gather_len_kernel(const double* __restrict__ gt_len, int64_t n_pairs,
                                                             const int32_t* __restrict__ gt_first, int64_t n_gt_pairs,
                                                             double* __restrict__ out, int64_t* __restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_gt_pairs) return;
    const int64_t p = gt_first ? (int64_t)gt_first[i] : i;
    if (p < 0 || p >= n_pairs) {
        met_raise(ctl, 2u);
        out[i * 2] = out[i * 2 + 1] = 0.0;
        return;
    }
    out[i * 2] = gt_len[p * 2];
    out[i * 2 + 1] = gt_len[p * 2 + 1];
}

// Ordered column sums of vals[n][NCOL], sampled at group ends (keys[i] != keys[i + 1], and the last row; keys == nullptr:
// the last row only).  ONE workgroup.  out_sums[g][NCOL] / out_score[g] are written for g < cap; *n_groups = their number.
template <int NCOL>
__global__ __launch_bounds__(256) void seg_accumulate_kernel(const double* __restrict__ vals, int64_t n,
                                                             const uint64_t* __restrict__ keys, double* __restrict__ out_sums,
                                                             double* __restrict__ out_score, int64_t cap,
                                                             int64_t* __restrict__ n_groups) {
    __shared__ double s_in[256 * NCOL];
    __shared__ double s_run[256 * NCOL];
    __shared__ int s_flag[256];
    const int tid = threadIdx.x;
    double run = 0.0;
    int64_t groups = 0;
    for (int64_t i0 = 0; i0 < n; i0 += 256) {
        const int cnt = (int)(n - i0 < 256 ? n - i0 : 256);
        for (int x = tid; x < cnt * NCOL; x += 256) s_in[x] = vals[i0 * NCOL + x];
        const int64_t i = i0 + tid;
        const bool end = tid < cnt && (i == n - 1 || (keys && keys[i] != keys[i + 1]));
        s_flag[tid] = end ? 1 : 0;
        __syncthreads();
        if (tid < NCOL) {  // strictly in rank order, one lane per column
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) {
                run += s_in[j * NCOL + tid];
                s_run[j * NCOL + tid] = run;
            }
        }
        for (int off = 1; off < 256; off <<= 1) {  // inclusive scan of the flags (integers: the schedule does not matter)
            const int v = tid >= off ? s_flag[tid - off] : 0;
            __syncthreads();
            s_flag[tid] += v;
            __syncthreads();
        }
        if (end) {
            const int64_t g = groups + s_flag[tid] - 1;
            if (g < cap) {
#pragma unroll
                for (int c = 0; c < NCOL; ++c) out_sums[g * NCOL + c] = s_run[tid * NCOL + c];
                if (keys) out_score[g] = key2d(keys[i]);
            }
        }
        groups += s_flag[255];
        __syncthreads();  // (the staging arrays are rewritten by the next chunk)
    }
    if (tid == 0) *n_groups = groups;
}

// HIP events around a stage of the call, only while the process-wide accounting is on.  (AuxTimer adds into one of the
// accounting classes, whose number is part of the ABI; this one hands the time to the call's stats block.)
struct StageTimer {
    hipEvent_t a = nullptr, b = nullptr;
    StageTimer() = default;
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer() { drop(); }  // (an early return between begin() and microseconds() leaks nothing)
    void drop() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr;
    }
    void begin(hipStream_t s) {
        if (!g_aux.on) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, s);
    }
    void end(hipStream_t s) { if (a && b) (void)hipEventRecord(b, s); }
    int64_t microseconds() {  // after the stream has been synchronised
        float t = 0.0f;
        const bool ok = a && b && hipEventElapsedTime(&t, a, b) == hipSuccess;
        drop();
        return ok ? (int64_t)(t * 1000.0f + 0.5f) : 0;
    }
};

static int met_bits_for(uint64_t maxval) {
    int b = 1;
    while (b < 32 && (maxval >> b)) ++b;
    return b;
}
static unsigned met_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// Everything between the uploaded tables and the host-side results (include/vscmi.h, vsc_match_metric).  The stream is
// synchronised on return.  While vsc_aux_profile is on, the sorts, the pair kernels and the ordered sums are timed with
// HIP events: out.stats[4..6], microseconds.
int match_metric_device(const MetricIn& in, MetricScratch& sc, MetricOut& out, hipStream_t stream) {
    const int64_t n_pred = in.n_pred, n_gt = in.n_gt, n_pairs = in.n_pairs, n_gtp = in.n_gt_pairs;
    if (n_pred > 0x7fffffffLL || n_gt > 0x7fffffffLL || n_pairs > 0x7ffffff0LL) {
        set_error("vsc_match_metric: %lld predictions / %lld ground-truth rows / %lld pairs are beyond the supported size",
                  (long long)n_pred, (long long)n_gt, (long long)n_pairs);
        return VSC_ERR_INVALID;
    }
    enum { K64A, K64B, V32A, V32B, PKA, PKB, PVA, PVB, GKA, GKB, GVA, GVB, TMP, BOUNDS, DELTAS, GTLEN, GTORD, CTL, BIGP, BIGO, SLAB,
           OSUM, OSCORE, OGT };
    const int64_t np1 = n_pred > 0 ? n_pred : 1, ng1 = n_gt > 0 ? n_gt : 1;
    for (int b : {K64A, K64B}) VSC_TRY(sc.buf[b].reserve((size_t)np1 * 8));
    for (int b : {V32A, V32B, PKA, PKB, PVA, PVB}) VSC_TRY(sc.buf[b].reserve((size_t)np1 * 4));
    for (int b : {GKA, GKB, GVA, GVB}) VSC_TRY(sc.buf[b].reserve((size_t)ng1 * 4));
    VSC_TRY(sc.buf[TMP].reserve(radix_tmp_bytes(std::max(np1, ng1))));
    VSC_TRY(sc.buf[BOUNDS].reserve((size_t)(n_pairs + 1) * 8));
    VSC_TRY(sc.buf[DELTAS].reserve((size_t)np1 * 32));
    VSC_TRY(sc.buf[GTLEN].reserve((size_t)(n_pairs + 1) * 16));
    VSC_TRY(sc.buf[GTORD].reserve((size_t)(n_gtp + 1) * 16));
    VSC_TRY(sc.buf[CTL].reserve(64));
    const int64_t big_cap = (n_pred + n_gt) / (MET_LDS_ITEMS + 1) + 1;
    VSC_TRY(sc.buf[BIGP].reserve((size_t)big_cap * 4));
    VSC_TRY(sc.buf[BIGO].reserve((size_t)big_cap * 8));
    const int64_t ocap = std::max<int64_t>(std::min(out.cap, n_pred), 1);
    VSC_TRY(sc.buf[OSUM].reserve((size_t)ocap * 32));
    VSC_TRY(sc.buf[OSCORE].reserve((size_t)ocap * 8));
    VSC_TRY(sc.buf[OGT].reserve(16));

    MetricArgs a;
    memset(&a, 0, sizeof(a));
    a.gt_pair = in.gt_pair; a.gt_times = in.gt_times; a.n_gt = n_gt;
    a.pred_pair = in.pred_pair; a.pred_score = in.pred_score; a.pred_times = in.pred_times; a.n_pred = n_pred;
    a.n_pairs = n_pairs;
    a.deltas = sc.buf[DELTAS].as<double>();
    a.gt_len = sc.buf[GTLEN].as<double>();
    a.ctl = sc.buf[CTL].as<int64_t>();  // [0..2] see MetricArgs, [4] groups, [5] the one "group" of the length sums
    a.big_pair = sc.buf[BIGP].as<int32_t>();
    a.big_off = sc.buf[BIGO].as<int64_t>();
    a.big_cap = big_cap;
    VSC_HIP(hipMemsetAsync(a.ctl, 0, 64, stream));
    VSC_HIP(hipMemsetAsync(a.deltas, 0, (size_t)np1 * 32, stream));  // (rows of no pair keep 0: the call fails anyway)
    VSC_HIP(hipMemsetAsync(sc.buf[OGT].p, 0, 16, stream));

    StageTimer tm_sort, tm_pair, tm_acc;
    tm_sort.begin(stream);
    uint64_t *ka = sc.buf[K64A].as<uint64_t>(), *kb = sc.buf[K64B].as<uint64_t>();
    uint32_t *va = sc.buf[V32A].as<uint32_t>(), *vb = sc.buf[V32B].as<uint32_t>();
    uint32_t *pka = sc.buf[PKA].as<uint32_t>(), *pkb = sc.buf[PKB].as<uint32_t>();
    uint32_t *pva = sc.buf[PVA].as<uint32_t>(), *pvb = sc.buf[PVB].as<uint32_t>();
    uint32_t *gka = sc.buf[GKA].as<uint32_t>(), *gkb = sc.buf[GKB].as<uint32_t>();
    uint32_t *gva = sc.buf[GVA].as<uint32_t>(), *gvb = sc.buf[GVB].as<uint32_t>();
    const int64_t n_rows = std::max(n_pred, n_gt);
    if (n_rows > 0) hipLaunchKernelGGL(seg_keys_kernel, dim3(met_grid(n_rows)), dim3(256), 0, stream, a, ka, va, gka, gva);
    int w = radix_sort_pairs<uint64_t, uint32_t>(ka, kb, va, vb, n_pred, 0, 64, true, sc.buf[TMP].p, stream);
    if (w < 0) { set_error("radix sort launch failed"); return VSC_ERR_HIP; }
    if (w) { std::swap(ka, kb); std::swap(va, vb); }  // ka: keys by rank, va: rank -> row
    const int pair_bits = met_bits_for((uint64_t)n_pairs);  // (the key n_pairs itself marks rows of no pair)
    if (n_pred > 0) hipLaunchKernelGGL(seg_rank_pairs_kernel, dim3(met_grid(n_pred)), dim3(256), 0, stream, a, va, pka, pva);
    w = radix_sort_pairs<uint32_t, uint32_t>(pka, pkb, pva, pvb, n_pred, 0, pair_bits, false, sc.buf[TMP].p, stream);
    if (w < 0) { set_error("radix sort launch failed"); return VSC_ERR_HIP; }
    if (w) { std::swap(pka, pkb); std::swap(pva, pvb); }
    w = radix_sort_pairs<uint32_t, uint32_t>(gka, gkb, gva, gvb, n_gt, 0, pair_bits, false, sc.buf[TMP].p, stream);
    if (w < 0) { set_error("radix sort launch failed"); return VSC_ERR_HIP; }
    if (w) { std::swap(gka, gkb); std::swap(gva, gvb); }
    uint32_t* pstart = sc.buf[BOUNDS].as<uint32_t>();
    uint32_t* gstart = pstart + (n_pairs + 1);
    hipLaunchKernelGGL(seg_bounds_kernel, dim3(met_grid(n_pairs + 1)), dim3(256), 0, stream, pka, n_pred, gka, n_gt, n_pairs, pstart, gstart);
    VSC_HIP(hipGetLastError());
    tm_sort.end(stream);
    a.rank_row = va; a.pos_rank = pva; a.gpos_row = gva; a.pstart = pstart; a.gstart = gstart;

    tm_pair.begin(stream);
    if (n_pairs > 0) hipLaunchKernelGGL(seg_pair_kernel<false>, dim3((unsigned)n_pairs), dim3(64), 0, stream, a);
    VSC_HIP(hipGetLastError());
    int64_t ctl[8] = {};
    VSC_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, stream));
    VSC_HIP(hipStreamSynchronize(stream));
    const int64_t n_big = ctl[0], big_items = ctl[1];
    if (!ctl[2] && n_big > 0) {
        if (n_big > big_cap || big_items > n_pred + n_gt) {
            set_error("vsc_match_metric: inconsistent work list (%lld pairs, %lld items)", (long long)n_big, (long long)big_items);
            return VSC_ERR_HIP;
        }
        VSC_TRY(sc.buf[SLAB].reserve((size_t)big_items * 44 + 64));
        a.slab_items = big_items;
        a.slab_t = sc.buf[SLAB].as<double>();
        a.slab_tag = reinterpret_cast<int32_t*>(a.slab_t + big_items * 4);
        a.slab_perm = reinterpret_cast<uint32_t*>(a.slab_tag + big_items);
        hipLaunchKernelGGL(seg_pair_kernel<true>, dim3((unsigned)n_big), dim3(64), 0, stream, a);
        VSC_HIP(hipGetLastError());
    }
    tm_pair.end(stream);

    tm_acc.begin(stream);
    double* gord = sc.buf[GTORD].as<double>();
    if (!ctl[2]) {
        if (n_gtp > 0) {
            hipLaunchKernelGGL(seg_gather_len_kernel, dim3(met_grid(n_gtp)), dim3(256), 0, stream, a.gt_len, n_pairs, in.gt_first, n_gtp,
                               gord, a.ctl);
            hipLaunchKernelGGL(seg_accumulate_kernel<2>, dim3(1), dim3(256), 0, stream, gord, n_gtp, (const uint64_t*)nullptr,
                               sc.buf[OGT].as<double>(), (double*)nullptr, (int64_t)1, a.ctl + 5);
        }
        if (n_pred > 0)
            hipLaunchKernelGGL(seg_accumulate_kernel<4>, dim3(1), dim3(256), 0, stream, a.deltas, n_pred, ka, sc.buf[OSUM].as<double>(),
                               sc.buf[OSCORE].as<double>(), std::min(out.cap, n_pred), a.ctl + 4);
        VSC_HIP(hipGetLastError());
    }
    tm_acc.end(stream);
    VSC_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, stream));
    VSC_HIP(hipStreamSynchronize(stream));
    out.stats[4] = tm_sort.microseconds();
    out.stats[5] = tm_pair.microseconds();
    out.stats[6] = tm_acc.microseconds();
    out.stats[7] = 0;
    if (ctl[2]) {
        const unsigned e = (unsigned)ctl[2];
        set_error("vsc_match_metric: %s", (e & 1u) ? "a prediction row has a pair ordinal out of range"
                                          : (e & 2u) ? "a ground-truth row (or the ground-truth pair list) has a pair ordinal out of range"
                                          : (e & 4u) ? "a score is not finite"
                                          : (e & 8u) ? "a time is not finite, or an end lies before its start"
                                                     : "a pair has more than VSC_METRIC_MAX_PAIR_ROWS = 8192 rows");
        return VSC_ERR_INVALID;
    }
    const int64_t groups = ctl[4];
    out.n_groups = groups;
    out.stats[0] = n_pairs - n_big;
    out.stats[1] = n_big;
    out.stats[2] = n_pred;
    out.stats[3] = groups;
    if (groups > out.cap) {
        set_error("vsc_match_metric: output capacity %lld < %lld groups", (long long)out.cap, (long long)groups);
        return VSC_ERR_CAPACITY;
    }
    VSC_HIP(hipMemcpyAsync(out.gt_len, sc.buf[OGT].p, 16, hipMemcpyDeviceToHost, stream));
    if (groups > 0) {
        VSC_HIP(hipMemcpyAsync(out.scores, sc.buf[OSCORE].p, (size_t)groups * 8, hipMemcpyDeviceToHost, stream));
        VSC_HIP(hipMemcpyAsync(out.sums, sc.buf[OSUM].p, (size_t)groups * 32, hipMemcpyDeviceToHost, stream));
    }
    VSC_HIP(hipStreamSynchronize(stream));
    return VSC_OK;
}

}  // namespace vscmi
