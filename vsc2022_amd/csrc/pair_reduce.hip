// (query video, ref video) aggregation of a hit list by max, sum, mean or the mean of the m best (gfx950, wave64):
// vsc_pair_aggregate / vsc_index_candidates_agg -- the regroup loop of VideoIndex.search (vsc/index.py:121-140) fused with a
// ScoreAggregation (vsc/candidates.py:14-26) and the stable descending sort of CandidateGeneration.query
// (vsc/candidates.py:36-40), for the aggregations sortpairs.hip's pair_max cannot shortcut.
//
// The contract (include/vscmi.h): per pair, d = its hit scores as float64 sorted descending;
//   max = the largest fp32 score; sum = float32(((0.0 + d_1) + d_2) + ...), ONE float64 add per hit, in that order;
//   mean = float32(that / c); topmean(m) = the same chain over the first min(m, c) entries / min(m, c).
// The order of the adds IS the contract: no atomics, no butterfly, no tree -- one lane walks one run.
//
// Launches:
//   pa_score_keys     (hits in any order, not for max) score keys + ranks, then ONE stable radix sort by score descending:
//                     every later stable sort keeps each pair's hits score-descending;
//   pa_key            pair key (query video << 32 | ref video) of every hit in that order + the largest ordinals (they
//                     bound the key bits the sort looks at); a hit row outside the maps raises the error word and gets
//                     no key from the maps -- nothing is read outside the tables whatever the list holds;
//   radix sort        stable, by pair key: one contiguous score-descending run per pair;
//   pa_heads          first position of every run, compacted (order of the compaction: irrelevant, see pa_reduce);
//   pa_reduce         ONE LANE PER PAIR walks its run: the float64 chain, the max by key, the hit count and the smallest
//                     rank (= first appearance in the caller's list); emits the final sort key
//                     (~key(score + 0.0f) << 32 | first rank);
//   radix sort        by that key: score descending with -0.0 == +0.0, ties in first-appearance order -- what Python's
//                     stable sort makes of the dict-ordered pairs;
//   pa_out            gathers the columns in that order.
//
// What bounds it: the two sorts are the HBM-bound plumbing of radix.h (12 B per hit and pass).  pa_reduce is bound by the
// LATENCY of its dependent gathers, not by bytes or adds: per hit a lane reads key[x] and rank[x] (coalesced across the
// lanes only where neighbouring runs are short) and then hs[rank[x]], a 4-byte gather whose address depends on the load
// before it (~900 cycles on an HBM miss, ~545 from the Infinity Cache) before one 64-bit add; a run of c hits is c such
// round trips on one lane, and a wave lasts as long as its longest run.  Occupancy (8 waves per SIMD of independent
// chains) is what hides it; a pair with thousands of hits is still one sequential chain -- accepted, the order is the
// contract.  Measured times: profiles/candidates_agg.md.
#include <utility>

#include "kernels.h"
#include "radix.h"

namespace vscmi {

namespace {

inline unsigned pa_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

int pa_bits(uint64_t maxval) {
    int b = 1;
    while (b < 64 && (maxval >> b)) ++b;
    return b;
}

// control words: [0] number of pairs, [1] error word, [2] largest query-video ordinal (low word), [3] ... ref-video
constexpr int PA_CTL_WORDS = 4;

}  // namespace

__global__ __launch_bounds__(256) void pa_score_keys_kernel(const float* __restrict__ hs, int64_t n, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ rank) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    keys[x] = f2key(hs[x] + 0.0f);   // (-0.0 == +0.0 in the stable score sort; the scores are read back through rank[])
    rank[x] = (uint32_t)x;
}

// `order`: the ranks in the order the keys are wanted in (nullptr: list order, and rank[] is written here)
__global__ __launch_bounds__(256) void pa_key_kernel(const int32_t* __restrict__ hi, const int32_t* __restrict__ hj,
                                                     const uint32_t* __restrict__ order, int64_t n,
                                                     const int32_t* __restrict__ row2q, int64_t nq_rows,
                                                     const int32_t* __restrict__ row2r, int64_t nr_rows,
                                                     uint64_t* __restrict__ key, uint32_t* __restrict__ rank,
                                                     unsigned long long* __restrict__ ctl) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned q = 0, r = 0;
    bool bad = false;
    if (x < n) {
        const uint32_t src = order ? order[x] : (uint32_t)x;
        const int64_t i = hi[src], j = hj[src];
        bad = i < 0 || i >= nq_rows || j < 0 || j >= nr_rows;
        if (!bad) {
            q = (unsigned)row2q[i];
            r = (unsigned)row2r[j];
        }
        key[x] = bad ? ~0ull : (((uint64_t)q << 32) | r);  // (a skipped hit: the call fails before the keys are sorted)
        if (!order) rank[x] = src;
    }
    // (no lane has left: the whole wave takes part in the shuffles)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        q = max(q, (unsigned)__shfl_xor((int)q, off));
        r = max(r, (unsigned)__shfl_xor((int)r, off));
    }
    const unsigned long long any_bad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        // a wave raises a maximum only where it would move it: one atomic per wave on a single word serialises the whole
        // launch (measured: 17.3 of 33 ms at 48 M hits), the relaxed look before it leaves a handful per launch
        unsigned* mq = reinterpret_cast<unsigned*>(ctl + 2);
        unsigned* mr = reinterpret_cast<unsigned*>(ctl + 3);
        if (q > __hip_atomic_load(mq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mq, q);
        if (r > __hip_atomic_load(mr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mr, r);
        if (any_bad) atomicOr(reinterpret_cast<unsigned*>(ctl + 1), 1u);
    }
}

__global__ __launch_bounds__(256) void pa_heads_kernel(const uint64_t* __restrict__ key, int64_t n, uint32_t* __restrict__ head_start,
                                                       unsigned long long* __restrict__ count) {
    // one atomic per workgroup on the (single) counter, as sortpairs.hip's pair_heads_kernel
    __shared__ unsigned int wave_cnt[4];
    __shared__ unsigned long long block_base;
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool head = (x < n) && (x == 0 || key[x] != key[x - 1]);
    const unsigned long long m = __ballot(head);
    if (lane == 0) wave_cnt[wave] = (unsigned int)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int tot = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        block_base = tot ? atomicAdd(count, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    if (head) {
        unsigned long long pos = block_base + __popcll(m & ((1ull << lane) - 1));
        for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
        head_start[pos] = (uint32_t)x;  // (pos < number of heads <= n)
    }
}

// one lane per pair: the run [head_start[p], ...) of equal keys, score-descending
__global__ __launch_bounds__(256) void pa_reduce_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ rank,
                                                        const float* __restrict__ hs, int64_t n,
                                                        const uint32_t* __restrict__ head_start, int64_t np, int agg, int64_t top_m,
                                                        float* __restrict__ res_s, uint32_t* __restrict__ res_first,
                                                        int32_t* __restrict__ res_cnt, uint64_t* __restrict__ key2,
                                                        uint32_t* __restrict__ val2) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    int64_t x = head_start[p];
    const uint64_t k = key[x];
    const int64_t lim = agg == VSC_AGG_TOPMEAN ? top_m : INT64_MAX;  // entries of the chain
    double acc = 0.0;
    uint32_t best = 0, first = 0xffffffffu;
    int64_t c = 0;
    do {
        const uint32_t r = rank[x];  // (< n: the ranks are a permutation of the list's positions)
        const float v = hs[r];
        first = min(first, r);
        if (agg == VSC_AGG_MAX) best = max(best, f2key(v));
        else if (c < lim) acc = acc + (double)v;  // one IEEE float64 add per hit, in run order
        ++c;
        ++x;
    } while (x < n && key[x] == k);
    float out;
    if (agg == VSC_AGG_MAX) out = key2f(best);
    else if (agg == VSC_AGG_SUM) out = (float)acc;
    else out = (float)(acc / (double)(c < lim ? c : lim));
    res_s[p] = out;
    res_first[p] = first;
    res_cnt[p] = (int32_t)c;
    key2[p] = ((uint64_t)(~f2key(out + 0.0f)) << 32) | first;  // ascending = score descending, then first appearance
    val2[p] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void pa_out_kernel(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ key,
                                                     const uint32_t* __restrict__ head_start, const float* __restrict__ res_s,
                                                     const uint32_t* __restrict__ res_first, const int32_t* __restrict__ res_cnt,
                                                     int64_t np, int32_t* __restrict__ out_q, int32_t* __restrict__ out_r,
                                                     float* __restrict__ out_s, int64_t* __restrict__ out_first,
                                                     int32_t* __restrict__ out_count) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= np) return;
    const uint32_t p = perm[x];
    const uint64_t k = key[head_start[p]];
    out_q[x] = (int32_t)(k >> 32);
    out_r[x] = (int32_t)(k & 0xffffffffu);
    out_s[x] = res_s[p];
    if (out_first) out_first[x] = (int64_t)res_first[p];
    if (out_count) out_count[x] = res_cnt[p];
}

// (row, rank) hit list of a k-NN result: row = slot / k, ref = the int64 id as int32 (k <= ntotal: no empty slot)
__global__ __launch_bounds__(256) void knn_to_hits_kernel(const int64_t* __restrict__ ids, int64_t n, int k, int32_t* __restrict__ hi,
                                                          int32_t* __restrict__ hj) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    hi[x] = (int32_t)(x / k);
    hj[x] = (int32_t)ids[x];  // (-1 of an empty slot stays -1: pa_key_kernel refuses it)
}

int launch_knn_to_hits(const int64_t* ids, int64_t nq, int k, int32_t* hi, int32_t* hj, hipStream_t stream) {
    const int64_t n = nq * k;
    if (n <= 0) return VSC_OK;
    hipLaunchKernelGGL(knn_to_hits_kernel, dim3(pa_grid(n)), dim3(256), 0, stream, ids, n, k, hi, hj);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

int pair_agg_check(const char* who, int agg, int64_t top_m) {
    if (agg != VSC_AGG_MAX && agg != VSC_AGG_SUM && agg != VSC_AGG_MEAN && agg != VSC_AGG_TOPMEAN) {
        set_error("%s: unknown aggregation %d (VSC_AGG_MAX, _SUM, _MEAN, _TOPMEAN)", who, agg);
        return VSC_ERR_INVALID;
    }
    if (agg == VSC_AGG_TOPMEAN && top_m < 1) {
        set_error("%s: VSC_AGG_TOPMEAN needs top_m >= 1 (got %lld)", who, (long long)top_m);
        return VSC_ERR_INVALID;
    }
    return VSC_OK;
}

// All pointers device.  Synchronises the stream twice (the key bits and the error word; the pair count).
int pair_aggregate_device(const int32_t* hi, const int32_t* hj, const float* hs, int64_t n, const int32_t* row2q,
                          const int32_t* row2r, int64_t nq_rows, int64_t nr_rows, int hits_order, int agg, int64_t top_m,
                          SortScratch& sc, PairAggScratch& pa, int32_t* out_q, int32_t* out_r, float* out_s, int64_t* out_first,
                          int32_t* out_count, int64_t cap, int64_t* n_pairs, hipStream_t stream) {
    *n_pairs = 0;
    VSC_TRY(pair_agg_check("pair_aggregate", agg, top_m));
    if (n <= 0) return VSC_OK;
    if (n > 0x7fffffffLL) {
        set_error("pair_aggregate: more than 2^31 - 1 hits");
        return VSC_ERR_INVALID;
    }
    VSC_TRY(sc.w0.reserve(sizeof(uint64_t) * n));
    VSC_TRY(sc.w1.reserve(sizeof(uint64_t) * n));
    VSC_TRY(sc.w2.reserve(sizeof(uint32_t) * n));
    VSC_TRY(sc.w3.reserve(sizeof(uint32_t) * n));
    VSC_TRY(sc.tmp.reserve(radix_tmp_bytes(n)));
    VSC_TRY(pa.ctl.reserve(sizeof(unsigned long long) * PA_CTL_WORDS));
    uint64_t* ka = sc.w0.as<uint64_t>();
    uint64_t* kb = sc.w1.as<uint64_t>();
    uint32_t* ra = sc.w2.as<uint32_t>();
    uint32_t* rb = sc.w3.as<uint32_t>();
    unsigned long long* ctl = pa.ctl.as<unsigned long long>();
    VSC_HIP(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * PA_CTL_WORDS, stream));
    const uint32_t* order = nullptr;
    if (!hits_order && agg != VSC_AGG_MAX) {
        // score descending first (the 32-bit score keys borrow the 64-bit key buffers, free until pa_key_kernel)
        uint32_t* sa = sc.w0.as<uint32_t>();
        uint32_t* sb = sc.w1.as<uint32_t>();
        hipLaunchKernelGGL(pa_score_keys_kernel, dim3(pa_grid(n)), dim3(256), 0, stream, hs, n, sa, ra);
        VSC_HIP(hipGetLastError());
        const int w = radix_sort_pairs<uint32_t, uint32_t>(sa, sb, ra, rb, n, 0, 32, true, sc.tmp.p, stream);
        if (w < 0) { set_error("radix sort launch failed"); return VSC_ERR_HIP; }
        if (w) std::swap(ra, rb);
        order = ra;
    }
    hipLaunchKernelGGL(pa_key_kernel, dim3(pa_grid(n)), dim3(256), 0, stream, hi, hj, order, n, row2q, nq_rows, row2r, nr_rows,
                       ka, ra, ctl);
    VSC_HIP(hipGetLastError());
    unsigned long long ch[PA_CTL_WORDS] = {0, 0, 0, 0};
    VSC_HIP(hipMemcpyAsync(ch, ctl, sizeof(ch), hipMemcpyDeviceToHost, stream));
    VSC_HIP(hipStreamSynchronize(stream));
    if (ch[1]) {
        set_error("pair_aggregate: a hit names a row outside the row -> video maps (%lld query rows, %lld reference rows)",
                  (long long)nq_rows, (long long)nr_rows);
        return VSC_ERR_INVALID;
    }
    // only the bits the largest ordinals occupy are sorted (sortpairs.hip, pair_max_device)
    const int bits_q = pa_bits(std::max<uint64_t>(ch[2] & 0xffffffffull, 1)), bits_r = pa_bits(std::max<uint64_t>(ch[3] & 0xffffffffull, 1));
    int w = radix_sort_pairs<uint64_t, uint32_t>(ka, kb, ra, rb, n, 0, bits_r, false, sc.tmp.p, stream, 32, 32 + bits_q);
    if (w < 0) { set_error("radix sort launch failed"); return VSC_ERR_HIP; }
    if (!w) { std::swap(ka, kb); std::swap(ra, rb); }  // sorted runs in (kb, rb); (ka, ra) are free
    uint32_t* head_start = ra;
    hipLaunchKernelGGL(pa_heads_kernel, dim3(pa_grid(n)), dim3(256), 0, stream, kb, n, head_start, ctl);
    VSC_HIP(hipGetLastError());
    unsigned long long np = 0;
    VSC_HIP(hipMemcpyAsync(&np, ctl, sizeof(np), hipMemcpyDeviceToHost, stream));
    VSC_HIP(hipStreamSynchronize(stream));
    *n_pairs = (int64_t)np;
    if ((int64_t)np > cap) {
        set_error("pair_aggregate: output capacity %lld < %llu pairs", (long long)cap, np);
        return VSC_ERR_CAPACITY;
    }
    if (np == 0 || np > (unsigned long long)n) {  // (n > 0 hits always make a pair)
        set_error("pair_aggregate: inconsistent pair count %llu for %lld hits", np, (long long)n);
        return VSC_ERR_HIP;
    }
    VSC_TRY(pa.k2.reserve(sizeof(uint64_t) * np));
    VSC_TRY(pa.v2a.reserve(sizeof(uint32_t) * np));
    VSC_TRY(pa.v2b.reserve(sizeof(uint32_t) * np));
    VSC_TRY(pa.rs.reserve(sizeof(float) * np));
    VSC_TRY(pa.rfirst.reserve(sizeof(uint32_t) * np));
    VSC_TRY(pa.rcnt.reserve(sizeof(int32_t) * np));
    uint64_t* k2a = ka;  // (n >= np entries, free since the pair sort)
    uint64_t* k2b = pa.k2.as<uint64_t>();
    uint32_t* v2a = pa.v2a.as<uint32_t>();
    uint32_t* v2b = pa.v2b.as<uint32_t>();
    hipLaunchKernelGGL(pa_reduce_kernel, dim3(pa_grid((int64_t)np)), dim3(256), 0, stream, kb, rb, hs, n, head_start, (int64_t)np, agg,
                       top_m, pa.rs.as<float>(), pa.rfirst.as<uint32_t>(), pa.rcnt.as<int32_t>(), k2a, v2a);
    VSC_HIP(hipGetLastError());
    w = radix_sort_pairs<uint64_t, uint32_t>(k2a, k2b, v2a, v2b, (int64_t)np, 0, pa_bits((uint64_t)n), false, sc.tmp.p, stream, 32, 64);
    if (w < 0) { set_error("radix sort launch failed"); return VSC_ERR_HIP; }
    hipLaunchKernelGGL(pa_out_kernel, dim3(pa_grid((int64_t)np)), dim3(256), 0, stream, w ? v2b : v2a, kb, head_start, pa.rs.as<float>(),
                       pa.rfirst.as<uint32_t>(), pa.rcnt.as<int32_t>(), (int64_t)np, out_q, out_r, out_s, out_first, out_count);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

}  // namespace vscmi
