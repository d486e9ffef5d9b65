// The exact stage of the thresholded and k-NN searches (gfx950): what every pre-filter route (sim_f16.hip,
// sim_f16p.hip, sim_i8p.hip) hands its candidate list to.
//
//   rescore_kernel        four lanes per candidate run the exact ascending-k fp32 fma chain on the packed fp32 rows
//                         (or the SQfp16 store), the running sum hopping between them (one 128-byte line per row and
//                         load), over the segments and the tail of a candidate list.  HBM/L2-bound: 8*dpad bytes
//                         per candidate.
//   cand_count / cand_compact   the list's length / its entries as one dense (ref, row) list for the sort by reference row
//   f16_screen_kernel     fp16 screen between the int8 pre-filter and the exact stage
//   rescore_dense_kernel  the same chain over a dense (sorted, screened) list
#include <algorithm>

#include "prefilter_dev.h"

namespace vscmi {

// acc = fmaf(q[k], r[k], acc), k ascending from +0 (the arithmetic contract of the engine; packed rows hold
// every group of 8 k as [k0 k2 k4 k6 | k1 k3 k5 k7]).  The chain is serial, but nothing says it must stay
// in one lane: FOUR lanes share a candidate.  In every round of 32 k, lane g of the quad loads the g-th
// 32-byte group of both rows (so one load instruction touches one full 128-byte line per candidate and
// row instead of four different lines), and the running sum hops from lane to lane with a quad-rotate
// DPP move: lane 0 does k 0-7, hands over to lane 1 for k 8-15, ... and lane 3 hands back to lane 0 for the
// next round.  Every lane executes every step (the other three results are discarded), which costs 4x
// the fma issue slots of a chain that needs ~3 % of the VALU anyway; the kernel is bound by row traffic.
__device__ __forceinline__ float quad_rotate(float v) {  // lane g of every quad receives lane (g - 1) & 3
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x93, 0xf, 0xf, true));
}

// Hits are collected per wave in LDS and appended to the global list 49-64 at a time: one atomic on the
// (single, hot) list counter per flush instead of one per 16 candidates.
struct WaveHits {
    int i[64];
    int j[64];
    float s[64];
};

__device__ __forceinline__ void flush_hits(const RescoreArgs& a, WaveHits& buf, int& pend) {
    if (pend == 0) return;
    const int lane = threadIdx.x & 63;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes are visible to its other lanes
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(a.counter, (unsigned long long)pend);
    base = __shfl(base, 0);
    if ((long long)(base + pend) > a.cap) {
        if (lane == 0) atomicOr(a.list.overflow, 1);
    } else if (lane < pend) {
        a.out_i[base + lane] = buf.i[lane];
        a.out_j[base + lane] = buf.j[lane];
        a.out_s[base + lane] = buf.s[lane];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the buffer is refilled
    pend = 0;
}

// one 16-byte piece of the fp16 store (k ascending) -> the even / odd operands of the packed query's group of 8
__device__ __forceinline__ void half_piece(const f16x8 h, f32x4& even, f32x4& odd) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        even[s] = (float)h[2 * s];
        odd[s] = (float)h[2 * s + 1];
    }
}

// candidates of one list; thread x serves candidate x >> 2 (x0 = first thread index, `step` threads apart)
// SRC: where the reference row comes from -- 0 the packed fp32 image (Flat codec), 1 / 2 the SQfp16 store in natural /
// fragment-major layout.  The store keeps natural k order inside a 16-byte piece: lane g's piece of round rd
// (k = 32 rd + 8 g .. + 7) is ONE 16-byte load, its even / odd halves are the operands of the packed query's
// [k0 k2 k4 k6 | k1 k3 k5 k7]; the conversions are exact and the chain is the same.
template <int SRC>
__device__ __forceinline__ void rescore_list(const RescoreArgs& a, float radius, const int32_t* ci,
                                             const int32_t* cj, long long n, long long x0, long long step,
                                             WaveHits& buf, int& pend, const int* fill = nullptr, int shift = 0) {
    const int lane = threadIdx.x & 63, g = lane & 3;
    const long long n_thr = (4 * n + 63) & ~63ll;  // whole waves stay together (DPP, ballot)
    const int rounds = a.dpad / 32;
    for (long long x = x0; x < n_thr; x += step) {
        const long long c = x >> 2;
        // (the tail is a sequence of chunks, each filled up to its own level: cand_list.h)
        const bool valid = c < n && (fill == nullptr || (int)(c & ((1ll << shift) - 1)) < fill[c >> shift]);
        int i = valid ? ci[c] : 0;
        const int j = valid ? cj[c] + a.j0 : 0;
        if (a.perm && valid) i = a.perm_i0 + a.perm[i - a.perm_i0];  // position inside a permuted int8 launch -> row
        const f32x4* q = reinterpret_cast<const f32x4*>(a.Q + (int64_t)i * a.dpad) + 2 * g;
        const f32x4* r = reinterpret_cast<const f32x4*>(a.R + (int64_t)j * a.dpad) + 2 * g;
        // (fp16 store: piece 4 rd + g of row j; fragment-major pieces of one row lie 512 B / 2 KiB apart)
        // The fragment-major index is frag_piece(j, g, a.dpadh) (kernels.h), written out: through the function the two
        // SRC == 2 kernels came out with other registers and instructions (profiles/prefilter_dev_refactor.md).
        const f16x8* rh = reinterpret_cast<const f16x8*>(a.Rh) +
                            (SRC == 2 ? (int64_t)(j >> 6) * (a.dpadh / 16) * 128 + ((j >> 5) & 1) * 64 + (j & 31) + (g >> 1) * 128 + (g & 1) * 32
                                      : (int64_t)j * (a.dpadh / 8) + g);
        constexpr int RH_STEP = SRC == 2 ? 256 : 4;  // pieces between two rounds of one lane
        float acc = 0.0f;  // the live value sits in lane 0 of the quad at the top of every round
        f32x4 qe = q[0], qo = q[1], re, ro;
        if constexpr (SRC == 0) {
            re = r[0];
            ro = r[1];
        } else {
            half_piece(rh[0], re, ro);
        }
        for (int rd = 0; rd < rounds; ++rd) {
            const int nx = rd + 1 < rounds ? rd + 1 : rd;  // prefetch the next round's groups
            const f32x4 nqe = q[8 * nx], nqo = q[8 * nx + 1];
            f32x4 nre, nro;
            f16x8 nrh;
            if constexpr (SRC == 0) {
                nre = r[8 * nx];
                nro = r[8 * nx + 1];
            } else {
                nrh = rh[(int64_t)RH_STEP * nx];
            }
#pragma unroll
            for (int gp = 0; gp < 4; ++gp) {
                float v = acc;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    v = __fmaf_rn(qe[s], re[s], v);
                    v = __fmaf_rn(qo[s], ro[s], v);
                }
                const float passed = quad_rotate(v);  // lane gp's (the only meaningful) v -> lane gp + 1
                acc = (g == ((gp + 1) & 3)) ? passed : acc;
            }
            qe = nqe;
            qo = nqo;
            if constexpr (SRC == 0) {
                re = nre;
                ro = nro;
            } else {
                half_piece(nrh, re, ro);
            }
        }
        const bool hit = valid && g == 0 && (a.row_thr ? acc >= a.row_thr[i] : acc > radius);
        const unsigned long long m = __ballot(hit);  // <= 16 hits per pass
        if (hit) {
            const int p = pend + __popcll(m & ((1ull << lane) - 1));
            buf.i[p] = i;
            buf.j[p] = j;
            buf.s[p] = acc;
        }
        pend += __popcll(m);
        if (pend > 48) flush_hits(a, buf, pend);
    }
}

#ifndef VSC_RESCORE_SHARE
#define VSC_RESCORE_SHARE 4
#endif
constexpr int RESCORE_SHARE = VSC_RESCORE_SHARE;

template <int SRC>
__global__ __launch_bounds__(256) void rescore_kernel(RescoreArgs a) {
    // After an overflow the candidate list has holes (a wave whose tail reservation did not fit skipped its
    // writes but the tail counter moved on): the host reruns the search with larger buffers, so do nothing
    // rather than chase unwritten (row, ref) pairs through memory.
    if (*a.list.overflow) return;
    __shared__ WaveHits wave_hits[4];
    WaveHits& buf = wave_hits[threadIdx.x >> 6];
    int pend = 0;
    const float radius = a.row_thr ? 0.0f : *a.radius;
    unsigned long long seen = 0;
    // RESCORE_SHARE workgroups walk one segment together (the segments fill unevenly: more, smaller pieces balance
    // better and keep more loads in flight)
    {
        const int seg = blockIdx.x / RESCORE_SHARE, part = blockIdx.x % RESCORE_SHARE;
        const int n = min(a.list.seg_count[seg], a.list.seg_cap);
        if (part == 0) seen += (unsigned long long)n;
        rescore_list<SRC>(a, radius, a.list.i + (int64_t)seg * a.list.seg_cap, a.list.j + (int64_t)seg * a.list.seg_cap, n,
                     part * 256 + threadIdx.x, 256 * RESCORE_SHARE, buf, pend);
    }
    // shared tail (normally empty)
    const unsigned long long nt_all = *a.list.tail_count;
    const long long nt = nt_all < (unsigned long long)a.list.tail_cap ? (long long)nt_all : a.list.tail_cap;
    if (nt > 0) {
        rescore_list<SRC>(a, radius, a.list.i + a.list.tail_base, a.list.j + a.list.tail_base, nt,
                     (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, buf, pend, a.list.tail_fill,
                     a.list.tail_shift);
        if (blockIdx.x == 0) seen += (unsigned long long)nt;
    }
    flush_hits(a, buf, pend);
    if (threadIdx.x == 0 && seen) atomicAdd(a.n_cand_total, seen);
}

__global__ void tail_reset_kernel(unsigned long long* tail_count) { *tail_count = 0; }

// ---- candidates ordered by reference row
// The candidates of a launch hit every reference row several times (int8 batches of the search: ~4 x, k-NN passes:
// 10-80 x).  Compacted out of the waves' segments and sorted by reference row, the chains of one reference row sit in
// neighbouring lanes: their loads of that row are one cache line request instead of several, and the row comes out of
// HBM once.  cand_compact: one workgroup per segment / tail chunk, dense position by one atomic per workgroup (the
// order inside the dense list does not matter: it is sorted next).
__global__ __launch_bounds__(256) void cand_compact_kernel(RescoreArgs a, uint32_t* __restrict__ key_j,
                                                           uint32_t* __restrict__ val_i, unsigned long long* n_out) {
    __shared__ unsigned long long base_sh;
    if (*a.list.overflow) return;
    const int b = blockIdx.x;
    const int32_t *ci, *cj;
    int n;
    if (b < a.list.n_seg) {
        n = min(a.list.seg_count[b], a.list.seg_cap);
        ci = a.list.i + (int64_t)b * a.list.seg_cap;
        cj = a.list.j + (int64_t)b * a.list.seg_cap;
    } else {
        const long long chunk = b - a.list.n_seg;
        const unsigned long long nt = *a.list.tail_count;
        if ((unsigned long long)(chunk << a.list.tail_shift) >= nt || (long long)nt > a.list.tail_cap) return;
        n = a.list.tail_fill[chunk];
        ci = a.list.i + a.list.tail_base + (chunk << a.list.tail_shift);
        cj = a.list.j + a.list.tail_base + (chunk << a.list.tail_shift);
    }
    if (n <= 0) return;
    if (a.d_i) {
        // a list written with a floor (deferred rescoring): entries with DEFER_MARK join the deferred set D -- (row,
        // absolute ref), any order, no score --, the others the dense list.  Two walks over the (L2-resident) segment:
        // the marked entries are counted first, so that the workgroup still takes one position per list
        __shared__ unsigned int marked_sh, cur_sh[2];
        __shared__ unsigned long long base_d_sh;
        if (threadIdx.x == 0) { marked_sh = 0; cur_sh[0] = 0; cur_sh[1] = 0; }
        __syncthreads();
        unsigned int mine = 0;
        for (int x = threadIdx.x; x < n; x += 256) mine += (uint32_t)ci[x] >> 31;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&marked_sh, mine);
        __syncthreads();
        const unsigned int nm = marked_sh;
        if (threadIdx.x == 0) {
            base_sh = atomicAdd(n_out, (unsigned long long)(n - (int)nm));
            base_d_sh = nm ? atomicAdd(a.d_count, (unsigned long long)nm) : 0ull;
            if (nm) {
                atomicAdd(a.d_total, (unsigned long long)nm);
                atomicAdd(a.n_cand_total, (unsigned long long)nm);  // (the dense list's share is added by its re-scoring)
            }
        }
        __syncthreads();
        const unsigned long long base = base_sh, base_d = base_d_sh;
        // (D is as large as the kept-hit list: a full D means the kept hits -- scored + deferred -- outgrew it)
        const bool d_fits = (long long)(base_d + nm) <= a.d_cap;
        if (!d_fits && threadIdx.x == 0) atomicOr(a.list.overflow, 1);
        const int lane = threadIdx.x & 63;
        for (int x0 = 0; x0 < n; x0 += 256) {
            const int x = x0 + threadIdx.x;
            const bool valid = x < n;
            const uint32_t v = valid ? (uint32_t)ci[x] : 0u;
            const bool marked = valid && (v & DEFER_MARK) != 0u, plain = valid && !marked;
            const unsigned long long bm = __ballot(marked), bp = __ballot(plain);
            unsigned int pm = 0, pp = 0;
            if (lane == 0) {
                if (bm) pm = atomicAdd(&cur_sh[1], (unsigned int)__popcll(bm));
                if (bp) pp = atomicAdd(&cur_sh[0], (unsigned int)__popcll(bp));
            }
            pm = __shfl(pm, 0);
            pp = __shfl(pp, 0);
            int i = (int)(v & ~DEFER_MARK);
            if (a.perm && valid) i = a.perm_i0 + a.perm[i - a.perm_i0];
            if (plain) {
                const unsigned long long p = base + pp + lanes_below(bp);
                key_j[p] = (uint32_t)(cj[x] + a.j0);
                val_i[p] = (uint32_t)i;
            } else if (marked && d_fits) {
                const unsigned long long p = base_d + pm + lanes_below(bm);
                a.d_i[p] = i;
                a.d_j[p] = cj[x] + a.j0;
            }
        }
        return;
    }
    if (threadIdx.x == 0) base_sh = atomicAdd(n_out, (unsigned long long)n);
    __syncthreads();
    const unsigned long long base = base_sh;
    for (int x = threadIdx.x; x < n; x += 256) {
        int i = ci[x];
        if (a.perm) i = a.perm_i0 + a.perm[i - a.perm_i0];  // position inside a permuted int8 launch -> row
        key_j[base + x] = (uint32_t)(cj[x] + a.j0);
        val_i[base + x] = (uint32_t)i;
    }
}

// fp16 screen between the int8 pre-filter and the exact stage.  The int8 bound is wide (one scale per row / panel:
// ~5-10 candidates per pair that really reaches the threshold); the fp16 bound is ~30x narrower, and an fp16 row is
// half the bytes of the fp32 row the exact stage gathers.  One candidate per quad: lane g takes the 16-byte pieces
// g, g + 4, ... of both rows (any summation order is inside the bound: products of two fp16 values are exact in fp32,
// each fma rounds once), the quad's sum is compared like the fp16 pre-filter compares its scores
// (prefilter_dev.h: candidate_edge).  Survivors are collected per wave in LDS and appended 49-64 at a time; the
// list stays (roughly) in reference-row order.
struct WavePairs {
    uint32_t i[64];
    uint32_t j[64];
};

// With a floor (deferred rescoring, ScreenArgs::floor) the screen has three outcomes: drop (as before: the pair cannot
// exceed the radius), defer (its exact score is proven to lie in (radius, floor]: it joins the deferred set D, score-less)
// and exact (everything else: the survivors).
template <bool FRAG>
__global__ __launch_bounds__(256) void f16_screen_kernel(ScreenArgs a) {
    if (*a.overflow) return;
    __shared__ WavePairs wave_pairs[4], wave_defer[4];
    WavePairs& buf = wave_pairs[threadIdx.x >> 6];
    WavePairs& dbuf = wave_defer[threadIdx.x >> 6];
    int pend = 0, dpend = 0;
    const int lane = threadIdx.x & 63, g = lane & 3;
    const long long n_thr = (4 * a.n + 63) & ~63ll;
    const int npiece = a.dpadh / 8, nks = a.dpadh / 16;
    const float radius = a.row_thr ? 0.0f : *a.radius;
    const float floor_v = !a.row_thr && a.floor ? *a.floor : INFINITY;
    const bool defer_on = floor_v < INFINITY;
    const f16x8* __restrict__ Rp = reinterpret_cast<const f16x8*>(a.Rh);
    auto flush = [&]() {
        if (pend == 0) return;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.n_out, (unsigned long long)pend);
        base = __shfl(base, 0);
        if (lane < pend) {
            a.out_i[base + lane] = buf.i[lane];
            a.out_j[base + lane] = buf.j[lane];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pend = 0;
    };
    auto flush_defer = [&]() {
        if (dpend == 0) return;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        unsigned long long base = 0;
        if (lane == 0) {
            base = atomicAdd(a.d_count, (unsigned long long)dpend);
            atomicAdd(a.d_total, (unsigned long long)dpend);
        }
        base = __shfl(base, 0);
        if ((long long)(base + dpend) > a.d_cap) {
            if (lane == 0) atomicOr(a.overflow, 1);
        } else if (lane < dpend) {
            a.d_i[base + lane] = (int32_t)dbuf.i[lane];
            a.d_j[base + lane] = (int32_t)dbuf.j[lane];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        dpend = 0;
    };
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < n_thr; x += (long long)gridDim.x * 256) {
        const long long c = x >> 2;
        const bool valid = c < a.n;
        const uint32_t i = valid ? a.si[c] : 0u, j = valid ? a.sj[c] : 0u;
        const f16x8* __restrict__ q = reinterpret_cast<const f16x8*>(a.Qh + (int64_t)i * a.dpadh);
        // (FRAG: frag_piece(j, p, a.dpadh) of kernels.h, written out like in rescore_list -- the row's part once per
        // candidate, the piece's part per load)
        const int64_t rbase = FRAG ? (int64_t)(j >> 6) * nks * 128 + ((j >> 5) & 1) * 64 + (j & 31)
                                   : (int64_t)j * npiece;
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll 8
        for (int p = g; p < npiece; p += 4) {
            const f16x8 qv = q[p];
            const f16x8 rv = FRAG ? Rp[rbase + (int64_t)(p >> 1) * 128 + (p & 1) * 32] : Rp[rbase + p];
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                s0 = __fmaf_rn((float)qv[e], (float)rv[e], s0);
                s1 = __fmaf_rn((float)qv[e + 1], (float)rv[e + 1], s1);
            }
        }
        float acc = s0 + s1;
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        const float eps = (a.c1 * a.qn[i] * a.rn[j] + a.c2 * (a.qn[i] + a.rn[j]) + a.c3) * 1.001f;
        bool pass = valid && g == 0 &&
                    (!(eps < INFINITY) || (a.row_thr ? acc >= candidate_edge(a.row_thr[i], eps) : acc > candidate_edge(radius, eps)));
        if (defer_on) {
            // exact >= acc - eps > radius and exact <= acc + eps <= floor, the sums' own roundings taken off as in
            // candidate_edge (an infinite or NaN bound: no score lies in the band)
            const float lo = (radius + eps) + 2.4e-7f * (fabsf(radius) + eps);
            const bool defer = pass && acc > lo && acc <= candidate_edge(floor_v, eps);
            pass = pass && !defer;
            const unsigned long long md = __ballot(defer);
            if (defer) {
                const int p = dpend + __popcll(md & ((1ull << lane) - 1));
                dbuf.i[p] = i;
                dbuf.j[p] = j;
            }
            dpend += __popcll(md);
            if (dpend > 48) flush_defer();
        }
        const unsigned long long m = __ballot(pass);  // <= 16 per pass
        if (pass) {
            const int p = pend + __popcll(m & ((1ull << lane) - 1));
            buf.i[p] = i;
            buf.j[p] = j;
        }
        pend += __popcll(m);
        if (pend > 48) flush();
    }
    flush();
    flush_defer();
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.n_cand_total, (unsigned long long)a.n);
}

int launch_f16_screen(const ScreenArgs& a, hipStream_t stream) {
    VSC_HIP(hipMemsetAsync(a.n_out, 0, sizeof(unsigned long long), stream));
    if (a.n > 0) {
        const unsigned grid = (unsigned)std::min<long long>(16384, (a.n * 4 + 255) / 256);
        if (a.frag) hipLaunchKernelGGL(f16_screen_kernel<true>, dim3(grid), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(f16_screen_kernel<false>, dim3(grid), dim3(256), 0, stream, a);
        VSC_HIP(hipGetLastError());
    }
    return VSC_OK;
}

// n_dev: the list's length lives on the device (the fp16 screen's survivors; n = an upper bound for the grid)
template <int SRC>
__global__ __launch_bounds__(256) void rescore_dense_kernel(RescoreArgs a, const uint32_t* __restrict__ sj,
                                                            const uint32_t* __restrict__ si, long long n,
                                                            const unsigned long long* __restrict__ n_dev) {
    if (*a.list.overflow) return;
    if (n_dev) n = (long long)*n_dev;
    __shared__ WaveHits wave_hits[4];
    WaveHits& buf = wave_hits[threadIdx.x >> 6];
    int pend = 0;
    const float radius = a.row_thr ? 0.0f : *a.radius;
    a.perm = nullptr;  // (rows already)
    a.j0 = 0;          // (absolute reference rows already: cand_compact added the launch's offset)
    rescore_list<SRC>(a, radius, reinterpret_cast<const int32_t*>(si), reinterpret_cast<const int32_t*>(sj), n,
                 (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256, buf, pend);
    flush_hits(a, buf, pend);
    if (blockIdx.x == 0 && threadIdx.x == 0 && !n_dev) atomicAdd(a.n_cand_total, (unsigned long long)n);
}

// How many candidates a launch left in its segments and tail chunks (one workgroup): the host sizes the dense lists
// of the sort from this number instead of from the list's capacity (round 4: 4 x 16 bytes per unit of CAPACITY went to
// buffers that a launch fills to a few percent).  An overflowed launch counts 0 (nothing of it is re-scored).
__global__ __launch_bounds__(1024) void cand_count_kernel(RescoreArgs a, int n_chunks_max, unsigned long long* n_out) {
    __shared__ unsigned long long red[16];
    unsigned long long s = 0;
    if (!*a.list.overflow) {
        for (int b = threadIdx.x; b < a.list.n_seg; b += 1024) s += (unsigned long long)max(0, min(a.list.seg_count[b], a.list.seg_cap));
        const unsigned long long nt = *a.list.tail_count;
        if ((long long)nt <= a.list.tail_cap) {
            const long long used = (long long)((nt + (1ull << a.list.tail_shift) - 1) >> a.list.tail_shift);
            for (long long c = threadIdx.x; c < used && c < n_chunks_max; c += 1024) s += (unsigned long long)max(0, a.list.tail_fill[c]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < 16; ++w) t += red[w];
        *n_out = t;
    }
}

int launch_cand_count(const RescoreArgs& a, int n_chunks_max, unsigned long long* n_out, hipStream_t stream) {
    hipLaunchKernelGGL(cand_count_kernel, dim3(1), dim3(1024), 0, stream, a, n_chunks_max, n_out);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

int launch_cand_compact(const RescoreArgs& a, int n_chunks_max, uint32_t* key_j, uint32_t* val_i, unsigned long long* n_out,
                        hipStream_t stream) {
    VSC_HIP(hipMemsetAsync(n_out, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(cand_compact_kernel, dim3((unsigned)(a.list.n_seg + n_chunks_max)), dim3(256), 0, stream, a, key_j, val_i, n_out);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

int launch_rescore_dense(const RescoreArgs& a, const uint32_t* sj, const uint32_t* si, long long n, hipStream_t stream,
                         const unsigned long long* n_dev) {
    if (n > 0) {
        const unsigned grid = (unsigned)std::min<long long>(16384, (n * 4 + 255) / 256);
        if (a.rsrc == 0) hipLaunchKernelGGL(rescore_dense_kernel<0>, dim3(grid), dim3(256), 0, stream, a, sj, si, n, n_dev);
        else if (a.rsrc == 1) hipLaunchKernelGGL(rescore_dense_kernel<1>, dim3(grid), dim3(256), 0, stream, a, sj, si, n, n_dev);
        else hipLaunchKernelGGL(rescore_dense_kernel<2>, dim3(grid), dim3(256), 0, stream, a, sj, si, n, n_dev);
    }
    hipLaunchKernelGGL(tail_reset_kernel, dim3(1), dim3(1), 0, stream, a.list.tail_count);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

int launch_rescore(const RescoreArgs& a, hipStream_t stream) {
    if (a.list.n_seg <= 0) return VSC_OK;
    const dim3 grid((unsigned)a.list.n_seg * RESCORE_SHARE);
    if (a.rsrc == 0) hipLaunchKernelGGL(rescore_kernel<0>, grid, dim3(256), 0, stream, a);
    else if (a.rsrc == 1) hipLaunchKernelGGL(rescore_kernel<1>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(rescore_kernel<2>, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(tail_reset_kernel, dim3(1), dim3(1), 0, stream, a.list.tail_count);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

}  // namespace vscmi
