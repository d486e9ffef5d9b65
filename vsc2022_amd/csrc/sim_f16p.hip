// Panel-stationary fp16 pre-filter of the thresholded searches (gfx950), dims <= 512.
//
// Same contract as sim_f16.hip (candidates = every pair whose fp16 score + rigorous error bound reaches the
// threshold; vsc/index.py:142-165 semantics are restored by the exact stage), different data flow:
//
//   * a 128-row QUERY PANEL (all of K: <= 128 KiB of fp16) sits in LDS for as long as a workgroup works on
//     it -- [k chunk of 128][row][16-byte slot ^ (row & 15)], conflict-free for the 32x32x16 A-fragment
//     reads (16 lanes of a ds_read_b128 phase = 16 rows with distinct row & 15 = all 64 banks);
//   * the REFERENCE rows stream straight into registers from a FRAGMENT-MAJOR fp16 image (layout.hip): the B
//     fragment of one MFMA is one fully coalesced 1 KiB buffer load, fetched PF-1 k-steps ahead into a
//     register ring.  No LDS-DMA, no barrier and no LDS write in the steady state;
//   * 8 waves; wave w owns all 128 panel rows x columns [64 w, 64 w + 64) of a 512-column step: 4 x 2 blocks
//     of v_mfma_f32_32x32x16_f16, 128 accumulator registers, 2 waves per SIMD;
//   * work = (panel, slice of reference col-steps) items behind one atomic counter per panel.  A workgroup
//     stays on its panel while slices are left (the panel is loaded once), then helps the panel with the
//     most slices left: the XCDs of one part run at speeds 10 % apart under the power cap, a static split
//     leaves the fast ones idle at the end of every launch.
//
// Against the 256x256 LDS-ring kernel: the same bytes per flop out of L2, but none of them crosses the LDS
// twice, a third less LDS read traffic, no barriers -- MFMA busy 84 % instead of 64 % of the cycles, and the
// workgroups of an XCD walk the same reference stream in step, so that every line is fetched once per XCD.
// MFMA-bound (power-capped): 2 * 128 * 512 * dpadh flop per workgroup col-step.
#include "prefilter_dev.h"

namespace vscmi {

namespace f16p {

constexpr int PR = F16P_PANEL_ROWS;  // 128
constexpr int CSW = F16P_COL_STEP;   // 512
#ifndef VSC_F16P_PF
#define VSC_F16P_PF 4
#endif
constexpr int PF = VSC_F16P_PF;      // register ring: k-steps (PF - 1 in flight, 2 KiB each per wave).  Measured in the
                                     // product build: 4 beats 8 (1314 vs 1284 TFLOP/s thresholded, 1178 vs 1031 k-NN):
                                     // with 8 the register file is full and the compiler shortens the LDS read pipeline

__device__ __forceinline__ f16x8 bload(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
}

// One output tile (128 panel rows x the wave's 64 columns, K = NKC x 128): A fragments from the LDS panel one
// k-step ahead, B fragments from the ring, refilled PF-1 k-steps ahead (voffset = 16 * lane + {0, 1024},
// soffset = position in the item's slice); the stream continues into the wave's next tile at `so_next`.
// Straight-line code, every LDS address = base register + immediate; the issue order is pinned (left alone
// the scheduler sinks every read to just before its use).  acc = (not +=) the product.
template <int NKC>
__device__ __forceinline__ void tile_mma(const char* smem, const int (&abase)[8], f16x8 (&a)[4], f16x8 (&ring)[PF][2],
                                         __amdgpu_buffer_rsrc_t rs, int so_tile, int so_next, int lane16,
                                         f32x16 (&acc)[4][2]) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int NKS = NKC * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int t = ks + PF - 1;  // k-step that goes into the ring slot freed by k-step ks - 1
        const int so = (t < NKS) ? so_tile + t * 2048 : so_next + (t - NKS) * 2048;
        const int kn = (ks + 1) % NKS;  // A fragments of the next k-step (the next tile starts at 0 again)
        const char* anext = smem + (kn >> 3) * 32768 + abase[kn & 7];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m], ring[ks % PF][0], ks == 0 ? zero : acc[m][0], 0, 0, 0);
            acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m], ring[ks % PF][1], ks == 0 ? zero : acc[m][1], 0, 0, 0);
            a[m] = *reinterpret_cast<const f16x8*>(anext + m * 8192);
            if (m < 2) ring[(ks + PF - 1) % PF][m] = bload(rs, lane16 + m * 1024, so);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (m < 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
    }
}

// Deferred rescoring (SimF16PArgs::floor): the band of fp16 scores whose exact score is proven to lie in (radius, floor],
// for the lane's column, derived on the flagged-block path from what is live there -- the column's candidate edge `thr`
// and the two wave-uniform scalars -- so that no per-lane value is added to the tile loop.  e = radius - thr is at least
// the column's error bound eps (candidate_edge only ever lowers the edge); then acc > lo >= radius + e proves
// exact > radius and acc <= hi <= floor - e proves exact <= floor, with the roundings of both sums taken off as in
// candidate_edge.  floor = +inf (off), an infinite or NaN bound: hi is NaN and no score lies in the band.
__device__ __forceinline__ void defer_band(float radius, float floor_v, float thr, float& lo, float& hi) {
    const float e = (radius - thr) * 1.000001f;
    lo = (radius + e) + 2.4e-7f * (fabsf(radius) + e);
    hi = candidate_edge(floor_v, e);
}

// Candidates of one wave tile -> the wave's PRIVATE segment of the candidate list (no atomics, no scans; a
// shared atomic tail only when the segment is full).  Per 32x32 block one question first (its per-lane
// maximum is known), then one ballot per accumulator register of the few blocks that hold a candidate.
//   ROWTHR = false: thr[n] = edge of *radius for the lane's column of block column n (strict test)
//   ROWTHR = true : rt = the panel's 128 row thresholds, rtmin[m] = smallest of row block m, eps[n] = the
//                   lane's column bounds (non-strict test: k-NN ties must survive)
// The lane id is recomputed where it is used (lane_now, prefilter_dev.h: no per-lane value may stay alive across a tile).
template <bool ROWTHR>
__device__ __forceinline__ void emit_candidates(const SimF16PArgs& a, const bool (&all)[2], const float (&thr)[2],
                                                const float (&eps)[2], const float* rt, const float (&rtmin)[4],
                                                int row0, int col0, bool interior, const f32x16 (&acc)[4][2],
                                                const float (&bm)[4][2], int64_t seg_base, int& count, TailExt* ext,
                                                float radius, float floor_v) {
    // C layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const bool blk = all[n] || (ROWTHR ? bm[m][n] >= candidate_edge(rtmin[m], eps[n]) : bm[m][n] > thr[n]);
            if (!__any(blk)) continue;
            // k-NN: the row thresholds of the lane's 16 rows of this block are looked up by row index: the lane id
            // is taken once per flagged block (live inside the block only)
            const int ln_blk = ROWTHR ? lane_now() : 0;
            float dlo = INFINITY, dhi = -INFINITY;
            if (!ROWTHR) defer_band(radius, floor_v, thr[n], dlo, dhi);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rb = m * 32 + (r & 3) + 8 * (r >> 2);  // + 4 * (lane >> 5) = row inside the panel
                bool cand;
                if (ROWTHR)
                    cand = acc[m][n][r] >= candidate_edge(rt[rb + 4 * (ln_blk >> 5)], eps[n]);
                else
                    cand = acc[m][n][r] > thr[n];
                const bool hit = all[n] || cand;
                const unsigned long long hits = __ballot(hit);
                if (hits == 0ull) continue;
                const int ln = ROWTHR ? ln_blk : lane_now();
                const int i = row0 + rb + 4 * (ln >> 5);
                const int j = col0 + n * 32 + (ln & 31);
                // (tiles that reach past the batch or the references drop their padding rows / columns)
                const bool mine = hit && (interior || (i < a.nq && j < a.nr));
                const unsigned long long ok = interior ? hits : __ballot(mine);
                if (ok == 0ull) continue;
                const int total = __popcll(ok);
                int64_t pos;
                if (!cand_reserve(a.list, seg_base, count, total, ln, ext, pos)) continue;
                if (mine) {
                    pos += lanes_below(ok);
                    const bool defer = !ROWTHR && acc[m][n][r] > dlo && acc[m][n][r] <= dhi;
                    a.list.i[pos] = (a.i0 + i) | (defer ? (int)DEFER_MARK : 0);
                    a.list.j[pos] = j;
                }
            }
        }
}

// The radius search's fast path: interior tile, room for a whole tile (8192 entries) left in the wave's segment.  Then
// nothing needs checking and the per-candidate code shrinks to: position = count + (lanes of this register's ballot
// below me), two buffer stores with a 32-bit offset into the wave's own segment (rs_i / rs_j: buffer resources on the
// segment, uniform per wave).  Per flagged block: 16 compares + lane id and column (5 VALU); per register that holds a
// candidate: 4 VALU + 2 stores -- a third of the instructions of the general form.  Everything else (edge tiles,
// segment nearly full, +inf error bounds, the k-NN thresholds) goes through emit_candidates.  Measured, pre-filter
// time of a bench step: 317 ms with emit_candidates everywhere, 304 ms with this fast path; a block-at-a-time emitter
// (per-lane bit masks + a wave prefix sum) gave 310 ms there and 354 against 348 ms on the k-NN (k = 1), and is gone.
__device__ __forceinline__ void emit_candidates_seg(const SimF16PArgs& a, const float (&thr)[2], int row0, int col0,
                                                    const f32x16 (&acc)[4][2], const float (&bm)[4][2],
                                                    __amdgpu_buffer_rsrc_t rs_i, __amdgpu_buffer_rsrc_t rs_j, int& count,
                                                    float radius, float floor_v) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (!__any(bm[m][n] > thr[n])) continue;
            const int ln = lane_now();  // (live inside the block only, see above)
            const int ibase = a.i0 + row0 + m * 32 + 4 * (ln >> 5);
            const int j = col0 + n * 32 + (ln & 31);
            float dlo, dhi;
            defer_band(radius, floor_v, thr[n], dlo, dhi);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool cand = acc[m][n][r] > thr[n];
                const unsigned long long hits = __ballot(cand);
                if (hits == 0ull) continue;
                if (cand) {
                    const int off = (count + (int)lanes_below(hits)) << 2;
                    const bool defer = acc[m][n][r] > dlo && acc[m][n][r] <= dhi;
                    __builtin_amdgcn_raw_buffer_store_b32((ibase + (r & 3) + 8 * (r >> 2)) | (defer ? (int)DEFER_MARK : 0), rs_i, off, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(j, rs_j, off, 0, 0);
                }
                count += __popcll(hits);
            }
        }
}

}  // namespace f16p

template <int NKC, bool ROWTHR>
__global__ __launch_bounds__(512) void sim_f16p_kernel(SimF16PArgs a) {
    using namespace f16p;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // the panel: NKC x 32 KiB
    __shared__ float qn_max_w[8];
    __shared__ float rt_sh[ROWTHR ? PR : 1];
    __shared__ int item_sh[2];
    __shared__ TailExt tail_sh[8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NKS = NKC * 8;
    constexpr int ROWB = NKC * 256;    // bytes per fp16 row
    constexpr int TILEB = NKS * 2048;  // bytes per 64-row wave tile of the fragment-major image
    const int lane16 = lane * 16;
    // LDS byte offset of the lane's A fragment at k-step u of a k chunk (+ chunk * 32768 + block m * 8192)
    int abase[8];
    {
        const int hi = lane >> 5, r15 = lane & 15, rl = lane & 31;
#pragma unroll
        for (int u = 0; u < 8; ++u) abase[u] = rl * 256 + ((((2 * u) | hi) ^ r15) << 4);
    }
    const float radius = ROWTHR ? 0.0f : *a.radius;
    const float floor_v = !ROWTHR && a.floor ? *a.floor : INFINITY;  // (+inf: nothing is deferred)
    const int seg = blockIdx.x * 8 + wave;  // this wave's private segment of the candidate list
    const int64_t seg_base = (int64_t)seg * a.list.seg_cap;
    int count = 0;
    tail_init(&tail_sh[wave], lane);  // the wave's chunk of the shared tail once its segment is full (cand_list.h)
    // the wave's segment of the two candidate arrays as buffer resources (emit_candidates_seg)
    const __amdgpu_buffer_rsrc_t rs_ci = __builtin_amdgcn_make_buffer_rsrc(
        (void*)uniform_ptr(reinterpret_cast<const char*>(a.list.i + seg_base)), 0, a.list.seg_cap * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_cj = __builtin_amdgcn_make_buffer_rsrc(
        (void*)uniform_ptr(reinterpret_cast<const char*>(a.list.j + seg_base)), 0, a.list.seg_cap * 4, 0x00020000);
    const int nslice = (a.nsteps + a.slice - 1) / a.slice;
    int cur_panel = -1;
    float nq_max = 0.f;
    float rtmin[4] = {0.f, 0.f, 0.f, 0.f};
    int panel = blockIdx.x % a.npanel;
    for (;;) {
        // ---- next work item: a slice of this workgroup's panel, else of the panel with the most left.  (The same loop
        // as the panel-major branch of sim_i8p.hip, written out in both: as one shared inline function it compiled to
        // different register allocations of both kernels -- profiles/prefilter_dev_refactor.md.)
        __syncthreads();
        if (wave == 0) {
            int p = panel, s = 0;
            // a launch whose candidate list has overflowed is lost (the host reruns it with larger buffers): stop
            // taking work
            const bool lost = __hip_atomic_load(a.list.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
            for (;;) {
                if (lost) { p = -1; break; }
                if (lane == 0) s = atomicAdd(&a.next_slice[p], 1);
                s = __shfl(s, 0);
                if (s < nslice) break;
                int best = 0x7fffffff, bp = 0x7fffffff;
                for (int q0 = 0; q0 < a.npanel; q0 += 64) {
                    const int q = q0 + lane;
                    const int pp = (q + (int)blockIdx.x) % a.npanel;  // ties: nearest after the workgroup's own
                    const int v = q < a.npanel ? __hip_atomic_load(&a.next_slice[pp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                               : 0x7fffffff;
                    if (v < best) { best = v; bp = pp; }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const int ob = __shfl_xor(best, off), op = __shfl_xor(bp, off);
                    if (ob < best || (ob == best && op < bp)) { best = ob; bp = op; }
                }
                if (best >= nslice) { p = -1; break; }
                p = bp;
            }
            if (lane == 0) { item_sh[0] = p; item_sh[1] = s; }
        }
        __syncthreads();
        panel = item_sh[0];
        const int sl = item_sh[1];
        if (panel < 0) break;
        const int cs0 = sl * a.slice, cs1 = min(a.nsteps, cs0 + a.slice);
        if (panel != cur_panel) {
            __syncthreads();  // (item_sh is read; nobody reads the old panel any more)
            // query panel -> LDS [k chunk][row][slot ^ (row & 15)]: the swizzle is applied to the SOURCE address,
            // an LDS-DMA instruction writes its 64 x 16 bytes to consecutive LDS addresses
            const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)uniform_ptr(reinterpret_cast<const char*>(a.Q) + (int64_t)panel * PR * ROWB), 0, PR * ROWB, 0x00020000);
#pragma unroll
            for (int n = 0; n < NKC * 4; ++n) {
                const int p = n * 512 + tid;
                const int kc = p >> 11, row = (p >> 4) & 127, slot = p & 15;
                const int c = kc * 16 + (slot ^ (row & 15));
                dma16(qrs, row * ROWB + c * 16, 0, smem + (n * 512 + wave * 64) * 16);
            }
            // largest row norm of the panel (rows past the batch do not count); k-NN: the row thresholds
            const bool in_batch = tid < PR && panel * PR + tid < a.nq;
            float nv = in_batch ? a.qn[(int64_t)panel * PR + tid] : 0.f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) nv = fmaxf(nv, __shfl_xor(nv, off));
            if (lane == 0) qn_max_w[wave] = nv;
            if (ROWTHR && tid < PR) rt_sh[tid] = in_batch ? a.row_thr[(int64_t)panel * PR + tid] : INFINITY;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces have landed ...
            __syncthreads();                                  // ... and so have everybody else's
            nq_max = fmaxf(qn_max_w[0], qn_max_w[1]);
            if (ROWTHR) {
                // smallest row threshold of each 32-row block
                float v0 = rt_sh[lane], v1 = rt_sh[64 + lane];
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) {
                    v0 = fminf(v0, __shfl_xor(v0, off));
                    v1 = fminf(v1, __shfl_xor(v1, off));
                }
                // (wave-uniform: kept in scalar registers, the vector file is full)
                rtmin[0] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v0), 0));
                rtmin[1] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v0), 32));
                rtmin[2] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v1), 0));
                rtmin[3] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v1), 32));
            }
            cur_panel = panel;
        }
        // ---- this wave's stream: tiles (cs * 8 + wave), cs = cs0 .. cs1-1, TILEB contiguous bytes each.
        // Buffer resource = the item's slice of the fragment-major image (reads past its end return 0).
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)uniform_ptr(reinterpret_cast<const char*>(a.Rf) + (int64_t)cs0 * 8 * TILEB), 0, (cs1 - cs0) * 8 * TILEB,
            0x00020000);
        int so_tile = wave * TILEB;
        f16x8 ring[PF][2];
#pragma unroll
        for (int dd = 0; dd < PF - 1; ++dd) {
            // (NKS >= 8 > PF - 1: the ring never reaches into the next tile here)
            ring[dd][0] = bload(rs, lane16, so_tile + dd * 2048);
            ring[dd][1] = bload(rs, lane16 + 1024, so_tile + dd * 2048);
        }
        f16x8 afr[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) afr[m] = *reinterpret_cast<const f16x8*>(smem + abase[0] + m * 8192);
        for (int cs = cs0; cs < cs1; ++cs) {
            const int col0 = cs * CSW + wave * 64;
            // norm bounds of the lane's two columns (the image is padded to whole col-steps)
            const float rn0 = a.rn[col0 + (lane & 31)], rn1 = a.rn[col0 + 32 + (lane & 31)];
            f32x16 acc[4][2];
            tile_mma<NKC>(smem, abase, afr, ring, rs, so_tile, so_tile + 8 * TILEB, lane16, acc);
            so_tile += 8 * TILEB;
            const float eps[2] = {(a.c1 * nq_max * rn0 + a.c2 * (nq_max + rn0) + a.c3) * 1.001f,
                                  (a.c1 * nq_max * rn1 + a.c2 * (nq_max + rn1) + a.c3) * 1.001f};
            const bool all[2] = {!(eps[0] < INFINITY), !(eps[1] < INFINITY)};  // also catches NaN (inf * 0)
            const float thr[2] = {candidate_edge(radius, eps[0]), candidate_edge(radius, eps[1])};
            // candidates are rare: one max per 32x32 block first, one compare for the whole wave tile
            float bm[4][2];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    float x = fmaxf(fmaxf(acc[m][n][0], acc[m][n][1]), acc[m][n][2]);
#pragma unroll
                    for (int r = 3; r < 15; r += 2) x = fmaxf(fmaxf(x, acc[m][n][r]), acc[m][n][r + 1]);
                    bm[m][n] = fmaxf(x, acc[m][n][15]);
                }
            bool any_blk = all[0] || all[1];
            if (ROWTHR) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    any_blk |= bm[m][0] >= candidate_edge(rtmin[m], eps[0]) || bm[m][1] >= candidate_edge(rtmin[m], eps[1]);
            } else {
                const float x0 = fmaxf(fmaxf(bm[0][0], bm[1][0]), fmaxf(bm[2][0], bm[3][0]));
                const float x1 = fmaxf(fmaxf(bm[0][1], bm[1][1]), fmaxf(bm[2][1], bm[3][1]));
                any_blk |= x0 > thr[0] || x1 > thr[1];
            }
            if (__any(any_blk)) {
                const bool interior = panel * PR + PR <= a.nq && col0 + 64 <= a.nr;
                if (!ROWTHR && interior && !all[0] && !all[1] && count + 8192 <= a.list.seg_cap)
                    emit_candidates_seg(a, thr, panel * PR, col0, acc, bm, rs_ci, rs_cj, count, radius, floor_v);
                else
                    emit_candidates<ROWTHR>(a, all, thr, eps, rt_sh, rtmin, panel * PR, col0, interior, acc, bm,
                                            seg_base, count, &tail_sh[wave], radius, floor_v);
            }
        }
    }
    tail_close(a.list, lane, &tail_sh[wave]);
    if (lane == 0) a.list.seg_count[seg] = count;
}

// Work split of one launch: slices (in col-steps) such that every workgroup sees >= ~16 items when the
// problem allows it (the stealing balances to within one item), between 4 and 64 col-steps each
void sim_f16p_plan(int64_t nq, int64_t nr, int* npanel, int* nsteps, int* slice, int* grid) {
    using namespace f16p;
    const int64_t P = (nq + PR - 1) / PR, S = (nr + CSW - 1) / CSW;
    int64_t sl = (S * P) / (256 * 16);
    sl = std::max<int64_t>(4, std::min<int64_t>(64, sl));
    sl = std::min(sl, std::max<int64_t>(S, 1));
    const int64_t items = P * ((S + sl - 1) / sl);
    *npanel = (int)P;
    *nsteps = (int)S;
    *slice = (int)sl;
    *grid = (int)std::max<int64_t>(1, std::min<int64_t>(256, items));
}

template <int NKC>
static int launch_nkc(const SimF16PArgs& a, int grid, hipStream_t stream) {
    const int lds = NKC * 32768;
    static PerDeviceOnce once;
    if (once.first()) {
        VSC_HIP(hipFuncSetAttribute((const void*)sim_f16p_kernel<NKC, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        VSC_HIP(hipFuncSetAttribute((const void*)sim_f16p_kernel<NKC, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        once.commit();
    }
    if (a.row_thr)
        hipLaunchKernelGGL((sim_f16p_kernel<NKC, true>), dim3((unsigned)grid), dim3(512), lds, stream, a);
    else
        hipLaunchKernelGGL((sim_f16p_kernel<NKC, false>), dim3((unsigned)grid), dim3(512), lds, stream, a);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

int launch_sim_f16p(const SimF16PArgs& a, int grid, hipStream_t stream) {
    if (grid <= 0 || a.npanel <= 0 || a.nsteps <= 0) {
        // nothing to search: the caller's exact stage must see empty segments, not stale fill levels
        if (grid > 0) VSC_HIP(hipMemsetAsync(a.list.seg_count, 0, (size_t)a.list.n_seg * sizeof(int), stream));
        return VSC_OK;
    }
    VSC_HIP(hipMemsetAsync(a.next_slice, 0, (size_t)a.npanel * sizeof(int), stream));
    switch (a.dpadh) {
        case 128: return launch_nkc<1>(a, grid, stream);
        case 256: return launch_nkc<2>(a, grid, stream);
        case 384: return launch_nkc<3>(a, grid, stream);
        case 512: return launch_nkc<4>(a, grid, stream);
    }
    set_error("sim_f16p: dpadh %d is not one of 128, 256, 384, 512", a.dpadh);
    return VSC_ERR_INVALID;
}

}  // namespace vscmi
