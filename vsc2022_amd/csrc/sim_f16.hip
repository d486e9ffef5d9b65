// fp16 pre-filter of the thresholded search: the 256x256 LDS-ring kernel (gfx950).
//
// The exact similarity (fp32 fma chain, sim_mfma.hip) runs at the fp32 matrix rate, 1/16 of the fp16
// rate.  Almost every (query row, ref row) pair is far below the search radius, so the bulk of the
// score matrix is first evaluated in fp16 with fp32 accumulation (v_mfma_f32_32x32x16_f16) and a pair
// goes on to the exact stage only if its fp16 score PLUS a rigorous error bound exceeds the radius:
//
//     |fp16 score - exact score| <= c1 * |q| * |r| + c2 * (|q| + |r|)            (api.hip derives c1, c2)
//
// so the candidate set is a superset of the exact hit set and the final result is bit-identical to
// the all-fp32 path (vsc/index.py:142-165 semantics unchanged; tests/test_gpu_prefilter.py).  The exact
// stage that takes the candidates is rescore.hip.
//
//   sim_f16_kernel   : 256x256 output tile per workgroup step, 8 waves (2 x 4), wave tile 128x64 =
//                      4x2 blocks of 32x32x16 MFMAs; operands by LDS-DMA into an XOR-swizzled image
//                      (2 stages x 64 KiB); persistent workgroups (1 per CU) walk an XCD-aware raster.
//                      MFMA-bound: 2*256*256*dpadh flop per tile.
#include <algorithm>

#include "prefilter_dev.h"

namespace vscmi {

namespace f16 {

// Ablation switches for timing studies only (results are WRONG when set): 1 = no barrier / DMA drain,
// 2 = no LDS-DMA in the loop, 4 = no fragment reads.  scripts/ablate_f16.sh builds the variants.
#ifndef VSC_F16_ABLATE
#define VSC_F16_ABLATE 0
#endif

constexpr int BM = 256, BN = 256;
constexpr int BK = 64;                       // fp16 elements per K-tile
constexpr int ROWB = BK * 2;                 // bytes per row per K-tile (128)
constexpr int TILE_BYTES = BM * ROWB;        // 32 KiB per operand
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // A + B
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 128 KiB

// cache policy of the LDS-DMA loads (aux bits of the buffer instruction: 1 = sc0, 2 = nt, 16 = sc1), per operand.
// Measured on one box (fp16 kernel ms per step): default 366; nt on the ref side 438, on the query side 438, on
// both 495 (the panels ARE reused out of L2 by the workgroups of an XCD); sc0 / sc1 366.
#ifndef VSC_F16_AUX_Q
#define VSC_F16_AUX_Q 0
#endif
#ifndef VSC_F16_AUX_R
#define VSC_F16_AUX_R 0
#endif
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* base, int row_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)uniform_ptr(reinterpret_cast<const char*>(base)), 0, BM * row_bytes,
                                             0x00020000);
}

// Per-thread constants.  LDS image of one operand K-tile: 128 lines of 256 B; line l holds rows 2l
// and 2l+1 (128 B each = 8 pieces of 16 B); piece c of a row sits at slot c ^ (l & 7) of its half
// line, so the 16 lanes of one ds_read_b128 phase (16 consecutive rows, same piece) cover all 64 banks.
struct TileThread {
    int src_off[4];  // byte offset (inside the tile's rows) of the 4 DMA pieces per operand
    int dst_off[4];  // wave-uniform LDS byte offset of those pieces
    int rdA[4];      // LDS byte offset of A block m at k-step 0 (k-step ks: ^ (ks << 5))
    int rdB[2];
};

__device__ __forceinline__ void tile_thread_init(TileThread& t, int tid, int row_bytes) {
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int p = n * 512 + tid;
        const int line = p >> 4, s = p & 15;
        const int row = 2 * line + (s >> 3);
        const int chunk = (s & 7) ^ (line & 7);
        t.src_off[n] = row * row_bytes + chunk * 16;
        t.dst_off[n] = (n * 512 + __builtin_amdgcn_readfirstlane(wave) * 64) * 16;
    }
    const int hi = lane >> 5;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int row = wr * 128 + m * 32 + (lane & 31);
        const int line = row >> 1;
        t.rdA[m] = line * 256 + ((((row & 1) << 3) | (hi ^ (line & 7))) << 4);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int row = wc * 64 + n * 32 + (lane & 31);
        const int line = row >> 1;
        t.rdB[n] = line * 256 + ((((row & 1) << 3) | (hi ^ (line & 7))) << 4);
    }
}

struct Frags {
    f16x8 a[4], b[2];
};

__device__ __forceinline__ Frags read_frags(const char* stage, const TileThread& t, int ks) {
    Frags f;
#pragma unroll
    for (int m = 0; m < 4; ++m) f.a[m] = *reinterpret_cast<const f16x8*>(stage + (t.rdA[m] ^ (ks << 5)));
#pragma unroll
    for (int n = 0; n < 2; ++n)
        f.b[n] = *reinterpret_cast<const f16x8*>(stage + TILE_BYTES + (t.rdB[n] ^ (ks << 5)));
    return f;
}

__device__ __forceinline__ void mfma8(const Frags& f, f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[m], f.b[n], acc[m][n], 0, 0, 0);
}

__device__ __forceinline__ void stage_tiles(__amdgpu_buffer_rsrc_t ars, __amdgpu_buffer_rsrc_t brs, int kt,
                                            char* stage, const TileThread& t) {
#pragma unroll
    for (int n = 0; n < 4; ++n) dma16<VSC_F16_AUX_Q>(ars, t.src_off[n], kt * ROWB, stage + t.dst_off[n]);
#pragma unroll
    for (int n = 0; n < 4; ++n) dma16<VSC_F16_AUX_R>(brs, t.src_off[n], kt * ROWB, stage + TILE_BYTES + t.dst_off[n]);
}

// The tile stream.  A workgroup is persistent: the K-tiles of the output tiles it walks form ONE stream
// through the 2-stage LDS ring (K-tile n of the stream lives in stage n & 1), so only the first tile of a
// workgroup pays a load prologue: while the last two K-tiles of tile T are multiplied, the first two of
// tile T+1 are already in flight, and they land during T's epilogue.
struct TileStream {
    const _Float16* q;  // operand panels of the current tile (wave-uniform)
    const _Float16* r;
    Frags cur;          // fragments (K-tile 0, k-step 0) of the current tile
    int sp;             // LDS stage holding K-tile 0 of the current tile
};

__device__ __forceinline__ void stream_begin(TileStream& st, const _Float16* qrows, const _Float16* rrows,
                                             int dpadh, char* smem, const TileThread& t) {
    st.q = qrows;
    st.r = rrows;
    st.sp = 0;
    const __amdgpu_buffer_rsrc_t ars = tile_rsrc(qrows, dpadh * 2), brs = tile_rsrc(rrows, dpadh * 2);
    stage_tiles(ars, brs, 0, smem, t);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // K-tile 1 (dpadh >= 128: it always exists): query side only, the ref side is issued by K-tile 0's
    // first k-step like in the steady state
#pragma unroll
    for (int n = 0; n < 4; ++n) dma16<VSC_F16_AUX_Q>(ars, t.src_off[n], ROWB, smem + STAGE_BYTES + t.dst_off[n]);
    st.cur = read_frags(smem, t, 0);
}

// acc += Q[256 rows] . R[256 rows]^T of the stream's current tile; the stream is left on the tile whose
// panels start at (nq, nr).  For the last tile of a workgroup pass the current panels again: the loop
// body has no conditionals (the two K-tiles it then fetches past the end are never read).
//
// Per K-tile (4 k-steps of 8 MFMAs): the barrier sits before the LAST k-step, whose operands are already
// in registers; after it the stage is free, and the DMA of the K-tile two ahead goes into it: the query
// side interleaved with those 8 MFMAs, the ref side with the first 8 of the next K-tile.  Register budget: 2 waves per SIMD => 256 VGPRs per lane, 128 of them accumulators; the A
// fragment of the NEXT k-step is read right after the two MFMAs that consumed the current one (same
// registers), only the two B fragments are double-buffered.
//
// FIRST = first K-tile of an output tile: its first k-step multiplies onto a literal zero (srcC is an
// inline constant), so the 128 accumulators are never cleared with VALU moves.
template <bool FIRST>
__device__ __forceinline__ void stream_ktile(TileStream& st, const _Float16* nq, const _Float16* nr, int dpadh,
                                             int kt, int nkt, Frags& cur, int& sp, char* smem,
                                             const TileThread& t, f32x16 (&acc)[4][2]) {
    const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const char* stage = smem + sp * STAGE_BYTES;
    // The 8 LDS-DMA issues a wave owes per K-tile are split so that none of them competes with more than
    // two MFMAs (an issue occupies the wave ~60 cycles, an MFMA the matrix pipe 32): the query side of
    // K-tile kt+2 goes out in this K-tile's last k-step (below), the ref side of K-tile kt+1 here, in the
    // first k-step -- its stage was freed by the previous K-tile's barrier.
    const int k1 = kt + 1;
    const bool in_cur1 = k1 < nkt;
    const __amdgpu_buffer_rsrc_t brs1 = tile_rsrc(in_cur1 ? st.r : nr, dpadh * 2);
    const int soff1 = (in_cur1 ? k1 : k1 - nkt) * ROWB;
    char* wstage1 = smem + (sp ^ 1) * STAGE_BYTES + TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
        f16x8 nb[2];
#pragma unroll
        for (int n = 0; n < 2; ++n)
            nb[n] = (VSC_F16_ABLATE & 4) ? cur.b[n]
                                         : *reinterpret_cast<const f16x8*>(stage + TILE_BYTES + (t.rdB[n] ^ ((ks + 1) << 5)));
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.a[m], cur.b[0], (FIRST && ks == 0) ? zero : acc[m][0], 0, 0, 0);
            acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.a[m], cur.b[1], (FIRST && ks == 0) ? zero : acc[m][1], 0, 0, 0);
            if (!(VSC_F16_ABLATE & 4)) cur.a[m] = *reinterpret_cast<const f16x8*>(stage + (t.rdA[m] ^ ((ks + 1) << 5)));
            if (ks == 0 && !(VSC_F16_ABLATE & 2)) dma16<VSC_F16_AUX_R>(brs1, t.src_off[m], soff1, wstage1 + t.dst_off[m]);
        }
        // pin the order: left alone, the scheduler sinks every fragment read to just before its use
        // and exposes the LDS latency once per k-step
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (ks == 0 && !(VSC_F16_ABLATE & 2)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        cur.b[0] = nb[0];
        cur.b[1] = nb[1];
    }
    // last k-step of the K-tile: every fragment of this stage is in registers
    const int k2 = kt + 2;
    const bool in_cur = k2 < nkt;
    const __amdgpu_buffer_rsrc_t ars = tile_rsrc(in_cur ? st.q : nq, dpadh * 2);
    const int soff = (in_cur ? k2 : k2 - nkt) * ROWB;
    const char* nstage = smem + (sp ^ 1) * STAGE_BYTES;
    char* wstage = smem + sp * STAGE_BYTES;
    // The next K-tile of the stream has landed once EVERY wave's own LDS-DMA pieces have: drain this
    // wave's count before the barrier (the compiler does not always do it for the builtin -- without
    // the wait a wave could read pieces another wave's DMA has not delivered yet).
    if (!(VSC_F16_ABLATE & 1)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // ... and nobody reads this stage any more
    }
    f16x8 nb[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
        nb[n] = (VSC_F16_ABLATE & 4) ? cur.b[n] : *reinterpret_cast<const f16x8*>(nstage + TILE_BYTES + t.rdB[n]);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.a[m], cur.b[0], acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.a[m], cur.b[1], acc[m][1], 0, 0, 0);
        if (!(VSC_F16_ABLATE & 4)) cur.a[m] = *reinterpret_cast<const f16x8*>(nstage + t.rdA[m]);
        if (!(VSC_F16_ABLATE & 2)) dma16<VSC_F16_AUX_Q>(ars, t.src_off[m], soff, wstage + t.dst_off[m]);
    }
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        if (!(VSC_F16_ABLATE & 2)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
    cur.b[0] = nb[0];
    cur.b[1] = nb[1];
    sp ^= 1;
}

// acc = (not +=) the tile's product; acc needs no initialisation.
__device__ __forceinline__ void stream_tile(TileStream& st, const _Float16* nq, const _Float16* nr, int dpadh,
                                            char* smem, const TileThread& t, f32x16 (&acc)[4][2]) {
    const int nkt = dpadh / BK;  // >= 2
    Frags cur = st.cur;
    int sp = st.sp;
    stream_ktile<true>(st, nq, nr, dpadh, 0, nkt, cur, sp, smem, t, acc);
    for (int kt = 1; kt < nkt; ++kt) stream_ktile<false>(st, nq, nr, dpadh, kt, nkt, cur, sp, smem, t, acc);
    st.cur = cur;
    st.sp = sp;
    st.q = nq;
    st.r = nr;
}

// XCD-aware raster (workgroup b runs on XCD b % 8): every XCD owns a contiguous run of tiles and walks
// it in bands of GQ query tiles, ref tile fastest inside... query tile fastest inside a band column, so
// the tiles in flight on one XCD share GQ query panels and a short run of ref panels in its L2.
// 32-bit arithmetic on purpose (the host guarantees tq * tr < 2^31): every wave evaluates this once per
// tile, and 64-bit divisions cost more instructions than the whole epilogue.
__device__ __forceinline__ bool raster(int xcd, int64_t local64, int tq, int64_t tr64, int& tqi, int64_t& tri) {
    const unsigned local = (unsigned)local64, tr = (unsigned)tr64;
    const unsigned nblk = (unsigned)tq * tr;
    const unsigned per_xcd = (nblk + 7u) >> 3;
    const unsigned logical = (unsigned)xcd * per_xcd + local;
    if (local >= per_xcd || logical >= nblk) return false;
#ifndef VSC_F16_GQ
#define VSC_F16_GQ 8
#endif
    constexpr unsigned GQ = VSC_F16_GQ;  // band height in query tiles (swept 4..32 on one box: see DESIGN.md)
    const unsigned band_sz = GQ * tr;
    const unsigned band = logical / band_sz, rem = logical - band * band_sz;
    const unsigned q0 = band * GQ;
    const unsigned gq = ((unsigned)tq - q0) < GQ ? ((unsigned)tq - q0) : GQ;
    const unsigned t = gq == GQ ? rem / GQ : rem / gq;
    tri = (int64_t)t;
    tqi = (int)(q0 + rem - t * gq);
    return true;
}

// Candidates of one wave tile -> the wave's PRIVATE segment of the candidate list: no atomics, no
// scans.  Per accumulator register one ballot; the (rare) non-empty ones are ranked with mbcnt.
// `count` is the wave-uniform fill level of the segment.
// ROWTHR = false: one threshold for the launch (`thr` = edge of *radius, strict test: thresholded search).
// ROWTHR = true : one threshold per query row (`rt` = the tile's 256 row thresholds in LDS, `thrb[m]` = edge
//                 of the smallest one of each 32-row block; non-strict test: k-NN, where ties must survive).
template <bool ROWTHR>
__device__ __forceinline__ void emit_candidates(const SimF16Args& a, bool all, float thr, const float (&thrb)[4],
                                                const float* rt, float eps, int row0, int row0_tile, int64_t col0,
                                                const f32x16 (&acc)[4][2], const float (&bm)[4][2], int lane,
                                                int64_t seg_base, int& count, TailExt* ext) {
    // C layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int row_base = row0 + 4 * (lane >> 5);
    const int col_base = (int)col0 + (lane & 31);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            // first ask per 32x32 block (its max is already known), then per accumulator register
            if (!all && !__any(ROWTHR ? bm[m][n] >= thrb[m] : bm[m][n] > thr)) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                bool cand;
                if (ROWTHR) {
                    const int rl = row0_tile + 4 * (lane >> 5) + m * 32 + (r & 3) + 8 * (r >> 2);
                    cand = acc[m][n][r] >= candidate_edge(rt[rl], eps);
                } else {
                    cand = acc[m][n][r] > thr;
                }
                const unsigned long long hits = __ballot(all || cand);
                if (hits == 0ull) continue;
                const int i = row_base + m * 32 + (r & 3) + 8 * (r >> 2);
                const int j = col_base + n * 32;
                const unsigned long long ok = __ballot(((hits >> lane) & 1ull) && i < a.nq && j < a.nr);
                if (ok == 0ull) continue;
                const int total = __popcll(ok);
                int64_t pos;
                if (!cand_reserve(a.list, seg_base, count, total, lane, ext, pos)) continue;
                if ((ok >> lane) & 1ull) {
                    pos += __popcll(ok & ((1ull << lane) - 1));
                    a.list.i[pos] = a.i0 + i;
                    a.list.j[pos] = j;
                }
            }
        }
}

}  // namespace f16

template <bool ROWTHR>
__global__ __launch_bounds__(512, 1) void sim_f16_kernel(SimF16Args a) {
    using namespace f16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float norm_max_buf[2][8];  // double-buffered by tile parity (no barrier between tiles)
    __shared__ float row_thr_buf[2][ROWTHR ? 256 : 1];
    __shared__ TailExt tail_sh[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;
    TileThread t;
    tile_thread_init(t, tid, a.dpadh * 2);
    const float radius = ROWTHR ? 0.0f : *a.radius;
    const int xcd = blockIdx.x & 7;
    const int64_t lstride = gridDim.x >> 3;  // gridDim.x is a multiple of 8
    // this wave's private segment of the candidate list
    const int seg = blockIdx.x * 8 + __builtin_amdgcn_readfirstlane(wave);
    const int64_t seg_base = (int64_t)seg * a.list.seg_cap;
    int count = 0;
    tail_init(&tail_sh[wave], lane);
    int64_t local = blockIdx.x >> 3;
    int tqi;
    int64_t tri;
    if (!raster(xcd, local, a.tq, a.tr, tqi, tri)) {
        if (lane == 0) a.list.seg_count[seg] = 0;
        return;
    }
    TileStream st;
    stream_begin(st, a.Q + (int64_t)tqi * BM * a.dpadh, a.R + tri * BN * a.dpadh, a.dpadh, smem, t);
    for (int parity = 0;; parity ^= 1) {
        int ntq = 0;
        int64_t ntr = 0;
        const bool has_next = raster(xcd, local + lstride, a.tq, a.tr, ntq, ntr);
        float* norm_max = norm_max_buf[parity];
        // largest row norm of each side of the tile (waves 0-3: query rows, 4-7: ref rows)
        float nv = tid < 256 ? a.qn[(int64_t)tqi * BM + tid] : a.rn[tri * BN + (tid - 256)];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nv = fmaxf(nv, __shfl_xor(nv, off));
        if (lane == 0) norm_max[wave] = nv;
        if (ROWTHR && tid < 256) row_thr_buf[parity][tid] = a.row_thr[(int64_t)tqi * BM + tid];
        f32x16 acc[4][2];
        stream_tile(st, has_next ? a.Q + (int64_t)ntq * BM * a.dpadh : st.q,
                    has_next ? a.R + ntr * BN * a.dpadh : st.r, a.dpadh, smem, t, acc);
        // (the barriers of the K loop ordered the norm_max writes)
        const float nq = fmaxf(fmaxf(norm_max[0], norm_max[1]), fmaxf(norm_max[2], norm_max[3]));
        const float nr = fmaxf(fmaxf(norm_max[4], norm_max[5]), fmaxf(norm_max[6], norm_max[7]));
        const float eps = (a.c1 * nq * nr + a.c2 * (nq + nr) + a.c3) * 1.001f;
        const bool all = !(eps < INFINITY);  // also catches NaN (inf * 0)
        const float thr = candidate_edge(radius, eps);
        float thrb[4] = {thr, thr, thr, thr};
        const float* rt = row_thr_buf[ROWTHR ? parity : 0];
        if (ROWTHR) {
            // smallest row threshold of each of the wave's four 32-row blocks
            float v0 = rt[wr * 128 + lane], v1 = rt[wr * 128 + 64 + lane];
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                v0 = fminf(v0, __shfl_xor(v0, off));
                v1 = fminf(v1, __shfl_xor(v1, off));
            }
            thrb[0] = candidate_edge(__shfl(v0, 0), eps);
            thrb[1] = candidate_edge(__shfl(v0, 32), eps);
            thrb[2] = candidate_edge(__shfl(v1, 0), eps);
            thrb[3] = candidate_edge(__shfl(v1, 32), eps);
        }
        // candidates are rare: one max per 32x32 block first, one compare for the whole wave tile
        float bm[4][2];
        float mx = -INFINITY;
        bool any_blk = false;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                float v = fmaxf(acc[m][n][0], acc[m][n][1]);
#pragma unroll
                for (int r = 2; r < 16; r += 2) v = fmaxf(v, fmaxf(acc[m][n][r], acc[m][n][r + 1]));
                bm[m][n] = v;
                mx = fmaxf(mx, v);
                if (ROWTHR) any_blk |= v >= thrb[m];
            }
        if (VSC_F16_ABLATE & 7) {
            count += mx == 12345.678f;  // keeps the accumulators alive; garbage results are not emitted
        } else if (all || __any(ROWTHR ? any_blk : mx > thr))
            emit_candidates<ROWTHR>(a, all, thr, thrb, rt, eps, tqi * BM + wr * 128, wr * 128,
                                    tri * BN + wc * 64, acc, bm, lane, seg_base, count, &tail_sh[wave]);
        if (!has_next) break;
        local += lstride;
        tqi = ntq;
        tri = ntr;
    }
    // the stream fetched two K-tiles past its end: let them land before the LDS is handed back
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    tail_close(a.list, lane, &tail_sh[wave]);
    if (lane == 0) a.list.seg_count[seg] = count;
}

// grid of a launch: one persistent workgroup per CU (fewer for tiny problems); 8 segments each
int sim_f16_grid(int tq, int tr) {
    const int64_t nblk = (int64_t)tq * tr;
    int64_t grid = ((nblk + 7) / 8) * 8;
    if (grid > 256) grid = 256;
    return (int)grid;
}

int launch_sim_f16(const SimF16Args& a, hipStream_t stream) {
    static PerDeviceOnce once;
    if (once.first()) {
        VSC_HIP(hipFuncSetAttribute((const void*)sim_f16_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    f16::LDS_BYTES));
        VSC_HIP(hipFuncSetAttribute((const void*)sim_f16_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    f16::LDS_BYTES));
        once.commit();
    }
    if ((int64_t)a.tq * a.tr >= 0x7fffffffLL) {
        set_error("sim_f16: more than 2^31 output tiles in one launch");
        return VSC_ERR_INVALID;
    }
    const int grid = sim_f16_grid(a.tq, a.tr);
    if (grid <= 0) return VSC_OK;
    if (a.row_thr)
        hipLaunchKernelGGL(sim_f16_kernel<true>, dim3((unsigned)grid), dim3(512), f16::LDS_BYTES, stream, a);
    else
        hipLaunchKernelGGL(sim_f16_kernel<false>, dim3((unsigned)grid), dim3(512), f16::LDS_BYTES, stream, a);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

}  // namespace vscmi
