// Region Chamfer similarity of a batch of candidate pairs on 1-BIT fine descriptors (gfx950): the VSC_FINE_BITS store of
// include/vscmi.h "DnS localisation on the device".  The twin of fine_sim.hip for DnS's binary student: the same work
// item (64 / R whole frames of each side of one pair, a 64 x 64 piece of G in LDS, 256 threads, the (pair, tile) work
// list), the same steps 2-4 (fine_chamfer.h, one copy); only step 1 differs.
//
// Step 1: with q, r in {-1, +1} every partial sum of the contract's chain acc = fmaf(q[d], r[d], acc) is an integer of
// magnitude <= D, so for D <= 2^24 no step rounds and, reading the values as bits (+1 = 1),
//     acc == (float)(D - 2 popcount(q xor r)),
// followed by the contract's one __fdiv_rn(acc, (float)D): the bits of the fp32 BIN route, from integers.
//
// Store: one row of w16 = ceil(D / 128) 16-byte words per (frame, region), bit d of the row = element d (bit d % 8 of
// byte d / 8: np.packbits(..., bitorder="little")), the bits from D on zero on BOTH sides -- they xor to zero and never
// enter a popcount -- and the rows past a side's last frame zero (the +64 slack rows that the last tile of the last
// video reads, as in fine_sim.hip: their G lands where no maximum reads).
//
// Structure: the piece's 64 + 64 bit rows go to LDS in K chunks of 512 bits (64 B per row; D = 512 is one chunk), in a
// row stride of 80 B.  Thread (ty, tx) of a 16 x 16 grid owns the 4 x 4 block of G of query rows ty + 16 i and reference
// rows tx + 16 j: per 128-bit step 4 + 4 ds_read_b128, then 64 v_xor + 64 v_bcnt_u32_b32 (popcount with its add operand)
// into 16 integer accumulators -- 128 VALU operations for 2048 bit products.  LDS pattern (CDNA4 serves a ds_read_b128 in
// 4 groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, over 64 banks of 4 bytes, bank =
// (address / 4) mod 64; equal addresses broadcast): every group holds all 16 tx and two ty, so a query-row read is 2
// addresses per group, 20 dwords apart (different banks), and a reference-row read is 16 addresses at 20 tx dwords, 4
// dwords each, which cover the 64 banks exactly once (20 tx mod 64 runs through the 16 multiples of 4): no conflict on
// either side.  The staging area is the forward-maxima scratch, which nothing uses before step 2.
//
// Bound: by instruction count step 1 is ~1 k bit products / clk / CU against ~128 MAC / clk / CU of the fp32 MFMA route.
// Measured (profiles/fine_bits.md: 512 pairs of 60 x 60 frames, R = 9, D = 512): 323 us per launch against 2634 us of
// fine_sim_kernel on the +-1 fp32 rows, 236 T bit products / s = 385 / clk / CU -- at D = 512 a tile is one chunk, so its
// fixed part (the load, three barriers, the LDS epilogue of steps 2-3) is what is left; not attributed with counters.
#include "fine_chamfer.h"
#include "kernels.h"

namespace vscmi {

constexpr int FB_CHUNK = 4;  // 16-byte words of a row per K chunk (512 bits)
constexpr int FB_LD = 5;     // row stride of the staged chunk in 16-byte words (80 B: see the bank pattern above)
static_assert(2 * FS_TILE * FB_LD * 16 <= FS_TILE * FS_TILE * 4, "the staged chunk lives in the forward-maxima scratch");

int fine_bits_row_words(int fdim) { return (fdim + 127) / 128; }

__global__ __launch_bounds__(256) void fine_bits_kernel(FineBitsArgs a) {
    __shared__ float G[FS_TILE * FS_LD];
    __shared__ __attribute__((aligned(16))) float fwd[FS_TILE * FS_TILE];  // [frame pair][a]: max over b; step 1: the staged bit rows
    __shared__ float bwd[FS_TILE * FS_TILE];                               // [frame pair][b]: max over a (symmetric only)
    const int tid = threadIdx.x;
    const int32_t* w = a.work + 3 * (int64_t)blockIdx.x;
    const int p = w[0], qf0 = w[1], rf0 = w[2];
    const int qv = a.pair_q[p], rv = a.pair_r[p];
    if (qv < 0 || qv >= a.n_qvid || rv < 0 || rv >= a.n_rvid) {  // (uniform over the workgroup)
        if (tid == 0) atomicOr(a.err, 1);
        return;
    }
    const int64_t q0 = a.q_off[qv], r0 = a.r_off[rv];
    const int lq = (int)(a.q_off[qv + 1] - q0), lr = (int)(a.r_off[rv + 1] - r0);
    const int R = a.regions, F = FS_TILE / R;
    if (qf0 < 0 || rf0 < 0 || qf0 >= lq || rf0 >= lr) return;  // (the host builds the list from the same offsets)
    const int nfq = lq - qf0 < F ? lq - qf0 : F, nfr = lr - rf0 < F ? lr - rf0 : F;

    // ---- 1. the 64 x 64 piece of G: D - 2 popcount(q xor r), K in chunks through LDS ----
    uint4* stage = reinterpret_cast<uint4*>(fwd);  // [0, 64): query rows, [64, 128): reference rows, FB_LD words each
    const int w16 = a.w16;
    const int row = tid >> 2, piece = tid & 3;  // the 16-byte word of the chunk this thread brings in, on both sides
    // (rows past the tile's last frame are the neighbours' or the zero slack rows: in bounds, read by no maximum)
    const uint4* gq = a.qbits + ((q0 + qf0) * R + row) * w16;
    const uint4* gr = a.rbits + ((r0 + rf0) * R + row) * w16;
    const int tx = tid & 15, ty = tid >> 4;
    int pop[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) pop[i][j] = 0;
    for (int c0 = 0; c0 < w16; c0 += FB_CHUNK) {
        const int nk = w16 - c0 < FB_CHUNK ? w16 - c0 : FB_CHUNK;
        if (c0) __syncthreads();  // (the previous chunk has been read)
        if (piece < nk) {
            stage[row * FB_LD + piece] = gq[c0 + piece];
            stage[(FS_TILE + row) * FB_LD + piece] = gr[c0 + piece];
        }
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            uint4 qw[4], rw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qw[i] = stage[(ty + 16 * i) * FB_LD + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) rw[j] = stage[(FS_TILE + tx + 16 * j) * FB_LD + k];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int c = pop[i][j];
                    c += __builtin_popcount(qw[i].x ^ rw[j].x);
                    c += __builtin_popcount(qw[i].y ^ rw[j].y);
                    c += __builtin_popcount(qw[i].z ^ rw[j].z);
                    c += __builtin_popcount(qw[i].w ^ rw[j].w);
                    pop[i][j] = c;
                }
        }
    }
    const float width = (float)a.fdim;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            G[(ty + 16 * i) * FS_LD + tx + 16 * j] = __fdiv_rn((float)(a.fdim - 2 * pop[i][j]), width);
    __syncthreads();  // (G is complete; the staged rows are dead: fwd is free)

    fine_chamfer_reduce(G, fwd, bwd, tid, R, nfq, nfr, a.symmetric, a.out, a.out_off, p, lr, qf0, rf0);
}

int launch_fine_bits(const FineBitsArgs& a, hipStream_t stream) {
    if (a.n_work <= 0) return VSC_OK;
    hipLaunchKernelGGL(fine_bits_kernel, dim3((unsigned)a.n_work), dim3(256), 0, stream, a);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

// ---- pack kernels: one thread per 32-bit word of the store; rows from `rows` on and bits from fdim on are zeros ----

// bytes {0, 1}, [rows][fdim] -> bit rows
__global__ __launch_bounds__(256) void pack_bits_from_bytes_kernel(const uint8_t* __restrict__ src, int64_t rows, int fdim,
                                                                   uint32_t* __restrict__ dst, int64_t n_words, int w32) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n_words) return;
    const int64_t r = x / w32;
    const int d0 = (int)(x - r * w32) * 32;
    uint32_t word = 0;
    if (r < rows && d0 < fdim) {
        const uint8_t* s = src + r * fdim + d0;
        const int n = fdim - d0 < 32 ? fdim - d0 : 32;
        for (int b = 0; b < n; ++b) word |= (uint32_t)(s[b] != 0) << b;
    }
    dst[x] = word;
}

// np.packbits(..., axis=-1, bitorder="little"), [rows][ceil(fdim / 8)] bytes -> bit rows; the unused high bits of a
// row's last byte are the caller's and are masked here
__global__ __launch_bounds__(256) void pack_bits_from_packed_kernel(const uint8_t* __restrict__ src, int64_t rows, int fdim,
                                                                    uint32_t* __restrict__ dst, int64_t n_words, int w32) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n_words) return;
    const int64_t r = x / w32;
    const int d0 = (int)(x - r * w32) * 32;
    uint32_t word = 0;
    if (r < rows && d0 < fdim) {
        const int row_bytes = (fdim + 7) / 8;
        const uint8_t* s = src + r * row_bytes + d0 / 8;
        const int n = fdim - d0 < 32 ? fdim - d0 : 32;  // valid bits of this word
        for (int b = 0; b < (n + 7) / 8; ++b) word |= (uint32_t)s[b] << (8 * b);
        if (n < 32) word &= (1u << n) - 1u;
    }
    dst[x] = word;
}

// `rows` source rows (bytes or packed bytes, device memory) -> rows_out bit rows of w16 16-byte words at dst
int launch_pack_bits(const uint8_t* src, bool packed, int64_t rows, int fdim, uint32_t* dst, int64_t rows_out, int w16,
                     hipStream_t stream) {
    const int w32 = 4 * w16;
    const int64_t n_words = rows_out * w32, blocks = (n_words + 255) / 256;
    if (n_words <= 0) return VSC_OK;
    if (blocks > 0x7fffffffLL) {
        set_error("fine bit rows: %lld words in one launch are beyond the supported size", (long long)n_words);
        return VSC_ERR_INVALID;
    }
    if (packed) hipLaunchKernelGGL(pack_bits_from_packed_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, rows, fdim, dst, n_words, w32);
    else hipLaunchKernelGGL(pack_bits_from_bytes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, rows, fdim, dst, n_words, w32);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

}  // namespace vscmi
