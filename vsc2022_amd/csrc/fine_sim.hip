// Region Chamfer similarity of a batch of candidate pairs (gfx950): the part of a ViSiL / DnS fine-grained student that
// has no weights, F[i][j] of include/vscmi.h "DnS localisation on the device", steps 1-4.
//
// Replaces, per candidate pair (paths relative to /root/reference):
//   vsc/baseline/dns_baseline.py:139-147   sim = model(query, ref); (sim + model(ref, query).mT) / 2; sim / 2 + 0.5
// where `model` is the frame-to-frame Chamfer similarity on region descriptors [L, R, D]: inner products of all region
// pairs, max over one side's regions, mean over the other's (vsc2022_amd.vsc.baseline.dns_baseline.ChamferSimilarity).
//
// Structure: the region matrix G of a pair ((Lq R) x (Lr R), 1.1 MB at 540 x 540 frames) never exists as a whole.  One
// work item is FQ x FR WHOLE frames of one pair, FQ = FR = 64 / R (R = 9: 7 frames = 63 of 64 rows), so its 64 x 64 piece
// of G holds every region pair of its frame pairs.  Four wavefronts compute one 32 x 32 block each with the block routine
// of tn_sims.h (v_mfma_f32_32x32x2_f32, operands straight from L2 / HBM in the engine's k-interleaved layout, ascending-k
// fp32 chain from +0: the bits of oracle.pair_sims on the region rows) and leave it in LDS; one lane per (frame pair,
// region) takes the row and column maxima, one lane per frame pair sums them in region order and writes F.  The work
// list is (pair, tile): long and short pairs share a launch.  No atomics on floats; every F is written exactly once.
// Rows past a video's last frame read the (zero padded) neighbour rows: their products land in rows / columns of the LDS
// piece that no maximum reads.  The k padding is zeros: fmaf(0, 0, acc) == acc.
//
// Bound: matrix cores.  2 Lq Lr R^2 D flops per pair against 4 D R (Lq + Lr) bytes of region rows read once from HBM and
// 4 Lq Lr bytes written: 0.3 GFLOP against 2.2 MB at 60 x 60 frames, R = 9, D = 512 (135 flop / byte; the exact fp32
// similarity kernel reaches 137 TFLOP/s).  Every tile re-reads its rows from L2 (no operand staging in LDS) and a
// quarter of the lanes idle in the reductions at R = 16.  Measured at that shape (profiles/dns_device.md): 58 TFLOP/s.
//
// VSC_FINE_F16 (the attention student's descriptors as the half floats its indexer writes) is this kernel with the rows
// of both operands read as halves (FineRows<true>): half the bytes from L2, the same chain, the bits of the fp32 store
// of the decoded values.  Measured: profiles/fine_f16.md.
//
// VSC_FINE_BIN rows are +-1 fp32 here (the chain's result divided once by the width).  The 1-bit store of the same
// descriptors (VSC_FINE_BITS) has its own step 1 in fine_bits.hip -- xor + popcount, the same bits -- and shares steps
// 2-4 with this kernel through fine_chamfer.h (FS_TILE = 64 region rows / columns per work item: 2 x 2 MFMA blocks here).
#include "fine_chamfer.h"
#include "kernels.h"
#include "tn_sims.h"

namespace vscmi {

int fine_sim_frames(int regions) { return FS_TILE / regions; }

// Where step 1 reads its operand rows from (template parameter H16 of fine_sim_kernel), as TnRef of tn_sims.h:
//   false: the packed fp32 rows -- the 16-byte load at float offset hi * 4 of k-group g hands lane half `hi` its
//          k = 8 g + 2 s + hi, s = 0..3.
//   true:  the half-float rows of a VSC_FINE_F16 context on BOTH operands (natural k order): both lane halves load the
//          whole 16-byte piece g and keep their even or odd elements, converted by the hardware cvt (exact) --
//          tn_ref_piece.  The same values in the same order enter the chain as from the packed fp32 image of dec(X).
template <bool H16> struct FineRows;
template <> struct FineRows<false> {
    typedef float T;
    static __device__ __forceinline__ const T* q(const FineSimArgs& a, int64_t row, int hi) { return a.qfine + row * a.dpad + hi * 4; }
    static __device__ __forceinline__ const T* r(const FineSimArgs& a, int64_t row, int hi) { return a.rfine + row * a.dpad + hi * 4; }
};
template <> struct FineRows<true> {
    typedef _Float16 T;
    static __device__ __forceinline__ const T* q(const FineSimArgs& a, int64_t row, int) { return a.qfine_h + row * a.dpad; }
    static __device__ __forceinline__ const T* r(const FineSimArgs& a, int64_t row, int) { return a.rfine_h + row * a.dpad; }
};

template <bool H16>
__global__ __launch_bounds__(256) void fine_sim_kernel(FineSimArgs a) {
    __shared__ float G[FS_TILE * FS_LD];
    __shared__ float fwd[FS_TILE * FS_TILE];  // [frame pair][a]: max over b
    __shared__ float bwd[FS_TILE * FS_TILE];  // [frame pair][b]: max over a (symmetric only)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
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

    // ---- 1. the 64 x 64 piece of G: one 32 x 32 block per wavefront, K ascending; blocks of padding only are skipped ----
    const int qb = (wave >> 1) * 32, rb = (wave & 1) * 32;
    if (qb < nfq * R && rb < nfr * R) {
        const typename FineRows<H16>::T* ap = FineRows<H16>::q(a, (q0 + qf0) * R + qb + l31, hi);
        const typename FineRows<H16>::T* bp = FineRows<H16>::r(a, (r0 + rf0) * R + rb + l31, hi);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const int nkg = a.dpad / 8;
#pragma unroll 4
        for (int g = 0; g < nkg; ++g) {
            const f32x4 av = tn_ref_piece(ap, g, hi);
            const f32x4 bv = tn_ref_piece(bp, g, hi);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
        }
        const float width = (float)a.fdim;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = qb + (r & 3) + 8 * (r >> 2) + 4 * hi;
            G[row * FS_LD + rb + l31] = a.bin ? __fdiv_rn(acc[r], width) : acc[r];
        }
    }
    __syncthreads();

    // ---- 2-4. maxima, sums in region order, the mapping to [0, 1] (fine_chamfer.h) ----
    fine_chamfer_reduce(G, fwd, bwd, tid, R, nfq, nfr, a.symmetric, a.out, a.out_off, p, lr, qf0, rf0);
}

int launch_fine_sim(const FineSimArgs& a, hipStream_t stream, bool half_rows) {
    if (a.n_work <= 0) return VSC_OK;
    if (half_rows) hipLaunchKernelGGL(fine_sim_kernel<true>, dim3((unsigned)a.n_work), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(fine_sim_kernel<false>, dim3((unsigned)a.n_work), dim3(256), 0, stream, a);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

// bin descriptors: {0, 1} bytes -> 2 x - 1 as fp32 (exact)
__global__ __launch_bounds__(256) void bin_to_pm1_kernel(const uint8_t* __restrict__ src, int64_t n, float* __restrict__ dst) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < n) dst[x] = 2.0f * (float)src[x] - 1.0f;
}

int launch_bin_to_pm1(const uint8_t* src, int64_t n, float* dst, hipStream_t stream) {
    if (n <= 0) return VSC_OK;
    hipLaunchKernelGGL(bin_to_pm1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, n, dst);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

}  // namespace vscmi
