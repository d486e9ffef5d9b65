// The frame x frame similarity tile of one candidate pair, shared by the per-pair kernels (tn.hip: Temporal Network,
// align.hip: DTW / DP): sims[q][r] = q.feature[q] . r.feature[r] + bias on the matrix cores (v_mfma_f32_32x32x2_f32,
// operands straight from L2/HBM in the engine's k-interleaved layout, ascending-k fp32 chain) -- the bits of
// vsc_tn_similarity's matrix.
#pragma once
#include "kernels.h"

namespace vscmi {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Where the similarity tile reads a reference row from (template parameter RH16 of the kernels).
//   false: the packed fp32 rows (vscmi_common.h: k-interleaved) -- the 16-byte load at float offset hi * 4 of k-group g
//          hands lane half `hi` its k = 8 g + 2 s + hi, s = 0..3.
//   true:  the half-float store of an SQfp16 context ([rows][dpad] halves, natural k order) -- both lane halves load
//          the whole 16-byte piece g; half `hi` keeps its even (hi = 0) or odd (hi = 1) elements, i.e. the low or the
//          high 16 bits of each of the four words, and converts them with the hardware cvt (exact).  The same values
//          in the same order reach the MFMA chain as from the packed fp32 image of the decoded rows.  One load
//          instruction per piece, as before (the phase waits on row loads), for half the bytes; the 4 shifts + 4 cvt
//          per piece issue beside the 4 or 8 MFMAs (64 cycles each) of the k-group.
template <bool RH16> struct TnRef;
template <> struct TnRef<false> {
    typedef float T;
    template <class A> static __device__ __forceinline__ const T* row(const A& a, int64_t r, int hi) { return a.rfeat + r * a.dpad + hi * 4; }
};
template <> struct TnRef<true> {
    typedef _Float16 T;
    template <class A> static __device__ __forceinline__ const T* row(const A& a, int64_t r, int) { return a.rfeat_h + r * a.dpad; }
};
__device__ __forceinline__ f32x4 tn_ref_piece(const float* p, int g, int) { return *reinterpret_cast<const f32x4*>(p + g * 8); }
__device__ __forceinline__ f32x4 tn_ref_piece(const _Float16* p, int g, int hi) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(p + g * 8);
    const int sh = hi * 16;
    f32x4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w[s] >> sh));
    return v;
}

// One wavefront writes the lq x lr tile of the pair whose rows start at qrow0 / rrow0 to sims (row-major, LDS or HBM):
// 32x32 output blocks, K ascending.  A: an argument block with qfeat, rfeat, rfeat_h, dpad and bias.
template <bool RH16, class A>
__device__ __forceinline__ void tn_sims_tile(const A& a, int64_t qrow0, int64_t rrow0, int lq, int lr, float* sims, int lane) {
    const int hi = lane >> 5, l31 = lane & 31;
    const int nkg = a.dpad / 8;
    // Two column blocks per pass share the A fragments: the phase waits on row loads (2 KB rows from HBM, one
    // pair's 75 rows are read once), so what counts is the number of loads in flight per wave, not the MFMAs.
    for (int qb = 0; qb < lq; qb += 32)
        for (int rb = 0; rb < lr; rb += 64) {
            // rows past the video end read the (padded) neighbour rows; their results are dropped
            const bool two = rb + 32 < lr;
            const float* ap = a.qfeat + (qrow0 + qb + l31) * a.dpad + hi * 4;
            const typename TnRef<RH16>::T* bp0 = TnRef<RH16>::row(a, rrow0 + rb + l31, hi);
            const typename TnRef<RH16>::T* bp1 = bp0 + (two ? 32 * (int64_t)a.dpad : 0);
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
            if (two) {
#pragma unroll 4
                for (int g = 0; g < nkg; ++g) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + g * 8);
                    const f32x4 bv0 = tn_ref_piece(bp0, g, hi);
                    const f32x4 bv1 = tn_ref_piece(bp1, g, hi);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv0[s], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv1[s], acc1, 0, 0, 0);
                    }
                }
            } else {
#pragma unroll 4
                for (int g = 0; g < nkg; ++g) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + g * 8);
                    const f32x4 bv = tn_ref_piece(bp0, g, hi);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc0, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = qb + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const int rr = rb + l31;
                if (q < lq && rr < lr) sims[(int64_t)q * lr + rr] = acc0[r] + a.bias;
                if (two && q < lq && rr + 32 < lr) sims[(int64_t)q * lr + rr + 32] = acc1[r] + a.bias;
            }
        }
}

}  // namespace vscmi
