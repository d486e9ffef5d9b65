// Steps 2-4 of include/vscmi.h "DnS localisation on the device" on one 64 x 64 piece of the region matrix G in LDS: the
// one copy that fine_sim.hip (fp32 rows, matrix cores) and fine_bits.hip (bit rows, popcount) both call after their own
// step 1.  Every operation is one correctly rounded fp32 operation in the order the header states.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vscmi {

constexpr int FS_TILE = 64;  // region rows / columns of one work item
constexpr int FS_LD = 65;    // leading dimension of the LDS piece (odd: the column walks of the backward maxima spread over banks)

// G: the piece, [FS_TILE][FS_LD], complete and visible to the workgroup (the caller has synchronised).  fwd / bwd:
// FS_TILE * FS_TILE floats of scratch each.  nfq x nfr frame pairs of R regions are valid; F of frame pair (i, j) of
// pair p goes to out_base[out_off[p] + (qf0 + i) * lr + rf0 + j].  Called by all 256 threads.
__device__ __forceinline__ void fine_chamfer_reduce(const float* G, float* fwd, float* bwd, int tid, int R, int nfq, int nfr,
                                                    int symmetric, float* out_base, const int64_t* out_off, int p, int lr,
                                                    int qf0, int rf0) {
    // ---- 2. maxima: one lane per (frame pair, region) ----
    const int nfp = nfq * nfr;
    for (int x = tid; x < nfp * R; x += 256) {
        const int fp = x / R, c = x - fp * R;
        const int i = fp / nfr, j = fp - i * nfr;
        const float* g = G + (i * R + c) * FS_LD + j * R;  // region c of query frame i against the regions of frame j
        float m = g[0];
        for (int b = 1; b < R; ++b) {
            const float v = g[b];
            m = v > m ? v : m;
        }
        fwd[x] = m;
        if (symmetric) {
            const float* h = G + (i * R) * FS_LD + j * R + c;  // region c of reference frame j against the regions of frame i
            float m2 = h[0];
            for (int b = 1; b < R; ++b) {
                const float v = h[b * FS_LD];
                m2 = v > m2 ? v : m2;
            }
            bwd[x] = m2;
        }
    }
    __syncthreads();

    // ---- 3. sums in region order, the mapping to [0, 1]: one lane per frame pair ----
    const float regions = (float)R;
    float* out = out_base + out_off[p];
    for (int x = tid; x < nfp; x += 256) {
        const int i = x / nfr, j = x - i * nfr;
        float t = 0.0f;
        for (int c = 0; c < R; ++c) t = __fadd_rn(t, fwd[x * R + c]);
        float f0 = __fdiv_rn(t, regions);
        if (symmetric) {
            float u = 0.0f;
            for (int c = 0; c < R; ++c) u = __fadd_rn(u, bwd[x * R + c]);
            f0 = __fdiv_rn(__fadd_rn(f0, __fdiv_rn(u, regions)), 2.0f);
        }
        out[(int64_t)(qf0 + i) * lr + rf0 + j] = __fadd_rn(__fdiv_rn(f0, 2.0f), 0.5f);
    }
}

}  // namespace vscmi
