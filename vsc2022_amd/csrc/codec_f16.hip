// The SQfp16 codec (gfx950): reference rows live ONCE, as IEEE half floats, in the layout the fp16 pre-filter reads
// (fragment-major for dpadh <= 512, natural above: layout.hip).  HBM-bound layout transforms + the small helpers of
// the exact readers that run over decoded reference ranges (api_search.hip, api_knn.hip).
//   encode_rows       fp32 or fp16 rows -> store + per-row norm bounds; flags rows fp16 cannot hold
//   decode_rows       store rows -> packed fp32 (vscmi_common.h) or row-major fp32
//   unpack_rows       packed fp32 rows -> row-major fp32 (vsc_index_reconstruct of a Flat handle)
//   half_to_float     row-major fp16 -> row-major fp32 (vsc_index_add_f16 on a Flat handle)
//   score_matrix_h16  the explicit score matrix (L2, k > 64) with the reference side read from the store
// The exact stage's own fp16-source form is in rescore.hip (rescore_list<SRC>).
#include "kernels.h"

namespace vscmi {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// index of the 16-byte piece holding k = 8 p .. 8 p + 7 of row j
template <bool FRAG>
__device__ __forceinline__ int64_t store_piece(int64_t j, int p, int dpadh) {
    if (FRAG) return frag_piece(j, p, dpadh);
    return j * (dpadh / 8) + p;
}

// One wave per row, one piece per lane and step.  Rounding: round to nearest even, subnormals kept (the hardware
// conversion).  A source element that is NaN, +-inf or beyond +-65504 raises *bad: the caller undoes the add.  The
// norm bound is that of the DECODED row (what every search sees).  Rows [n, rows_out) are zero filled; the source is
// not read for them.
template <bool SRC16, bool FRAG>
__global__ __launch_bounds__(256) void encode_rows_kernel(const void* __restrict__ src, int64_t n, int dim,
                                                          _Float16* __restrict__ image, float* __restrict__ norms,
                                                          int64_t row0, int64_t rows_out, int dpadh, int* __restrict__ bad_out) {
    const int lane = threadIdx.x & 63;
    const int64_t rel = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rel >= rows_out) return;
    const int64_t row = row0 + rel;
    const float* r32 = reinterpret_cast<const float*>(src) + rel * dim;
    const _Float16* r16 = reinterpret_cast<const _Float16*>(src) + rel * dim;
    float ss = 0.0f;
    bool bad = false;
    for (int c = lane; c < dpadh / 8; c += 64) {
        f16x8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = c * 8 + e;
            const bool in = rel < n && k < dim;
            _Float16 v = (_Float16)0.0f;
            if (SRC16) {
                if (in) v = r16[k];
                bad |= !(fabsf((float)v) <= 65504.0f);
            } else {
                const float x = in ? r32[k] : 0.0f;
                bad |= !(fabsf(x) <= 65504.0f);
                v = (_Float16)x;  // round to nearest even
            }
            const float d = (float)v;
            ss = __fmaf_rn(d, d, ss);
            h[e] = v;
        }
        reinterpret_cast<f16x8*>(image)[store_piece<FRAG>(row, c, dpadh)] = h;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    const bool any_bad = __any(bad);
    if (lane == 0) {
        // (fp32 summation error <= dim 2^-24 relative: 1.0005 covers dim <= 8192; larger rows pass every pair)
        norms[rel] = (any_bad || dim > 8192) ? INFINITY : sqrtf(ss) * 1.0005f;
        if (any_bad) atomicOr(bad_out, 1);
    }
}

int launch_encode_rows(const void* src, bool src16, int64_t n, int dim, _Float16* image, float* norms, int64_t row0,
                       int64_t rows_out, int dpadh, bool frag, int* bad, hipStream_t stream) {
    if (rows_out <= 0) return VSC_OK;
    const dim3 grid((unsigned)((rows_out + 3) / 4)), block(256);
#define VSC_ENC(S, F) hipLaunchKernelGGL((encode_rows_kernel<S, F>), grid, block, 0, stream, src, n, dim, image, norms, row0, rows_out, dpadh, bad)
    if (src16) { if (frag) VSC_ENC(true, true); else VSC_ENC(true, false); }
    else { if (frag) VSC_ENC(false, true); else VSC_ENC(false, false); }
#undef VSC_ENC
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

// One thread per (row, piece): store rows [row0, row0 + rows_out) -> dst.  packed: [rows_out][ld] floats in the
// engine's k-interleaved order (ld = dpad; pieces past dpad / 8 are not written, the pieces inside hold the store's
// zero padding); else row-major [rows_out][ld = dim].  Rows >= n_valid come out as zeros (the store is not read).
template <bool FRAG>
__global__ __launch_bounds__(256) void decode_rows_kernel(const _Float16* __restrict__ image, int dpadh, int64_t row0,
                                                          int64_t rows_out, int64_t n_valid, float* __restrict__ dst,
                                                          int ld, int packed) {
    const int npiece = packed ? ld / 8 : (ld + 7) / 8;
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= rows_out * npiece) return;
    const int64_t rel = x / npiece;
    const int p = (int)(x % npiece);
    const int64_t row = row0 + rel;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.0f;
    if (row < n_valid) {
        const f16x8 h = reinterpret_cast<const f16x8*>(image)[store_piece<FRAG>(row, p, dpadh)];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
    }
    if (packed) {
        float4* o = reinterpret_cast<float4*>(dst + rel * ld + p * 8);
        o[0] = make_float4(v[0], v[2], v[4], v[6]);
        o[1] = make_float4(v[1], v[3], v[5], v[7]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (p * 8 + e < ld) dst[rel * ld + p * 8 + e] = v[e];
    }
}

int launch_decode_rows(const _Float16* image, int dpadh, bool frag, int64_t row0, int64_t rows_out, int64_t n_valid,
                       float* dst, int ld, bool packed, hipStream_t stream) {
    const int npiece = packed ? ld / 8 : (ld + 7) / 8;
    const int64_t total = rows_out * npiece;
    if (total <= 0) return VSC_OK;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (frag) hipLaunchKernelGGL(decode_rows_kernel<true>, grid, block, 0, stream, image, dpadh, row0, rows_out, n_valid, dst, ld, packed ? 1 : 0);
    else hipLaunchKernelGGL(decode_rows_kernel<false>, grid, block, 0, stream, image, dpadh, row0, rows_out, n_valid, dst, ld, packed ? 1 : 0);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

__global__ __launch_bounds__(256) void unpack_rows_kernel(const float* __restrict__ packed, int dpad, int64_t rows, int dim,
                                                          float* __restrict__ dst) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= rows * dim) return;
    const int64_t row = x / dim;
    const int k = (int)(x % dim);
    dst[x] = packed[row * dpad + k_slot(k)];
}

int launch_unpack_rows(const float* packed, int dpad, int64_t rows, int dim, float* dst, hipStream_t stream) {
    const int64_t total = rows * dim;
    if (total <= 0) return VSC_OK;
    hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, packed, dpad, rows, dim, dst);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

__global__ __launch_bounds__(256) void half_to_float_kernel(const _Float16* __restrict__ src, int64_t n, float* __restrict__ dst) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < n) dst[x] = (float)src[x];
}

int launch_half_to_float(const _Float16* src, int64_t n, float* dst, hipStream_t stream) {
    if (n <= 0) return VSC_OK;
    hipLaunchKernelGGL(half_to_float_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, n, dst);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

// score_matrix_kernel (sim_mfma.hip) with the reference row read from the store: the same ascending-k chain.
template <bool FRAG>
__global__ __launch_bounds__(256) void score_matrix_h16_kernel(ScoreMatArgs a, const _Float16* __restrict__ image, int dpadh) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= (int64_t)a.nq * a.nr) return;
    const int i = (int)(x / a.nr), j = (int)(x % a.nr);
    const float* q = a.Q + (int64_t)i * a.dpad;
    float acc = 0.0f;
    for (int k = 0; k < a.dim; ++k) {
        const float r = (float)image[store_piece<FRAG>(j, k >> 3, dpadh) * 8 + (k & 7)];
        if (a.metric == VSC_METRIC_INNER_PRODUCT) {
            acc = __fmaf_rn(q[k_slot(k)], r, acc);
        } else {
            const float d = q[k_slot(k)] - r;
            acc = __fmaf_rn(d, d, acc);
        }
    }
    a.S[x] = a.metric == VSC_METRIC_INNER_PRODUCT ? acc : -acc;
}

int launch_score_matrix_h16(const ScoreMatArgs& a, const _Float16* image, int dpadh, bool frag, hipStream_t stream) {
    const int64_t n = (int64_t)a.nq * a.nr;
    if (n <= 0) return VSC_OK;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (frag) hipLaunchKernelGGL(score_matrix_h16_kernel<true>, grid, block, 0, stream, a, image, dpadh);
    else hipLaunchKernelGGL(score_matrix_h16_kernel<false>, grid, block, 0, stream, a, image, dpadh);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

// ---- exact kernels over a decoded reference RANGE [j0, j0 + rows): their outputs hold refs relative to the range
// hits appended since `mark` (a copy of the list counter taken before the launch) get the range's offset
__global__ void hits_mark_kernel(const unsigned long long* __restrict__ counter, unsigned long long* __restrict__ mark) {
    *mark = *counter;
}
__global__ __launch_bounds__(256) void hits_add_offset_kernel(int32_t* __restrict__ out_j, const unsigned long long* __restrict__ mark,
                                                              const unsigned long long* __restrict__ counter, long long cap,
                                                              int j0) {
    const unsigned long long b = *mark;
    unsigned long long e = *counter;
    if (e > (unsigned long long)cap) e = (unsigned long long)cap;  // (overflowed: the search is rerun anyway)
    for (unsigned long long x = b + (unsigned long long)blockIdx.x * 256 + threadIdx.x; x < e; x += (unsigned long long)gridDim.x * 256)
        out_j[x] += j0;
}

int launch_hits_mark(const unsigned long long* counter, unsigned long long* mark, hipStream_t stream) {
    hipLaunchKernelGGL(hits_mark_kernel, dim3(1), dim3(1), 0, stream, counter, mark);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}
int launch_hits_add_offset(int32_t* out_j, const unsigned long long* mark, const unsigned long long* counter, long long cap,
                           int j0, hipStream_t stream) {
    hipLaunchKernelGGL(hits_add_offset_kernel, dim3(1024), dim3(256), 0, stream, out_j, mark, counter, cap, j0);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

// the partial k-NN lists of one range ([rows][nch][k], sim_knn_kernel's layout) -> slot `range` of the lists of all
// ranges ([rows][nranges * nch][k]), refs made absolute: knn_merge_kernel then merges them like the runs of one launch
__global__ __launch_bounds__(256) void knn_parts_scatter_kernel(const float* __restrict__ ps, const int32_t* __restrict__ pj,
                                                                int64_t rows, int nch, int k, int range, int nranges, int j0,
                                                                float* __restrict__ out_s, int32_t* __restrict__ out_j) {
    const int64_t per = (int64_t)nch * k;
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= rows * per) return;
    const int64_t row = x / per, e = x % per;
    const int64_t o = (row * nranges + range) * per + e;
    const int32_t j = pj[x];
    out_s[o] = ps[x];
    out_j[o] = j < 0 ? j : j + j0;
}

int launch_knn_parts_scatter(const float* ps, const int32_t* pj, int64_t rows, int nch, int k, int range, int nranges, int j0,
                             float* out_s, int32_t* out_j, hipStream_t stream) {
    const int64_t total = rows * nch * k;
    if (total <= 0) return VSC_OK;
    hipLaunchKernelGGL(knn_parts_scatter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ps, pj, rows, nch, k,
                       range, nranges, j0, out_s, out_j);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

}  // namespace vscmi
