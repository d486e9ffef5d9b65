// Region stage of the DnS L3-iMAC extractor (`--baseline dns --fast`): the ResNet's four stage outputs, bf16 NHWC as
// the trunk kernels leave them, are max-pooled over overlapping square windows and every region vector is L2-normalised
// over its channels.  Stock PyTorch runs this as max_pool2d + a norm + a division per tap; here one kernel per tap reads
// the bf16 activation and writes the normalised fp32 region vectors straight into the tap's column slice of the
// [frames, regions, 3840] descriptor block, and one more kernel normalises the rows of that block.
//
// One workgroup per (image, region): its lanes run along the channels in 16-byte pieces (a wave reads 1 KiB contiguous
// per pixel), groups of lanes share the window's pixels, the per-channel maxima meet in LDS, and the workgroup reduces
// the sum of squares and writes its row.  The windows of a tap overlap (by half for win = 2 * stride), and the overlap
// is left to the L2, which takes two things (profiles/dns_inference.md: FETCH_SIZE 2.13x the activation without them,
// 1.38x with the first, 1.00x with both): the regions of one image run on ONE XCD (region_block), and regions that
// share image rows read them at the same step (the rotated row walk in the kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/vscmi.h"
#include "vscmi_common.h"

namespace vscmi {

typedef unsigned short rp_u16x8 __attribute__((ext_vector_type(8)));

constexpr int RP_THREADS = 256;  // (512 and 1024 threads, and 8 loads in flight instead of 4, measured no faster)
constexpr int RP_LOADS = 4;      // independent 16-byte loads in flight per lane
constexpr int RP_MAX_C = 4096;
constexpr int RP_XCDS = 8;       // workgroup i is dispatched to XCD i % 8

// sum over the workgroup (256 threads); every thread gets the result
__device__ __forceinline__ float rp_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // (red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Consecutive workgroup ids go to consecutive XCDs; this turns the id around so that every XCD owns one contiguous
// range of (image, region) pairs: the regions of an image, which share pixels, run on the same L2 at about the same time.
__device__ __forceinline__ long long region_block(long long n_regions) {
    const long long per_xcd = (n_regions + RP_XCDS - 1) / RP_XCDS;
    return (long long)(blockIdx.x % RP_XCDS) * per_xcd + blockIdx.x / RP_XCDS;
}

__global__ __launch_bounds__(RP_THREADS) void region_pool_l2_bf16_kernel(const unsigned short* __restrict__ x, float* __restrict__ out,
                                                                         long long n_regions, int H, int W, int C8, int win, int stride,
                                                                         int gh, int gw, long long out_row, long long out_col, float eps) {
    __shared__ unsigned keys[RP_MAX_C];  // order-preserving keys of the region's channel maxima (f2key)
    __shared__ float red[RP_THREADS / 64];
    const long long reg = region_block(n_regions);
    if (reg >= n_regions) return;  // (the whole workgroup: reg is uniform)
    const int gx = (int)(reg % gw), gy = (int)((reg / gw) % gh);
    const long long b = reg / ((long long)gw * gh);
    const int C = C8 * 8, tid = threadIdx.x;
    for (int c = tid; c < C; c += RP_THREADS) keys[c] = f2key(-INFINITY);
    __syncthreads();

    // lanes: piece c8 (8 channels) of the pixels g, g + G, g + 2 G, ... of the window, row by row
    const int L = C8 < RP_THREADS ? C8 : RP_THREADS, G = RP_THREADS / L, g = tid / L;
    const int npix = win * win;
    // The window's rows are walked starting at the one whose image row is a multiple of win (the maximum does not care
    // about the order): vertical neighbours, which share image rows, then read them at the same step (exactly so for
    // win = 2 * stride) and the second reader finds them in L2.  Horizontal neighbours are half a row apart as it is.
    const int rot = (win - (int)(((long long)gy * stride) % win)) % win;
    const rp_u16x8* base = reinterpret_cast<const rp_u16x8*>(x) + (((b * H + (long long)gy * stride) * W) + (long long)gx * stride) * C8;
    if (g < G) {
        for (int c8 = tid % L; c8 < C8; c8 += L) {
            float m[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
            int dy = g / win + rot, dx = g % win;  // (dy, dx) < (win, win) inside the window for every pixel loaded
            dy = dy >= win ? dy - win : dy;
            int left = g < npix ? (npix - g + G - 1) / G : 0;
            while (left > 0) {
                rp_u16x8 v[RP_LOADS];
#pragma unroll
                for (int u = 0; u < RP_LOADS; ++u) {
                    if (u < left) v[u] = base[((long long)dy * W + dx) * C8 + c8];
                    dx += G;
                    while (dx >= win) { dx -= win; dy = dy + 1 == win ? 0 : dy + 1; }
                }
#pragma unroll
                for (int u = 0; u < RP_LOADS; ++u) {
                    if (u < left) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float f = __uint_as_float((unsigned)v[u][e] << 16);  // bf16 widens exactly
                            m[e] = f > m[e] ? f : m[e];
                        }
                    }
                }
                left -= RP_LOADS;
            }
            if (G == 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) keys[c8 * 8 + e] = f2key(m[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) atomicMax(&keys[c8 * 8 + e], f2key(m[e]));
            }
        }
    }
    __syncthreads();
    float ss = 0.0f;
    for (int c = tid; c < C; c += RP_THREADS) {
        const float f = key2f(keys[c]);
        ss += f * f;
    }
    ss = rp_block_sum(ss, red);
    const float nrm = sqrtf(ss), den = nrm > eps ? nrm : eps;
    float* o = out + reg * out_row + out_col;
    for (int c = tid; c < C; c += RP_THREADS) o[c] = key2f(keys[c]) / den;
}

// x[r, :] /= max(||x[r, :]||_2, eps): one workgroup per row, the second pass re-reads the row from cache
__global__ __launch_bounds__(RP_THREADS) void rows_l2norm_f32_kernel(float* __restrict__ x, long long rows, long long cols, float eps) {
    __shared__ float red[RP_THREADS / 64];
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        float* row = x + r * cols;
        float ss = 0.0f;
        for (long long c = threadIdx.x; c < cols; c += RP_THREADS) {
            const float f = row[c];
            ss += f * f;
        }
        ss = rp_block_sum(ss, red);
        const float nrm = sqrtf(ss), den = nrm > eps ? nrm : eps;
        for (long long c = threadIdx.x; c < cols; c += RP_THREADS) row[c] = row[c] / den;
    }
}

}  // namespace vscmi

extern "C" int vsc_region_pool_l2_bf16(const void* x, float* out, int64_t B, int64_t H, int64_t W, int64_t C, int win, int stride,
                                       int64_t out_row, int64_t out_col, float eps, void* hip_stream) {
    using namespace vscmi;
    const int64_t lim = 1 << 20;
    if (B < 0 || C <= 0 || (C & 7) || C > RP_MAX_C || win < 1 || stride < 1 || H < win || W < win || H > lim || W > lim ||
        out_col < 0 || out_row < out_col + C || !(eps >= 0.0f) || (B > 0 && (!x || !out)) || ((uintptr_t)x & 15) || ((uintptr_t)out & 3)) {
        set_error("vsc_region_pool_l2_bf16: invalid argument (C a multiple of 8 and <= 4096, 1 <= win <= H, W, stride >= 1, "
                  "out_row >= out_col + C, eps >= 0, x 16-byte aligned)");
        return VSC_ERR_INVALID;
    }
    const int gh = (int)((H - win) / stride + 1), gw = (int)((W - win) / stride + 1);
    const int64_t max_blocks = (int64_t)0x7fffffff - RP_XCDS;
    if ((int64_t)gh * gw > max_blocks || (B > 0 && (int64_t)gh * gw > max_blocks / B)) {
        set_error("vsc_region_pool_l2_bf16: B * regions = %lld * %lld is more than one launch holds", (long long)B, (long long)gh * gw);
        return VSC_ERR_INVALID;
    }
    const long long n_regions = (long long)B * gh * gw;
    if (n_regions == 0) return VSC_OK;
    const unsigned grid = (unsigned)((n_regions + RP_XCDS - 1) / RP_XCDS * RP_XCDS);
    hipLaunchKernelGGL(region_pool_l2_bf16_kernel, dim3(grid), dim3(RP_THREADS), 0, (hipStream_t)hip_stream, (const unsigned short*)x, out,
                       n_regions, (int)H, (int)W, (int)(C / 8), win, stride, gh, gw, (long long)out_row, (long long)out_col, eps);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

extern "C" int vsc_rows_l2norm_f32(float* x, int64_t rows, int64_t cols, float eps, void* hip_stream) {
    using namespace vscmi;
    if (rows < 0 || cols <= 0 || !(eps >= 0.0f) || (rows > 0 && !x) || ((uintptr_t)x & 3)) {
        set_error("vsc_rows_l2norm_f32: invalid argument (rows >= 0, cols >= 1, eps >= 0, x not null)");
        return VSC_ERR_INVALID;
    }
    if (rows == 0) return VSC_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(rows, 256 * 32);
    hipLaunchKernelGGL(rows_l2norm_f32_kernel, dim3(grid), dim3(RP_THREADS), 0, (hipStream_t)hip_stream, x, (long long)rows, (long long)cols, eps);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}
