// Frame transform of the inference CLI (`--packed_batch`): uint8 HWC frames of different sizes -> PIL's 8-bit BILINEAR
// resize (ImagingResample, integer arithmetic, bit for bit) -> window -> ToTensor + Normalize -> fp32 NCHW or bf16 NHWC.
// The arithmetic contract is in include/vscmi.h; the numpy restatement is vsc/baseline/frame_transform.py.
//
// Two launches per call with the uint8 intermediate in HBM (profiles/frame_transform.md):
//   h-pass  source rows the window's rows need x the window's columns, horizontal taps, rounded and clipped to uint8;
//   v-pass  vertical taps over that intermediate, the 3 x 256 value table (built per block in LDS), the output layout.
// A fused kernel would hold the input patch of an output tile in LDS; at 1920 -> 224 a pixel has 19 taps per axis and
// at the limits (8192 -> 1) a tile's patch is the whole frame, so the fused form needs a second, unfused path anyway.
// The intermediate is what PIL itself materialises, costs out_w / src_w of the source's bytes once more each way, and
// keeps every tap count inside one code path.  An axis with in == out gets the identity table (one tap of 2^22),
// which passes the levels through untouched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/vscmi.h"
#include "vscmi_common.h"

namespace vscmi {

constexpr int FT_PRECISION_BITS = 22;
constexpr int FT_MAX_SRC = 8192;
constexpr int FT_MAX_DST = 4096;
constexpr int64_t FT_MAX_FRAMES = 1 << 20;
constexpr int FT_TX = 64;    // h-pass: output columns per block (one per lane of a wave)
constexpr int FT_RPT = 4;    // h-pass: rows per thread (a coefficient is loaded once for them)
constexpr int FT_TY = 4;     // waves per block, both passes
constexpr int FT_TABLE_CAP = 2048;  // cached (in, out) tables per device before the cache is dropped

struct FtFrame {
    long long src_off;  // bytes from src to the frame
    long long mid_off;  // bytes from the intermediate's base to the frame's first row
    const int* hb;      // [dst_w][2]: first tap, taps
    const int* hk;      // [dst_w][hks], hks a multiple of 4, zeros behind a row's taps
    const int* vb;      // [dst_h][2]
    const int* vk;      // [dst_h][vks], likewise
    int row_bytes;      // src_w * 3
    int hks, vks;
    int top, left;
    int r0, nrows;      // source rows [r0, r0 + nrows) are the ones the window's rows read
    int sw;             // src_w
};

struct FtNorm {
    float mean[3], std[3];
};

__device__ __forceinline__ int ft_clip8(int acc) {
    const int v = acc >> FT_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One thread: output column x of FT_RPT consecutive intermediate rows, all three channels.
__global__ __launch_bounds__(FT_TX * FT_TY) void frame_hpass_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ mid,
                                                                      const FtFrame* __restrict__ frames,
                                                                      const int* __restrict__ blk_start, int n, int ow, int mid_stride) {
    const int b = blockIdx.x;
    int lo = 0, hi = n;  // blk_start[lo] <= b < blk_start[hi]
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (blk_start[m] <= b) lo = m; else hi = m;
    }
    const FtFrame f = frames[lo];
    const int lb = b - blk_start[lo], xt = (ow + FT_TX - 1) / FT_TX;
    const int x = (lb % xt) * FT_TX + threadIdx.x;
    const int row0 = (lb / xt) * (FT_TY * FT_RPT) + threadIdx.y * FT_RPT;
    if (x >= ow || row0 >= f.nrows) return;
    const int nr = f.nrows - row0 < FT_RPT ? f.nrows - row0 : FT_RPT;
    const int xmin = f.hb[2 * (f.left + x)], cnt = f.hb[2 * (f.left + x) + 1];
    const int* __restrict__ K = f.hk + (long long)(f.left + x) * f.hks;
    const uint8_t* s[FT_RPT];
#pragma unroll
    for (int r = 0; r < FT_RPT; ++r)  // rows past the frame's last read its last row again and store nothing
        s[r] = src + f.src_off + (long long)(f.r0 + row0 + (r < nr ? r : nr - 1)) * f.row_bytes + (long long)xmin * 3;
    int acc[FT_RPT][3];
#pragma unroll
    for (int r = 0; r < FT_RPT; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[r][c] = 1 << (FT_PRECISION_BITS - 1);
    // Four taps a step: their 12 bytes as three (unaligned) dword loads per row, their coefficients as one 16-byte load
    // (rows of K are padded with zeros to a multiple of 4, so taps past cnt add nothing).  Where the 4 pixels would leave
    // the source row -- the frame's right edge -- the step goes byte by byte over the taps that exist.
    for (int t = 0; t < cnt; t += 4) {
        if (xmin + t + 4 <= f.sw) {
            const int4 k = *reinterpret_cast<const int4*>(K + t);
#pragma unroll
            for (int r = 0; r < FT_RPT; ++r) {
                unsigned d0, d1, d2;
                __builtin_memcpy(&d0, s[r] + t * 3, 4);
                __builtin_memcpy(&d1, s[r] + t * 3 + 4, 4);
                __builtin_memcpy(&d2, s[r] + t * 3 + 8, 4);
                acc[r][0] += (int)(d0 & 255u) * k.x + (int)(d0 >> 24) * k.y + (int)((d1 >> 16) & 255u) * k.z + (int)((d2 >> 8) & 255u) * k.w;
                acc[r][1] += (int)((d0 >> 8) & 255u) * k.x + (int)(d1 & 255u) * k.y + (int)(d1 >> 24) * k.z + (int)((d2 >> 16) & 255u) * k.w;
                acc[r][2] += (int)((d0 >> 16) & 255u) * k.x + (int)((d1 >> 8) & 255u) * k.y + (int)(d2 & 255u) * k.z + (int)(d2 >> 24) * k.w;
            }
        } else {
            for (int tt = t; tt < cnt && tt < t + 4; ++tt) {
                const int k = K[tt];
#pragma unroll
                for (int r = 0; r < FT_RPT; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[r][c] += (int)s[r][tt * 3 + c] * k;
            }
        }
    }
    uint8_t* o = mid + f.mid_off + (long long)row0 * mid_stride + x * 3;
#pragma unroll
    for (int r = 0; r < FT_RPT; ++r)
        if (r < nr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(long long)r * mid_stride + c] = (uint8_t)ft_clip8(acc[r][c]);
        }
}

__device__ __forceinline__ unsigned short ft_bf16(float v) {  // round to nearest even; the table holds no NaN
    const unsigned u = __float_as_uint(v);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// One wave: one output row of one frame; a lane takes 4 consecutive bytes of the row's (x, c) sequence per step.
template <int FMT>
__global__ __launch_bounds__(FT_TX * FT_TY) void frame_vpass_kernel(const uint8_t* __restrict__ mid, void* __restrict__ out,
                                                                   const FtFrame* __restrict__ frames, int oh, int ow, int mid_stride,
                                                                   int yblocks, int vec, FtNorm nm) {
    __shared__ float lut[3 * 256];
    for (int i = threadIdx.y * FT_TX + threadIdx.x; i < 3 * 256; i += FT_TX * FT_TY) {
        const int c = i >> 8;
        lut[i] = ((float)(i & 255) / 255.0f - nm.mean[c]) / nm.std[c];  // ToTensor, then Normalize: three fp32 roundings
    }
    __syncthreads();
    const int frame = blockIdx.x / yblocks;
    const int y = __builtin_amdgcn_readfirstlane((blockIdx.x % yblocks) * FT_TY + threadIdx.y);
    if (y >= oh) return;
    const FtFrame f = frames[frame];
    const int ymin = f.vb[2 * (f.top + y)], cnt = f.vb[2 * (f.top + y) + 1];
    const int* __restrict__ K = f.vk + (long long)(f.top + y) * f.vks;
    const uint8_t* m = mid + f.mid_off + (long long)(ymin - f.r0) * mid_stride;
    const int row_elems = ow * 3, ndw = (row_elems + 3) >> 2;
    for (int j = threadIdx.x; j < ndw; j += FT_TX) {
        int acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = 1 << (FT_PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) {
            const int k = K[t];
            // (rows of the intermediate are padded to 16 bytes: the last dword of a row is inside the allocation)
            const unsigned v = *reinterpret_cast<const unsigned*>(m + (long long)t * mid_stride + 4 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += (int)((v >> (8 * e)) & 255u) * k;
        }
        if (FMT == VSC_FRAME_OUT_BF16_NHWC && vec) {  // rows of whole 4-element steps at 8-byte aligned addresses: one store
            unsigned short h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = ft_bf16(lut[((4 * j + e) % 3) * 256 + ft_clip8(acc[e])]);
            uint2 pk;
            pk.x = (unsigned)h[0] | ((unsigned)h[1] << 16);
            pk.y = (unsigned)h[2] | ((unsigned)h[3] << 16);
            *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(out) + ((long long)frame * oh + y) * row_elems + 4 * j) = pk;
            continue;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = 4 * j + e;
            if (idx < row_elems) {
                const int x = idx / 3, c = idx - 3 * x;
                const float val = lut[c * 256 + ft_clip8(acc[e])];
                if (FMT == VSC_FRAME_OUT_BF16_NHWC)
                    reinterpret_cast<unsigned short*>(out)[((long long)frame * oh + y) * row_elems + idx] = ft_bf16(val);
                else
                    reinterpret_cast<float*>(out)[(((long long)frame * 3 + c) * oh + y) * ow + x] = val;
            }
        }
    }
}

// ---- host: PIL's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter, in double
struct FtTable {
    int ksize = 0;
    std::vector<int> bounds;  // host copy: the call reads the first and last window row's taps from it
    int* d_bounds = nullptr;
    int* d_k = nullptr;
};

static void ft_build_table(int in, int out, int& ksize, std::vector<int>& bounds, std::vector<int>& kk) {
    bounds.assign((size_t)out * 2, 0);
    if (in == out) {  // the axis is skipped: its data passes through
        ksize = 4;
        kk.assign((size_t)out * ksize, 0);
        for (int xx = 0; xx < out; ++xx) { bounds[2 * xx] = xx; bounds[2 * xx + 1] = 1; kk[(size_t)xx * ksize] = 1 << FT_PRECISION_BITS; }
        return;
    }
    const double scale = (double)in / (double)out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    ksize = round_up((int)std::ceil(support) * 2 + 1, 4);  // PIL's ksize, padded: the stride of a row of K
    kk.assign((size_t)out * ksize, 0);
    std::vector<double> w((size_t)ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        for (int x = 0; x < xmax; ++x) {
            const double k = ww != 0.0 ? w[x] / ww : w[x];
            kk[(size_t)xx * ksize + x] = k < 0.0 ? (int)(-0.5 + k * (1 << FT_PRECISION_BITS)) : (int)(0.5 + k * (1 << FT_PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

struct FtDevice {
    std::map<std::pair<int, int>, FtTable> tables;
    DevBuf desc, mid;          // one call's frame records and intermediate; calls on other streams wait for `done`
    std::vector<char> host;
    hipEvent_t done = nullptr;
    void* last_stream = nullptr;
    bool pending = false;
};

static std::mutex g_ft_mu;
static std::map<int, FtDevice> g_ft_dev;

static int ft_table(FtDevice& d, int in, int out, const FtTable** res) {
    auto it = d.tables.find({in, out});
    if (it == d.tables.end()) {
        FtTable t;
        std::vector<int> kk;
        ft_build_table(in, out, t.ksize, t.bounds, kk);
        hipError_t e = hipMalloc((void**)&t.d_bounds, t.bounds.size() * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void**)&t.d_k, kk.size() * sizeof(int));
        if (e != hipSuccess) {
            if (t.d_bounds) (void)hipFree(t.d_bounds);
            set_error("vsc_frame_transform_u8: hipMalloc of a coefficient table failed: %s", hipGetErrorString(e));
            return VSC_ERR_NOMEM;
        }
        // synchronous copies: the table is complete before any stream can use it
        e = hipMemcpy(t.d_bounds, t.bounds.data(), t.bounds.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(t.d_k, kk.data(), kk.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(t.d_bounds);
            (void)hipFree(t.d_k);
            set_error("vsc_frame_transform_u8: upload of a coefficient table failed: %s", hipGetErrorString(e));
            return VSC_ERR_HIP;
        }
        it = d.tables.emplace(std::make_pair(in, out), std::move(t)).first;
    }
    *res = &it->second;
    return VSC_OK;
}

}  // namespace vscmi

extern "C" int vsc_frame_transform_u8(const uint8_t* src, const int64_t* src_off, const int32_t* src_h, const int32_t* src_w,
                                      const int32_t* dst_h, const int32_t* dst_w, const int32_t* top, const int32_t* left, int64_t n,
                                      int out_h, int out_w, const float* mean, const float* stdv, int out_format, void* out,
                                      void* hip_stream) {
    using namespace vscmi;
    if (n < 0 || n > FT_MAX_FRAMES) {
        set_error("vsc_frame_transform_u8: n = %lld outside 0..%lld", (long long)n, (long long)FT_MAX_FRAMES);
        return VSC_ERR_INVALID;
    }
    if (out_format != VSC_FRAME_OUT_F32_NCHW && out_format != VSC_FRAME_OUT_BF16_NHWC) {
        set_error("vsc_frame_transform_u8: unknown out_format %d", out_format);
        return VSC_ERR_INVALID;
    }
    if (out_h < 1 || out_w < 1 || out_h > FT_MAX_DST || out_w > FT_MAX_DST) {
        set_error("vsc_frame_transform_u8: output %d x %d outside 1..%d", out_h, out_w, FT_MAX_DST);
        return VSC_ERR_INVALID;
    }
    if (!mean || !stdv) {
        set_error("vsc_frame_transform_u8: mean / std is NULL");
        return VSC_ERR_INVALID;
    }
    for (int c = 0; c < 3; ++c)
        if (!(stdv[c] != 0.0f)) {  // (NaN too)
            set_error("vsc_frame_transform_u8: std[%d] must be a number other than 0", c);
            return VSC_ERR_INVALID;
        }
    if (n == 0) return VSC_OK;
    if (!src || !src_off || !src_h || !src_w || !dst_h || !dst_w || !top || !left || !out) {
        set_error("vsc_frame_transform_u8: NULL pointer with n > 0");
        return VSC_ERR_INVALID;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (src_h[i] < 1 || src_w[i] < 1 || src_h[i] > FT_MAX_SRC || src_w[i] > FT_MAX_SRC) {
            set_error("vsc_frame_transform_u8: frame %lld: source %d x %d outside 1..%d", (long long)i, src_h[i], src_w[i], FT_MAX_SRC);
            return VSC_ERR_INVALID;
        }
        if (dst_h[i] < 1 || dst_w[i] < 1 || dst_h[i] > FT_MAX_DST || dst_w[i] > FT_MAX_DST) {
            set_error("vsc_frame_transform_u8: frame %lld: resize target %d x %d outside 1..%d", (long long)i, dst_h[i], dst_w[i], FT_MAX_DST);
            return VSC_ERR_INVALID;
        }
        if (top[i] < 0 || left[i] < 0 || (int64_t)top[i] + out_h > dst_h[i] || (int64_t)left[i] + out_w > dst_w[i]) {
            set_error("vsc_frame_transform_u8: frame %lld: window %d x %d at (%d, %d) leaves the resized frame %d x %d", (long long)i,
                      out_h, out_w, top[i], left[i], dst_h[i], dst_w[i]);
            return VSC_ERR_INVALID;
        }
        if (src_off[i] < 0) {
            set_error("vsc_frame_transform_u8: frame %lld: negative src_off", (long long)i);
            return VSC_ERR_INVALID;
        }
    }

    std::lock_guard<std::mutex> lk(g_ft_mu);
    int dev = 0;
    VSC_HIP(hipGetDevice(&dev));
    FtDevice& d = g_ft_dev[dev];
    hipStream_t stream = (hipStream_t)hip_stream;
    if (!d.done) VSC_HIP(hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
    // the scratch buffers belong to the last call until its kernels have run: another stream waits for them
    if (d.pending && d.last_stream != hip_stream) VSC_HIP(hipStreamWaitEvent(stream, d.done, 0));
    if ((int)d.tables.size() >= FT_TABLE_CAP) {  // between calls only; kernels in flight may read the tables: drain first
        VSC_HIP(hipDeviceSynchronize());
        for (auto& kv : d.tables) {
            (void)hipFree(kv.second.d_bounds);
            (void)hipFree(kv.second.d_k);
        }
        d.tables.clear();
    }

    const int mid_stride = round_up(out_w * 3, 16);
    const int xt = (out_w + FT_TX - 1) / FT_TX;
    const size_t rec_bytes = (size_t)n * sizeof(FtFrame), blk_bytes = ((size_t)n + 1) * sizeof(int);
    d.host.resize(rec_bytes + blk_bytes);
    FtFrame* rec = reinterpret_cast<FtFrame*>(d.host.data());
    int* blk = reinterpret_cast<int*>(d.host.data() + rec_bytes);
    long long mid_bytes = 0, blocks = 0;
    for (int64_t i = 0; i < n; ++i) {
        const FtTable *h = nullptr, *v = nullptr;
        VSC_TRY(ft_table(d, src_w[i], dst_w[i], &h));
        VSC_TRY(ft_table(d, src_h[i], dst_h[i], &v));  // (std::map: h stays valid)
        FtFrame& f = rec[i];
        f.src_off = src_off[i];
        f.mid_off = mid_bytes;
        f.hb = h->d_bounds; f.hk = h->d_k; f.vb = v->d_bounds; f.vk = v->d_k;
        f.row_bytes = src_w[i] * 3;
        f.hks = h->ksize; f.vks = v->ksize;
        f.top = top[i]; f.left = left[i];
        const int ylast = top[i] + out_h - 1;
        f.r0 = v->bounds[2 * top[i]];
        f.nrows = v->bounds[2 * ylast] + v->bounds[2 * ylast + 1] - f.r0;
        f.sw = src_w[i];
        blk[i] = (int)blocks;
        mid_bytes += (long long)f.nrows * mid_stride;
        blocks += (long long)xt * ((f.nrows + FT_TY * FT_RPT - 1) / (FT_TY * FT_RPT));
        if (blocks > 0x7fffffffLL) {
            set_error("vsc_frame_transform_u8: %lld frames of these sizes are more than one launch holds", (long long)n);
            return VSC_ERR_INVALID;
        }
    }
    blk[n] = (int)blocks;
    const int yblocks = (out_h + FT_TY - 1) / FT_TY;
    if ((long long)n * yblocks > 0x7fffffffLL) {
        set_error("vsc_frame_transform_u8: %lld frames of %d rows are more than one launch holds", (long long)n, out_h);
        return VSC_ERR_INVALID;
    }
    VSC_TRY(d.desc.reserve(rec_bytes + blk_bytes));
    VSC_TRY(d.mid.reserve((size_t)mid_bytes));
    VSC_HIP(hipMemcpyAsync(d.desc.p, d.host.data(), rec_bytes + blk_bytes, hipMemcpyHostToDevice, stream));
    const FtFrame* d_rec = d.desc.as<FtFrame>();
    const int* d_blk = reinterpret_cast<const int*>(d.desc.as<char>() + rec_bytes);
    FtNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.std[c] = stdv[c]; }
    const dim3 block(FT_TX, FT_TY);
    const int vec = (out_w * 3) % 4 == 0 && ((uintptr_t)out & 7) == 0;  // bf16: 4 elements as one 8-byte store
    hipLaunchKernelGGL(frame_hpass_u8_kernel, dim3((unsigned)blocks), block, 0, stream, src, d.mid.as<uint8_t>(), d_rec, d_blk, (int)n, out_w,
                       mid_stride);
    VSC_HIP(hipGetLastError());
    if (out_format == VSC_FRAME_OUT_BF16_NHWC)
        hipLaunchKernelGGL(frame_vpass_kernel<VSC_FRAME_OUT_BF16_NHWC>, dim3((unsigned)(n * yblocks)), block, 0, stream,
                           (const uint8_t*)d.mid.as<uint8_t>(), out, d_rec, out_h, out_w, mid_stride, yblocks, vec, nm);
    else
        hipLaunchKernelGGL(frame_vpass_kernel<VSC_FRAME_OUT_F32_NCHW>, dim3((unsigned)(n * yblocks)), block, 0, stream,
                           (const uint8_t*)d.mid.as<uint8_t>(), out, d_rec, out_h, out_w, mid_stride, yblocks, vec, nm);
    VSC_HIP(hipGetLastError());
    VSC_HIP(hipEventRecord(d.done, stream));
    d.pending = true;
    d.last_stream = hip_stream;
    return VSC_OK;
}
