// Match rows (vsc_tn_match_rows): the padded box table of one localize_all batch -> the dense table the reference's
// pipeline ends with -- one row per box with the index of its pair, the corners, the score and the four timestamps
// (vsc/baseline/localization.py:66-73: query_start = ts_q[x1][0], query_end = ts_q[x2][1], ref_start = ts_r[y1][0],
// ref_end = ts_r[y2][1]).  Every output is a copy or a gather: no arithmetic on values, the contract is exact.
//
// Three launches:
//   match_rows_count   one pair per lane, tiles of MR_TILE pairs: the exclusive scan of the tile's box counts (Hillis-
//                      Steele in LDS, as radix.h's scans) -> pair_off[pair], the tile's sum -> tile_off[tile];
//   match_rows_carry   ONE workgroup walks the tile sums in chunks of 256 with a running carry: tile_off becomes the
//                      exclusive scan, the carry at the end is the number of rows (ctl[0]) -- integer sums, so the
//                      schedule does not matter for the result;
//   match_rows_emit    one (pair, slot) per lane: row = tile_off[tile] + pair_off[pair] + slot; the lane gathers the
//                      two query-side and the two reference-side timestamps through q_off / r_off (64-bit row
//                      arithmetic) and writes the row.
// Nothing is read outside the tables whatever the inputs hold: a box count outside 0..16 counts as 0, a pair ordinal
// outside the context's videos or a corner outside [0, L) of its video skips the row; each raises the error word
// (ctl[1]) that the entry point turns into VSC_ERR_INVALID.
//
// What bounds it: algorithmic bytes are 8 + 4 + 16 * 20 read per pair and 12 + 16 + 32 written per row, plus four
// 8-byte timestamp gathers per row -- 67 MB read and ~25 MB written at 200 000 pairs / 400 000 rows, some 20 us at
// HBM rate.  NOT measured against that bound and not tuned: three dependent launches and the host's read of the row
// count between the second and the third are launch-latency territory at this size, and the stage replaces seconds
// of per-row host work, not a kernel (profiles/match_rows.md has the measured times).
#include "kernels.h"

namespace vscmi {

constexpr int MR_TILE = 256;  // pairs per workgroup of the count pass = lanes per workgroup

__device__ __forceinline__ void mr_raise(int64_t* ctl, unsigned bit) {
    atomicOr(reinterpret_cast<unsigned int*>(ctl + 1), bit);
}

__global__ __launch_bounds__(MR_TILE) void match_rows_count_kernel(MatchRowsArgs a) {
    __shared__ int part[MR_TILE];
    const int64_t p = (int64_t)blockIdx.x * MR_TILE + threadIdx.x;
    int c = p < a.n_pairs ? a.nbox[p] : 0;
    if (c < 0 || c > VSC_TN_MAX_BOXES) {
        c = 0;
        mr_raise(a.ctl, 1u);
    }
    part[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < MR_TILE; off <<= 1) {  // inclusive scan
        const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    if (p < a.n_pairs) a.pair_off[p] = part[threadIdx.x] - c;
    if (threadIdx.x == MR_TILE - 1) a.tile_off[blockIdx.x] = part[MR_TILE - 1];
}

__global__ __launch_bounds__(256) void match_rows_carry_kernel(int64_t* __restrict__ tile_off, int64_t ntiles,
                                                               int64_t* __restrict__ ctl) {
    __shared__ int64_t part[256];
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < ntiles; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const int64_t c = t < ntiles ? tile_off[t] : 0;
        part[threadIdx.x] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int64_t v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += v;
            __syncthreads();
        }
        if (t < ntiles) tile_off[t] = carry + part[threadIdx.x] - c;
        carry += part[255];
        __syncthreads();  // (part is rewritten by the next chunk)
    }
    if (threadIdx.x == 0) ctl[0] = carry;
}

__global__ __launch_bounds__(256) void match_rows_emit_kernel(MatchRowsArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t p = idx / VSC_TN_MAX_BOXES;
    const int slot = (int)(idx % VSC_TN_MAX_BOXES);
    if (p >= a.n_pairs) return;
    const int c = a.nbox[p];
    if (c < 0 || c > VSC_TN_MAX_BOXES || slot >= c) return;  // (a count out of range was raised by the count pass)
    const int64_t row = a.tile_off[p / MR_TILE] + a.pair_off[p] + slot;
    const int32_t qv = a.pair_q[p], rv = a.pair_r[p];
    if (qv < 0 || qv >= a.n_qvid || rv < 0 || rv >= a.n_rvid) {
        mr_raise(a.ctl, 2u);
        return;
    }
    const int64_t q0 = a.q_off[qv], lq = a.q_off[qv + 1] - q0;
    const int64_t r0 = a.r_off[rv], lr = a.r_off[rv + 1] - r0;
    // (element accesses throughout: the caller's arrays promise the alignment of their element type, no more)
    const int32_t* bp = a.boxes + (p * VSC_TN_MAX_BOXES + slot) * 4;
    const int4 box = make_int4(bp[0], bp[1], bp[2], bp[3]);  // q_lo, r_lo, q_hi, r_hi
    if (box.x < 0 || box.x >= lq || box.z < 0 || box.z >= lq || box.y < 0 || box.y >= lr || box.w < 0 || box.w >= lr) {
        mr_raise(a.ctl, 4u);
        return;
    }
    a.out_pair[row] = (int32_t)p;
    if (a.out_box) {
        int32_t* ob = a.out_box + row * 4;
        ob[0] = box.x; ob[1] = box.y; ob[2] = box.z; ob[3] = box.w;
    }
    a.out_score[row] = a.boxmax[p * VSC_TN_MAX_BOXES + slot];
    double* ot = a.out_times + row * 4;
    ot[0] = a.q_ts[(q0 + box.x) * 2];
    ot[1] = a.q_ts[(q0 + box.z) * 2 + 1];
    ot[2] = a.r_ts[(r0 + box.y) * 2];
    ot[3] = a.r_ts[(r0 + box.w) * 2 + 1];
}

int64_t match_rows_tiles(int64_t n_pairs) { return (n_pairs + MR_TILE - 1) / MR_TILE; }

// pair_off, tile_off and ctl[0] (the row count) of the batch; ctl is zeroed here
int launch_match_rows_scan(const MatchRowsArgs& a, hipStream_t stream) {
    const int64_t ntiles = match_rows_tiles(a.n_pairs);
    if (hipMemsetAsync(a.ctl, 0, 2 * sizeof(int64_t), stream) != hipSuccess) {
        set_error("match rows: clearing the control words failed");
        return VSC_ERR_HIP;
    }
    if (a.n_pairs <= 0) return VSC_OK;
    if (ntiles > 0x7fffffffLL) {
        set_error("match rows: %lld pairs are beyond the supported size", (long long)a.n_pairs);
        return VSC_ERR_INVALID;
    }
    hipLaunchKernelGGL(match_rows_count_kernel, dim3((unsigned)ntiles), dim3(MR_TILE), 0, stream, a);
    hipLaunchKernelGGL(match_rows_carry_kernel, dim3(1), dim3(256), 0, stream, a.tile_off, ntiles, a.ctl);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

// the rows themselves (after launch_match_rows_scan on the same arguments); the caller has checked the capacity
int launch_match_rows_emit(const MatchRowsArgs& a, hipStream_t stream) {
    if (a.n_pairs <= 0) return VSC_OK;
    const int64_t blocks = (a.n_pairs * VSC_TN_MAX_BOXES + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        set_error("match rows: %lld pairs are beyond the supported size", (long long)a.n_pairs);
        return VSC_ERR_INVALID;
    }
    hipLaunchKernelGGL(match_rows_emit_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

}  // namespace vscmi
