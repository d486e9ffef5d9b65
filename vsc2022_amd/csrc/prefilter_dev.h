// Device helpers of the search kernels (gfx950), each written once: the pre-filters (sim_f16.hip, sim_f16p.hip,
// sim_i8p.hip), the exact stage (rescore.hip) and the fp32 tile kernels (sim_mfma.hip) include this header.
#pragma once
#include "kernels.h"

namespace vscmi {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// LDS-DMA of one 16-byte piece per lane: buffer_load_dwordx4 ... lds.  The buffer descriptor is wave-uniform (tile or
// panel base), the per-lane part is a 32-bit byte offset, a K-tile advance rides in the scalar offset (the panel
// kernels pass 0): no 64-bit address arithmetic per issue.  AUX = cache policy bits (1 = sc0, 2 = nt, 16 = sc1).
template <int AUX = 0>
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff, char* lds) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds, 16, voff,
                                             soff, 0, AUX);
}

// makes an (already wave-uniform) pointer provably uniform, so that a buffer descriptor built on it lives in SGPRs
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

// The lane id, recomputed where it is used (two VALU instructions).  The emission code of the panel kernels must not
// keep per-lane values (row / column offsets of the lane) alive across a tile: the register file is full, the compiler
// spills them, and a scratch reload in the hit path costs an s_waitcnt vmcnt(0) that also waits for the acknowledgement
// of every candidate store issued before it (~2 us per hit: half of a tile's time in the early, dense batches).
__device__ __forceinline__ int lane_now() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// how many lanes below this one are set in a ballot mask: the lane's rank among the mask's lanes
__device__ __forceinline__ unsigned lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// The exactness contract of every pre-filter: the lower edge of the candidate test for an exact threshold t.  A pair
// with exact score >(=) t has a low-precision score >= t - eps (eps = the rigorous error bound of the pair's tile or
// column); the subtraction's own rounding (< 2^-23 relative to the larger operand) is subtracted again.
// t = +inf (k-NN: the rows of a panel that lie past the batch) gives inf - inf = NaN.  That is safe for the fp16 tests,
// which compare a score against the edge with >= or >: every comparison with NaN is false, so such a row -- and a
// 32-row block whose smallest threshold is +inf -- yields no candidate, which is what +inf asks for.  eps = +inf never
// gets here (the kernels pass every pair of such a tile or column).  The int8 kernel turns the edge into an integer
// threshold first, which does not survive NaN the same way: it keeps +inf apart (sim_i8p.hip: edge_keep_inf).
__device__ __forceinline__ float candidate_edge(float t, float eps) { return (t - eps) - 2.4e-7f * (fabsf(t) + eps); }

}  // namespace vscmi
