// DTW and DP alignment, one candidate pair per (single-wavefront) workgroup (gfx950).
//
// Device forms of `dtw` and `dp` of vsc2022_amd/vcsl/aligners.py (the module docstring there writes both algorithms down
// choice by choice); the boxes are the host functions' on the same fp32 matrix, integer for integer.  What makes that
// possible: every float64 value the host computes is ONE operation on operands the device has too (cost + min of three
// neighbours; gain + best predecessor; score += sim along the path), so the bits agree whatever the schedule -- lanes
// walk the anti-diagonals of D (DTW) or the columns of a row of S (DP) -- and everything else is integer or comparison
// logic in the host's order.  The match / alive test compares in fp32 (NumPy keeps a Python float weak against an fp32
// matrix); cost, gain, scores and the IoU are float64.  -ffp-contract=off (Makefile): no fused multiply-adds.
//
// The similarity tile is tn_pair_kernel's (tn_sims.h) and is held in LDS with the whole working state (kernels.h:
// AlignLayout); in forward_sim mode the caller's matrix is read in place.  Pairs beyond VSC_ALIGN_MAX_CELLS are refused
// with status 1 before anything is computed.
//
// Every loop's trip count is fixed by the shapes: the DTW traceback takes lq + lr steps at most and cannot leave the
// matrix whatever the direction bytes hold, the DP walk-back lq steps, the extraction loop max_path rounds.
//
// Bound: not measured against a roofline -- serial chains of LDS round trips of one wave (lq + lr diagonals; lq rows x
// (discontinue + 1)^2 predecessor reads per DP round); profiles/aligners_device.md has the timings.
#include <cmath>

#include "kernels.h"
#include "tn_sims.h"

namespace vscmi {

// The keep filter of aligners.py (`_keep` / `_iou`), one box at a time, evaluated by every lane alike (LDS broadcast
// reads); lane 0 records a kept box.  0: rejected, 1: kept, 2: passed, but VSC_TN_MAX_BOXES are kept already.
__device__ __forceinline__ int align_keep(int* kept, int& nkept, int q0, int r0, int q1, int r1, const vsc_align_params& prm, int lane) {
    const int dq = q1 - q0, dr = r1 - r0;
    if (!((dq < dr ? dq : dr) > prm.min_length)) return 0;
    if (nkept > 0) {
        double best = 0.0;
        for (int k = 0; k < nkept; ++k) {
            const int* o = kept + 4 * k;
            const int w = (q1 < o[2] ? q1 : o[2]) - (q0 > o[0] ? q0 : o[0]);
            const int h = (r1 < o[3] ? r1 : o[3]) - (r0 > o[1] ? r0 : o[1]);
            const long long inter = (long long)(w > 0 ? w : 0) * (h > 0 ? h : 0);
            const long long uni = (long long)dq * dr + (long long)(o[2] - o[0]) * (o[3] - o[1]) - inter;
            if (uni > 0) {
                const double v = (double)inter / (double)uni;
                best = v > best ? v : best;
            }
        }
        if (!(best < prm.max_iou)) return 0;
    }
    if (nkept >= VSC_TN_MAX_BOXES) return 2;
    if (lane == 0) {
        kept[4 * nkept + 0] = q0;
        kept[4 * nkept + 1] = r0;
        kept[4 * nkept + 2] = q1;
        kept[4 * nkept + 3] = r1;
    }
    ++nkept;
    __syncthreads();
    return 1;
}

// (value, index) first maximum over the wave: the larger value, of equal values the smaller index; index < 0 = no entry
__device__ __forceinline__ void wave_first_max_f64(double& v, int& o) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oo = __shfl_xor(o, off);
        const bool take = oo >= 0 && (o < 0 || ov > v || (ov == v && oo < o));
        v = take ? ov : v;
        o = take ? oo : o;
    }
}

// DTW.  Returns the status (0 / 2); the kept boxes are in `kept`.
__device__ __forceinline__ int align_dtw(char* smem, const AlignLayout& L, const float* sims, int lq, int lr, const vsc_align_params& prm,
                                         int* kept, int& nkept, int lane) {
    double* diag = reinterpret_cast<double*>(smem + L.f64);
    double* run_score = reinterpret_cast<double*>(smem + L.runs);
    const int run_cap = (lq + lr) / 2 + 1;
    unsigned short* run_box = reinterpret_cast<unsigned short*>(run_score + run_cap);
    unsigned char* dirs = reinterpret_cast<unsigned char*>(smem + L.bytes);
    unsigned char* steps = dirs + (size_t)lq * lr;

    // ---- 1. D over anti-diagonals k = i + j of the (lq + 1) x (lr + 1) table; lanes go along the SHORTER axis t (a
    // diagonal holds min(lq, lr) + 1 entries at most), o = k - t is the other one.  Entry [t] of a diagonal buffer is
    // D at (t, o); the borders t == 0 / o == 0 are +inf, D[0, 0] = 0.
    const bool t_is_q = lq <= lr;
    const int T = t_is_q ? lq : lr, O = t_is_q ? lr : lq;
    double* p2 = diag;                // diagonal k - 2
    double* p1 = diag + (T + 1);      // diagonal k - 1
    double* cur = diag + 2 * (T + 1);
    if (lane == 0) {
        p2[0] = 0.0;
        p1[0] = INFINITY;
        p1[1] = INFINITY;  // (T >= 1)
    }
    __syncthreads();
    for (int k = 2; k <= lq + lr; ++k) {
        const int tlo = k - O > 0 ? k - O : 0, thi = k < T ? k : T;
        for (int t = tlo + lane; t <= thi; t += 64) {
            const int o = k - t;
            double v = INFINITY;
            if (t != 0 && o != 0) {
                const double d = p2[t - 1], x = p1[t - 1], y = p1[t];
                const double u = t_is_q ? x : y, l = t_is_q ? y : x;  // D[i-1, j], D[i, j-1]
                const int i = t_is_q ? t : o, j = t_is_q ? o : t;
                const int cell = (i - 1) * lr + (j - 1);
                const double cost = 1.0 - (double)sims[cell];
                const double ud = u < d ? u : d;
                v = cost + (ud < l ? ud : l);
                // the traceback's choice at this cell: diagonal, else the step in q, else the step in r
                dirs[cell] = (d <= u && d <= l) ? 0 : (u <= l ? 1 : 2);
            }
            cur[t] = v;
        }
        __syncthreads();
        double* const x = p2;
        p2 = p1;
        p1 = cur;
        cur = x;
    }

    // ---- 2. traceback from the far corner, then the path forwards: runs (lane 0; O(lq + lr)) ----
    int nruns = 0;
    if (lane == 0) {
        int i = lq, j = lr, P = 0;
        for (int s = 0; s < lq + lr; ++s) {
            if (i == 1 && j == 1) break;
            // (row 1 can only go left and column 1 only up: whatever the byte holds, the walk stays inside the matrix)
            const int dir = i == 1 ? 2 : (j == 1 ? 1 : dirs[(i - 1) * lr + (j - 1)]);
            steps[P++] = (unsigned char)dir;
            if (dir != 2) --i;
            if (dir != 1) --j;
        }
        const float min_sim_f = (float)prm.min_sim;
        bool open = false;
        int misses = 0, qa = 0, ra = 0, qb = 0, rb = 0;
        double score = 0.0;
        i = j = 0;
        for (int p = 0; p <= P; ++p) {
            if (p > 0) {
                const int dir = steps[P - p];
                if (dir != 2) ++i;
                if (dir != 1) ++j;
            }
            const float s = sims[i * lr + j];
            bool close = false;
            if (s >= min_sim_f) {
                if (!open) {
                    open = true;
                    score = 0.0;
                    qa = i;
                    ra = j;
                }
                qb = i;
                rb = j;
                misses = 0;
                score += (double)s;
            } else if (open) {
                close = ++misses > prm.discontinue;
            }
            if ((close || (p == P && open)) && nruns < run_cap) {
                // (the path is monotone: the run's box is spanned by its first and last matching cell)
                run_score[nruns] = score;
                run_box[4 * nruns + 0] = (unsigned short)qa;
                run_box[4 * nruns + 1] = (unsigned short)ra;
                run_box[4 * nruns + 2] = (unsigned short)qb;
                run_box[4 * nruns + 3] = (unsigned short)rb;
                ++nruns;
                open = false;
            }
        }
    }
    nruns = __shfl(nruns, 0);
    __syncthreads();

    // ---- 3. runs by (-score, run number) through the keep filter: one wave-wide selection per run ----
    double prev_s = INFINITY;
    int prev_k = -1;
    for (int it = 0; it < nruns; ++it) {
        double bs = 0.0;
        int bk = -1;
        for (int k = lane; k < nruns; k += 64) {
            const double s = run_score[k];
            const bool after = s < prev_s || (s == prev_s && k > prev_k);
            if (after && (bk < 0 || s > bs)) {  // (k ascends per lane: of equal scores the first stays)
                bs = s;
                bk = k;
            }
        }
        wave_first_max_f64(bs, bk);
        if (bk < 0) break;
        const unsigned short* b = run_box + 4 * bk;
        if (align_keep(kept, nkept, b[0], b[1], b[2], b[3], prm, lane) == 2) return 2;
        prev_s = bs;
        prev_k = bk;
    }
    return 0;
}

// DP.  Always status 0: max_path <= VSC_TN_MAX_BOXES paths are extracted at most.
__device__ __forceinline__ int align_dp(char* smem, const AlignLayout& L, const float* sims, int lq, int lr, const vsc_align_params& prm,
                                        int* kept, int& nkept, int lane) {
    double* S = reinterpret_cast<double*>(smem + L.f64);
    int* boxes = reinterpret_cast<int*>(smem + L.runs);
    unsigned short* back = reinterpret_cast<unsigned short*>(smem + L.u16);
    unsigned char* row_dead = reinterpret_cast<unsigned char*>(smem + L.bytes);
    unsigned char* col_dead = row_dead + lq;
    for (int x = lane; x < lq + lr; x += 64) row_dead[x] = 0;
    __syncthreads();
    const float min_sim_f = (float)prm.min_sim;
    const int reach = prm.discontinue + 1;
    int nb = 0;
    for (int round = 0; round < prm.max_path; ++round) {
        // S of every cell on what is still alive; the first maximum in row-major order is picked up on the way (a lane
        // sees its cells in ascending flat index)
        double best = -INFINITY;
        int bidx = -1;
        for (int i = 0; i < lq; ++i) {
            const bool rdead = row_dead[i] != 0;
            for (int j = lane; j < lr; j += 64) {
                double pb = 0.0;
                int arg = 0;
                // predecessor steps (a, b) in the host's order: by a + b, then a; replaced on strict '>' only
                for (int sum = 2; sum <= 2 * reach; ++sum) {
                    const int a_lo = sum - reach > 1 ? sum - reach : 1, a_hi = sum - 1 < reach ? sum - 1 : reach;
                    for (int a = a_lo; a <= a_hi; ++a) {
                        const int b = sum - a;
                        if (i - a < 0 || b >= lr) continue;
                        if (j >= b) {
                            const double prev = S[(i - a) * lr + (j - b)];
                            if (prev > pb) {
                                pb = prev;
                                arg = (a << 8) | b;
                            }
                        }
                    }
                }
                const float s = sims[i * lr + j];
                const bool alive = s >= min_sim_f && !rdead && col_dead[j] == 0;
                const double gain = (double)s - prm.min_sim;
                const double v = alive ? gain + pb : -INFINITY;
                S[i * lr + j] = v;
                back[i * lr + j] = (unsigned short)arg;
                if (v > best) {
                    best = v;
                    bidx = i * lr + j;
                }
            }
            __syncthreads();
        }
        wave_first_max_f64(best, bidx);
        if (bidx < 0 || !(best < INFINITY)) break;  // nothing alive (all -inf), or not finite
        // walk back to the start of the path (every lane alike): q strictly decreases, lq steps at most
        const int q1 = bidx / lr, r1 = bidx - q1 * lr;
        int q0 = q1, r0 = r1;
        for (int s = 0; s < lq; ++s) {
            const int bk = back[q0 * lr + r0];
            const int a = bk >> 8, b = bk & 255;
            if (a == 0 || q0 - a < 0 || r0 - b < 0) break;
            q0 -= a;
            r0 -= b;
        }
        if (lane == 0) {
            boxes[4 * nb + 0] = q0;
            boxes[4 * nb + 1] = r0;
            boxes[4 * nb + 2] = q1;
            boxes[4 * nb + 3] = r1;
        }
        ++nb;
        // the frames of this path take part in no further path
        for (int x = q0 + lane; x <= q1; x += 64) row_dead[x] = 1;
        for (int x = r0 + lane; x <= r1; x += 64) col_dead[x] = 1;
        __syncthreads();
    }
    __syncthreads();
    for (int k = 0; k < nb; ++k) align_keep(kept, nkept, boxes[4 * k], boxes[4 * k + 1], boxes[4 * k + 2], boxes[4 * k + 3], prm, lane);
    return 0;
}

template <bool RH16>
__global__ __launch_bounds__(64) void align_pair_kernel(AlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.n_work) return;
    const int pidx = a.work[blockIdx.x];
    int64_t qrow0 = 0, rrow0 = 0;
    int lq, lr;
    if (a.sims_in) {  // forward_sim mode: the caller supplies the similarity matrices
        lq = a.sims_lq[pidx];
        lr = a.sims_lr[pidx];
    } else {
        const int qv = a.pair_q[pidx], rv = a.pair_r[pidx];
        qrow0 = a.q_off[qv];
        rrow0 = a.r_off[rv];
        const int64_t nq = a.q_off[qv + 1] - qrow0, nr = a.r_off[rv + 1] - rrow0;
        lq = (int)(nq < 0x7fffffff ? nq : 0x7fffffff);
        lr = (int)(nr < 0x7fffffff ? nr : 0x7fffffff);
    }
    int32_t* o_boxes = a.out_boxes + (int64_t)pidx * VSC_TN_MAX_BOXES * 4;
    float* o_bmax = a.out_boxmax + (int64_t)pidx * VSC_TN_MAX_BOXES;
    const bool empty = lq <= 0 || lr <= 0;
    if (empty || (int64_t)lq * lr > VSC_ALIGN_MAX_CELLS) {
        if (lane == 0) {
            a.out_nbox[pidx] = 0;
            a.out_status[pidx] = empty ? 0 : 1;
        }
        return;
    }
    const AlignLayout L = align_layout(a.prm.method, lq, lr, a.sims_in == nullptr);
    const float* sims;
    if (a.sims_in) {
        sims = a.sims_in + a.sims_off[pidx];
    } else {
        float* tile = reinterpret_cast<float*>(smem + L.tile);
        tn_sims_tile<RH16>(a, qrow0, rrow0, lq, lr, tile, lane);
        sims = tile;
    }
    __syncthreads();
    int* kept = reinterpret_cast<int*>(smem + L.kept);
    int nkept = 0;
    const int status = a.prm.method == VSC_ALIGN_DTW ? align_dtw(smem, L, sims, lq, lr, a.prm, kept, nkept, lane)
                                                     : align_dp(smem, L, sims, lq, lr, a.prm, kept, nkept, lane);
    if (status != 0) nkept = 0;
    for (int k = 0; k < nkept; ++k) {
        const int bq0 = kept[4 * k], br0 = kept[4 * k + 1], bq1 = kept[4 * k + 2], br1 = kept[4 * k + 3];
        // MaxSim box score: max of sims[q_lo:q_hi, r_lo:r_hi] (half-open, localization.py:91) - bias
        float m = -INFINITY;
        const int w = br1 - br0, h = bq1 - bq0;
        for (int y = 0; y < h; ++y) {
            const float* srow = sims + (int64_t)(bq0 + y) * lr + br0;
            for (int x = lane; x < w; x += 64) {
                const float s = srow[x];
                m = s > m ? s : m;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float o2 = __shfl_xor(m, off);
            m = o2 > m ? o2 : m;
        }
        if (lane == 0) {
            o_boxes[4 * k + 0] = bq0;
            o_boxes[4 * k + 1] = br0;
            o_boxes[4 * k + 2] = bq1;
            o_boxes[4 * k + 3] = br1;
            o_bmax[k] = __fsub_rn(m, a.bias);
        }
    }
    if (lane == 0) {
        a.out_nbox[pidx] = nkept;
        a.out_status[pidx] = status;
    }
}

template <bool RH16>
static int launch_align_pairs_from(const AlignArgs& a, size_t lds_bytes, hipStream_t stream) {
    static PerDeviceOnce once;  // (one per reference source: the attribute belongs to the instantiation)
    if (once.first()) {
        VSC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&align_pair_kernel<RH16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)ALIGN_LDS_MAX));
        once.commit();
    }
    hipLaunchKernelGGL((align_pair_kernel<RH16>), dim3((unsigned)a.n_work), dim3(64), lds_bytes, stream, a);
    VSC_HIP(hipGetLastError());
    return VSC_OK;
}

int launch_align_pairs(const AlignArgs& a, size_t lds_bytes, hipStream_t stream) {
    if (a.n_work <= 0) return VSC_OK;
    if (lds_bytes > ALIGN_LDS_MAX) {
        set_error("align: %zu bytes of LDS asked for, %zu at most", lds_bytes, (size_t)ALIGN_LDS_MAX);
        return VSC_ERR_INVALID;
    }
    // (forward_sim mode reads no descriptors: rfeat_h is never set there)
    return a.rfeat_h ? launch_align_pairs_from<true>(a, lds_bytes, stream) : launch_align_pairs_from<false>(a, lds_bytes, stream);
}

}  // namespace vscmi
