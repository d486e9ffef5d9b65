// C ABI of libvscmi.so, part 2: the thresholded searches -- the batch schedule of vsc_index_global_topk
// (vsc/index.py:142-165), its seeded form, vsc_index_candidates, vsc_index_range_search -- and the batch machinery
// (pre-filter launch + candidate list + exact stage) that the k-NN's threshold passes share (api_knn.hip).
#include "api_internal.h"

// One pre-filtered batch as its steps see it: query rows [i0, i0 + nq) of the packed image against the reference rows
// [nr_begin, nr_end); row_thr = the k-NN's per-row thresholds (indexed by absolute row), nullptr = the search radius.
struct F16Batch {
    const float* qpacked;
    int64_t i0;
    int nq;
    const float* row_thr;
    int64_t nr_begin, nr_end;
    int64_t nrefs() const { return nr_end - nr_begin; }  // rows the kernels see
};

// |fp16 score - exact score| <= c1 |q||r| + c2 (|q| + |r|) + c3   (|x| = L2 norm):
//   rounding to fp16: |x - h(x)| <= 2^-11 |x| + 2^-25 per element (normal / subnormal range)
//     => sum |q r - h(q) h(r)| <= (2^-10 + 2^-22) |q||r| + 2^-25 * 1.001 * sqrt(D) (|q|+|r|) + D 2^-50
//   accumulation: the exact fp32 fma chain (D roundings) and the MFMA's fp32 accumulation
//     (D/16 instructions of 16 products + addend) each stay within 2^-23 |q||r| per operation
struct F16Bound { float c1, c2, c3; };
static F16Bound f16_bound(int dpadh) {
    const double D = (double)dpadh;
    return {(float)(ldexp(1.0, -10) + ldexp(1.0, -22) + (2.0 * D + D / 16.0 + 16.0) * ldexp(1.0, -23)),
            (float)(ldexp(1.0, -25) * 1.001 * sqrt(D)), (float)(D * ldexp(1.0, -50))};
}

// The candidate list of one pre-filter launch of `grid` workgroups (cand_list.h): `ccap` entries in per-wave segments +
// the chunked tail behind them, in the workspace's arrays.  The same block goes to the launch and to the exact stage.
static int cand_list_plan(vsc_index* idx, int64_t ccap, int grid, CandList& l) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    l.i = idx->ws.ci.as<int32_t>();
    l.j = idx->ws.cj.as<int32_t>();
    l.n_seg = grid * 8;
    l.seg_cap = (int)std::min<int64_t>(ccap / l.n_seg, 0x7fffffff);
    l.seg_count = idx->ws.segcnt.as<int>();
    l.tail_base = (int64_t)l.seg_cap * l.n_seg;
    l.tail_cap = cand_entries(ccap) - l.tail_base;
    l.tail_shift = tail_chunk_shift_for(l.tail_cap, l.n_seg);
    VSC_TRY(idx->ws.tailfill.reserve((size_t)((l.tail_cap >> l.tail_shift) + 2) * sizeof(int)));
    l.tail_fill = idx->ws.tailfill.as<int>();
    l.tail_count = &ctl->n_tail;
    l.overflow = &ctl->overflow;
    return VSC_OK;
}

// The three pre-filter launches.  Each fills its kernel's arg block, plans the candidate list `cl` for its grid and
// opens its profiling bracket right before the launch (`stop`; enqueue_f16 closes it).

// dims > 512: 256x256 LDS-ring kernel (sim_f16.hip) on the natural image
static int prefilter_f16_ring(vsc_index* idx, const F16Batch& b, int64_t ccap, const F16Bound& fb, CandList& cl, hipEvent_t* stop) {
    SimF16Args f;
    f.Q = idx->ws.qh.as<_Float16>() + b.i0 * idx->dpadh;
    f.R = idx->refh.as<_Float16>() + b.nr_begin * idx->dpadh;
    f.qn = idx->ws.qn.as<float>() + b.i0;
    f.rn = idx->refn.as<float>() + b.nr_begin;
    f.dpadh = idx->dpadh;
    f.nq = b.nq;
    f.i0 = (int)b.i0;
    f.nr = (int)b.nrefs();
    f.tq = (b.nq + 255) / 256;
    f.tr = (int)((b.nrefs() + 255) / 256);
    f.c1 = fb.c1; f.c2 = fb.c2; f.c3 = fb.c3;
    f.radius = &idx->ws.ctl.as<SelectCtl>()->radius;
    f.row_thr = b.row_thr ? b.row_thr + b.i0 : nullptr;
    VSC_TRY(cand_list_plan(idx, ccap, sim_f16_grid(f.tq, f.tr), cl));
    f.list = cl;
    VSC_TRY(prof_begin(idx, stop, 1));
    return launch_sim_f16(f, idx->stream);
}

// panel-stationary kernel (sim_f16p.hip): LDS-resident query panels x the fragment-major reference image
static int prefilter_f16_panel(vsc_index* idx, const F16Batch& b, int64_t ccap, const F16Bound& fb, CandList& cl, hipEvent_t* stop) {
    SimF16PArgs f;
    int grid = 0;
    sim_f16p_plan(b.nq, b.nrefs(), &f.npanel, &f.nsteps, &f.slice, &grid);
    VSC_TRY(idx->ws.slices.reserve((size_t)f.npanel * sizeof(int)));
    f.Q = idx->ws.qh.as<_Float16>() + b.i0 * idx->dpadh;
    f.Rf = static_cast<const char*>(idx->refh.p) + b.nr_begin * idx->dpadh * 2;
    f.qn = idx->ws.qn.as<float>() + b.i0;
    f.rn = idx->refn.as<float>() + b.nr_begin;
    f.dpadh = idx->dpadh;
    f.nq = b.nq;
    f.i0 = (int)b.i0;
    f.nr = (int)b.nrefs();
    f.next_slice = idx->ws.slices.as<int>();
    f.c1 = fb.c1; f.c2 = fb.c2; f.c3 = fb.c3;
    f.radius = &idx->ws.ctl.as<SelectCtl>()->radius;
    f.row_thr = b.row_thr ? b.row_thr + b.i0 : nullptr;
    f.floor = idx->defer_now && !b.row_thr ? &idx->ws.ctl.as<SelectCtl>()->floor : nullptr;
    VSC_TRY(cand_list_plan(idx, ccap, grid, cl));
    f.list = cl;
    VSC_TRY(prof_begin(idx, stop, 1));
    return launch_sim_f16p(f, grid, idx->stream);
}

// The int8 launch's preamble: the rows' thresholds with what the images leave out folded in, the order the launch sees
// its rows in, and the launch's own int8 image (`npanel_q` panels, one scale per 128-row panel).  Returns `perm`
// (perm[position] = row; nullptr: the rows' own order) and `rt_pos`, the thresholds in position order (nullptr: the
// search radius for all rows).
static int i8_preamble(vsc_index* idx, const F16Batch& b, int npanel_q, const int32_t** perm_out, float** rt_pos_out) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    Workspace& ws = idx->ws;
    const float* q = b.qpacked + b.i0 * idx->dpad;
    const int nqb = b.nq;
    const int32_t* perm = nullptr;
    float* rt_pos = nullptr;
    const float* thr_src = b.row_thr ? b.row_thr + b.i0 : nullptr;
    if (idx->i8_ex.n > 0 || idx->i8_mu_on) {
        // coordinates the images leave out (all references agree on them) act through the rows' thresholds:
        // t_row - sum_c q_c v_c, with t_row the row's k-NN threshold or the search radius; a centred reference
        // image (quant_i8.hip) adds the rows' x . mu the same way
        VSC_TRY(ws.rt8b.reserve((size_t)nqb * sizeof(float)));
        const float *cen = nullptr, *cmag = nullptr;
        if (idx->i8_mu_on) {
            VSC_TRY(ws.rt8d.reserve((size_t)2 * nqb * sizeof(float)));
            VSC_TRY(launch_row_center(q, idx->dpad, nqb, idx->i8_mu.as<float>(), ws.rt8d.as<float>(), ws.rt8d.as<float>() + nqb,
                                      idx->stream));
            cen = ws.rt8d.as<float>();
            cmag = cen + nqb;
        }
        VSC_TRY(launch_row_bias_thresholds(q, idx->dpad, nqb, thr_src, &ctl->radius, idx->i8_ex, cen, cmag, ws.rt8b.as<float>(),
                                           idx->stream));
        thr_src = ws.rt8b.as<float>();
    }
    // VSC_I8_SORT=0: rows in their own order (A/B; the kernel then gates blocks of unrelated thresholds)
    const bool sort_rows = idx->i8_sort_rows;
    if (thr_src) {
        VSC_TRY(ws.rt8.reserve((size_t)npanel_q * F16P_PANEL_ROWS * sizeof(float)));
        rt_pos = ws.rt8.as<float>();
    }
    if (thr_src && sort_rows) {
        // thresholds that differ from row to row: the launch sees its rows sorted by threshold (the kernel
        // gates a tile by its panel's smallest threshold and a 16-row block by the block's)
        if (idx->i8_group_shift > 0 && !b.row_thr && nqb >= (4 << idx->i8_group_shift)) {
            // ... and, inside groups of 512 positions of that order, by the rows' largest element (sortpairs.hip).
            // Only for the radius search over excluded coordinates (thresholds = radius - the rows' bias: a
            // narrow spread): configs[3] 1162 -> 1086 M candidates, exact stage 367 -> 341 ms (groups of 256 /
            // 512 / 1024 / 2048 / 4096: 1110 / 1086 / 1090 / 1125 / 1205 M).  The k-NN's thresholds -- each
            // row's best score so far -- spread far more: there the same grouping cost 2 % (892 -> 907 ms).
            VSC_TRY(ws.rt8c.reserve((size_t)nqb * sizeof(float)));
            VSC_TRY(launch_row_absmax(q, idx->dpad, nqb, idx->i8_ex, ws.rt8c.as<float>(), idx->stream));
            VSC_TRY(sort_rows_by_threshold_then_scale(thr_src, ws.rt8c.as<float>(), nqb, idx->i8_group_shift, ws.sort, &perm,
                                                      idx->stream));
        } else {
            VSC_TRY(sort_rows_by_threshold(thr_src, nqb, ws.sort, &perm, idx->stream));
        }
    } else if (!thr_src && sort_rows && nqb >= 2 * F16P_PANEL_ROWS) {
        // one threshold for all rows (the search radius): sort by the rows' largest element instead, so that
        // a panel's shared scale is close to what each of its rows would have chosen (VSC_I8_SORT=0: off)
        VSC_TRY(ws.rt8b.reserve((size_t)nqb * sizeof(float)));
        VSC_TRY(launch_row_absmax(q, idx->dpad, nqb, idx->i8_ex, ws.rt8b.as<float>(), idx->stream));
        VSC_TRY(sort_rows_by_threshold(ws.rt8b.as<float>(), nqb, ws.sort, &perm, idx->stream));
    }
    VSC_TRY(launch_quant_query_panels(q, idx->dpad, nqb, npanel_q, ws.q8.p, idx->dpad8, ws.pstat.as<float4>(), perm, thr_src,
                                      rt_pos, idx->i8_ex, idx->stream));
    *perm_out = perm;
    *rt_pos_out = rt_pos;
    return VSC_OK;
}

// int8 panel kernel (sim_i8p.hip): this launch's rows are quantised first, one scale per 128-row panel.  `perm` is set
// when the candidate list will hold positions of a permuted launch.
static int prefilter_i8(vsc_index* idx, const F16Batch& b, int64_t ccap, CandList& cl, const int32_t** perm, hipEvent_t* stop) {
    SimI8PArgs f;
    int grid = 0;
    sim_f16p_plan(b.nq, b.nrefs(), &f.npanel, &f.nsteps, &f.slice, &grid);
    {
        // work order: slice-major items.  r03 (32x32x32 kernel): items of 16 col-steps (4 MiB of the int8 image at
        // 512-d: what an XCD's L2 holds) +3 % on the bench over panel-major (2431 -> 2507-2515 TOP/s).  r04
        // (16x16x64 kernel, configs[3]): 8 / 16 / 32 / 64 col-steps 2456 / 2390 / 2363 / 2368 ms per query set
        // -- the faster K loop makes the hand-over (panel load + two barriers) the larger share: 32.
        // VSC_I8P_ORDER=0: panel-major with stealing as in sim_f16p
        const int slice_env = idx->i8p_slice;
        f.order = idx->i8p_order;
        if (f.order == 1) f.slice = std::max(1, std::min(f.nsteps, slice_env > 0 ? slice_env : 32));
        else if (slice_env > 0) f.slice = std::max(1, std::min(f.nsteps, slice_env));
    }
    // work items of two panels (wave tiles of 256 rows x 32 columns: half the reference bytes per MFMA) where the
    // launch is large enough; the quantised image then holds an even number of panels.  VSC_I8P_PAIR=0: off
    f.pair = idx->i8p_pair && sim_i8p_pairs(idx->dpad8, f.npanel, f.nsteps, f.slice, idx->i8p_pair == 2) ? 1 : 0;
    const int npanel_q = f.pair ? (f.npanel + 1) & ~1 : f.npanel;
    VSC_TRY(idx->ws.slices.reserve(((size_t)f.npanel + 1) * sizeof(int)));
    VSC_TRY(idx->ws.q8.reserve((size_t)npanel_q * F16P_PANEL_ROWS * idx->dpad8));
    VSC_TRY(idx->ws.pstat.reserve((size_t)npanel_q * sizeof(float4)));
    hipEvent_t prep_stop;
    VSC_TRY(prof_begin(idx, &prep_stop, 6));
    float* rt_pos = nullptr;
    VSC_TRY(i8_preamble(idx, b, npanel_q, perm, &rt_pos));
    f.Q = idx->ws.q8.p;
    f.pstat = idx->ws.pstat.as<float4>();
    f.Rf = static_cast<const char*>(idx->ref8.p) + b.nr_begin * idx->dpad8;  // (whole 64-row tiles: dpad8 x 64 B each)
    f.rmeta = idx->ref8m.as<float4>() + b.nr_begin;
    f.dpad8 = idx->dpad8;
    f.nq = b.nq;
    f.i0 = (int)b.i0;
    f.nr = (int)b.nrefs();
    f.next_slice = idx->ws.slices.as<int>();
    // the exact fp32 chain is within dpad 2^-24 |q||r| (1 + tiny) of the real inner product
    f.c_acc = (float)(((double)idx->dpad + 2.0) * ldexp(1.0, -23));
    f.radius = &idx->ws.ctl.as<SelectCtl>()->radius;
    f.row_thr = rt_pos;
    VSC_TRY(cand_list_plan(idx, ccap, grid, cl));
    f.list = cl;
    VSC_TRY(prof_end(idx, prep_stop, 0.0, 6));
    VSC_TRY(prof_begin(idx, stop, 5));  // (the kernel alone: what the roofline figure is about)
    return launch_sim_i8p(f, grid, idx->stream);
}

// What every launch of the exact stage shares: the images, the kept-hit list behind the search's control block.
static RescoreArgs rescore_args(vsc_index* idx, const float* qpacked, int64_t cap) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    const HitView kept = idx->ws.hits_a();
    RescoreArgs r;
    r.Q = qpacked;
    r.R = idx->ref.as<float>();
    r.dpad = idx->dpad;
    r.perm = nullptr;
    r.perm_i0 = 0;
    r.n_cand_total = &ctl->n_cand_total;
    r.radius = &ctl->radius;
    r.out_i = kept.i;
    r.out_j = kept.j;
    r.out_s = kept.s;
    r.counter = &ctl->n;
    r.cap = cap;
    r.row_thr = nullptr;
    if (sq16(idx)) {  // the reference rows come from the fp16 store (rescore.hip: rescore_list<SRC>)
        r.R = nullptr;
        r.Rh = idx->refh.as<_Float16>();
        r.dpadh = idx->dpadh;
        r.rsrc = idx->frag ? 2 : 1;
    }
    return r;
}

// Exact scores of a launch's candidates `cl`; those above the radius (at or above the row's threshold) join the kept
// hits, at most `cap` of them.  `perm`: the list holds positions of a permuted int8 launch; `from_i8`: the candidates
// may pass the fp16 screen first.
static int exact_stage(vsc_index* idx, const F16Batch& b, int64_t cap, const CandList& cl, const int32_t* perm,
                       const F16Bound& fb, bool from_i8) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    Workspace& ws = idx->ws;
    RescoreArgs r = rescore_args(idx, b.qpacked, cap);
    r.list = cl;
    r.perm = perm;
    r.perm_i0 = (int)b.i0;
    r.row_thr = b.row_thr;
    r.j0 = (int)b.nr_begin;
    // The candidates are compacted out of the waves' segments, sorted by reference row and re-scored as one dense
    // list (rescore.hip, "candidates ordered by reference row"): 74 -> 54 ms per bench step, k-NN k = 20 140 ->
    // 100 ms.  It needs the candidate count on the host (buffer sizes, grid of the sort): one stream sync per
    // launch, ~20 us against launches of 3-30 ms.  VSC_RESCORE_SORT=0: the segments as they are.
    if (!idx->rescore_by_ref) return launch_rescore(r, idx->stream);
    // count first (one tiny kernel + the stream sync the sort needs anyway), then size the four dense lists of
    // the sort from what the launch really left behind -- not from the list's capacity (96 bytes
    // per unit of capacity, 26 GB for a default range search whose launches hold a few percent of that)
    VSC_TRY(ws.csn.reserve(3 * sizeof(unsigned long long)));
    unsigned long long* csn = ws.csn.as<unsigned long long>();
    const int n_chunks_max = (int)std::min<long long>((cl.tail_cap >> cl.tail_shift) + 1, 1 << 20);
    VSC_TRY(launch_cand_count(r, n_chunks_max, csn + 2, idx->stream));
    unsigned long long n_c = 0;
    VSC_HIP(hipMemcpyAsync(&n_c, csn + 2, sizeof(n_c), hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    // (grown in steps of a quarter so that launches of slowly varying size do not reallocate every time)
    const size_t cap_e = (size_t)(n_c + n_c / 4 + 4096);
    for (auto& buf : ws.cs)
        if (buf.bytes < (size_t)(n_c + 1) * sizeof(uint32_t)) VSC_TRY(buf.reserve(cap_e * sizeof(uint32_t)));
    uint32_t* cs[4] = {ws.cs[0].as<uint32_t>(), ws.cs[1].as<uint32_t>(), ws.cs[2].as<uint32_t>(), ws.cs[3].as<uint32_t>()};
    // Deferred rescoring: this batch runs with a floor.  The deferred set D is as large as the kept-hit list (its pairs
    // are kept hits); an fp16 launch has marked the pairs that go there (cand_compact moves them, and the dense list's
    // length is then read back: the one extra read of a deferring batch), an int8 launch's pairs are told apart by
    // the fp16 screen below.
    const bool defer = idx->defer_now && !b.row_thr;
    if (defer) {
        for (auto& buf : ws.dd) VSC_TRY(buf.reserve((size_t)cap * sizeof(int32_t)));
        if (!from_i8) {
            r.d_i = ws.dd[0].as<int32_t>();
            r.d_j = ws.dd[1].as<int32_t>();
            r.d_count = &ctl->n_d;
            r.d_total = &ctl->n_deferred;
            r.d_cap = cap;
        }
    }
    VSC_TRY(launch_cand_compact(r, n_chunks_max, cs[0], cs[2], csn, idx->stream));
    if (r.d_i) {
        VSC_HIP(hipMemcpyAsync(&n_c, csn, sizeof(n_c), hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipStreamSynchronize(idx->stream));
    }
    const uint32_t *sj = nullptr, *si = nullptr;
    VSC_TRY(sort_candidates_by_ref(cs[0], cs[1], cs[2], cs[3], (int64_t)n_c, b.nr_end, ws.cstmp, &sj, &si, idx->stream));
    // VSC_I8_SCREEN=1: int8 launches pass an fp16 screen first (rescore.hip: f16_screen_kernel).  Measured
    // neutral and therefore OFF by default: 29 % of the int8 candidates survive it (bench, 128 M -> 37 M per
    // step), the screen moves half the bytes per pair (23.8 ms) and the exact stage then costs 35.6 instead of
    // 59.8 ms -- both stages gather one query row per pair from the Infinity Cache at ~6 TB/s, which is the
    // bound (profiles/r03_prefilter_attribution.md).  Kept because it pays once the survivor share drops
    // (descriptors with outlier coordinates widen the int8 bound, not the fp16 one) -- and in a batch that defers: there
    // the screen also takes out the pairs whose exact score can wait (configs[3]: the step gains 20 ms by it,
    // profiles/deferred_rescoring.md).
    if (!(from_i8 && (idx->i8_screen || defer) && n_c > 0)) return launch_rescore_dense(r, sj, si, (long long)n_c, idx->stream);
    ScreenArgs sa;
    if (defer) {
        sa.floor = &ctl->floor;
        sa.d_i = ws.dd[0].as<int32_t>();
        sa.d_j = ws.dd[1].as<int32_t>();
        sa.d_count = &ctl->n_d;
        sa.d_total = &ctl->n_deferred;
        sa.d_cap = cap;
    }
    sa.Qh = ws.qh.as<_Float16>();
    sa.qn = ws.qn.as<float>();
    sa.Rh = idx->refh.as<_Float16>();
    sa.rn = idx->refn.as<float>();
    sa.dpadh = idx->dpadh;
    sa.frag = idx->frag ? 1 : 0;
    sa.c1 = fb.c1; sa.c2 = fb.c2; sa.c3 = fb.c3;
    sa.radius = &ctl->radius;
    sa.row_thr = b.row_thr;
    sa.sj = sj;
    sa.si = si;
    sa.n = (long long)n_c;
    sa.out_j = sj == cs[0] ? cs[1] : cs[0];
    sa.out_i = si == cs[2] ? cs[3] : cs[2];
    sa.n_out = csn + 1;
    sa.n_cand_total = &ctl->n_cand_total;
    sa.overflow = &ctl->overflow;
    VSC_TRY(launch_f16_screen(sa, idx->stream));
    VSC_TRY(launch_rescore_dense(r, sa.out_j, sa.out_i, (long long)n_c, idx->stream, sa.n_out));
    if (idx->debug_screen) {
        unsigned long long n_s = 0;
        VSC_HIP(hipMemcpyAsync(&n_s, sa.n_out, sizeof(n_s), hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipStreamSynchronize(idx->stream));
        fprintf(stderr, "[vscmi] fp16 screen: %llu of %llu int8 candidates left (rows %d)\n", n_s, n_c, b.nq);
    }
    return VSC_OK;
}

// fp16 pre-filter + exact re-scoring of query rows [i0, i1): appends to hit buffer A every (row, ref, score)
// with score > *radius -- or, when `row_thr` (one threshold per query row, padded like the fp16 query
// image) is given, with score >= row_thr[row].
int enqueue_f16(vsc_index* idx, const float* qpacked, int64_t i0, int64_t i1, int64_t cap,
                const float* row_thr, int64_t ccap, int64_t nr_limit, bool use_i8, int64_t nr_begin) {
    if (ccap < 0) ccap = cap;  // capacity of the candidate list (cap: of the hit list)
    // [nr_begin, nr_limit): search only these reference rows (the levels of the k-NN); nr_begin a multiple of 64
    // (whole wave tiles of the fragment-major images).  The kernels see the images from row nr_begin on and emit
    // refs relative to it; the exact stage adds the offset back (RescoreArgs::j0).
    const int64_t nr_end = nr_limit >= 0 ? std::min<int64_t>(nr_limit, idx->ntotal) : idx->ntotal;
    if (nr_begin < 0 || nr_begin % 64 != 0 || nr_begin > nr_end) {
        set_error("enqueue_f16: reference range [%lld, %lld) does not start on a 64-row tile", (long long)nr_begin, (long long)nr_end);
        return VSC_ERR_INVALID;
    }
    const F16Batch b{qpacked, i0, (int)(i1 - i0), row_thr, nr_begin, nr_end};
    const F16Bound fb = f16_bound(idx->dpadh);
    // 1. pre-filter: candidates = pairs whose low-precision score + error bound reaches the threshold
    const bool i8 = use_i8 && idx->i8_mode;
    CandList cl;
    const int32_t* perm = nullptr;
    hipEvent_t stop;
    if (i8) VSC_TRY(prefilter_i8(idx, b, ccap, cl, &perm, &stop));
    else if (idx->frag) VSC_TRY(prefilter_f16_panel(idx, b, ccap, fb, cl, &stop));
    else VSC_TRY(prefilter_f16_ring(idx, b, ccap, fb, cl, &stop));
    VSC_TRY(prof_end(idx, stop, 2.0 * (double)b.nq * (double)b.nrefs() * (double)idx->dim, i8 ? 5 : 1));
    // 2. exact scores of the candidates; those above the radius join the kept hits
    VSC_TRY(prof_begin(idx, &stop, 2));
    VSC_TRY(exact_stage(idx, b, cap, cl, perm, fb, i8));
    return prof_end(idx, stop, 0.0, 2);
}

// Append every (row, ref) of query rows [i0, i1) with score > *radius (score space: IP as is, L2
// negated) to the hit buffer A.
static int enqueue_batch(vsc_index* idx, const float* qpacked, int64_t i0, int64_t i1, int64_t cap,
                         bool use_f16 = false, bool use_i8 = false) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    const int nqb = (int)(i1 - i0);
    const HitView kept = idx->ws.hits_a();
    if (use_f16) return enqueue_f16(idx, qpacked, i0, i1, cap, nullptr, -1, -1, use_i8);
    if (idx->metric == VSC_METRIC_INNER_PRODUCT) {
        SimThreshArgs a;
        a.Q = qpacked + i0 * idx->dpad;
        a.dpad = idx->dpad;
        a.nq = nqb;
        a.i0 = (int)i0;
        a.tq = (nqb + 127) / 128;
        a.radius = &ctl->radius;
        a.out_i = kept.i;
        a.out_j = kept.j;
        a.out_s = kept.s;
        a.counter = &ctl->n;
        a.cap = cap;
        a.overflow = &ctl->overflow;
        // the kernel streams whole packed rows, one range of them after the other; the hits a range after the first
        // appends carry refs relative to it and get the range's offset afterwards
        return for_ref_ranges(idx, 0, idx->ntotal, [&](const float* rows, int64_t j0, int64_t n) -> int {
            unsigned long long* mark = nullptr;
            if (j0 > 0) {
                VSC_TRY(idx->ws.flag.reserve(16));
                mark = idx->ws.flag.as<unsigned long long>() + 1;
                VSC_TRY(launch_hits_mark(&ctl->n, mark, idx->stream));
            }
            a.R = rows;
            a.nr = (int)n;
            a.tr = (int)((n + 127) / 128);
            hipEvent_t stop;
            VSC_TRY(prof_begin(idx, &stop));
            VSC_TRY(launch_sim_thresh(a, idx->stream));
            VSC_TRY(prof_end(idx, stop, 2.0 * (double)nqb * (double)n * (double)idx->dim));
            if (j0 > 0) VSC_TRY(launch_hits_add_offset(a.out_j, mark, &ctl->n, cap, (int)j0, idx->stream));
            return VSC_OK;
        });
    }
    // generic metric: explicit score matrix in row chunks
    const int64_t nr = idx->ntotal;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nqb, (int64_t)(1ll << 28) / std::max<int64_t>(nr, 1)));
    VSC_TRY(idx->ws.mat.reserve((size_t)chunk * nr * 4));
    for (int64_t r0 = i0; r0 < i1; r0 += chunk) {
        const int rows = (int)std::min(chunk, i1 - r0);
        ScoreMatArgs m{qpacked + r0 * idx->dpad, idx->ref.as<float>(), idx->dpad, idx->dim, rows, (int)nr,
                       idx->metric, idx->ws.mat.as<float>()};
        if (sq16(idx)) VSC_TRY(launch_score_matrix_h16(m, idx->refh.as<_Float16>(), idx->dpadh, idx->frag, idx->stream));
        else VSC_TRY(launch_score_matrix(m, idx->stream));
        MatThreshArgs t{idx->ws.mat.as<float>(), rows, (int)nr, (int)r0, &ctl->radius, kept.i, kept.j, kept.s,
                        &ctl->n, cap, &ctl->overflow};
        VSC_TRY(launch_matrix_thresh(t, idx->stream));
    }
    return VSC_OK;
}

// ---- the deferred set
// range_search_max_results searches every batch at the radius of the LAST event, far below the one the next event will
// set: about half of a batch's new hits are dropped again by that event.  Their exact scores are never looked at -- the
// event only needs to know that they exist (the predicate kept > 2K) and that they lie at or below the new radius.  So
// the kept set is held in two parts: A, the hit buffer with exact scores, and D, (row, ref) pairs whose exact score is
// PROVEN (by the pre-filter's score and error bound) to lie in (radius, floor] and has not been computed.  The floor is a
// guess of where the next radius will land: the score of rank (K + 1) b / b_next (1 + margin) among the kept hits of the
// b rows seen so far, b_next = the boundary at which the predicate is expected to pass.
//   event (select.hip, PICK_TRIAL): predicate n_A + n_D > 2K; v = (K+1)-th best of A alone.  v >= floor: every pair of D
//     is <= floor <= v, so v is the (K+1)-th best of A and D together and D falls to the strict re-filter -- exactly the
//     reference's step, with D never scored.  Else D is re-scored into A first (force_deferred) and the ordinary round
//     runs: a wrong guess costs D's own re-scoring and one more selection, never a restart.
//   no event: D stays outstanding (the radius has not moved, so its proof holds); the end of the search re-scores it.
// Results, order, radius and the number of events are those of defer = 0 whatever the floor is.

// Re-score the n_d pairs of D into the kept hits (sorted by reference row, the exact stage's dense form).  Every one of
// them must pass score > radius: anything else means a pair was deferred without proof.
static int force_deferred(vsc_index* idx, const float* qpacked, int64_t cap, unsigned long long n_d, unsigned long long n_before) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    Workspace& ws = idx->ws;
    if (n_d == 0) return launch_defer_reset(ctl, idx->stream);
    hipEvent_t stop;
    VSC_TRY(prof_begin(idx, &stop, 2));
    const size_t cap_e = (size_t)(n_d + n_d / 4 + 4096);
    for (auto& buf : ws.cs)
        if (buf.bytes < (size_t)(n_d + 1) * sizeof(uint32_t)) VSC_TRY(buf.reserve(cap_e * sizeof(uint32_t)));
    uint32_t* cs[4] = {ws.cs[0].as<uint32_t>(), ws.cs[1].as<uint32_t>(), ws.cs[2].as<uint32_t>(), ws.cs[3].as<uint32_t>()};
    VSC_HIP(hipMemcpyAsync(cs[0], ws.dd[1].p, (size_t)n_d * 4, hipMemcpyDeviceToDevice, idx->stream));
    VSC_HIP(hipMemcpyAsync(cs[2], ws.dd[0].p, (size_t)n_d * 4, hipMemcpyDeviceToDevice, idx->stream));
    const uint32_t *sj = nullptr, *si = nullptr;
    VSC_TRY(sort_candidates_by_ref(cs[0], cs[1], cs[2], cs[3], (int64_t)n_d, idx->ntotal, ws.cstmp, &sj, &si, idx->stream));
    RescoreArgs r = rescore_args(idx, qpacked, cap);
    r.list = CandList{};  // (a dense list: only the overflow word and the tail counter are looked at)
    VSC_TRY(ws.csn.reserve(3 * sizeof(unsigned long long)));
    r.n_cand_total = ws.csn.as<unsigned long long>() + 1;  // (these pairs were counted as candidates when they were deferred)
    r.list.overflow = &ctl->overflow;
    r.list.tail_count = &ctl->n_tail;
    VSC_TRY(launch_rescore_dense(r, sj, si, (long long)n_d, idx->stream));
    VSC_TRY(launch_defer_reset(ctl, idx->stream));
    VSC_TRY(prof_end(idx, stop, 0.0, 2));
    SelectCtl h;
    VSC_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    if (!h.overflow && h.n != n_before + n_d) {
        set_error("global_topk: %llu of %llu deferred pairs did not pass the radius when they were re-scored",
                  n_before + n_d - h.n, n_d);
        return VSC_ERR_INVALID;
    }
    idx->stat_defer_forced += n_d;
    return VSC_OK;
}

// The floor for the batches from row b on (batch [b, i1) of `bs` rows comes next), or none.  n_a kept hits over b rows:
// about n_a e / b at boundary e, so the predicate is expected to pass at the first boundary with n_a e > 2K b.
static int choose_floor(vsc_index* idx, int64_t K, int64_t nq, int64_t b, int64_t i1, int64_t bs, bool* chosen, bool* no_event_left) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    const bool forced = idx->defer == 2;
    *chosen = false;
    SelectCtl h;
    VSC_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    if (h.overflow || h.n == 0 || b <= 0) return VSC_OK;
    int64_t b_next = -1;
    for (int64_t e = i1, sb = bs;;) {
        if ((double)e * (double)h.n > 2.0 * (double)K * (double)b) { b_next = e; break; }
        if (e >= nq) break;
        if (sb < 20000) sb *= 2;
        e = std::min(nq, e + sb);
    }
    if (b_next < 0) {
        // no event can follow: deferring would only add D's re-scoring at the end (and the later batches need not ask)
        if (!forced) { *no_event_left = true; return VSC_OK; }
        b_next = 2 * b;
    }
    const double m = std::ceil(((double)K + 1.0) * ((double)b / (double)b_next) * (1.0 + idx->defer_margin));
    if ((!(m >= 1.0) || m > (double)h.n) && !forced) return VSC_OK;
    const unsigned long long rank = (unsigned long long)std::min(std::max(m, 1.0), (double)h.n) - 1ull;
    hipEvent_t stop;
    VSC_TRY(prof_begin(idx, &stop, 3));
    VSC_TRY(enqueue_floor_select(ctl, idx->ws.hits_a().s, rank, idx->stream));
    VSC_TRY(prof_end(idx, stop, 0.0, 3));
    *chosen = true;
    return VSC_OK;
}

// The batch boundary while a floor is set.  *open stays true when no event took place (D is carried on).
static int deferred_event(vsc_index* idx, const float* qpacked, int64_t K, int64_t cap, bool* open) {
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    hipEvent_t stop;
    VSC_TRY(prof_begin(idx, &stop, 3));
    VSC_TRY(enqueue_rethreshold_deferred(ctl, idx->ws.hits_a(), idx->ws.hits_b(), (unsigned long long)K, idx->stream));
    VSC_TRY(prof_end(idx, stop, 0.0, 3));
    SelectCtl h;
    VSC_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    if (h.overflow) { *open = false; return VSC_OK; }  // (the schedule is rerun with larger buffers)
    if (h.need_force) {
        VSC_TRY(force_deferred(idx, qpacked, cap, h.n_d, h.n));
        idx->stat_defer_events_forced += 1;
        VSC_TRY(prof_begin(idx, &stop, 3));
        VSC_TRY(enqueue_rethreshold(ctl, idx->ws.hits_a(), idx->ws.hits_b(), (unsigned long long)K, idx->stream));
        VSC_TRY(prof_end(idx, stop, 0.0, 3));
        *open = false;
    } else if (!(h.floor < INFINITY)) {
        *open = false;  // the event took place with D left out (or no floor could be chosen)
    }
    return VSC_OK;
}

int init_ctl(vsc_index* idx, float radius_score_space) {
    // (a one-workgroup kernel instead of a host-staged copy + synchronisation: the sharded schedule calls the seeded
    // search once per batch and rank, and every host round trip is ~40 us of idle GPU there -- profiles/r06_rank_work.md)
    return launch_ctl_init(idx->ws.ctl.as<SelectCtl>(), radius_score_space, idx->stream);
}


// The body of vsc_index_global_topk.  seeded = false: the reference's schedule (batches of 32, 64, ... rows doubling
// while < 20000, radius from -1e10).  seeded = true (vsc_index_global_topk_seeded): the caller already knows a radius
// below the K-th best score -- every batch is a steady 32768-row batch from the first row on, pre-filtered from the
// first row on; the re-threshold rule stays (kept > 2K: radius <- (K+1)-th best), so the buffers stay bounded when the
// seed was low.
static int global_topk_impl(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K, bool seeded,
                            float radius0, int32_t* out_i, int32_t* out_j, float* out_s, int64_t cap_out, int out_mem,
                            int64_t* n_out, float* final_radius) {
    if (!idx || nq < 0 || K < 0 || !n_out || (nq > 0 && !q)) {
        set_error("vsc_index_global_topk: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_out = 0;
    const bool ip = idx->metric == VSC_METRIC_INNER_PRODUCT;
    if (final_radius) *final_radius = ip ? -1e10f : 1e10f;
    if (nq == 0 || idx->ntotal == 0) return VSC_OK;
    VSC_HIP(hipSetDevice(idx->device));
    float* qp = nullptr;
    VSC_TRY(pack_queries(idx, q, nq, q_mem, &qp, idx->prefilter));
    VSC_TRY(i8_prepare(idx));
    const int64_t cap_max = nq * idx->ntotal + 1024;  // the whole score matrix always fits
    int64_t cap = idx->hit_cap_user;
    if (cap <= 0) cap = std::max(std::max<int64_t>(32 * idx->ntotal, 2 * K) + 2 * K + 1024, idx->hit_cap_learned);
    cap = std::min<int64_t>(cap, cap_max);
    SelectCtl h;
    bool allow_i8 = i8_usable(idx);
    // deferred rescoring ("the deferred set" above): the reference's own schedule only -- a seeded search has no event to
    // wait for, an unsorted result (the sharded schedule) and a caller-sized hit buffer keep their exact buffer use
    const bool can_defer = idx->defer > 0 && !seeded && ip && idx->sort_hits && idx->hit_cap_user <= 0 && idx->rescore_by_ref && K >= 1;
    for (;;) {
        bool used_i8 = false;
        bool d_open = false;  // a floor is set: the pre-filtered batches defer, D may hold pairs
        bool no_event_left = false;
        idx->stat_deferred = idx->stat_defer_forced = idx->stat_defer_events_ok = idx->stat_defer_events_forced = 0;
        VSC_TRY(ensure_hit_buffers(idx, cap));
        // initial radius -1e10 (IP) / +1e10 (L2) -> -1e10 in score space either way (vsc/index.py:146)
        VSC_TRY(init_ctl(idx, seeded ? (ip ? radius0 : -radius0) : -1e10f));
        SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
        // exponential_query_iterator: 32, 64, ... doubling while bs < 20000
        int64_t bs = seeded ? 32768 : 32, i0 = 0;
        while (i0 < nq) {
            const int64_t i1 = std::min(nq, i0 + bs);
            // (seeded: the radius is already near its final value -- the expected density is that of the whole search)
            const double seen = seeded ? (double)nq : (double)i0;
            // After i0 rows the radius sits near the K-th best of i0 * ntotal scores, so about
            // K / (i0 * ntotal) of this batch's pairs are hits.  While that density is high the
            // exact kernel is cheaper than pre-filtering and re-scoring nearly everything
            // (exact: ~7.5 ps per pair; re-scoring: ~0.5 ns per candidate; measured optimum near 2 % with the segment-wise exact stage, 5 % with the sorted one).
            // (option "density_hint": the caller knows the batch's expected hit density better than K / (rows x refs) says --
            // the sharded schedule's budgets K are several times the hits it expects, which sent int8 batches to fp16)
            const double dens = idx->density_hint > 0.0 ? idx->density_hint
                                                         : (seen > 0 ? (double)K / (seen * (double)idx->ntotal) : 1.0);
            const bool f16 = idx->prefilter_force || (idx->prefilter && (seen > 0 || idx->density_hint > 0.0) && dens < idx->prefilter_density);
            // ... and once it is low enough that the int8 kernel's 4-5x candidates cost less than the fp16 kernel's
            // second half (the bound of 8-bit rows is ~16x looser), the batch runs on int8
            const bool i8 = f16 && allow_i8 && (idx->i8_mode == 2 || dens < idx->i8_density);
            used_i8 |= i8;
            // can this batch defer?  fp16: the panel kernel marks its candidates; int8 (option defer_i8): the fp16 screen
            const bool defers = can_defer && !no_event_left && f16 && (i8 ? idx->defer_i8 : idx->frag);
            if (defers && !d_open) VSC_TRY(choose_floor(idx, K, nq, i0, i1, bs, &d_open, &no_event_left));
            idx->defer_now = defers && d_open;
            const int rc_batch = enqueue_batch(idx, qp, i0, i1, cap, f16, i8);
            idx->defer_now = false;
            VSC_TRY(rc_batch);
            // The re-threshold round is predicated on the device (kept > 2K) and costs twelve launches even when it does
            // nothing.  Behind the LAST batch the control block is read back anyway: the round is enqueued there only
            // if that read says it has work to do (the one-batch calls of the sharded schedule almost never do).
            if (d_open) {
                // (with D outstanding the round is the deferred form, and the host reads its outcome: the one sync a
                // boundary behind a deferring batch adds)
                VSC_TRY(deferred_event(idx, qp, K, cap, &d_open));
            } else if (i1 < nq) {
                hipEvent_t stop;
                VSC_TRY(prof_begin(idx, &stop, 3));
                VSC_TRY(enqueue_rethreshold(ctl, idx->ws.hits_a(), idx->ws.hits_b(), (unsigned long long)K, idx->stream));
                VSC_TRY(prof_end(idx, stop, 0.0, 3));
            }
            if (!seeded && bs < 20000) bs *= 2;
            i0 = i1;
        }
        VSC_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipStreamSynchronize(idx->stream));
        if (d_open && !h.overflow) {
            // the end of the search with D outstanding (no event behind the last batches): its pairs are kept hits
            VSC_TRY(force_deferred(idx, qp, cap, h.n_d, h.n));
            VSC_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, idx->stream));
            VSC_HIP(hipStreamSynchronize(idx->stream));
        }
        if (!h.overflow && h.n > 2ull * (unsigned long long)K) {
            hipEvent_t stop;
            VSC_TRY(prof_begin(idx, &stop, 3));
            VSC_TRY(enqueue_rethreshold(ctl, idx->ws.hits_a(), idx->ws.hits_b(), (unsigned long long)K, idx->stream));
            VSC_TRY(prof_end(idx, stop, 0.0, 3));
            VSC_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, idx->stream));
            VSC_HIP(hipStreamSynchronize(idx->stream));
        }
        idx->stat_deferred = h.n_deferred;
        idx->stat_defer_events_ok = h.ev_ok;
        idx->stat_n_rethreshold = h.n_rethreshold;
        if (idx->debug_i8 && can_defer)
            fprintf(stderr, "[vscmi] deferred rescoring (defer %d, margin %g): %llu of %llu candidates deferred, %llu re-scored after all; "
                    "%llu events decided without them, %llu needed them (%llu events)\n", idx->defer, idx->defer_margin,
                    idx->stat_deferred, h.n_cand_total, idx->stat_defer_forced, idx->stat_defer_events_ok,
                    idx->stat_defer_events_forced, idx->stat_n_rethreshold);
        VSC_TRY(prof_collect(idx));
        idx->stat_candidates = h.n_cand_total;
        if (!h.overflow) break;
        if (used_i8 && (h.overflow & 2) && idx->i8_mode != 2) {
            // the candidate list overflowed with int8 batches in the schedule: their bound may simply be too loose for
            // these rows -- same buffers, fp16 pre-filter throughout
            allow_i8 = false;
            idx->stat_i8_fallbacks += 1;
            if (idx->debug_i8)
                fprintf(stderr, "[vscmi] int8 batches overflowed the candidate list (cap %lld, candidates so far %llu, tail %llu, "
                        "kept %llu): fp16 pre-filter for this search\n", (long long)cap, h.n_cand_total, h.n_tail, h.n);
            continue;
        }
        // A batch emitted more hits than the buffer holds (heavy score ties keep the radius low).
        // The schedule is deterministic, so simply rerun it with a larger buffer.
        if (idx->hit_cap_user > 0 || cap >= cap_max) {
            set_error("global_topk: kept-hit buffer (%lld entries) overflowed; raise it with "
                      "vsc_index_set_hit_capacity", (long long)cap);
            return VSC_ERR_OVERFLOW;
        }
        cap = std::min<int64_t>(cap * 4, cap_max);
        idx->hit_cap_learned = cap;  // the next search of this handle starts here instead of overflowing again
    }
    if (final_radius) *final_radius = ip ? h.radius : -h.radius;
    const int64_t n = (int64_t)h.n;
    const int64_t m = std::min(n, K);
    if (m > cap_out) {
        *n_out = m;
        set_error("global_topk: output capacity %lld < %lld", (long long)cap_out, (long long)m);
        return VSC_ERR_CAPACITY;
    }
    HitView d{out_i, out_j, out_s};
    if (out_mem == VSC_MEM_HOST) {
        for (int c = 0; c < 3; ++c) VSC_TRY(idx->ws.out[c].reserve((size_t)std::max<int64_t>(m, 1) * 4));
        d = idx->ws.hits_out();
    }
    int64_t mm = 0;
    hipEvent_t sort_stop;
    VSC_TRY(prof_begin(idx, &sort_stop, 4));
    if (idx->sort_hits || !ip) {
        VSC_TRY(sort_hits_topk(idx->ws.hits_a(), n, K, nq, idx->ntotal, idx->ws.sort, d, ip ? 0 : 1, &mm, idx->stream));
    } else {
        // option "sort_hits" = 0 (the column-sharded schedule, vsc2022_amd/dist.py: a batch's hits only join a list that
        // is counted, filtered and sorted ONCE at the end; inner product only): the kept hits as they lie; a
        // list of K entries may be a truncated one (n > K) -- the caller then asks again with a larger budget
        mm = m;
        if (mm > 0) {
            VSC_HIP(hipMemcpyAsync(d.i, idx->ws.hA[0].p, (size_t)mm * 4, hipMemcpyDeviceToDevice, idx->stream));
            VSC_HIP(hipMemcpyAsync(d.j, idx->ws.hA[1].p, (size_t)mm * 4, hipMemcpyDeviceToDevice, idx->stream));
            VSC_HIP(hipMemcpyAsync(d.s, idx->ws.hA[2].p, (size_t)mm * 4, hipMemcpyDeviceToDevice, idx->stream));
        }
    }
    VSC_TRY(prof_end(idx, sort_stop, 12.0 * (double)n, 4));  // (row, ref, score) of every kept hit in
    if (out_mem == VSC_MEM_HOST && mm > 0) {
        VSC_HIP(hipMemcpyAsync(out_i, d.i, (size_t)mm * 4, hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipMemcpyAsync(out_j, d.j, (size_t)mm * 4, hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipMemcpyAsync(out_s, d.s, (size_t)mm * 4, hipMemcpyDeviceToHost, idx->stream));
    }
    VSC_HIP(hipStreamSynchronize(idx->stream));
    VSC_TRY(prof_collect(idx));
    *n_out = mm;
    return VSC_OK;
}


// The proven route of vsc_index_global_topk (inner product, large query sets).
//
// What the reference returns (vsc/index.py:142-165): range_search_max_results leaves every pair with s > tau_final, where
// tau_final -- the radius after the last re-threshold event -- is the (K+1)-th best score of the ROW PREFIX searched up to
// that event (or -1e10 without an event); then the stable sort and the cut at K.  A prefix holds fewer pairs than the
// whole matrix, so tau_final <= s_(K+1), the (K+1)-th best score of ALL pairs.  Hence, whenever s_K > s_(K+1):
//     {s > tau_final}  contains  {s >= s_K}  = exactly K pairs,  and the first K of the sorted list are those K pairs
// -- the reference's result IS the exact top-K under (score desc, row asc, ref asc), whatever its batch schedule did on
// the way ("What's weak" 1; the query-sharded pipeline rests on the same argument, vsc2022_amd/dist.py).
// The two results differ only when a tie sits on the cut (s_K == s_(K+1)) AND the schedule's last event ends on that very
// score; that case is not decided here: the schedule is replayed (the caller's fall-through).
//
// So: (1) the reference's schedule over a strided SAMPLE of the query rows (<= 4096) gives a radius just below the cut --
// the 1.25 K (sample share)-th best sample score; (2) ALL rows run as steady 32768-row batches from that radius with the
// budget K + 1 (vsc_index_global_topk_seeded's body: pre-filtered from the first row on, re-threshold rule active); (3) the
// run returns every pair above its final radius: with >= K + 1 of them the K-th and (K+1)-th best of the whole matrix are
// known exactly, and s_K > s_(K+1) proves the first K to be the reference's result.  Anything else -- seed too high,
// a tie on the cut, an overflow -- leaves *done false.  What the doubling batches 32 ... 16384 of the schedule cost at
// BASELINE configs[3] (each hands ~K hits to the exact stage at a radius far below the final one): ~280 of 2050 ms.
static int global_topk_proven(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K, int32_t* out_i,
                              int32_t* out_j, float* out_s, int64_t cap_out, int out_mem, int64_t* n_out,
                              float* final_radius, bool* done) {
    *done = false;
    const int64_t nr = idx->ntotal;
    const bool force = idx->topk_shortcut == 2;
    if (idx->metric != VSC_METRIC_INNER_PRODUCT || idx->hit_cap_user > 0 || K < 1 || nq < 4 || nr < 1) return VSC_OK;
    const double pairs = (double)nq * (double)nr;
    if ((double)K + 1.0 > (force ? pairs - 1.0 : 0.25 * pairs) || cap_out < K) return VSC_OK;
    if (!force && (nq < 65536 || pairs < 4e10 || nq < 16 * idx->topk_sample_rows)) return VSC_OK;
    VSC_HIP(hipSetDevice(idx->device));
    Workspace& ws = idx->ws;
    // ---- 1. the sample: every stride-th row, the reference's own schedule over them
    const int64_t stride = std::max<int64_t>(2, nq / std::max<int64_t>(2, std::min(idx->topk_sample_rows, nq / 2)));
    const int64_t ns = (nq + stride - 1) / stride;
    VSC_TRY(ws.sample.reserve((size_t)ns * idx->dim * sizeof(float)));
    VSC_HIP(hipMemcpy2DAsync(ws.sample.p, (size_t)idx->dim * sizeof(float), q, (size_t)stride * idx->dim * sizeof(float),
                             (size_t)idx->dim * sizeof(float), (size_t)ns, q_mem == VSC_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                             idx->stream));
    const double share = (double)ns / (double)nq;
    // (x = the sample's share of the K best: the seed is the score below which 1.25 x + 4 sqrt(x) + 8 sample pairs lie -- a
    // quarter of slack for rows that are not like the sample, four standard deviations of the count itself for small K)
    const double x = (double)K * share;
    const int64_t k_tot = std::max<int64_t>(1, (int64_t)std::ceil(1.25 * x + 4.0 * std::sqrt(x) + 8.0));
    const int64_t k_s = (int64_t)std::min((double)ns * (double)nr, std::ceil(2.0 * x + 8.0 * std::sqrt(x)) + 1024.0);
    for (auto& b : ws.sk) VSC_TRY(b.reserve((size_t)std::max<int64_t>(k_s, 1) * 4));
    int64_t n_s = 0;
    float r_s = -1e10f;
    int rc = global_topk_impl(idx, ws.sample.as<float>(), ns, VSC_MEM_DEVICE, k_s, false, 0.0f, ws.sk[0].as<int32_t>(),
                              ws.sk[1].as<int32_t>(), ws.sk[2].as<float>(), k_s, VSC_MEM_DEVICE, &n_s, &r_s);
    if (rc == VSC_ERR_OVERFLOW || rc == VSC_ERR_CAPACITY) return VSC_OK;
    VSC_TRY(rc);
    const unsigned long long cand_sample = idx->stat_candidates;
    float seed = -1e10f;
    if (n_s >= k_tot) {
        float tau = 0.0f;
        VSC_HIP(hipMemcpyAsync(&tau, ws.sk[2].as<float>() + (k_tot - 1), sizeof(float), hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipStreamSynchronize(idx->stream));
        if (tau == tau && std::fabs(tau) < 1e10f) seed = std::nextafterf(tau, -INFINITY);
    } else if (r_s == r_s && std::fabs(r_s) < 1e10f) {
        seed = r_s;  // (fewer sample hits than asked for: everything above the sample's own final radius)
    }
    // ---- 2. all rows as steady batches from the seed, budget K + 1
    for (auto& b : ws.tk) VSC_TRY(b.reserve((size_t)(K + 1) * 4));
    int64_t n2 = 0;
    float r2 = -1e10f;
    rc = global_topk_impl(idx, q, nq, q_mem, K + 1, true, seed, ws.tk[0].as<int32_t>(), ws.tk[1].as<int32_t>(),
                          ws.tk[2].as<float>(), K + 1, VSC_MEM_DEVICE, &n2, &r2);
    idx->stat_candidates += cand_sample;
    idx->last_topk_route = 2;
    if (rc == VSC_ERR_OVERFLOW || rc == VSC_ERR_CAPACITY) return VSC_OK;
    VSC_TRY(rc);
    if (idx->debug_i8)
        fprintf(stderr, "[vscmi] proven top-K route: %lld sample rows (stride %lld), %lld sample hits, seed %.9g (the %lld-th best); "
                "steady run: %lld hits, radius %.9g (K = %lld)\n", (long long)ns, (long long)stride, (long long)n_s, (double)seed,
                (long long)k_tot, (long long)n2, (double)r2, (long long)K);
    if (n2 < K + 1) return VSC_OK;  // seed too high (or ties dropped by an event of the steady run): nothing is proven
    // ---- 3. the proof: s_K > s_(K+1)
    float cut[2] = {0.0f, 0.0f};
    VSC_HIP(hipMemcpyAsync(cut, ws.tk[2].as<float>() + (K - 1), 2 * sizeof(float), hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    if (idx->debug_i8) fprintf(stderr, "[vscmi] proven top-K route: s_K = %.9g, s_(K+1) = %.9g\n", (double)cut[0], (double)cut[1]);
    if (!(cut[0] > cut[1])) return VSC_OK;  // a tie on the cut: the schedule's final radius decides -- replay it
    const hipMemcpyKind kind = out_mem == VSC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    VSC_HIP(hipMemcpyAsync(out_i, ws.tk[0].p, (size_t)K * 4, kind, idx->stream));
    VSC_HIP(hipMemcpyAsync(out_j, ws.tk[1].p, (size_t)K * 4, kind, idx->stream));
    VSC_HIP(hipMemcpyAsync(out_s, ws.tk[2].p, (size_t)K * 4, kind, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    *n_out = K;
    // (the steady run's last radius: every returned hit lies above it.  The reference schedule's own final radius is
    // not computed on this route -- it is not part of what vsc/index.py returns; topk_shortcut = 0 yields it)
    if (final_radius) *final_radius = r2;
    idx->last_topk_route = 1;
    *done = true;
    return VSC_OK;
}

extern "C" {

int vsc_index_global_topk(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K,
                          int32_t* out_i, int32_t* out_j, float* out_s, int64_t cap_out, int out_mem,
                          int64_t* n_out, float* final_radius) {
    if (idx) idx->last_topk_route = 0;
    if (idx && idx->topk_shortcut && nq > 0 && q && n_out && K >= 0 && out_i && out_j && out_s) {
        bool done = false;
        VSC_TRY(global_topk_proven(idx, q, nq, q_mem, K, out_i, out_j, out_s, cap_out, out_mem, n_out, final_radius, &done));
        if (done) return VSC_OK;
    }
    return global_topk_impl(idx, q, nq, q_mem, K, false, 0.0f, out_i, out_j, out_s, cap_out, out_mem, n_out, final_radius);
}

int vsc_index_global_topk_seeded(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K, float radius0,
                                 int32_t* out_i, int32_t* out_j, float* out_s, int64_t cap_out, int out_mem,
                                 int64_t* n_out, float* final_radius) {
    if (!(radius0 == radius0) || std::fabs(radius0) > 1e10f) {
        set_error("vsc_index_global_topk_seeded: the seed radius must be a finite score (got %g)", (double)radius0);
        return VSC_ERR_INVALID;
    }
    return global_topk_impl(idx, q, nq, q_mem, K, true, radius0, out_i, out_j, out_s, cap_out, out_mem, n_out, final_radius);
}

int vsc_index_candidates(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K,
                         const int32_t* row2q, const int32_t* row2r, int32_t* out_q, int32_t* out_r,
                         float* out_s, int64_t cap_out, int64_t* n_pairs, int64_t* n_hits) {
    if (!idx || nq < 0 || K < 0 || !n_pairs || (nq > 0 && (!q || !row2q || !row2r))) {
        set_error("vsc_index_candidates: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_pairs = 0;
    if (n_hits) *n_hits = 0;
    if (idx->metric != VSC_METRIC_INNER_PRODUCT) {
        set_error("vsc_index_candidates: max aggregation needs a larger-is-better metric (inner product)");
        return VSC_ERR_INVALID;
    }
    if (nq == 0 || idx->ntotal == 0 || K == 0) return VSC_OK;
    VSC_HIP(hipSetDevice(idx->device));
    // 1. the score-sorted top-K hits stay in HBM
    const int64_t hcap = std::max<int64_t>(1, std::min<int64_t>(K, nq * idx->ntotal));
    for (int c = 0; c < 3; ++c) VSC_TRY(idx->cand[c].reserve((size_t)hcap * 4));
    int64_t n = 0;
    float radius = 0.0f;
    VSC_TRY(vsc_index_global_topk(idx, q, nq, q_mem, K, idx->cand[0].as<int32_t>(), idx->cand[1].as<int32_t>(),
                                  idx->cand[2].as<float>(), hcap, VSC_MEM_DEVICE, &n, &radius));
    if (n_hits) *n_hits = n;
    if (n == 0) return VSC_OK;
    // 2. (query video, ref video) max aggregation on the device
    Workspace& ws = idx->ws;
    VSC_TRY(ws.maps0.reserve((size_t)nq * 4));
    VSC_TRY(ws.maps1.reserve((size_t)idx->ntotal * 4));
    VSC_HIP(hipMemcpyAsync(ws.maps0.p, row2q, (size_t)nq * 4, hipMemcpyHostToDevice, idx->stream));
    VSC_HIP(hipMemcpyAsync(ws.maps1.p, row2r, (size_t)idx->ntotal * 4, hipMemcpyHostToDevice, idx->stream));
    for (int c = 0; c < 3; ++c) VSC_TRY(ws.out[c].reserve((size_t)n * 4));
    VSC_TRY(ws.out[3].reserve((size_t)n * 8));
    int64_t np = 0;
    VSC_TRY(pair_max_device(idx->cand[0].as<int32_t>(), idx->cand[1].as<int32_t>(), idx->cand[2].as<float>(), n,
                            ws.maps0.as<int32_t>(), ws.maps1.as<int32_t>(), nq, idx->ntotal, ws.sort,
                            ws.cnt, ws.out[0].as<int32_t>(), ws.out[1].as<int32_t>(), ws.out[2].as<float>(),
                            ws.out[3].as<int64_t>(), n, &np, idx->stream));
    *n_pairs = np;
    if (np > cap_out) {
        set_error("vsc_index_candidates: output capacity %lld < %lld pairs", (long long)cap_out, (long long)np);
        return VSC_ERR_CAPACITY;
    }
    if (np > 0) {
        VSC_HIP(hipMemcpyAsync(out_q, ws.out[0].p, (size_t)np * 4, hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipMemcpyAsync(out_r, ws.out[1].p, (size_t)np * 4, hipMemcpyDeviceToHost, idx->stream));
        VSC_HIP(hipMemcpyAsync(out_s, ws.out[2].p, (size_t)np * 4, hipMemcpyDeviceToHost, idx->stream));
    }
    VSC_HIP(hipStreamSynchronize(idx->stream));
    return VSC_OK;
}

int vsc_index_candidates_agg(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, int64_t K, const int32_t* row2q,
                             const int32_t* row2r, int agg, int64_t top_m, int32_t* out_q, int32_t* out_r, float* out_s,
                             int64_t cap_out, int64_t* n_pairs, int64_t* n_hits) {
    VSC_TRY(pair_agg_check("vsc_index_candidates_agg", agg, top_m));
    if (!idx || nq < 0 || !n_pairs || cap_out < 0 || (nq > 0 && (!q || !row2q || !row2r))) {
        set_error("vsc_index_candidates_agg: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_pairs = 0;
    if (n_hits) *n_hits = 0;
    if (idx->metric != VSC_METRIC_INNER_PRODUCT) {
        set_error("vsc_index_candidates_agg: the aggregations need a larger-is-better metric (inner product)");
        return VSC_ERR_INVALID;
    }
    const bool knn = K < 0;
    if (knn && (-K > idx->ntotal || -K > 0x7fffffffLL)) {
        set_error("vsc_index_candidates_agg: k = %lld neighbours of %lld reference rows (an empty slot has no video)",
                  (long long)-K, (long long)idx->ntotal);
        return VSC_ERR_INVALID;
    }
    if (nq == 0 || idx->ntotal == 0 || K == 0) return VSC_OK;
    VSC_HIP(hipSetDevice(idx->device));
    // 1. the hits stay in HBM: the score-sorted top-K, or the (row, rank) lists of the k-NN
    const int64_t hcap = knn ? nq * -K : std::max<int64_t>(1, std::min<int64_t>(K, nq * idx->ntotal));
    if (hcap > 0x7fffffffLL) {
        set_error("vsc_index_candidates_agg: %lld hits are beyond the supported size", (long long)hcap);
        return VSC_ERR_INVALID;
    }
    for (int c = 0; c < 3; ++c) VSC_TRY(idx->cand[c].reserve((size_t)hcap * 4));
    int64_t n = 0;
    if (knn) {
        const int k = (int)-K;
        VSC_TRY(idx->cand_ids.reserve((size_t)hcap * 8));
        VSC_TRY(vsc_index_knn(idx, q, nq, q_mem, k, idx->cand[2].as<float>(), idx->cand_ids.as<int64_t>(), VSC_MEM_DEVICE));
        VSC_TRY(launch_knn_to_hits(idx->cand_ids.as<int64_t>(), nq, k, idx->cand[0].as<int32_t>(), idx->cand[1].as<int32_t>(), idx->stream));
        n = hcap;
    } else {
        float radius = 0.0f;
        VSC_TRY(vsc_index_global_topk(idx, q, nq, q_mem, K, idx->cand[0].as<int32_t>(), idx->cand[1].as<int32_t>(),
                                      idx->cand[2].as<float>(), hcap, VSC_MEM_DEVICE, &n, &radius));
    }
    if (n_hits) *n_hits = n;
    if (n == 0) return VSC_OK;
    // 2. the (query video, ref video) aggregation on the device
    Workspace& ws = idx->ws;
    VSC_TRY(ws.maps0.reserve((size_t)nq * 4));
    VSC_TRY(ws.maps1.reserve((size_t)idx->ntotal * 4));
    VSC_HIP(hipMemcpyAsync(ws.maps0.p, row2q, (size_t)nq * 4, hipMemcpyHostToDevice, idx->stream));
    VSC_HIP(hipMemcpyAsync(ws.maps1.p, row2r, (size_t)idx->ntotal * 4, hipMemcpyHostToDevice, idx->stream));
    for (int c = 0; c < 3; ++c) VSC_TRY(ws.out[c].reserve((size_t)n * 4));
    int64_t np = 0;
    VSC_TRY(pair_aggregate_device(idx->cand[0].as<int32_t>(), idx->cand[1].as<int32_t>(), idx->cand[2].as<float>(), n,
                                  ws.maps0.as<int32_t>(), ws.maps1.as<int32_t>(), nq, idx->ntotal, knn ? 0 : 1, agg, top_m, ws.sort,
                                  ws.agg, ws.out[0].as<int32_t>(), ws.out[1].as<int32_t>(), ws.out[2].as<float>(), nullptr, nullptr,
                                  n, &np, idx->stream));
    *n_pairs = np;
    if (np > cap_out) {
        set_error("vsc_index_candidates_agg: output capacity %lld < %lld pairs", (long long)cap_out, (long long)np);
        return VSC_ERR_CAPACITY;
    }
    if (np > 0 && (!out_q || !out_r || !out_s)) {
        set_error("vsc_index_candidates_agg: invalid argument (no output arrays)");
        return VSC_ERR_INVALID;
    }
    VSC_HIP(hipMemcpyAsync(out_q, ws.out[0].p, (size_t)np * 4, hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipMemcpyAsync(out_r, ws.out[1].p, (size_t)np * 4, hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipMemcpyAsync(out_s, ws.out[2].p, (size_t)np * 4, hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    return VSC_OK;
}

int vsc_index_range_search(vsc_index_t* idx, const float* q, int64_t nq, int q_mem, float radius,
                           int64_t* lims, float* D, int64_t* I, int64_t cap_out, int64_t* n_out) {
    if (!idx || nq < 0 || !lims || !n_out || (nq > 0 && !q)) {
        set_error("vsc_index_range_search: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_out = 0;
    for (int64_t i = 0; i <= nq; ++i) lims[i] = 0;
    if (nq == 0 || idx->ntotal == 0) return VSC_OK;
    const bool ip = idx->metric == VSC_METRIC_INNER_PRODUCT;
    VSC_HIP(hipSetDevice(idx->device));
    float* qp = nullptr;
    VSC_TRY(pack_queries(idx, q, nq, q_mem, &qp, idx->prefilter));
    VSC_TRY(i8_prepare(idx));
    int64_t cap = idx->hit_cap_user > 0 ? idx->hit_cap_user : std::min<int64_t>(nq * idx->ntotal, (int64_t)1 << 28);
    cap = std::max<int64_t>(cap, 1024);
    VSC_TRY(ensure_hit_buffers(idx, cap));
    VSC_TRY(init_ctl(idx, ip ? radius : -radius));
    SelectCtl* ctl = idx->ws.ctl.as<SelectCtl>();
    const int64_t step = 32768;
    // fixed radius: the pre-filter is used throughout (a radius so low that most pairs pass would
    // overflow the hit capacity on either route)
    for (int64_t i0 = 0; i0 < nq; i0 += step)
        VSC_TRY(enqueue_batch(idx, qp, i0, std::min(nq, i0 + step), cap, idx->prefilter, idx->i8_mode == 2));
    SelectCtl h;
    VSC_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    VSC_TRY(prof_collect(idx));
    if (h.overflow) {
        set_error("range_search: more than %lld hits; raise vsc_index_set_hit_capacity", (long long)cap);
        return VSC_ERR_OVERFLOW;
    }
    const int64_t n = (int64_t)h.n;
    *n_out = n;
    if (n == 0) return VSC_OK;
    // rows ascending, refs ascending (reuse B as the sorted target)
    VSC_TRY(sort_hits_rowcol(idx->ws.hits_a(), n, idx->ws.sort, idx->ws.hits_b(), ip ? 0 : 1, idx->stream));
    std::vector<int32_t> hi((size_t)n);
    VSC_HIP(hipMemcpyAsync(hi.data(), idx->ws.hB[0].p, (size_t)n * 4, hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    for (int64_t x = 0; x < n; ++x) lims[hi[(size_t)x] + 1] += 1;
    for (int64_t i = 0; i < nq; ++i) lims[i + 1] += lims[i];
    if (!D || !I || cap_out < n) {
        if (D || I) {
            set_error("range_search: output capacity %lld < %lld", (long long)cap_out, (long long)n);
            return VSC_ERR_CAPACITY;
        }
        return VSC_OK;  // size query
    }
    std::vector<int32_t> hj((size_t)n);
    VSC_HIP(hipMemcpyAsync(hj.data(), idx->ws.hB[1].p, (size_t)n * 4, hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipMemcpyAsync(D, idx->ws.hB[2].p, (size_t)n * 4, hipMemcpyDeviceToHost, idx->stream));
    VSC_HIP(hipStreamSynchronize(idx->stream));
    for (int64_t x = 0; x < n; ++x) I[x] = hj[(size_t)x];
    return VSC_OK;
}


}  // extern "C"
