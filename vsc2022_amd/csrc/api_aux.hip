// C ABI of libvscmi.so, part 4: the device ops that own no handle (vsc_pair_max, vsc_pair_aggregate, vsc_sort_hits, the
// score histogram / pick / filter / argsort / merge steps, vsc_row_normalize, vsc_match_metric) and the per-device context
// they share with the handle-less forward-sim entry points of api_tn.hip (api_internal.h: DeviceCtx).
#include "api_internal.h"

// ------------------------------------------------------------------ stand-alone device ops

namespace vscmi {

DeviceCtx* device_ctx(int device) {
    static std::mutex g_mu;
    static std::vector<DeviceCtx*> ctxs;
    std::lock_guard<std::mutex> lk(g_mu);
    if ((int)ctxs.size() <= device) ctxs.resize(device + 1, nullptr);
    if (!ctxs[device]) {
        DeviceCtx* c = new DeviceCtx();
        if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return nullptr;
        }
        c->stream = c->own_stream;
        ctxs[device] = c;
    }
    return ctxs[device];
}

int to_device(const void* p, size_t bytes, int mem, DevBuf& buf, const void** out, hipStream_t s) {
    if (mem == VSC_MEM_DEVICE) {
        *out = p;
        return VSC_OK;
    }
    VSC_TRY(buf.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) VSC_HIP(hipMemcpyAsync(buf.p, p, bytes, hipMemcpyHostToDevice, s));
    *out = buf.p;
    return VSC_OK;
}

}  // namespace vscmi

extern "C" {

int vsc_set_aux_stream(int device, void* hip_stream, int own) {
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_set_aux_stream: device context unavailable");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->stream == c->own_stream) VSC_HIP(hipStreamSynchronize(c->own_stream));
    else (void)hipDeviceSynchronize();  // (a caller's stream may be gone: never touched again, see vsc_index_set_stream)
    c->stream = own ? c->own_stream : (hipStream_t)hip_stream;
    return VSC_OK;
}

int vsc_pair_max(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n,
                 int hits_mem, const int32_t* row2q, int64_t nq_rows, const int32_t* row2r,
                 int64_t nr_rows, int maps_mem, int32_t* out_q, int32_t* out_r, float* out_s,
                 int64_t* out_first, int64_t cap, int out_mem, int64_t* n_pairs, int device) {
    if (n < 0 || !n_pairs || (n > 0 && (!hit_i || !hit_j || !hit_s || !row2q || !row2r))) {
        set_error("vsc_pair_max: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_pairs = 0;
    if (n == 0) return VSC_OK;
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_pair_max: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    Workspace& ws = c->ws;
    const void *di, *dj, *ds, *dq, *dr;
    VSC_TRY(to_device(hit_i, (size_t)n * 4, hits_mem, ws.hA[0], &di, c->stream));
    VSC_TRY(to_device(hit_j, (size_t)n * 4, hits_mem, ws.hA[1], &dj, c->stream));
    VSC_TRY(to_device(hit_s, (size_t)n * 4, hits_mem, ws.hA[2], &ds, c->stream));
    VSC_TRY(to_device(row2q, (size_t)nq_rows * 4, maps_mem, ws.maps0, &dq, c->stream));
    VSC_TRY(to_device(row2r, (size_t)nr_rows * 4, maps_mem, ws.maps1, &dr, c->stream));
    int32_t *oq = out_q, *orr = out_r;
    float* os = out_s;
    int64_t* of = out_first;
    const int64_t ocap = out_mem == VSC_MEM_HOST ? n : cap;
    if (out_mem == VSC_MEM_HOST) {
        VSC_TRY(ws.out[0].reserve((size_t)n * 4));
        VSC_TRY(ws.out[1].reserve((size_t)n * 4));
        VSC_TRY(ws.out[2].reserve((size_t)n * 4));
        VSC_TRY(ws.out[3].reserve((size_t)n * 8));
        oq = ws.out[0].as<int32_t>();
        orr = ws.out[1].as<int32_t>();
        os = ws.out[2].as<float>();
        of = ws.out[3].as<int64_t>();
    }
    int64_t np = 0;
    AuxTimer tm;
    tm.begin(0, c->stream);
    VSC_TRY(pair_max_device((const int32_t*)di, (const int32_t*)dj, (const float*)ds, n, (const int32_t*)dq,
                            (const int32_t*)dr, nq_rows, nr_rows, ws.sort, ws.cnt, oq, orr, os, of,
                            ocap, &np, c->stream));
    tm.end(12.0 * (double)n + 20.0 * (double)np, c->stream);  // hits in, (q, r, score, first hit) per pair out
    *n_pairs = np;
    if (out_mem == VSC_MEM_HOST) {
        if (np > cap) {
            set_error("vsc_pair_max: output capacity %lld < %lld pairs", (long long)cap, (long long)np);
            return VSC_ERR_CAPACITY;
        }
        VSC_HIP(hipMemcpyAsync(out_q, oq, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_r, orr, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_s, os, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_first) VSC_HIP(hipMemcpyAsync(out_first, of, (size_t)np * 8, hipMemcpyDeviceToHost, c->stream));
    }
    VSC_HIP(hipStreamSynchronize(c->stream));
    tm.collect();
    return VSC_OK;
}

int vsc_pair_aggregate(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n, int hits_mem,
                       const int32_t* row2q, int64_t nq_rows, const int32_t* row2r, int64_t nr_rows, int maps_mem,
                       int hits_order, int agg, int64_t top_m, int32_t* out_q, int32_t* out_r, float* out_s,
                       int64_t* out_first, int32_t* out_count, int64_t cap, int out_mem, int64_t* n_pairs, int device) {
    // (the aggregation is judged first: a bad one is refused whatever else the call holds, with no device looked at)
    VSC_TRY(pair_agg_check("vsc_pair_aggregate", agg, top_m));
    if (n < 0 || n > 0x7fffffffLL || nq_rows < 0 || nr_rows < 0 || cap < 0 || !n_pairs ||
        (n > 0 && (!hit_i || !hit_j || !hit_s || !row2q || !row2r || !out_q || !out_r || !out_s))) {
        set_error("vsc_pair_aggregate: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_pairs = 0;
    if (n == 0) return VSC_OK;
    if (hits_mem == VSC_MEM_HOST) {
        for (int64_t x = 0; x < n; ++x) {
            if (hit_i[x] < 0 || hit_i[x] >= nq_rows || hit_j[x] < 0 || hit_j[x] >= nr_rows) {
                set_error("vsc_pair_aggregate: hit %lld names row (%d, %d) outside the row -> video maps (%lld query rows, %lld "
                          "reference rows)", (long long)x, (int)hit_i[x], (int)hit_j[x], (long long)nq_rows, (long long)nr_rows);
                return VSC_ERR_INVALID;
            }
        }
    }
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_pair_aggregate: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    Workspace& ws = c->ws;
    const void *di, *dj, *ds, *dq, *dr;
    VSC_TRY(to_device(hit_i, (size_t)n * 4, hits_mem, ws.hA[0], &di, c->stream));
    VSC_TRY(to_device(hit_j, (size_t)n * 4, hits_mem, ws.hA[1], &dj, c->stream));
    VSC_TRY(to_device(hit_s, (size_t)n * 4, hits_mem, ws.hA[2], &ds, c->stream));
    VSC_TRY(to_device(row2q, (size_t)nq_rows * 4, maps_mem, ws.maps0, &dq, c->stream));
    VSC_TRY(to_device(row2r, (size_t)nr_rows * 4, maps_mem, ws.maps1, &dr, c->stream));
    int32_t *oq = out_q, *orr = out_r, *oc = out_count;
    float* os = out_s;
    int64_t* of = out_first;
    const int64_t ocap = out_mem == VSC_MEM_HOST ? n : cap;
    if (out_mem == VSC_MEM_HOST) {
        VSC_TRY(ws.out[0].reserve((size_t)n * 4));
        VSC_TRY(ws.out[1].reserve((size_t)n * 4));
        VSC_TRY(ws.out[2].reserve((size_t)n * 4));
        VSC_TRY(ws.out[3].reserve((size_t)n * 8));
        VSC_TRY(ws.parts.reserve((size_t)n * 4));
        oq = ws.out[0].as<int32_t>();
        orr = ws.out[1].as<int32_t>();
        os = ws.out[2].as<float>();
        of = ws.out[3].as<int64_t>();
        oc = ws.parts.as<int32_t>();
    }
    int64_t np = 0;
    VSC_TRY(pair_aggregate_device((const int32_t*)di, (const int32_t*)dj, (const float*)ds, n, (const int32_t*)dq, (const int32_t*)dr,
                                  nq_rows, nr_rows, hits_order, agg, top_m, ws.sort, ws.agg, oq, orr, os, of, oc, ocap, &np, c->stream));
    *n_pairs = np;
    if (out_mem == VSC_MEM_HOST) {
        if (np > cap) {
            set_error("vsc_pair_aggregate: output capacity %lld < %lld pairs", (long long)cap, (long long)np);
            return VSC_ERR_CAPACITY;
        }
        VSC_HIP(hipMemcpyAsync(out_q, oq, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_r, orr, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_s, os, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_first) VSC_HIP(hipMemcpyAsync(out_first, of, (size_t)np * 8, hipMemcpyDeviceToHost, c->stream));
        if (out_count) VSC_HIP(hipMemcpyAsync(out_count, oc, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_sort_hits(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n, int hits_mem, int64_t max_row,
                  int64_t max_ref, int32_t* out_i, int32_t* out_j, float* out_s, int out_mem, int device) {
    if (n < 0 || (n > 0 && (!hit_i || !hit_j || !hit_s || !out_i || !out_j || !out_s))) {
        set_error("vsc_sort_hits: invalid argument");
        return VSC_ERR_INVALID;
    }
    if (n == 0) return VSC_OK;
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_sort_hits: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    Workspace& ws = c->ws;
    const void *di, *dj, *ds;
    VSC_TRY(to_device(hit_i, (size_t)n * 4, hits_mem, ws.hA[0], &di, c->stream));
    VSC_TRY(to_device(hit_j, (size_t)n * 4, hits_mem, ws.hA[1], &dj, c->stream));
    VSC_TRY(to_device(hit_s, (size_t)n * 4, hits_mem, ws.hA[2], &ds, c->stream));
    int32_t *oi = out_i, *oj = out_j;
    float* os = out_s;
    if (out_mem == VSC_MEM_HOST) {
        for (int k = 0; k < 3; ++k) VSC_TRY(ws.out[k].reserve((size_t)n * 4));
        oi = ws.out[0].as<int32_t>();
        oj = ws.out[1].as<int32_t>();
        os = ws.out[2].as<float>();
    }
    const int64_t all = (int64_t)1 << 31;
    int64_t m = 0;
    VSC_TRY(sort_hits_topk({(const int32_t*)di, (const int32_t*)dj, (const float*)ds}, n, n, max_row > 0 ? max_row : all,
                           max_ref > 0 ? max_ref : all, ws.sort, {oi, oj, os}, 0, &m, c->stream));
    if (out_mem == VSC_MEM_HOST) {
        VSC_HIP(hipMemcpyAsync(out_i, oi, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_j, oj, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_s, os, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

// One level of an order statistic over unsorted scores that are spread over ranks (include/vscmi.h).  Device pointers
// only; on a caller's stream (vsc_set_aux_stream) the work is merely enqueued -- the caller's next operation on that
// stream (the all-reduce of the histogram) is ordered behind it --, on the library's own stream the call waits.
int vsc_score_histogram(const float* scores, int64_t n, const int64_t* state, int shift, int64_t* hist, int device) {
    if (n < 0 || (n > 0 && !scores) || !state || !hist || (shift != 0 && shift != 8 && shift != 16 && shift != 24)) {
        set_error("vsc_score_histogram: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_score_histogram: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    VSC_TRY(launch_score_hist(scores, (long long)n, reinterpret_cast<const long long*>(state), shift,
                              reinterpret_cast<long long*>(hist), c->stream));
    if (c->stream == c->own_stream) VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_score_pick(const int64_t* hist, int64_t* state, int shift, int device) {
    if (!hist || !state || (shift != 0 && shift != 8 && shift != 16 && shift != 24)) {
        set_error("vsc_score_pick: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_score_pick: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    VSC_TRY(launch_score_pick(reinterpret_cast<const long long*>(hist), reinterpret_cast<long long*>(state), shift, c->stream));
    if (c->stream == c->own_stream) VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_filter_hits(const int32_t* hit_i, const int32_t* hit_j, const float* hit_s, int64_t n, float radius, int32_t* out_i,
                    int32_t* out_j, float* out_s, int64_t* n_out, int device) {
    if (n < 0 || !n_out || (n > 0 && (!hit_i || !hit_j || !hit_s || !out_i || !out_j || !out_s)) || !(radius == radius)) {
        set_error("vsc_filter_hits: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_out = 0;
    if (n == 0) return VSC_OK;
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_filter_hits: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    VSC_TRY(c->ws.cnt.reserve(sizeof(unsigned long long)));
    VSC_TRY(launch_filter_hits({hit_i, hit_j, hit_s}, (long long)n, radius, {out_i, out_j, out_s}, c->ws.cnt.as<unsigned long long>(),
                               c->stream));
    unsigned long long kept = 0;
    VSC_HIP(hipMemcpyAsync(&kept, c->ws.cnt.p, sizeof(kept), hipMemcpyDeviceToHost, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    *n_out = (int64_t)kept;
    return VSC_OK;
}

int vsc_argsort_scores(const float* scores, int64_t n, int mem, int32_t* perm, int perm_mem, int device) {
    if (n < 0 || (n > 0 && (!scores || !perm))) {
        set_error("vsc_argsort_scores: invalid argument");
        return VSC_ERR_INVALID;
    }
    if (n == 0) return VSC_OK;
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_argsort_scores: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    Workspace& ws = c->ws;
    const void* ds;
    VSC_TRY(to_device(scores, (size_t)n * 4, mem, ws.hA[2], &ds, c->stream));
    const int32_t* p = nullptr;
    VSC_TRY(argsort_scores_desc((const float*)ds, n, ws.sort, &p, c->stream));
    VSC_HIP(hipMemcpyAsync(perm, p, (size_t)n * 4, perm_mem == VSC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_merge_topk(const float* scores, const int64_t* ids, int64_t nq, int m, int k, float* out_s, int64_t* out_ids,
                   int device) {
    if (nq < 0 || m <= 0 || k <= 0 || m > 1024 || k > m || (nq > 0 && (!scores || !ids || !out_s || !out_ids))) {
        set_error("vsc_merge_topk: invalid argument (1 <= k <= m <= 1024 candidates per row)");
        return VSC_ERR_INVALID;
    }
    if (nq == 0) return VSC_OK;
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_merge_topk: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    VSC_TRY(launch_merge_topk(scores, reinterpret_cast<const long long*>(ids), (long long)nq, m, k, out_s,
                              reinterpret_cast<long long*>(out_ids), c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_row_normalize(const float* x, int64_t n, int dim, int x_mem, float* out, int out_mem, int device) {
    if (n < 0 || dim <= 0 || (n > 0 && (!x || !out))) {
        set_error("vsc_row_normalize: invalid argument");
        return VSC_ERR_INVALID;
    }
    if (n == 0) return VSC_OK;
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_row_normalize: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    const void* dx;
    VSC_TRY(to_device(x, (size_t)n * dim * 4, x_mem, c->ws.stage, &dx, c->stream));
    float* dout = out;
    if (out_mem == VSC_MEM_HOST) {
        VSC_TRY(c->ws.out[0].reserve((size_t)n * dim * 4));
        dout = c->ws.out[0].as<float>();
    }
    VSC_TRY(launch_row_normalize((const float*)dx, n, dim, dout, c->stream));
    if (out_mem == VSC_MEM_HOST)
        VSC_HIP(hipMemcpyAsync(out, dout, (size_t)n * dim * 4, hipMemcpyDeviceToHost, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

// Segment AP of the matching track (include/vscmi.h): uploads, then metric.hip's match_metric_device
int vsc_match_metric(const int32_t* gt_pair, const double* gt_times, int64_t n_gt, const int32_t* gt_first, int64_t n_gt_pairs,
                     int gt_mem, const int32_t* pred_pair, const double* pred_score, const double* pred_times, int64_t n_pred,
                     int pred_mem, int64_t n_pairs, double* out_score, double* out_sums, int64_t cap, int64_t* n_groups,
                     double* gt_len, int64_t* stats, int device) {
    if (!n_groups || !gt_len || n_gt < 0 || n_pred < 0 || n_pairs < 0 || n_gt_pairs < 0 || n_gt_pairs > n_pairs || cap < 0 ||
        (n_gt > 0 && (!gt_pair || !gt_times)) || (n_pred > 0 && (!pred_pair || !pred_score || !pred_times)) ||
        (cap > 0 && (!out_score || !out_sums))) {
        set_error("vsc_match_metric: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_groups = 0;
    gt_len[0] = gt_len[1] = 0.0;
    if (stats) memset(stats, 0, 8 * sizeof(int64_t));
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_match_metric: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    const void *dgp, *dgt, *dgf = nullptr, *dpp, *dps, *dpt;
    VSC_TRY(to_device(gt_pair, (size_t)n_gt * 4, gt_mem, c->metric_in[0], &dgp, c->stream));
    VSC_TRY(to_device(gt_times, (size_t)n_gt * 32, gt_mem, c->metric_in[1], &dgt, c->stream));
    if (gt_first) VSC_TRY(to_device(gt_first, (size_t)n_gt_pairs * 4, gt_mem, c->metric_in[2], &dgf, c->stream));
    VSC_TRY(to_device(pred_pair, (size_t)n_pred * 4, pred_mem, c->metric_in[3], &dpp, c->stream));
    VSC_TRY(to_device(pred_score, (size_t)n_pred * 8, pred_mem, c->metric_in[4], &dps, c->stream));
    VSC_TRY(to_device(pred_times, (size_t)n_pred * 32, pred_mem, c->metric_in[5], &dpt, c->stream));
    MetricIn in{(const int32_t*)dgp, (const double*)dgt, n_gt, (const int32_t*)dgf, n_gt_pairs,
                (const int32_t*)dpp, (const double*)dps, (const double*)dpt, n_pred, n_pairs};
    MetricOut out{out_score, out_sums, cap, 0, gt_len, {0, 0, 0, 0, 0, 0, 0, 0}};
    const int rc = match_metric_device(in, c->metric, out, c->stream);
    *n_groups = out.n_groups;
    if (stats) for (int k = 0; k < 8; ++k) stats[k] = out.stats[k];
    return rc;
}

}  // extern "C"
