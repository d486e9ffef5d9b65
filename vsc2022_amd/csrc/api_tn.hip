// C ABI of libvscmi.so, part 5: the Temporal-Network localisation contexts (vsc_tn_*), the DTW / DP aligners on them
// (vsc_tn_align), the handle-less forms of both over caller matrices (vsc_tn_forward_sim, vsc_align_forward_sim), the
// match-rows stage behind them (vsc_tn_set_timestamps, vsc_tn_match_rows) and the DnS fine descriptors (vsc_tn_set_fine,
// vsc_tn_set_fine_bits, vsc_tn_set_fine_f16 -- one FineStore, written by tn_set_fine --, vsc_tn_fine_similarity,
// vsc_tn_localize_fine, vsc_tn_similarity_fine).  Host plumbing only: the kernels are in tn.hip, align.hip, match_rows.hip,
// fine_sim.hip and fine_bits.hip; rows come up through the staging loop of api_internal.h (for_row_chunks).
#include "api_internal.h"

// ------------------------------------------------------------------------ TN launches

// Algorithmic bytes a pair reads: its descriptor rows once (fused), or its matrix (forward_sim)
static double pair_bytes(bool fused, int dpad, bool half_refs, double lq, double lr) {
    return fused ? dpad * (4.0 * lq + (half_refs ? 2.0 : 4.0) * lr) : 4.0 * lq * lr;
}

// Split the pairs of one call into launches by LDS footprint and run them.  `base` carries
// everything except the per-launch fields.  In forward_sim mode (base.sims_in set) tiles are read
// in place; otherwise they live in LDS when they fit the launch's budget and spill to `slab`.
// Pairs whose working state does not fit LDS, or whose node / frame indices do not fit 16 bits
// (query videos beyond ~1000 frames at the default parameters, references beyond 32767), run
// from an HBM state slab with 32-bit indices, in chunks of bounded memory.
static int tn_run_buckets(TnPairArgs base, const std::vector<int32_t>& lqs, const std::vector<int32_t>& lrs,
                          DevBuf& d_work, DevBuf& slab, hipStream_t stream) {
    const int64_t n_pairs = (int64_t)lqs.size();
    const int ms = base.prm.tn_max_step > 1 ? base.prm.tn_max_step : 1;
    const int topc = base.prm.tn_top_k;
    const bool fused = base.sims_in == nullptr;
    constexpr size_t LDS_STATE_MAX = 150 * 1024;
    constexpr int64_t BIG_CHUNK_BYTES = (int64_t)4 << 30;  // state + similarity slab of one launch of the HBM route
    struct Bucket { int max_lq; int64_t max_tile; std::vector<int32_t> work; int seen_lq; int64_t seen_tile; };
    Bucket buckets[4] = {{64, 4096, {}, 0, 0}, {256, 24576, {}, 0, 0}, {0x7fffffff, 0, {}, 0, 0}, {0x7fffffff, 0, {}, 0, 0}};
    // The state grows with top^2 * step: an LDS-tile bucket (fused route) takes pairs only when the state of its
    // longest video plus its largest tile fit one launch.  Otherwise its pairs go to the slab bucket -- same results.
    // (Both fit at the default and the reference's parameters: 143 488 and 134 336 bytes for bucket 1.)
    bool tile_ok[2];
    for (int b = 0; b < 2; ++b)
        tile_ok[b] = tn_state_bytes_host(buckets[b].max_lq, topc, ms) + (size_t)buckets[b].max_tile * 4 <= TN_LAUNCH_LDS_MAX;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t lq = lqs[(size_t)p], lr = lrs[(size_t)p];
        if (lq * std::max<int64_t>(1, topc) * ms * topc > 0x7fff0000LL || lq * lr > ((int64_t)1 << 40)) {
            set_error("TN: a %lld x %lld frame pair is beyond the supported size", (long long)lq, (long long)lr);
            return VSC_ERR_INVALID;
        }
        int b = 2;
        if (lq * topc + 1 > 32767 || lr > 32767 || tn_state_bytes_host((int)std::max<int64_t>(lq, 1), topc, ms) > LDS_STATE_MAX) b = 3;
        else if (lq <= 64 && (!fused || (tile_ok[0] && lq * lr <= 4096))) b = 0;
        else if (lq <= 256 && (!fused || (tile_ok[1] && lq * lr <= 24576))) b = 1;
        buckets[b].work.push_back((int32_t)p);
        buckets[b].seen_lq = std::max<int>(buckets[b].seen_lq, (int)lq);
        buckets[b].seen_tile = std::max<int64_t>(buckets[b].seen_tile, lq * lr);
    }
    VSC_TRY(d_work.reserve((size_t)std::max<int64_t>(n_pairs, 1) * 4));
    DevBuf big_state;  // HBM route only; freed on return
    int64_t woff = 0;
    for (int b = 0; b < 4; ++b) {
        Bucket& B = buckets[b];
        if (B.work.empty()) continue;
        const bool big = b == 3;
        const int max_lq = std::max(1, B.seen_lq);
        const size_t state = tn_state_bytes_host(max_lq, topc, ms, big ? 4 : 2);
        int tile_floats = 0;
        int64_t slab_floats = 0;
        if (fused) {
            if (b < 2) tile_floats = (int)std::min<int64_t>(B.seen_tile, B.max_tile);
            else slab_floats = (B.seen_tile + 63) / 64 * 64;
        }
        // pairs per launch: everything, or as many as the HBM route's memory bound allows
        int64_t per_launch = (int64_t)B.work.size();
        if (big) per_launch = std::max<int64_t>(1, std::min<int64_t>(per_launch, BIG_CHUNK_BYTES / (int64_t)(state + (size_t)slab_floats * 4)));
        if (slab_floats) VSC_TRY(slab.reserve((size_t)slab_floats * 4 * (size_t)per_launch));
        if (big) VSC_TRY(big_state.reserve(state * (size_t)per_launch));
        const size_t lds = big ? 0 : state + (size_t)tile_floats * 4;
        for (int64_t c0 = 0; c0 < (int64_t)B.work.size(); c0 += per_launch) {
            const int64_t cn = std::min<int64_t>(per_launch, (int64_t)B.work.size() - c0);
            int32_t* dwork = d_work.as<int32_t>() + woff;
            VSC_HIP(hipMemcpyAsync(dwork, B.work.data() + c0, (size_t)cn * 4, hipMemcpyHostToDevice, stream));
            TnPairArgs a = base;
            a.work = dwork;
            a.n_work = (int)cn;
            a.max_lq = max_lq;
            a.lds_tile_floats = tile_floats;
            a.slab = slab.as<float>();
            a.slab_floats = slab_floats;
            a.state = big ? big_state.as<char>() : nullptr;
            a.state_bytes = (int64_t)state;
            // algorithmic bytes of the launch: what every pair reads + the boxes out
            double bytes = 0.0;
            for (int64_t x = c0; x < c0 + cn; ++x) {
                const int32_t p = B.work[(size_t)x];
                bytes += pair_bytes(fused, base.dpad, base.rfeat_h != nullptr, lqs[(size_t)p], lrs[(size_t)p]);
                bytes += 4.0 + 20.0 * VSC_TN_MAX_BOXES;
            }
            AuxTimer tm;
            tm.begin(1, stream);
            VSC_TRY(launch_tn_pairs(a, lds, stream));
            tm.end(bytes, stream);
            VSC_HIP(hipStreamSynchronize(stream));  // B.work (host), the slab and the state are reused
            tm.collect();
            woff += cn;
        }
    }
    return VSC_OK;
}

// ------------------------------------------------------------------------ DTW / DP launches

static int tn_check_params(const char* who, const vsc_tn_params* p) {
    if (p->tn_top_k < 1 || p->tn_top_k > 16 || p->tn_max_step < 1 || p->tn_max_step > 64 || p->max_path < 0 ||
        p->max_path >= VSC_TN_MAX_BOXES) {
        // max_path + 1 extractions can accept max_path + 1 boxes: more than the output holds would silently change
        // the IoU-suppression history
        set_error("%s: unsupported TN parameters (tn_top_k 1..16, tn_max_step 1..64, max_path 0..%d)", who, VSC_TN_MAX_BOXES - 1);
        return VSC_ERR_INVALID;
    }
    return VSC_OK;
}

static int align_check_params(const char* who, const vsc_align_params* p) {
    if ((p->method != VSC_ALIGN_DTW && p->method != VSC_ALIGN_DP) || p->discontinue < 0 || p->discontinue > 15 || p->min_length < 0 ||
        p->max_path < 0 || p->max_path > VSC_TN_MAX_BOXES) {
        set_error("%s: unsupported aligner parameters (method VSC_ALIGN_DTW / VSC_ALIGN_DP, discontinue 0..15, min_length >= 0, "
                  "max_path 0..%d)", who, VSC_TN_MAX_BOXES);
        return VSC_ERR_INVALID;
    }
    return VSC_OK;
}

// The pairs of one call in launches by LDS footprint (a workgroup's allocation is the launch's largest: one long pair
// must not cost the short ones their occupancy).  Every pair is handed to the kernel, which answers the ones it does
// not run (an empty video; more than VSC_ALIGN_MAX_CELLS cells) with their status alone.
static int align_run_buckets(AlignArgs base, const std::vector<int32_t>& lqs, const std::vector<int32_t>& lrs, DevBuf& d_work,
                             hipStream_t stream) {
    const int64_t n_pairs = (int64_t)lqs.size();
    const bool fused = base.sims_in == nullptr;
    constexpr size_t kBucketMax[3] = {24 * 1024, 64 * 1024, ALIGN_LDS_MAX};
    struct Bucket { std::vector<int32_t> work; size_t lds = 0; double bytes = 0.0; } buckets[3];
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t lq = lqs[(size_t)p], lr = lrs[(size_t)p];
        size_t need = 0;
        double bytes = 8.0 + 20.0 * VSC_TN_MAX_BOXES;
        if (lq > 0 && lr > 0 && lq * lr <= VSC_ALIGN_MAX_CELLS) {
            need = align_layout(base.prm.method, (int)lq, (int)lr, fused).total;
            bytes += pair_bytes(fused, base.dpad, base.rfeat_h != nullptr, (double)lq, (double)lr);  // (+ the boxes out, above)
        }
        const int b = need <= kBucketMax[0] ? 0 : (need <= kBucketMax[1] ? 1 : 2);
        buckets[b].work.push_back((int32_t)p);
        buckets[b].lds = std::max(buckets[b].lds, need);
        buckets[b].bytes += bytes;
    }
    VSC_TRY(d_work.reserve((size_t)std::max<int64_t>(n_pairs, 1) * 4));
    int64_t woff = 0;
    AuxTimer tm;
    tm.begin(2, stream);
    for (Bucket& B : buckets) {
        if (B.work.empty()) continue;
        int32_t* dwork = d_work.as<int32_t>() + woff;
        VSC_HIP(hipMemcpyAsync(dwork, B.work.data(), B.work.size() * 4, hipMemcpyHostToDevice, stream));
        AlignArgs a = base;
        a.work = dwork;
        a.n_work = (int)B.work.size();
        VSC_TRY(launch_align_pairs(a, B.lds, stream));
        tm.end(B.bytes, stream);
        woff += (int64_t)B.work.size();
    }
    VSC_HIP(hipStreamSynchronize(stream));  // (the host work lists are read by the copies above)
    tm.collect();
    return VSC_OK;
}

// ------------------------------------------------------------------------ per-batch plumbing

// The box table of a batch -- nbox, boxes, boxmax and (aligners only) status, kBytes[] per pair -- where the caller wants
// it and where the kernel writes it: the caller's own arrays in device memory, device copies of host arrays.
struct BoxTable {
    static constexpr size_t kBytes[4] = {4, VSC_TN_MAX_BOXES * 16, VSC_TN_MAX_BOXES * 4, 4};
    void* host[4];  // the caller's: nbox, boxes, boxmax, status (nullptr: the entry point has none)
    void* dev[4];   // the kernel's
    BoxTable(int32_t* nbox, int32_t* boxes, float* boxmax, int32_t* status = nullptr)
        : host{nbox, boxes, boxmax, status}, dev{nbox, boxes, boxmax, status} {}
    int stage(int64_t n_pairs, int out_mem, DevBuf& b_nbox, DevBuf& b_boxes, DevBuf& b_boxmax, DevBuf& b_status) {
        if (out_mem != VSC_MEM_HOST) return VSC_OK;
        DevBuf* buf[4] = {&b_nbox, &b_boxes, &b_boxmax, &b_status};
        for (int k = 0; k < 4; ++k) {
            if (!host[k]) continue;
            VSC_TRY(buf[k]->reserve((size_t)n_pairs * kBytes[k]));
            dev[k] = buf[k]->p;
        }
        return VSC_OK;
    }
    int copy_back(int64_t n_pairs, hipStream_t stream) const {
        for (int k = 0; k < 4; ++k)
            if (dev[k] != host[k]) VSC_HIP(hipMemcpyAsync(host[k], dev[k], (size_t)n_pairs * kBytes[k], hipMemcpyDeviceToHost, stream));
        return VSC_OK;
    }
    // (every argument block names the kernel's three columns alike; `out_status` is AlignArgs' alone)
    template <class Args> void bind(Args& a) const {
        a.out_nbox = static_cast<int32_t*>(dev[0]);
        a.out_boxes = static_cast<int32_t*>(dev[1]);
        a.out_boxmax = static_cast<float*>(dev[2]);
    }
};

// The caller's matrices of a forward_sim call: pair p is lq[p] x lr[p] at sims + sims_off[p], all in host memory.
// Checked before any device is looked at ...
static int sims_check_shapes(const char* who, const int64_t* sims_off, const int32_t* lq, const int32_t* lr, int64_t n_pairs) {
    for (int64_t p = 0; p < n_pairs; ++p)
        if (lq[p] < 0 || lr[p] < 0 || sims_off[p + 1] - sims_off[p] < (int64_t)lq[p] * lr[p]) {
            set_error("%s: pair %lld has a negative shape or a matrix shorter than lq * lr", who, (long long)p);
            return VSC_ERR_INVALID;
        }
    return VSC_OK;
}
// ... then uploaded into the device context's workspace, where `a` (TnPairArgs / AlignArgs) reads them in place and
// writes the device copy of `out`
template <class Args>
static int upload_sims(DeviceCtx* c, const float* sims, const int64_t* sims_off, const int32_t* lq, const int32_t* lr,
                       int64_t n_pairs, BoxTable& out, Args& a) {
    Workspace& ws = c->ws;
    const int64_t total = sims_off[n_pairs];
    VSC_TRY(ws.mat.reserve((size_t)std::max<int64_t>(total, 1) * 4));
    VSC_TRY(ws.sort.w0.reserve((size_t)(n_pairs + 1) * 8));
    VSC_TRY(ws.sort.w2.reserve((size_t)n_pairs * 4));
    VSC_TRY(ws.sort.w3.reserve((size_t)n_pairs * 4));
    VSC_TRY(out.stage(n_pairs, VSC_MEM_HOST, ws.out[0], ws.out[1], ws.out[2], ws.out[3]));
    out.bind(a);
    if (total > 0) VSC_HIP(hipMemcpyAsync(ws.mat.p, sims, (size_t)total * 4, hipMemcpyHostToDevice, c->stream));
    VSC_HIP(hipMemcpyAsync(ws.sort.w0.p, sims_off, (size_t)(n_pairs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    VSC_HIP(hipMemcpyAsync(ws.sort.w2.p, lq, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
    VSC_HIP(hipMemcpyAsync(ws.sort.w3.p, lr, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
    a.sims_in = ws.mat.as<float>();
    a.sims_off = ws.sort.w0.as<int64_t>();
    a.sims_lq = ws.sort.w2.as<int32_t>();
    a.sims_lr = ws.sort.w3.as<int32_t>();
    return VSC_OK;
}

// ------------------------------------------------------------------------ TN context

// The DnS fine descriptors of a context (tn_set_fine): `regions` rows of row_bytes bytes per frame of either side.
// VSC_FINE_ATT / VSC_FINE_BIN (vsc_tn_set_fine): packed fp32 rows of round_up(dim, K_PAD) floats (bin: +-1);
// VSC_FINE_F16 (vsc_tn_set_fine_f16): as many half floats, natural k order; VSC_FINE_BITS (vsc_tn_set_fine_bits): bit rows
// of fine_bits_row_words(dim) 16-byte words.
struct FineStore {
    int kind = -1, regions = 0, dim = 0, row_bytes = 0;
    struct Side { DevBuf rows; bool has = false; int64_t bytes = 0; } side[2];  // query, reference
};

struct vsc_tn_ctx {
    int device = 0, dim = 0, dpad = 0;
    // VSC_CODEC_FLAT: `rfeat` holds the packed fp32 reference rows.  VSC_CODEC_SQFP16: `rfeat` is never allocated; the
    // rows live once, as half floats, in `rfeat_h` ([r_rows][dpad], natural k order, zero padded) and the kernels
    // convert them in registers.  The query side is packed fp32 either way
    int codec = VSC_CODEC_FLAT;
    int64_t ref_bytes = 0;  // bytes asked for the reference rows (vsc_tn_ref_bytes)
    int64_t n_qvid = 0, n_rvid = 0;
    std::vector<int64_t> q_off, r_off;  // host copies
    DevBuf qfeat, rfeat, rfeat_h, d_qoff, d_roff;
    DevBuf d_pq, d_pr, d_work, d_nbox, d_boxes, d_bmax, d_status, slab, sims;
    // match rows (vsc_tn_set_timestamps / vsc_tn_match_rows): the per-frame [start, end] tables of both sides as float64
    // [rows][2], the scan's scratch and control words, and the row columns when the caller wants them on the host
    DevBuf d_qts, d_rts, d_rowoff, d_tileoff, d_rowctl, d_rows[4];
    bool has_qts = false, has_rts = false;
    // DnS: the fine descriptors, the scratch of vsc_tn_fine_similarity (work list, offsets, error word, dense output for
    // host callers) and of vsc_tn_localize_fine / vsc_tn_similarity_fine (the fine slab of host callers, its offsets,
    // frame counts)
    FineStore fine;
    DevBuf d_fwork, d_foff, d_ferr, fine_out, fine_mat, d_flq, d_flr;
    Workspace ws;
    hipStream_t stream = nullptr;      // own_stream, or the caller's (vsc_tn_set_stream)
    hipStream_t own_stream = nullptr;
};

// The context's descriptors, offsets and the pair list of the current batch (tn_pair_shapes) as a kernel reads them:
// TnPairArgs and AlignArgs name these fields alike (kernels.h)
template <class Args>
static void bind_ctx(Args& a, const vsc_tn_ctx* c, float bias) {
    a.qfeat = c->qfeat.as<float>();
    a.rfeat = c->rfeat.as<float>();
    a.rfeat_h = c->rfeat_h.as<_Float16>();  // (nullptr in a Flat context)
    a.q_off = c->d_qoff.as<int64_t>();
    a.r_off = c->d_roff.as<int64_t>();
    a.dpad = c->dpad;
    a.pair_q = c->d_pq.as<int32_t>();
    a.pair_r = c->d_pr.as<int32_t>();
    a.bias = bias;
}

// What vsc_tn_set_fine, vsc_tn_set_fine_bits and vsc_tn_set_fine_f16 do once their arguments have passed: the store takes
// the new description, and each side that is given is written by write(side, x, rows, dst, rows_out) -- `rows` source
// rows at x -> rows_out rows at dst, those from `rows` on as zeros.  A side that is being replaced is not held, and
// counts 0 bytes, until its new rows are down -- for good if `write` fails: no half-written side is read.
template <class Write>
static int tn_set_fine(vsc_tn_ctx* c, int kind, int regions, int fdim, int row_bytes, const void* qfine, const void* rfine, Write write) {
    VSC_HIP(hipSetDevice(c->device));
    FineStore& f = c->fine;
    const void* x[2] = {qfine, rfine};
    const int64_t frames[2] = {c->q_off.back(), c->r_off.back()};
    // a side kept from another shape or kind could not meet the new one: both are dropped before anything can fail, the
    // ones given come back below
    if (regions != f.regions || fdim != f.dim || kind != f.kind)
        for (FineStore::Side& s : f.side) s.has = false, s.bytes = 0;
    f.kind = kind, f.regions = regions, f.dim = fdim, f.row_bytes = row_bytes;
    for (int k = 0; k < 2; ++k) {
        FineStore::Side& s = f.side[k];
        if (!x[k]) continue;
        s.has = false, s.bytes = 0;  // (until the new rows are down)
        const int64_t rows = frames[k] * regions;
        // +64 rows of slack, zeroed: the 64-row tiles of the last video's last frames read past its end (fine_sim.hip, fine_bits.hip)
        const int64_t rows_out = round_up64(rows + 64, ROW_PAD);
        VSC_TRY(s.rows.reserve((size_t)rows_out * row_bytes));
        VSC_TRY(write(k, x[k], rows, s.rows.p, rows_out));
        s.bytes = rows_out * row_bytes;
        s.has = true;
    }
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

extern "C" {

int vsc_tn_set_stream(vsc_tn_ctx_t* c, void* hip_stream, int own) {
    if (!c) {
        set_error("vsc_tn_set_stream: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_HIP(hipSetDevice(c->device));
    if (c->stream == c->own_stream) VSC_HIP(hipStreamSynchronize(c->own_stream));
    else (void)hipDeviceSynchronize();  // (a caller's stream may be gone: never touched again, see vsc_index_set_stream)
    c->stream = own ? c->own_stream : (hipStream_t)hip_stream;
    return VSC_OK;
}

// Half-float rows at `image` ([r_rows][dpad] halves, natural layout) from `n` fp32 or fp16 rows of `dim` elements, by the
// index codec's encoder (encode_rows): the reference store of an SQfp16 context and a side of a VSC_FINE_F16 fine store
// (vsc_tn_set_fine_f16).  All r_rows rows are written, those from n on as zeros; device sources are chunked like host
// sources; nobody reads the encoder's norm bounds.  *refused: the caller names it and drops what was written.
static int tn_encode_rows(vsc_tn_ctx* c, const void* x, bool src16, int64_t n, int dim, int dpad, int mem, _Float16* image,
                          int64_t r_rows, bool* refused) {
    const int64_t chunk_rows = std::max<int64_t>(ROW_PAD, (int64_t)(256ll << 20) / ((int64_t)dim * (src16 ? 2 : 4)));
    return encode_rows(c->ws, c->stream, x, src16, n, dim, mem, chunk_rows, image, nullptr, 0, r_rows, dpad, false, refused);
}

static int tn_store_rows(vsc_tn_ctx* c, const void* x, bool src16, int64_t n, int mem, int64_t r_rows) {
    bool refused = false;
    VSC_TRY(tn_encode_rows(c, x, src16, n, c->dim, c->dpad, mem, c->rfeat_h.as<_Float16>(), r_rows, &refused));
    if (refused) {
        set_error("vsc_tn_create_codec: a reference row holds NaN, +-inf or a value beyond +-65504, which the SQfp16 codec cannot store");
        return VSC_ERR_INVALID;
    }
    return VSC_OK;
}

int vsc_tn_create_codec(const float* qfeat, const int64_t* q_off, int64_t n_qvid, const void* rfeat, int ref_f16,
                        const int64_t* r_off, int64_t n_rvid, int dim, int feat_mem, int ref_mem, int codec, int device,
                        vsc_tn_ctx_t** out) {
    if (out) *out = nullptr;
    if (!out || dim <= 0 || n_qvid < 0 || n_rvid < 0 || !q_off || !r_off || (codec != VSC_CODEC_FLAT && codec != VSC_CODEC_SQFP16) ||
        (n_rvid > 0 && r_off[n_rvid] > 0 && !rfeat)) {
        set_error("vsc_tn_create_codec: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    vsc_tn_ctx* c = new vsc_tn_ctx();
    c->device = device;
    c->dim = dim;
    c->dpad = round_up(dim, K_PAD);
    c->codec = codec;
    c->n_qvid = n_qvid;
    c->n_rvid = n_rvid;
    c->q_off.assign(q_off, q_off + n_qvid + 1);
    c->r_off.assign(r_off, r_off + n_rvid + 1);
    int rc = VSC_OK;
    auto fail = [&](int code) {
        vsc_tn_destroy(c);
        return code;
    };
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess) c->stream = c->own_stream;
    if (!c->own_stream) {
        set_error("hipStreamCreate failed");
        delete c;
        return VSC_ERR_HIP;
    }
    const int64_t nq = c->q_off.back(), nr = c->r_off.back();
    // +32 rows of slack: the 32-row MFMA blocks of the last video read past its end
    const int64_t q_rows = round_up64(nq + 32, ROW_PAD), r_rows = round_up64(nr + 32, ROW_PAD);
    if ((rc = c->qfeat.reserve((size_t)q_rows * c->dpad * 4)) != VSC_OK) return fail(rc);
    if ((rc = pack_into(qfeat, nq, dim, feat_mem, c->qfeat.as<float>(), q_rows, c->dpad, c->ws, c->stream)) != VSC_OK) return fail(rc);
    if (codec == VSC_CODEC_SQFP16) {
        c->ref_bytes = r_rows * c->dpad * 2;
        if ((rc = c->rfeat_h.reserve((size_t)c->ref_bytes)) != VSC_OK) return fail(rc);
        if ((rc = tn_store_rows(c, rfeat, ref_f16 != 0, nr, ref_mem, r_rows)) != VSC_OK) return fail(rc);
    } else {
        c->ref_bytes = r_rows * c->dpad * 4;
        if ((rc = c->rfeat.reserve((size_t)c->ref_bytes)) != VSC_OK) return fail(rc);
        // (reference rows handed over as half floats: the context of the upcast array)
        if (ref_f16) rc = pack_converted(c->ws, c->stream, rfeat, 2, half_rows_to_float, nr, dim, ref_mem, c->rfeat.as<float>(), r_rows, c->dpad);
        else rc = pack_into(static_cast<const float*>(rfeat), nr, dim, ref_mem, c->rfeat.as<float>(), r_rows, c->dpad, c->ws, c->stream);
        if (rc != VSC_OK) return fail(rc);
    }
    if ((rc = c->d_qoff.reserve((size_t)(n_qvid + 1) * 8)) != VSC_OK) return fail(rc);
    if ((rc = c->d_roff.reserve((size_t)(n_rvid + 1) * 8)) != VSC_OK) return fail(rc);
    if (hipMemcpyAsync(c->d_qoff.p, c->q_off.data(), (size_t)(n_qvid + 1) * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->d_roff.p, c->r_off.data(), (size_t)(n_rvid + 1) * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        set_error("vsc_tn_create_codec: offset upload failed");
        return fail(VSC_ERR_HIP);
    }
    *out = c;
    return VSC_OK;
}

int vsc_tn_create(const float* qfeat, const int64_t* q_off, int64_t n_qvid, const float* rfeat,
                  const int64_t* r_off, int64_t n_rvid, int dim, int feat_mem, int device,
                  vsc_tn_ctx_t** out) {
    return vsc_tn_create_codec(qfeat, q_off, n_qvid, rfeat, 0, r_off, n_rvid, dim, feat_mem, feat_mem, VSC_CODEC_FLAT, device, out);
}

int64_t vsc_tn_ref_bytes(const vsc_tn_ctx_t* c) { return c ? c->ref_bytes : 0; }

int vsc_tn_set_queries(vsc_tn_ctx_t* c, const float* qfeat, const int64_t* q_off, int64_t n_qvid, int feat_mem) {
    if (!c || n_qvid < 0 || !q_off || (n_qvid > 0 && q_off[n_qvid] > 0 && !qfeat)) {
        set_error("vsc_tn_set_queries: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_HIP(hipSetDevice(c->device));
    c->has_qts = false;  // (the table described the rows that are being replaced: vsc_tn_set_timestamps)
    c->fine.side[0].has = false;  // (... and so did the fine descriptors: vsc_tn_set_fine)
    c->fine.side[0].bytes = 0;
    // everything that can fail (allocation, packing, upload) runs on local state first: the context keeps its old,
    // consistent query side if any of it does, and takes the new offsets only once the device holds the new rows
    std::vector<int64_t> off(q_off, q_off + n_qvid + 1);
    const int64_t nq = off.back();
    const int64_t q_rows = round_up64(nq + 32, ROW_PAD);  // (+32: see vsc_tn_create)
    int rc = c->qfeat.reserve((size_t)q_rows * c->dpad * 4);
    if (rc == VSC_OK) rc = pack_into(qfeat, nq, c->dim, feat_mem, c->qfeat.as<float>(), q_rows, c->dpad, c->ws, c->stream);
    if (rc == VSC_OK) rc = c->d_qoff.reserve((size_t)(n_qvid + 1) * 8);
    if (rc == VSC_OK) {
        hipError_t e = hipMemcpyAsync(c->d_qoff.p, off.data(), (size_t)(n_qvid + 1) * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            set_error("vsc_tn_set_queries: upload of the query offsets failed: %s", hipGetErrorString(e));
            rc = VSC_ERR_HIP;
        }
    }
    if (rc != VSC_OK) {
        // the packed rows may be half written: an empty query side is the only state that cannot index past them
        c->n_qvid = 0;
        c->q_off.assign(1, 0);
        return rc;
    }
    c->n_qvid = n_qvid;
    c->q_off.swap(off);
    return VSC_OK;
}

int vsc_tn_destroy(vsc_tn_ctx_t* c) {
    if (!c) return VSC_OK;
    (void)hipSetDevice(c->device);
    if (c->stream == c->own_stream) { if (c->own_stream) (void)hipStreamSynchronize(c->own_stream); }
    else (void)hipDeviceSynchronize();
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return VSC_OK;
}

// The pair list of one batch on both sides -- the context's device copy (d_pq / d_pr) for the kernel, the frame counts
// of every pair on the host for bucketing -- with the ordinals checked against the context's videos.
static int tn_pair_shapes(vsc_tn_ctx* c, const char* who, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                          std::vector<int32_t>& lqs, std::vector<int32_t>& lrs) {
    // pair lists on both sides: host for bucketing, device for the kernel
    std::vector<int32_t> hq((size_t)n_pairs), hr((size_t)n_pairs);
    VSC_TRY(c->d_pq.reserve((size_t)n_pairs * 4));
    VSC_TRY(c->d_pr.reserve((size_t)n_pairs * 4));
    if (pairs_mem == VSC_MEM_HOST) {
        memcpy(hq.data(), pair_q, (size_t)n_pairs * 4);
        memcpy(hr.data(), pair_r, (size_t)n_pairs * 4);
        VSC_HIP(hipMemcpyAsync(c->d_pq.p, pair_q, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
        VSC_HIP(hipMemcpyAsync(c->d_pr.p, pair_r, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
    } else {
        VSC_HIP(hipMemcpyAsync(hq.data(), pair_q, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(hr.data(), pair_r, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(c->d_pq.p, pair_q, (size_t)n_pairs * 4, hipMemcpyDeviceToDevice, c->stream));
        VSC_HIP(hipMemcpyAsync(c->d_pr.p, pair_r, (size_t)n_pairs * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    VSC_HIP(hipStreamSynchronize(c->stream));
    lqs.resize((size_t)n_pairs);
    lrs.resize((size_t)n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t qv = hq[(size_t)p], rv = hr[(size_t)p];
        if (qv < 0 || qv >= c->n_qvid || rv < 0 || rv >= c->n_rvid) {
            set_error("%s: pair %lld has video ordinal out of range", who, (long long)p);
            return VSC_ERR_INVALID;
        }
        lqs[(size_t)p] = (int32_t)std::min<int64_t>(c->q_off[qv + 1] - c->q_off[qv], 0x7fffffff);
        lrs[(size_t)p] = (int32_t)std::min<int64_t>(c->r_off[rv + 1] - c->r_off[rv], 0x7fffffff);
    }
    return VSC_OK;
}

// vsc_tn_localize, and vsc_tn_localize_fine when `fine` is set: the slab of fine matrices (pair p at fine + fine_off[p],
// both in fine_mem) is blended into the coarse tile (geometric) or aligned as it is.
static int tn_localize_run(vsc_tn_ctx_t* c, const char* who, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs,
                           int pairs_mem, const float* fine, const int64_t* fine_off, int fine_mem, bool geometric,
                           const vsc_tn_params* params, float bias, int32_t* out_nbox, int32_t* out_boxes, float* out_boxmax,
                           int out_mem) {
    if (!c || n_pairs < 0 || !params || (n_pairs > 0 && (!pair_q || !pair_r || !out_nbox || !out_boxes || !out_boxmax))) {
        set_error("%s: invalid argument", who);
        return VSC_ERR_INVALID;
    }
    if (n_pairs == 0) return VSC_OK;
    VSC_TRY(tn_check_params(who, params));
    VSC_HIP(hipSetDevice(c->device));
    std::vector<int32_t> lqs, lrs;
    VSC_TRY(tn_pair_shapes(c, who, pair_q, pair_r, n_pairs, pairs_mem, lqs, lrs));
    const float* d_fine = fine;
    const int64_t* d_foff = fine_off;
    if (fine && fine_mem == VSC_MEM_HOST) {  // the part of the host slab the pairs cover goes down in one copy
        int64_t extent = 0;
        for (int64_t p = 0; p < n_pairs; ++p) {
            const int64_t cells = (int64_t)lqs[(size_t)p] * lrs[(size_t)p];
            if (fine_off[p] < 0) {
                set_error("%s: pair %lld has a negative offset into the fine slab", who, (long long)p);
                return VSC_ERR_INVALID;
            }
            if (cells) extent = std::max(extent, fine_off[p] + cells);
        }
        VSC_TRY(c->fine_mat.reserve((size_t)std::max<int64_t>(extent, 1) * 4));
        VSC_TRY(c->d_foff.reserve((size_t)n_pairs * 8));
        if (extent) VSC_HIP(hipMemcpyAsync(c->fine_mat.p, fine, (size_t)extent * 4, hipMemcpyHostToDevice, c->stream));
        VSC_HIP(hipMemcpyAsync(c->d_foff.p, fine_off, (size_t)n_pairs * 8, hipMemcpyHostToDevice, c->stream));
        d_fine = c->fine_mat.as<float>();
        d_foff = c->d_foff.as<int64_t>();
    }
    BoxTable out(out_nbox, out_boxes, out_boxmax);
    VSC_TRY(out.stage(n_pairs, out_mem, c->d_nbox, c->d_boxes, c->d_bmax, c->d_status));
    TnPairArgs base;
    memset(&base, 0, sizeof(base));
    bind_ctx(base, c, bias);
    base.prm = *params;
    out.bind(base);
    if (fine && geometric) {
        base.fine = d_fine;
        base.fine_off = d_foff;
    } else if (fine) {
        // the fine matrices are the aligner's input as they are: forward_sim mode on device memory (no descriptor is read)
        VSC_TRY(c->d_flq.reserve((size_t)n_pairs * 4));
        VSC_TRY(c->d_flr.reserve((size_t)n_pairs * 4));
        VSC_HIP(hipMemcpyAsync(c->d_flq.p, lqs.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
        VSC_HIP(hipMemcpyAsync(c->d_flr.p, lrs.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->stream));
        base.rfeat_h = nullptr;
        base.sims_in = d_fine;
        base.sims_off = d_foff;
        base.sims_lq = c->d_flq.as<int32_t>();
        base.sims_lr = c->d_flr.as<int32_t>();
    }
    VSC_TRY(tn_run_buckets(base, lqs, lrs, c->d_work, c->slab, c->stream));
    VSC_TRY(out.copy_back(n_pairs, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_tn_localize(vsc_tn_ctx_t* c, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs,
                    int pairs_mem, const vsc_tn_params* params, float bias, int32_t* out_nbox,
                    int32_t* out_boxes, float* out_boxmax, int out_mem) {
    return tn_localize_run(c, "vsc_tn_localize", pair_q, pair_r, n_pairs, pairs_mem, nullptr, nullptr, VSC_MEM_HOST, false, params,
                           bias, out_nbox, out_boxes, out_boxmax, out_mem);
}

int vsc_tn_localize_fine(vsc_tn_ctx_t* c, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                         const float* fine, const int64_t* fine_off, int fine_mem, int geometric_mean,
                         const vsc_tn_params* params, float bias, int32_t* out_nbox, int32_t* out_boxes, float* out_boxmax,
                         int out_mem) {
    if (n_pairs > 0 && (!fine || !fine_off)) {
        set_error("vsc_tn_localize_fine: invalid argument (no fine slab)");
        return VSC_ERR_INVALID;
    }
    return tn_localize_run(c, "vsc_tn_localize_fine", pair_q, pair_r, n_pairs, pairs_mem, fine, fine_off, fine_mem,
                           geometric_mean != 0, params, bias, out_nbox, out_boxes, out_boxmax, out_mem);
}

int vsc_tn_forward_sim(const float* sims, const int64_t* sims_off, const int32_t* lq, const int32_t* lr,
                       int64_t n_pairs, const vsc_tn_params* params, int32_t* out_nbox, int32_t* out_boxes,
                       float* out_boxmax, int device) {
    if (n_pairs < 0 || !params || (n_pairs > 0 && (!sims || !sims_off || !lq || !lr || !out_nbox || !out_boxes || !out_boxmax))) {
        set_error("vsc_tn_forward_sim: invalid argument");
        return VSC_ERR_INVALID;
    }
    if (n_pairs == 0) return VSC_OK;
    VSC_TRY(tn_check_params("vsc_tn_forward_sim", params));
    VSC_TRY(sims_check_shapes("vsc_tn_forward_sim", sims_off, lq, lr, n_pairs));
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_tn_forward_sim: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    Workspace& ws = c->ws;
    TnPairArgs base;
    memset(&base, 0, sizeof(base));
    BoxTable out(out_nbox, out_boxes, out_boxmax);
    VSC_TRY(upload_sims(c, sims, sims_off, lq, lr, n_pairs, out, base));
    base.prm = *params;
    std::vector<int32_t> lqs(lq, lq + n_pairs), lrs(lr, lr + n_pairs);
    VSC_TRY(tn_run_buckets(base, lqs, lrs, ws.maps0, ws.maps1, c->stream));
    VSC_TRY(out.copy_back(n_pairs, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_tn_align(vsc_tn_ctx_t* c, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                 const vsc_align_params* params, float bias, int32_t* out_nbox, int32_t* out_boxes, float* out_boxmax,
                 int32_t* out_status, int out_mem) {
    if (!c || n_pairs < 0 || !params ||
        (n_pairs > 0 && (!pair_q || !pair_r || !out_nbox || !out_boxes || !out_boxmax || !out_status))) {
        set_error("vsc_tn_align: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_TRY(align_check_params("vsc_tn_align", params));
    if (n_pairs == 0) return VSC_OK;
    VSC_HIP(hipSetDevice(c->device));
    std::vector<int32_t> lqs, lrs;
    VSC_TRY(tn_pair_shapes(c, "vsc_tn_align", pair_q, pair_r, n_pairs, pairs_mem, lqs, lrs));
    BoxTable out(out_nbox, out_boxes, out_boxmax, out_status);
    VSC_TRY(out.stage(n_pairs, out_mem, c->d_nbox, c->d_boxes, c->d_bmax, c->d_status));
    AlignArgs base;
    memset(&base, 0, sizeof(base));
    bind_ctx(base, c, bias);
    base.prm = *params;
    out.bind(base);
    base.out_status = static_cast<int32_t*>(out.dev[3]);
    VSC_TRY(align_run_buckets(base, lqs, lrs, c->d_work, c->stream));
    VSC_TRY(out.copy_back(n_pairs, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_align_forward_sim(const float* sims, const int64_t* sims_off, const int32_t* lq, const int32_t* lr, int64_t n_pairs,
                          const vsc_align_params* params, int32_t* out_nbox, int32_t* out_boxes, float* out_boxmax,
                          int32_t* out_status, int device) {
    if (n_pairs < 0 || !params ||
        (n_pairs > 0 && (!sims || !sims_off || !lq || !lr || !out_nbox || !out_boxes || !out_boxmax || !out_status))) {
        set_error("vsc_align_forward_sim: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_TRY(align_check_params("vsc_align_forward_sim", params));
    if (n_pairs == 0) return VSC_OK;
    VSC_TRY(sims_check_shapes("vsc_align_forward_sim", sims_off, lq, lr, n_pairs));
    VSC_TRY(check_device(device));
    VSC_HIP(hipSetDevice(device));
    DeviceCtx* c = device_ctx(device);
    if (!c) {
        set_error("vsc_align_forward_sim: cannot create device context");
        return VSC_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    Workspace& ws = c->ws;
    AlignArgs base;
    memset(&base, 0, sizeof(base));
    BoxTable out(out_nbox, out_boxes, out_boxmax, out_status);
    VSC_TRY(upload_sims(c, sims, sims_off, lq, lr, n_pairs, out, base));
    base.out_status = static_cast<int32_t*>(out.dev[3]);
    base.prm = *params;
    std::vector<int32_t> lqs(lq, lq + n_pairs), lrs(lr, lr + n_pairs);
    VSC_TRY(align_run_buckets(base, lqs, lrs, ws.maps0, c->stream));
    VSC_TRY(out.copy_back(n_pairs, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

// ------------------------------------------------------------------------ match rows

int vsc_tn_set_timestamps(vsc_tn_ctx_t* c, const double* q_ts, const double* r_ts, int ts_mem) {
    if (!c) {
        set_error("vsc_tn_set_timestamps: invalid argument");
        return VSC_ERR_INVALID;
    }
    VSC_HIP(hipSetDevice(c->device));
    const hipMemcpyKind kind = ts_mem == VSC_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (q_ts) {
        const size_t bytes = (size_t)c->q_off.back() * 16;
        c->has_qts = false;
        VSC_TRY(c->d_qts.reserve(std::max<size_t>(bytes, 16)));
        if (bytes) VSC_HIP(hipMemcpyAsync(c->d_qts.p, q_ts, bytes, kind, c->stream));
    }
    if (r_ts) {
        const size_t bytes = (size_t)c->r_off.back() * 16;
        c->has_rts = false;
        VSC_TRY(c->d_rts.reserve(std::max<size_t>(bytes, 16)));
        if (bytes) VSC_HIP(hipMemcpyAsync(c->d_rts.p, r_ts, bytes, kind, c->stream));
    }
    VSC_HIP(hipStreamSynchronize(c->stream));
    c->has_qts = c->has_qts || q_ts != nullptr;
    c->has_rts = c->has_rts || r_ts != nullptr;
    return VSC_OK;
}

int vsc_tn_match_rows(vsc_tn_ctx_t* c, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                      const int32_t* nbox, const int32_t* boxes, const float* boxmax, int in_mem, int32_t* out_pair,
                      int32_t* out_box, float* out_score, double* out_times, int64_t cap, int out_mem, int64_t* n_rows) {
    const bool count_only = cap == 0 && !out_pair && !out_box && !out_score && !out_times;
    if (!n_rows || n_pairs < 0 || cap < 0 || (n_pairs > 0 && (!pair_q || !pair_r || !nbox || !boxes || !boxmax)) ||
        (!count_only && (!out_pair || !out_score || !out_times))) {
        set_error("vsc_tn_match_rows: invalid argument");
        return VSC_ERR_INVALID;
    }
    *n_rows = 0;
    // Host-memory inputs are checked here, before anything is launched; first what needs no context
    const bool host_in = in_mem == VSC_MEM_HOST, host_pairs = pairs_mem == VSC_MEM_HOST;
    if (host_in)
        for (int64_t p = 0; p < n_pairs; ++p) {
            if (nbox[p] < 0 || nbox[p] > VSC_TN_MAX_BOXES) {
                set_error("vsc_tn_match_rows: pair %lld has a box count of %d (0..%d)", (long long)p, nbox[p], VSC_TN_MAX_BOXES);
                return VSC_ERR_INVALID;
            }
            for (int x = 0; x < 4 * nbox[p]; ++x)
                if (boxes[p * VSC_TN_MAX_BOXES * 4 + x] < 0) {
                    set_error("vsc_tn_match_rows: pair %lld has a negative box corner", (long long)p);
                    return VSC_ERR_INVALID;
                }
        }
    if (host_pairs)
        for (int64_t p = 0; p < n_pairs; ++p)
            if (pair_q[p] < 0 || pair_r[p] < 0) {
                set_error("vsc_tn_match_rows: pair %lld has video ordinal out of range", (long long)p);
                return VSC_ERR_INVALID;
            }
    if (!c) {
        set_error("vsc_tn_match_rows: invalid argument (no context)");
        return VSC_ERR_INVALID;
    }
    if (host_pairs)
        for (int64_t p = 0; p < n_pairs; ++p) {
            const int32_t qv = pair_q[p], rv = pair_r[p];
            if (qv >= c->n_qvid || rv >= c->n_rvid) {
                set_error("vsc_tn_match_rows: pair %lld has video ordinal out of range", (long long)p);
                return VSC_ERR_INVALID;
            }
            if (!host_in) continue;
            const int64_t lq = c->q_off[qv + 1] - c->q_off[qv], lr = c->r_off[rv + 1] - c->r_off[rv];
            const int32_t* b = boxes + p * VSC_TN_MAX_BOXES * 4;
            for (int s = 0; s < nbox[p]; ++s, b += 4)
                if (b[0] >= lq || b[2] >= lq || b[1] >= lr || b[3] >= lr) {
                    set_error("vsc_tn_match_rows: box %d of pair %lld has a corner beyond its video (%lld x %lld frames)", s,
                              (long long)p, (long long)lq, (long long)lr);
                    return VSC_ERR_INVALID;
                }
        }
    if (!count_only && (!c->has_qts || !c->has_rts)) {
        set_error("vsc_tn_match_rows: the context has no %s timestamp table (vsc_tn_set_timestamps)", c->has_qts ? "reference" : "query");
        return VSC_ERR_INVALID;
    }
    if (n_pairs == 0) return VSC_OK;
    VSC_HIP(hipSetDevice(c->device));
    MatchRowsArgs a;
    memset(&a, 0, sizeof(a));
    const void *dq, *dr, *dn, *db, *dm;
    VSC_TRY(to_device(pair_q, (size_t)n_pairs * 4, pairs_mem, c->d_pq, &dq, c->stream));
    VSC_TRY(to_device(pair_r, (size_t)n_pairs * 4, pairs_mem, c->d_pr, &dr, c->stream));
    VSC_TRY(to_device(nbox, (size_t)n_pairs * 4, in_mem, c->d_nbox, &dn, c->stream));
    VSC_TRY(to_device(boxes, (size_t)n_pairs * VSC_TN_MAX_BOXES * 16, in_mem, c->d_boxes, &db, c->stream));
    VSC_TRY(to_device(boxmax, (size_t)n_pairs * VSC_TN_MAX_BOXES * 4, in_mem, c->d_bmax, &dm, c->stream));
    VSC_TRY(c->d_rowoff.reserve((size_t)n_pairs * 4));
    VSC_TRY(c->d_tileoff.reserve((size_t)match_rows_tiles(n_pairs) * 8));
    VSC_TRY(c->d_rowctl.reserve(16));
    a.pair_q = (const int32_t*)dq;
    a.pair_r = (const int32_t*)dr;
    a.n_pairs = n_pairs;
    a.nbox = (const int32_t*)dn;
    a.boxes = (const int32_t*)db;
    a.boxmax = (const float*)dm;
    a.q_off = c->d_qoff.as<int64_t>();
    a.r_off = c->d_roff.as<int64_t>();
    a.n_qvid = c->n_qvid;
    a.n_rvid = c->n_rvid;
    a.q_ts = c->d_qts.as<double>();
    a.r_ts = c->d_rts.as<double>();
    a.pair_off = c->d_rowoff.as<int32_t>();
    a.tile_off = c->d_tileoff.as<int64_t>();
    a.ctl = c->d_rowctl.as<int64_t>();
    int64_t ctl[2] = {0, 0};
    AuxTimer tm_scan, tm_emit;
    tm_scan.begin(3, c->stream);
    VSC_TRY(launch_match_rows_scan(a, c->stream));
    tm_scan.end(4.0 * (double)n_pairs, c->stream);  // the box counts in
    VSC_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));  // (the host copies of host-memory inputs are read by the uploads above)
    tm_scan.collect();
    const int64_t total = ctl[0];
    *n_rows = total;
    if (ctl[1]) {
        set_error("vsc_tn_match_rows: a pair has a box count outside 0..%d", VSC_TN_MAX_BOXES);
        return VSC_ERR_INVALID;
    }
    if (count_only) return VSC_OK;
    if (cap < total) {
        set_error("vsc_tn_match_rows: output capacity %lld < %lld rows", (long long)cap, (long long)total);
        return VSC_ERR_CAPACITY;
    }
    if (total == 0) return VSC_OK;
    a.out_pair = out_pair;
    a.out_box = out_box;
    a.out_score = out_score;
    a.out_times = out_times;
    if (out_mem == VSC_MEM_HOST) {
        const size_t width[4] = {4, 16, 4, 32};
        for (int k = 0; k < 4; ++k) VSC_TRY(c->d_rows[k].reserve((size_t)total * width[k]));
        a.out_pair = c->d_rows[0].as<int32_t>();
        a.out_box = out_box ? c->d_rows[1].as<int32_t>() : nullptr;
        a.out_score = c->d_rows[2].as<float>();
        a.out_times = c->d_rows[3].as<double>();
    }
    tm_emit.begin(3, c->stream);
    VSC_TRY(launch_match_rows_emit(a, c->stream));
    // pair list + box table in, (pair, box, score, times) per row out, four timestamp gathers per row
    tm_emit.end((8.0 + 20.0 * VSC_TN_MAX_BOXES) * (double)n_pairs + ((out_box ? 60.0 : 44.0) + 32.0) * (double)total, c->stream);
    VSC_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    tm_emit.collect();
    if (ctl[1]) {
        set_error("vsc_tn_match_rows: a pair has %s (rows skipped)",
                  (ctl[1] & 2) ? "a video ordinal out of range" : "a box corner outside its video");
        return VSC_ERR_INVALID;
    }
    if (out_mem == VSC_MEM_HOST) {
        VSC_HIP(hipMemcpyAsync(out_pair, a.out_pair, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_box) VSC_HIP(hipMemcpyAsync(out_box, a.out_box, (size_t)total * 16, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_score, a.out_score, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipMemcpyAsync(out_times, a.out_times, (size_t)total * 32, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipStreamSynchronize(c->stream));
    }
    return VSC_OK;
}

// vsc_tn_similarity, and vsc_tn_similarity_fine when `with_fine` is set: the pair's fine matrix (in fine_mem) is blended
// into the coarse one (geometric) or handed back as it is.
static int tn_similarity_run(vsc_tn_ctx_t* c, const char* who, int32_t q_vid, int32_t r_vid, float bias, bool with_fine,
                             const float* fine, int fine_mem, bool geometric, float* out, int64_t cap, int32_t* lq_out,
                             int32_t* lr_out) {
    if (!c || q_vid < 0 || q_vid >= c->n_qvid || r_vid < 0 || r_vid >= c->n_rvid) {
        set_error("%s: invalid argument", who);
        return VSC_ERR_INVALID;
    }
    const int64_t lq = c->q_off[q_vid + 1] - c->q_off[q_vid], lr = c->r_off[r_vid + 1] - c->r_off[r_vid];
    if (lq_out) *lq_out = (int32_t)lq;
    if (lr_out) *lr_out = (int32_t)lr;
    if (lq * lr > cap || !out) {
        set_error("%s: output capacity %lld < %lld", who, (long long)cap, (long long)(lq * lr));
        return VSC_ERR_CAPACITY;
    }
    if (lq * lr == 0) return VSC_OK;
    if (with_fine && !fine) {
        set_error("%s: invalid argument (no fine matrix)", who);
        return VSC_ERR_INVALID;
    }
    VSC_HIP(hipSetDevice(c->device));
    const size_t bytes = (size_t)lq * lr * 4;
    if (with_fine && !geometric) {  // S = F
        VSC_HIP(hipMemcpyAsync(out, fine, bytes, fine_mem == VSC_MEM_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost, c->stream));
        VSC_HIP(hipStreamSynchronize(c->stream));
        return VSC_OK;
    }
    const void* d_fine = nullptr;
    if (with_fine) VSC_TRY(to_device(fine, bytes, fine_mem, c->fine_mat, &d_fine, c->stream));
    VSC_TRY(c->sims.reserve(bytes));
    TnSimsArgs a{c->qfeat.as<float>(), c->rfeat.as<float>(), c->q_off[q_vid], c->r_off[r_vid], (int)lq, (int)lr,
                 c->dpad, bias, c->sims.as<float>(), c->rfeat_h.as<_Float16>(), static_cast<const float*>(d_fine)};
    VSC_TRY(launch_tn_sims(a, c->stream));
    VSC_HIP(hipMemcpyAsync(out, c->sims.p, bytes, hipMemcpyDeviceToHost, c->stream));
    VSC_HIP(hipStreamSynchronize(c->stream));
    return VSC_OK;
}

int vsc_tn_similarity(vsc_tn_ctx_t* c, int32_t q_vid, int32_t r_vid, float bias, float* out, int64_t cap,
                      int32_t* lq_out, int32_t* lr_out) {
    return tn_similarity_run(c, "vsc_tn_similarity", q_vid, r_vid, bias, false, nullptr, VSC_MEM_HOST, false, out, cap, lq_out, lr_out);
}

// ------------------------------------------------------------------------ DnS: fine descriptors, region Chamfer, blend

int vsc_tn_set_fine(vsc_tn_ctx_t* c, const void* qfine, const void* rfine, int regions, int fdim, int kind, int mem) {
    if (!c || regions < 1 || regions > VSC_FINE_MAX_REGIONS || fdim < 1 || (kind != VSC_FINE_ATT && kind != VSC_FINE_BIN)) {
        set_error("vsc_tn_set_fine: invalid argument (regions 1..%d, fdim >= 1, kind VSC_FINE_ATT / VSC_FINE_BIN)", VSC_FINE_MAX_REGIONS);
        return VSC_ERR_INVALID;
    }
    const int dpad = round_up(fdim, K_PAD);
    return tn_set_fine(c, kind, regions, fdim, dpad * 4, qfine, rfine, [&](int, const void* x, int64_t rows, void* dst, int64_t rows_out) {
        // att: fp32, packed like every other row upload; bin: {0, 1} bytes, converted to +-1 in bounded chunks first
        if (kind == VSC_FINE_ATT)
            return pack_into(static_cast<const float*>(x), rows, fdim, mem, static_cast<float*>(dst), rows_out, dpad, c->ws, c->stream);
        const ConvertRows to_pm1 = [](const void* src, int64_t elems, float* out, hipStream_t s) {
            return launch_bin_to_pm1(static_cast<const uint8_t*>(src), elems, out, s);
        };
        return pack_converted(c->ws, c->stream, x, 1, to_pm1, rows, fdim, mem, static_cast<float*>(dst), rows_out, dpad);
    });
}

// Bit rows: fdim bytes {0, 1} per source row, or ceil(fdim / 8) packed bytes -> w16 16-byte words.  Chunks of <= 64 MB of
// the larger of the two, device sources too; a chunk is one launch.
int vsc_tn_set_fine_bits(vsc_tn_ctx_t* c, const void* qfine, const void* rfine, int regions, int fdim, int packed, int mem) {
    if (!c || regions < 1 || regions > VSC_FINE_MAX_REGIONS || fdim < 1 || fdim > (1 << 24) || (packed != 0 && packed != 1)) {
        set_error("vsc_tn_set_fine_bits: invalid argument (regions 1..%d, fdim 1..%d, packed 0 / 1)", VSC_FINE_MAX_REGIONS, 1 << 24);
        return VSC_ERR_INVALID;
    }
    const int w16 = fine_bits_row_words(fdim);
    const int64_t src_row = packed ? (fdim + 7) / 8 : fdim;
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(64ll << 20) / std::max<int64_t>(src_row, 16 * (int64_t)w16));
    return tn_set_fine(c, VSC_FINE_BITS, regions, fdim, w16 * 16, qfine, rfine, [&](int, const void* x, int64_t rows, void* dst, int64_t rows_out) {
        return for_row_chunks(c->ws, c->stream, x, (size_t)src_row, mem, rows, rows_out, chunk_rows, false, [&](const void* src, const RowPiece& p) {
            return launch_pack_bits(static_cast<const uint8_t*>(src), packed != 0, p.rows, fdim, static_cast<uint32_t*>(dst) + p.r0 * 4 * w16,
                                    p.rows_out, w16, c->stream);
        });
    });
}

int vsc_tn_set_fine_f16(vsc_tn_ctx_t* c, const void* qfine, const void* rfine, int regions, int fdim, int src_f16, int mem) {
    if (!c || regions < 1 || regions > VSC_FINE_MAX_REGIONS || fdim < 1 || (src_f16 != 0 && src_f16 != 1)) {
        set_error("vsc_tn_set_fine_f16: invalid argument (regions 1..%d, fdim >= 1, src_f16 0 / 1)", VSC_FINE_MAX_REGIONS);
        return VSC_ERR_INVALID;
    }
    const int dpad = round_up(fdim, K_PAD);  // (halves per row: a multiple of 128 bytes, every 16-byte piece aligned)
    return tn_set_fine(c, VSC_FINE_F16, regions, fdim, dpad * 2, qfine, rfine, [&](int side, const void* x, int64_t rows, void* dst, int64_t rows_out) {
        bool refused = false;
        VSC_TRY(tn_encode_rows(c, x, src_f16 != 0, rows, fdim, dpad, mem, static_cast<_Float16*>(dst), rows_out, &refused));
        if (refused) {
            const char* name = side ? "reference" : "query";
            set_error("vsc_tn_set_fine_f16: a %s fine descriptor holds NaN, +-inf or a value beyond +-65504, which a half float "
                      "cannot store (the context keeps no %s fine descriptors)", name, name);
            return VSC_ERR_INVALID;
        }
        return VSC_OK;
    });
}

int64_t vsc_tn_fine_bytes(const vsc_tn_ctx_t* c) { return c ? c->fine.side[0].bytes + c->fine.side[1].bytes : 0; }

int vsc_tn_fine_similarity(vsc_tn_ctx_t* c, const int32_t* pair_q, const int32_t* pair_r, int64_t n_pairs, int pairs_mem,
                           int symmetric, float* out, const int64_t* out_off, int64_t cap, int out_mem) {
    if (!c || n_pairs < 0 || cap < 0 || (n_pairs > 0 && (!pair_q || !pair_r || !out_off))) {
        set_error("vsc_tn_fine_similarity: invalid argument");
        return VSC_ERR_INVALID;
    }
    if (n_pairs == 0) return VSC_OK;
    // (a side without frames needs no descriptors: no pair has a cell to fill)
    const FineStore& f = c->fine;
    if ((!f.side[0].has && c->q_off.back() > 0) || (!f.side[1].has && c->r_off.back() > 0)) {
        set_error("vsc_tn_fine_similarity: the context has no %s fine descriptors (vsc_tn_set_fine)", f.side[0].has ? "reference" : "query");
        return VSC_ERR_INVALID;
    }
    VSC_HIP(hipSetDevice(c->device));
    std::vector<int32_t> lqs, lrs;
    VSC_TRY(tn_pair_shapes(c, "vsc_tn_fine_similarity", pair_q, pair_r, n_pairs, pairs_mem, lqs, lrs));
    std::vector<int64_t> off((size_t)n_pairs);
    if (out_mem == VSC_MEM_HOST) memcpy(off.data(), out_off, (size_t)n_pairs * 8);
    else {
        VSC_HIP(hipMemcpyAsync(off.data(), out_off, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, c->stream));
        VSC_HIP(hipStreamSynchronize(c->stream));
    }
    // capacity first: nothing is written when one pair does not fit
    const int frames = fine_sim_frames(f.regions);
    int64_t total = 0, n_work = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t lq = lqs[(size_t)p], lr = lrs[(size_t)p], cells = lq * lr;
        if (cells == 0) continue;
        if (off[(size_t)p] < 0 || off[(size_t)p] + cells > cap || !out) {
            set_error("vsc_tn_fine_similarity: pair %lld (%lld x %lld frames at offset %lld) does not fit the output capacity %lld",
                      (long long)p, (long long)lq, (long long)lr, (long long)off[(size_t)p], (long long)cap);
            return VSC_ERR_CAPACITY;
        }
        total += cells;
        n_work += ((lq + frames - 1) / frames) * ((lr + frames - 1) / frames);
    }
    if (n_work == 0) return VSC_OK;
    if (n_work > 0x7fffffffLL / 3) {
        set_error("vsc_tn_fine_similarity: %lld tiles in one call are beyond the supported size", (long long)n_work);
        return VSC_ERR_INVALID;
    }
    // the work list: (pair, tile), pair after pair -- long and short pairs share the launch
    std::vector<int32_t> work;
    work.reserve((size_t)n_work * 3);
    std::vector<int64_t> dense;  // host callers: the device copy is dense, the matrices are scattered after the copy back
    if (out_mem == VSC_MEM_HOST) dense.resize((size_t)n_pairs);
    int64_t fill = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int lq = lqs[(size_t)p], lr = lrs[(size_t)p];
        if (out_mem == VSC_MEM_HOST) dense[(size_t)p] = fill;
        fill += (int64_t)lq * lr;
        if (lq == 0 || lr == 0) continue;
        for (int qf = 0; qf < lq; qf += frames)
            for (int rf = 0; rf < lr; rf += frames) {
                work.push_back((int32_t)p);
                work.push_back(qf);
                work.push_back(rf);
            }
    }
    VSC_TRY(c->d_fwork.reserve(work.size() * 4));
    VSC_TRY(c->d_ferr.reserve(16));
    VSC_HIP(hipMemcpyAsync(c->d_fwork.p, work.data(), work.size() * 4, hipMemcpyHostToDevice, c->stream));
    VSC_HIP(hipMemsetAsync(c->d_ferr.p, 0, sizeof(int), c->stream));
    float* d_out = out;
    const int64_t* d_off = out_off;
    if (out_mem == VSC_MEM_HOST) {
        VSC_TRY(c->fine_out.reserve((size_t)total * 4));
        VSC_TRY(c->d_foff.reserve((size_t)n_pairs * 8));
        VSC_HIP(hipMemcpyAsync(c->d_foff.p, dense.data(), (size_t)n_pairs * 8, hipMemcpyHostToDevice, c->stream));
        d_out = c->fine_out.as<float>();
        d_off = c->d_foff.as<int64_t>();
    }
    // what both kernels' argument blocks name alike (kernels.h)
    auto bind = [&](auto& a) {
        memset(&a, 0, sizeof(a));
        a.q_off = c->d_qoff.as<int64_t>();
        a.r_off = c->d_roff.as<int64_t>();
        a.n_qvid = c->n_qvid;
        a.n_rvid = c->n_rvid;
        a.pair_q = c->d_pq.as<int32_t>();
        a.pair_r = c->d_pr.as<int32_t>();
        a.work = c->d_fwork.as<int32_t>();
        a.n_work = (int)n_work;
        a.regions = f.regions;
        a.fdim = f.dim;
        a.symmetric = symmetric != 0;
        a.err = c->d_ferr.as<int>();
        a.out = d_out;
        a.out_off = d_off;
    };
    const DevBuf &qrows = f.side[0].rows, &rrows = f.side[1].rows;
    if (f.kind == VSC_FINE_BITS) {
        FineBitsArgs a;
        bind(a);
        a.qbits = qrows.as<uint4>();
        a.rbits = rrows.as<uint4>();
        a.w16 = f.row_bytes / 16;
        VSC_TRY(launch_fine_bits(a, c->stream));
    } else {
        const bool half_rows = f.kind == VSC_FINE_F16;
        FineSimArgs a;
        bind(a);
        a.qfine = qrows.as<float>();
        a.rfine = rrows.as<float>();
        a.qfine_h = qrows.as<_Float16>();  // (the same buffers: the store's kind says which of the two is read)
        a.rfine_h = rrows.as<_Float16>();
        a.dpad = f.row_bytes / (half_rows ? 2 : 4);
        a.bin = f.kind == VSC_FINE_BIN;
        VSC_TRY(launch_fine_sim(a, c->stream, half_rows));
    }
    int err = 0;
    VSC_HIP(hipMemcpyAsync(&err, c->d_ferr.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    std::vector<float> back;
    if (out_mem == VSC_MEM_HOST) {
        back.resize((size_t)total);
        VSC_HIP(hipMemcpyAsync(back.data(), c->fine_out.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VSC_HIP(hipStreamSynchronize(c->stream));  // (the host work list is read by the copy above)
    if (err) {
        set_error("vsc_tn_fine_similarity: a pair has a video ordinal out of range (tiles skipped)");
        return VSC_ERR_INVALID;
    }
    if (out_mem == VSC_MEM_HOST)
        for (int64_t p = 0; p < n_pairs; ++p) {
            const int64_t cells = (int64_t)lqs[(size_t)p] * lrs[(size_t)p];
            if (cells) memcpy(out + off[(size_t)p], back.data() + dense[(size_t)p], (size_t)cells * 4);
        }
    return VSC_OK;
}

int vsc_tn_similarity_fine(vsc_tn_ctx_t* c, int32_t q_vid, int32_t r_vid, float bias, const float* fine, int fine_mem,
                           int geometric_mean, float* out, int64_t cap, int32_t* lq_out, int32_t* lr_out) {
    return tn_similarity_run(c, "vsc_tn_similarity_fine", q_vid, r_vid, bias, true, fine, fine_mem, geometric_mean != 0, out, cap,
                             lq_out, lr_out);
}

}  // extern "C"
