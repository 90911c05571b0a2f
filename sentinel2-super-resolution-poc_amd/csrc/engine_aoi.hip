// libs2sr engine, the whole-image (area of interest) path: the tile plan, RealESRGAN.enhance with its chunked window loop, the
// device-side cut / stitch entries of the multi-GPU path, the staged device-to-host copies and the post-process drivers.
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "band_plan.h"
#include "blend_plan.h"
#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

namespace s2sr::engine {

static bool is_pinned_host(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // an ordinary malloc'd pointer is "invalid value" to the runtime: not an error of ours
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// Device -> caller's host buffer, `bytes` from `src`, ordered behind everything already on the copy stream; returns when the
// bytes are in `dst`.  The caller's buffer is ordinary pageable memory (a numpy array): handed to hipMemcpyAsync directly, the
// runtime moves it with copy KERNELS through its own staging at ~6 GB/s, and those kernels take CUs from the persistent conv
// workgroups of the chunk computing meanwhile (4096 x 4096 AOI: +20 ms of compute under 130 ms of copies).  Here: two pinned
// 32-MB slices filled by the DMA engines (pinned destination), emptied by this thread's memcpy while the next slice flies.
// `exposed`: nothing computes under this copy (the last band, or the only one): below 128 MB the runtime's own path is then as
// fast or faster (50 MB: 58.1 vs 60.3 ms per 1024 x 1024 call), and there are no conv workgroups for its copy kernels to displace.
int d2h_staged(s2sr_handle* h, uint8_t* dst, const uint8_t* src, size_t bytes, bool exposed) {
    if (is_pinned_host(dst)) {   // s2sr_host_alloc'd (or registered) destination: one DMA, nothing for this thread to copy
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->copy_stream));
        HIPCHK(h, hipStreamSynchronize(h->copy_stream));
        return S2SR_OK;
    }
    if (!h->d2h_staged_on || bytes < (exposed ? (128u << 20) : (24u << 20))) {
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->copy_stream));
        HIPCHK(h, hipStreamSynchronize(h->copy_stream));
        return S2SR_OK;
    }
    for (int i = 0; i < 2; ++i) {
        if (!h->stage_buf[i]) HIPCHK(h, host_malloc(&h->stage_buf[i], kStageBytes, hipHostMallocDefault));
        if (!h->stage_ev[i]) HIPCHK(h, hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming));
    }
    const size_t nsl = (bytes + kStageBytes - 1) / kStageBytes;
    auto len = [&](size_t k) { return k + 1 < nsl ? kStageBytes : bytes - k * kStageBytes; };
    for (size_t k = 0; k < nsl + 2; ++k) {
        const int i = (int)(k & 1);
        if (k >= 2) {   // slice k-2 sits in buffer i
            HIPCHK(h, ev_host_wait(h, h->stage_ev[i], SITE_STAGE_SLICE));
            memcpy(dst + (k - 2) * kStageBytes, h->stage_buf[i], len(k - 2));
        }
        if (k < nsl) {
            HIPCHK(h, hipMemcpyAsync(h->stage_buf[i], src + k * kStageBytes, len(k), hipMemcpyDeviceToHost, h->copy_stream));
            HIPCHK(h, ev_record(h, h->stage_ev[i], h->copy_stream, SITE_STAGE_SLICE));
        }
    }
    return S2SR_OK;
}

// Chunk sizes of a tiled enhance(), front to back, in row units (pure host arithmetic; s2sr_debug_plan_chunks exposes it to the
// CPU tests).  `unit_windows` windows per row unit, `per` windows per launch image (a mosaic; 1 without), `pimg` 32 x 32 patches per
// launch image, `ncu` persistent workgroups.  The tail (last, middle) is searched for the fewest trunk-conv rounds plus the
// exposed copy of the last band; what is left goes in front in pieces of at most u_max units.
void plan_chunk_sizes(int units, int u_max, long unit_windows, int per, long pimg, int ncu, std::vector<int>& sizes) {
    sizes.clear();
    if (units <= 0) return;
    if (u_max < 1) u_max = 1;
    if (per < 1) per = 1;
    if (ncu < 1) ncu = 1;
    auto rounds = [&](int u) -> double {                                        // trunk-conv rounds of a chunk of u units
        const long imgs = ((long)u * unit_windows + per - 1) / per;
        return (double)((imgs * pimg + ncu - 1) / ncu);
    };
    const double copy_per_unit = (double)unit_windows * pimg / per / ncu / 6.0;  // exposed copy of one unit, in rounds
    int best_last = 1, best_mid = 0;
    double best = 1e300;
    for (int last = 1; last <= 3 && last <= units; ++last)
        for (int mid = 0; mid <= 12 && last + mid <= units; ++mid) {
            if (mid > u_max || last > u_max || mid > 5 * last) continue;         // a band's copy must fit under the next chunk's compute (~6x)
            const int front = units - last - mid;
            if (front > 0 && mid == 0 && front > 5 * last) continue;            // a big chunk straight in front of the last one
            if (front > 0 && mid > 0 && front > 6 * mid && front <= u_max) continue;
            double c = rounds(last) + (mid ? rounds(mid) : 0.0) + last * copy_per_unit;
            for (int left = front; left > 0;) { const int u = left < u_max ? left : u_max; c += rounds(u); left -= u; }
            if (c < best - 1e-9) { best = c; best_last = last; best_mid = mid; }
        }
    for (int left = units - best_last - best_mid; left > 0;) { const int u = left < u_max ? left : u_max; sizes.push_back(u); left -= u; }
    if (best_mid) sizes.push_back(best_mid);
    sizes.push_back(best_last);
}

// The reference's window plan of a PH x PW image (s2sr_plan_tiles, in its y-outer / x-inner order): ny rows of nx windows, all of
// one shape wh x ww.
struct TilePlan {
    std::vector<s2sr_window> wins;
    int nx = 0, ny = 0, wh = 0, ww = 0;
};
constexpr const char* kBadPlan = "window plan: s2sr_plan_tiles refuses these image / tile / pad sizes";
static int plan_windows(int PH, int PW, int tile, int pad, int scale, TilePlan& p) {   // s2sr_plan_tiles' code
    int T = 0;
    int rc = s2sr_plan_tiles(PH, PW, tile, pad, scale, nullptr, 0, &T);
    if (rc) return rc;
    p.wins.resize(T);
    if ((rc = s2sr_plan_tiles(PH, PW, tile, pad, scale, p.wins.data(), T, &T))) return rc;
    p.nx = (PW + tile - 1) / tile; p.ny = (PH + tile - 1) / tile;
    p.wh = p.wins[0].y2 - p.wins[0].y1; p.ww = p.wins[0].x2 - p.wins[0].x1;
    return S2SR_OK;
}

// host-side maps of the paste rule; shared by enhance and the multi-GPU stitch
static void build_stitch_maps(const TilePlan& p, int OH, int OW, std::vector<int32_t>& rm, std::vector<int32_t>& cm) {
    rm.assign(2 * (size_t)OH, -1);
    cm.assign(2 * (size_t)OW, -1);
    // last window in loop order wins (:278): ascending index, later entries overwrite the map
    for (int y = 0; y < p.ny; ++y) {
        const s2sr_window& w = p.wins[(size_t)y * p.nx];
        for (int oy = w.oy1; oy < w.oy2; ++oy) { rm[2 * oy] = y; rm[2 * oy + 1] = oy - w.oy1 + w.crop_top; }
    }
    for (int x = 0; x < p.nx; ++x) {
        const s2sr_window& w = p.wins[x];
        for (int ox = w.ox1; ox < w.ox2; ++ox) { cm[2 * ox] = x; cm[2 * ox + 1] = ox - w.ox1 + w.crop_left; }
    }
}

// The window job of RealESRGAN.enhance on a PH x PW image (pure host arithmetic; s2sr_debug_plan_windows exposes it to the CPU
// tests).  Callers that crop read the first OH x OW entries of the maps.  Returns s2sr_plan_tiles' code (sizes it refuses).
int plan_window_job(int PH, int PW, int tile, int pad, int scale, bool tiled, WindowJob& job) {
    job = WindowJob();
    if (PH <= 0 || PW <= 0 || scale <= 0) return S2SR_E_INVALID;
    if (!tiled) {   // the image is its own window: identity maps
        job.wh = PH; job.ww = PW;
        job.rm.resize(2 * (size_t)PH * scale); job.cm.resize(2 * (size_t)PW * scale);
        for (int i = 0; i < PH * scale; ++i) { job.rm[2 * i] = 0; job.rm[2 * i + 1] = i; }
        for (int i = 0; i < PW * scale; ++i) { job.cm[2 * i] = 0; job.cm[2 * i + 1] = i; }
        return S2SR_OK;
    }
    TilePlan p;
    if (int rc = plan_windows(PH, PW, tile, pad, scale, p)) return rc;
    job.wh = p.wh; job.ww = p.ww;
    build_stitch_maps(p, PH * scale, PW * scale, job.rm, job.cm);
    // When a dimension ends within 2*pad of a tile multiple, the last two window rows (columns)
    // of the plan are the same rectangle: the reference runs the net on both (only the paste
    // ranges differ).  Identical inputs give identical outputs, so each distinct rectangle is
    // forwarded once and the paste maps point at it.
    std::vector<int> uy(p.ny), ux(p.nx), rows_y1, cols_x1;
    for (int y = 0; y < p.ny; ++y) {
        const int y1 = p.wins[(size_t)y * p.nx].y1;
        if (rows_y1.empty() || rows_y1.back() != y1) rows_y1.push_back(y1);
        uy[y] = (int)rows_y1.size() - 1;
    }
    for (int x = 0; x < p.nx; ++x) {
        const int x1 = p.wins[x].x1;
        if (cols_x1.empty() || cols_x1.back() != x1) cols_x1.push_back(x1);
        ux[x] = (int)cols_x1.size() - 1;
    }
    for (size_t i = 0; i < job.rm.size(); i += 2)
        if (job.rm[i] >= 0) job.rm[i] = uy[job.rm[i]];
    for (size_t i = 0; i < job.cm.size(); i += 2)
        if (job.cm[i] >= 0) job.cm[i] = ux[job.cm[i]];
    job.nx = (int)cols_x1.size(); job.ny = (int)rows_y1.size();
    job.rects.resize(4 * (size_t)job.nx * job.ny);
    for (int y = 0; y < job.ny; ++y)
        for (int x = 0; x < job.nx; ++x) {
            const int t = y * job.nx + x;
            job.rects[4 * t] = rows_y1[y]; job.rects[4 * t + 1] = rows_y1[y] + p.wh; job.rects[4 * t + 2] = cols_x1[x]; job.rects[4 * t + 3] = cols_x1[x] + p.ww;
        }
    return S2SR_OK;
}

// Window rectangles and the row / column tables of a paste (the paste maps, or the blend tables; empty: none) on the device, one
// behind the other in SL_TABLES: d[0 .. 3) point at them.  Uploaded before this returns.
static int upload_tables(s2sr_handle* h, hipStream_t st, const std::vector<int32_t>& rects, const std::vector<int32_t>& rows,
                         const std::vector<int32_t>& cols, int32_t* d[3]) {
    const std::vector<int32_t>* v[3] = {&rects, &rows, &cols};
    int rc = ensure_scratch(h, SL_TABLES, (rects.size() + rows.size() + cols.size()) * 4);
    if (rc) return rc;
    int32_t* at = scratch<int32_t>(h, SL_TABLES);
    for (int i = 0; i < 3; at += v[i++]->size()) {
        d[i] = at;
        if (!v[i]->empty()) HIPCHK(h, hipMemcpyAsync(at, v[i]->data(), v[i]->size() * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(h, hipStreamSynchronize(st));   // the vectors are host buffers of the caller
    return S2SR_OK;
}

// The chunks of a tiled job: the first window row of each chunk, plus ny at the end.
// Chunks of whole window rows.  An output row is final once the last window row that pastes into it is done (the row
// map is monotone), so each chunk is followed by the stitch of its band of final rows, and the band's device-to-host
// copy runs on the copy stream under the next chunk's compute.  A chunk holds whole launch groups: for windows that
// travel as mosaics (forward_dev) rows in multiples of what fills a mosaic, and as many mosaics as the workspace
// allows -- the patch count of a launch must be large against the 256 workgroups (one 4 x 4 mosaic of 276-pixel
// windows is 1225 patches = 4.8 per CU, five rounds for 4.8 rounds of work; five mosaics are 23.9 -> 24).
// Chunk sizes.  The device-to-host copy of a chunk's band hides under the NEXT chunk's compute and only the last band's
// copy is exposed, so chunks shrink towards the end (a row of 276-pixel windows computes ~6x longer than its 13 MB band
// takes to reach pageable host memory; a chunk may be up to 5x its successor).  What a small chunk costs is the rounding
// of its patch count to whole rounds of the persistent workgroups in the trunk convs (32 x 32 patches; a 4 x 4 mosaic
// of 276-pixel windows = 1225 patches = 4.8 rounds of 256: 1, 2, 3, 4 mosaics lose 4.3 %, 5 or 10 lose 0.3 %).  The
// tail (last, middle) is searched over small sizes for the fewest rounds + exposed copy; the rest goes in front in
// workspace-sized pieces.  4096 x 4096 at 256/10: 16 rows of 16 windows -> 10 + 5 + 1.
// `mo`: the ONE mosaic plan of the job -- every chunk runs in its workspace geometry.
static std::vector<int> plan_chunk_rows(const s2sr_handle* h, const WindowJob& job, const Mosaic& mo) {
    const int nx = job.nx, ny = job.ny, u = h->unshuffle(), per = mo.per();
    const int gw = group_windows(h, mo, nx * ny, job.wh, job.ww);               // windows per launch group
    const int r_min = (per + nx - 1) / nx;                                      // rows that fill a mosaic
    const int units = (ny + r_min - 1) / r_min;                                 // ... and how many such row units the image has
    int u_max = gw / nx / r_min;                                                // units per chunk the workspace allows
    if (u_max < 1) u_max = 1;
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device);
    std::vector<int> sizes, chunk_r0;                                           // sizes: in units, front to back
    plan_chunk_sizes(units, u_max, r_min * nx, per, mo.patches(job.wh / u, job.ww / u), ncu, sizes);
    int r = 0;
    for (int n : sizes) { chunk_r0.push_back(r); r += n * r_min; }
    chunk_r0.push_back(ny);
    return chunk_r0;
}

// The chunk loop of a whole-image job (the untiled image: one chunk of one window): forward(t0, n) runs the net on windows [t0, t0 + n), finish(t0, yb, ye) turns the band of output
// rows that chunk made final into image rows on the device (t0: the chunk's first window, for a door that keeps one chunk's
// tiles).  `copy`: each band (row_b bytes per row, at dev, to host) leaves on the copy stream under the next chunk's compute,
// the last one exposed.  Events group_done[0 .. nchunks) are the caller's to provide.
// band_end: the bands (plan_bands, band_plan.h) -- chunk c makes rows [band_end[c - 1], band_end[c]) final, the paste's band.
// out_end: the rows that are ready to leave behind chunk c, [out_end[c - 1], out_end[c]) -- band_end itself, unless a consistency
// pass trails the paste (cons_out_end); finish(t0, pyb, pye, yb, ye) gets both bands.
template <class Forward, class Finish>
static int run_chunks(s2sr_handle* h, hipStream_t st, int nx, const std::vector<int>& chunk_r0, const std::vector<int>& band_end,
                      const std::vector<int>& out_end, Forward forward, Finish finish, uint8_t* host, const uint8_t* dev, size_t row_b, bool copy) {
    const int nchunks = (int)band_end.size();
    int rc, pyb = 0, yb = 0, prev_yb = 0, prev_ye = 0;
    for (int c = 0; c < nchunks; ++c) {
        const int r0 = chunk_r0[c], r1 = chunk_r0[c + 1], pye = band_end[c], ye = out_end[c];
        if ((rc = forward(r0 * nx, (r1 - r0) * nx))) return rc;
        if ((pye > pyb || ye > yb) && (rc = finish(r0 * nx, pyb, pye, yb, ye))) return rc;
        HIPCHK(h, ev_record(h, h->group_done[c], st, SITE_CHUNK_BAND_D2H));
        if (copy && c > 0 && prev_ye > prev_yb) {
            HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->group_done[c - 1], SITE_CHUNK_BAND_D2H));
            if ((rc = d2h_staged(h, host + (size_t)prev_yb * row_b, dev + (size_t)prev_yb * row_b, (size_t)(prev_ye - prev_yb) * row_b, false))) return rc;
        }
        prev_yb = yb; prev_ye = ye; yb = ye; pyb = pye;
    }
    if (copy && prev_ye > prev_yb) {
        HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->group_done[nchunks - 1], SITE_CHUNK_BAND_D2H));
        if ((rc = d2h_staged(h, host + (size_t)prev_yb * row_b, dev + (size_t)prev_yb * row_b, (size_t)(prev_ye - prev_yb) * row_b, true))) return rc;
    }
    return S2SR_OK;
}

}  // namespace s2sr::engine

extern "C" {

int s2sr_plan_tiles(int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t scale, s2sr_window* out, int32_t cap,
                    int32_t* n) {
    if (H <= 0 || W <= 0 || tile <= 0 || pad < 0 || scale <= 0 || !n) return S2SR_E_INVALID;
    const int nx = (W + tile - 1) / tile, ny = (H + tile - 1) / tile;
    *n = nx * ny;
    if (!out) return S2SR_OK;
    if (cap < nx * ny) return S2SR_E_CAPACITY;
    const int win = tile + 2 * pad, op = pad * scale;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            s2sr_window& w = out[y * nx + x];
            // far edge first, then pull the near edge in so the window keeps its full extent
            w.x2 = (x * tile + win < W) ? x * tile + win : W;
            w.y2 = (y * tile + win < H) ? y * tile + win : H;
            w.x1 = (w.x2 - win > 0) ? w.x2 - win : 0;
            w.y1 = (w.y2 - win > 0) ? w.y2 - win : 0;
            // the halo is dropped on every side that has a neighbouring tile INDEX
            w.crop_left = x > 0 ? op : 0;
            w.crop_top = y > 0 ? op : 0;
            w.crop_right = x < nx - 1 ? op : 0;
            w.crop_bottom = y < ny - 1 ? op : 0;
            w.ox1 = w.x1 * scale + w.crop_left;
            w.oy1 = w.y1 * scale + w.crop_top;
            w.ox2 = w.x2 * scale - w.crop_right;
            w.oy2 = w.y2 * scale - w.crop_bottom;
        }
    return S2SR_OK;
}

// post-process on device buffers; the caller holds h->mu
static int postprocess_dev_locked(s2sr_handle* h, const void* d_rgb, int32_t B, int32_t H, int32_t W, const s2sr_pp_params* prm,
                                  void* d_out, hipStream_t st) {
    if (const char* why = pp_params_error(*prm)) return fail(h, S2SR_E_INVALID, why);
    const size_t wb = postprocess_work_bytes(B, H, W, *prm);
    int rc = ensure_scratch(h, SL_PP, wb);
    if (rc) return rc;
    Scope sc(h, st, F_POST, 0.0, (double)B * H * W * 9.0);
    HIPCHK(h, launch_postprocess((const uint8_t*)d_rgb, B, H, W, *prm, (uint8_t*)d_out, scratch(h, SL_PP), wb, st));
    return S2SR_OK;
}

int s2sr_postprocess_batch_u8_dev(s2sr_handle* h, const void* d_rgb, int32_t B, int32_t H, int32_t W,
                                  const s2sr_pp_params* prm, void* d_out, void* stream) {
    if (!h || !d_rgb || !d_out || !prm || B <= 0 || H <= 0 || W <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, as everywhere in HIP
    DOOR_ENTER(h, st);
    return door_leave(h, st, postprocess_dev_locked(h, d_rgb, B, H, W, prm, d_out, st));
}

// ---- the post-process over one device image in row bands (see postprocess.hip launch_pp_band_*) -------------------------------
// order: S2SR_PP_ORDER_BGR = the image's bytes are B,G,R; S2SR_PP_ORDER_SWAP_OUT = R and B exchanged in the rows written
static int pp_band_begin_locked(s2sr_handle* h, int H, int W, const s2sr_pp_params* prm, int order, hipStream_t st) {
    if (const char* why = pp_params_error(*prm)) {
        h->scratch.run_open = false;   // a refused begin leaves no run behind, the caller's earlier one included
        return fail(h, S2SR_E_INVALID, why);
    }
    int rc = ensure_scratch(h, SL_PP, postprocess_work_bytes(1, H, W, *prm));
    if (rc) return rc;
    s2sr_handle::PPBand& b = h->ppb;
    b = s2sr_handle::PPBand();
    b.H = H; b.W = W; b.prm = *prm;
    b.bgr = (order & S2SR_PP_ORDER_BGR) ? 1 : 0;
    b.swap_out = (order & S2SR_PP_ORDER_SWAP_OUT) ? 1 : 0;
    b.radius = pp_band_radius(*prm);
    HIPCHK(h, launch_pp_band_begin(H, W, *prm, scratch(h, SL_PP), st));
    h->scratch.run_open = true;
    return S2SR_OK;
}

static int pp_band_hist_locked(s2sr_handle* h, const void* d_img, int y0, int y1, hipStream_t st) {
    s2sr_handle::PPBand& b = h->ppb;
    if (!h->scratch.run_open || b.lut) return fail(h, S2SR_E_INVALID, "pp_band_hist: no banded post-process open (none begun, or another call took its scratch area since: begin again), or its LUTs are already built");
    if (y0 < 0 || y1 > b.H || y0 > y1) return fail(h, S2SR_E_INVALID, "pp_band_hist: rows outside the image");
    Scope sc(h, st, F_POST, 0.0, (double)(y1 - y0) * b.W * 3.0);
    HIPCHK(h, launch_pp_band_hist((const uint8_t*)d_img, b.H, b.W, b.prm, b.bgr, y0, y1, scratch(h, SL_PP), st));
    return S2SR_OK;
}

static int pp_band_lut_locked(s2sr_handle* h, hipStream_t st) {
    s2sr_handle::PPBand& b = h->ppb;
    if (!h->scratch.run_open || b.lut) return fail(h, S2SR_E_INVALID, "pp_band_lut: no banded post-process open (none begun, or another call took its scratch area since: begin again), or its LUTs are already built");
    HIPCHK(h, launch_pp_band_lut(b.H, b.W, b.prm, scratch(h, SL_PP), st));
    b.lut = true;
    return S2SR_OK;
}

static int pp_band_rows_locked(s2sr_handle* h, const void* d_img, int y0, int y1, void* d_out, hipStream_t st) {
    s2sr_handle::PPBand& b = h->ppb;
    if (!h->scratch.run_open || !b.lut) return fail(h, S2SR_E_INVALID, "pp_band_rows: no banded post-process open (none begun, or another call took its scratch area since: begin again), or its LUTs are not "
                                                          "built (begin, hist over every row, lut, then rows)");
    if (y0 != b.rows_end || y1 <= y0 || y1 > b.H) return fail(h, S2SR_E_INVALID, "pp_band_rows: bands must follow each other from row 0");
    const int need = y1 + b.radius < b.H ? y1 + b.radius : b.H;     // the blur of row y1-1 reads R rows below it
    Scope sc(h, st, F_POST, 0.0, (double)(y1 - y0) * b.W * 6.0);
    if (need > b.applied_end) {
        HIPCHK(h, launch_pp_band_apply((const uint8_t*)d_img, b.H, b.W, b.prm, b.bgr, b.applied_end, need, scratch(h, SL_PP), st));
        b.applied_end = need;
    }
    HIPCHK(h, launch_pp_band_sharpen(b.H, b.W, b.prm, b.bgr, b.swap_out, y0, y1, scratch(h, SL_PP), (uint8_t*)d_out, st));
    b.rows_end = y1;
    if (y1 == b.H) h->scratch.run_open = false;
    return S2SR_OK;
}

int s2sr_pp_band_begin_dev(s2sr_handle* h, int32_t H, int32_t W, const s2sr_pp_params* prm, int32_t order, void* stream) {
    if (!h || !prm || H <= 0 || W <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, (hipStream_t)stream);
    return door_leave(h, (hipStream_t)stream, pp_band_begin_locked(h, H, W, prm, order, (hipStream_t)stream));
}

int s2sr_pp_band_hist_dev(s2sr_handle* h, const void* d_img, int32_t y0, int32_t y1, void* stream) {
    if (!h || !d_img) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, (hipStream_t)stream);
    return door_leave(h, (hipStream_t)stream, pp_band_hist_locked(h, d_img, y0, y1, (hipStream_t)stream));
}

int s2sr_pp_band_lut_dev(s2sr_handle* h, void* stream) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, (hipStream_t)stream);
    return door_leave(h, (hipStream_t)stream, pp_band_lut_locked(h, (hipStream_t)stream));
}

int s2sr_pp_band_rows_dev(s2sr_handle* h, const void* d_img, int32_t y0, int32_t y1, void* d_out, void* stream) {
    if (!h || !d_img || !d_out) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, (hipStream_t)stream);
    return door_leave(h, (hipStream_t)stream, pp_band_rows_locked(h, d_img, y0, y1, d_out, (hipStream_t)stream));
}

// Host image in, host image out.  ONE lock scope from the upload to the download: the staging buffers
// (SL_SRC, SL_DST) belong to the handle, and the app shares one post-process handle per device between
// all jobs (app/wow_sr.py), which the reference runs from concurrent worker threads (main.py:247-368).
int s2sr_postprocess_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, const s2sr_pp_params* prm, uint8_t* out) {
    if (!h || !rgb || !out || !prm || H <= 0 || W <= 0) return S2SR_E_INVALID;
    const size_t nb = (size_t)H * W * 3;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    int rc = ensure_scratch(h, {{SL_SRC, nb}, {SL_DST, nb}});
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), rgb, nb, hipMemcpyHostToDevice, h->stream));
    if ((rc = postprocess_dev_locked(h, scratch(h, SL_SRC), 1, H, W, prm, scratch(h, SL_DST), h->stream))) return rc;
    HIPCHK(h, hipMemcpyAsync(out, scratch(h, SL_DST), nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

// The image a tile plan is made for.  Scale 2: H x W reflect-padded by one row / column at the bottom / right to even sizes
// (RealESRGANer's mod-2 rule; the pad is read by index, see pack.hip), and an even tile, so that every window of the padded image
// has even origin and extent.
static int plan_dims(s2sr_handle* h, int H, int W, int tile, int* PH, int* PW) {
    *PH = H; *PW = W;
    if (h->unshuffle() == 1) return S2SR_OK;
    if (H < 2 || W < 2) return fail(h, S2SR_E_INVALID, "scale 2 needs an image of at least 2 x 2 (the mod-2 reflect pad)");
    if (tile % 2) return fail(h, S2SR_E_INVALID, "scale 2 needs an even tile: every window of the padded image must have even origin and size");
    *PH = H + (H & 1); *PW = W + (W & 1);
    return S2SR_OK;
}

// The device copy of a masked call's `valid` (SL_VALID) and what the mask kernel needs with it.
struct MaskDev {
    const uint8_t* d_valid = nullptr;         // null: the call is not masked
    int H = 0, W = 0, scale = 0, out_nodata = 0;
    bool u16 = false;
};

// out_nodata over the output pixels of the invalid input pixels, rows [yb, ye) of the quantised image at d_img
static int mask_rows(s2sr_handle* h, hipStream_t st, const MaskDev& m, void* d_img, int yb, int ye) {
    if (!m.d_valid) return S2SR_OK;
    Scope sc(h, st, F_NMASK, 0.0, (double)(ye - yb) / m.scale * m.W);
    if (m.u16) HIPCHK(h, launch_nodata_mask(m.d_valid, m.H, m.W, m.scale, yb, ye, m.out_nodata, (uint16_t*)d_img, st));
    else HIPCHK(h, launch_nodata_mask(m.d_valid, m.H, m.W, m.scale, yb, ye, m.out_nodata, (uint8_t*)d_img, st));
    return S2SR_OK;
}

// `valid` (host) to SL_VALID and the fill of the image at d_img [H, W, 3] (uint8, or uint16), both on st.  The caller has asked for
// SL_VALID (H * W bytes) already: a scratch request may free and synchronise, which belongs in front of a call's first launch.
static int fill_locked(s2sr_handle* h, hipStream_t st, const uint8_t* valid, int H, int W, int radius, bool u16, void* d_img) {
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_VALID), valid, (size_t)H * W, hipMemcpyHostToDevice, st));
    Scope sc(h, st, F_NFILL, 0.0, (double)H * W);
    if (u16) HIPCHK(h, launch_nodata_fill((uint16_t*)d_img, scratch<const uint8_t>(h, SL_VALID), H, W, radius, st));
    else HIPCHK(h, launch_nodata_fill((uint8_t*)d_img, scratch<const uint8_t>(h, SL_VALID), H, W, radius, st));
    return S2SR_OK;
}

// A consistency pass over one quantised image on the device (consistency.hip), in place, in bands of whole block
// rows behind whatever makes the image's rows final (the paste of a whole-image call, the upload of s2sr_consistency_*).  A band
// may end on a row that is no multiple of S, and mode 2 reads the residuals of the block row below: the pass trails.  SL_CONS:
// the inexact counters (uint64[3]) in the first 256 bytes, behind them mode 2's residual plane (int32 [H, W, 3]).
struct ConsRun {
    int mode = 0;                             // 0: no pass
    int H = 0, W = 0, S = 0, lo = 0, hi = 255, swap = 0;
    bool u16 = false;
    const void* d_lr = nullptr;               // the input the net saw [H, W, 3]
    void* d_img = nullptr;                    // the image [S H, S W, 3]
    int e_end = 0, done = 0;                  // block rows whose residuals are taken (mode 2); block rows finished
};
constexpr size_t kConsHead = 256;
static size_t cons_scratch_bytes(int mode, int H, int W) { return kConsHead + (mode == S2SR_CONSISTENCY_SMOOTH ? (size_t)H * W * 3 * sizeof(int32_t) : 0); }

// The image rows the pass can finish once rows [0, final_rows) are final (last: and nothing more comes): the whole block rows
// among them, in mode 2 less the last one, whose lower neighbour's residual does not exist yet.
static int cons_out_end(int mode, int S, int H, int final_rows, bool last) {
    if (last) return H * S;
    const int b = final_rows / S - (mode == S2SR_CONSISTENCY_SMOOTH ? 1 : 0);
    return b > 0 ? b * S : 0;
}

// zeroes the counters; the caller has asked for SL_CONS (cons_scratch_bytes) in front of its first launch
static int cons_begin(s2sr_handle* h, hipStream_t st, ConsRun& r) {
    r.e_end = r.done = 0;
    HIPCHK(h, hipMemsetAsync(scratch(h, SL_CONS), 0, kConsHead, st));
    return S2SR_OK;
}

// rows [0, final_rows) of the image are final: the pass up to row out_end (cons_out_end of them)
static int cons_advance(s2sr_handle* h, hipStream_t st, ConsRun& r, int final_rows, int out_end) {
    const int fb = final_rows / r.S, target = out_end / r.S;
    unsigned long long* cnt = scratch<unsigned long long>(h, SL_CONS);
    int32_t* d_e = (int32_t*)(scratch<char>(h, SL_CONS) + kConsHead);
    auto launch = [&](int form, int b0, int b1) -> int {
        const double img_b = (double)(b1 - b0) * r.S * r.S * r.W * 3.0 * (r.u16 ? 2 : 1);
        Scope sc(h, st, F_CONS, 0.0, form == 0 ? img_b : 2.0 * img_b);
        if (r.u16) HIPCHK(h, launch_consistency(form, (uint16_t*)r.d_img, (const uint16_t*)r.d_lr, d_e, cnt, r.H, r.W, r.S, b0, b1, r.lo, r.hi, st));
        else HIPCHK(h, launch_consistency(form, (uint8_t*)r.d_img, (const uint8_t*)r.d_lr, d_e, cnt, r.H, r.W, r.S, b0, b1, r.swap, st));
        return S2SR_OK;
    };
    int rc;
    if (r.mode == S2SR_CONSISTENCY_SMOOTH && fb > r.e_end) {
        if ((rc = launch(0, r.e_end, fb))) return rc;
        r.e_end = fb;
    }
    if (target > r.done) {
        if (r.mode == S2SR_CONSISTENCY_SMOOTH && r.e_end < (target + 1 < r.H ? target + 1 : r.H))
            return fail(h, S2SR_E_INVALID, "consistency: a band ran ahead of its residuals");
        if ((rc = launch(r.mode, r.done, target))) return rc;
        r.done = target;
    }
    return S2SR_OK;
}

// the counters to the host, behind everything on st; returns when they are there
static int cons_counts(s2sr_handle* h, hipStream_t st, uint64_t* inexact) {
    unsigned long long n[3];
    HIPCHK(h, hipMemcpyAsync(n, scratch(h, SL_CONS), sizeof n, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (inexact) for (int c = 0; c < 3; ++c) inexact[c] = n[c];
    return S2SR_OK;
}

static const char* kConsMode = "consistency: mode must be 1 (S2SR_CONSISTENCY_EXACT) or 2 (S2SR_CONSISTENCY_SMOOTH)";
static const char* mask_error(const uint8_t* valid, int radius, int out_nodata, bool u16) {
    if (!valid) return "nodata: a mask (valid, uint8 [H, W]) is required";
    if (radius < 1 || radius > 64) return "nodata: the fill radius must be 1..64";
    if (out_nodata < 0 || out_nodata > (u16 ? 65535 : 255)) return u16 ? "nodata: out_nodata must be 0..65535" : "nodata: out_nodata must be 0..255";
    return nullptr;
}

// The finish of a banded post-process whose histograms hold every row (pp_band_hist_locked over each stitched band): the LUTs, then
// the image in nfin row bands of fin_rows rows, each followed by its copy out.  group_done[nchunks .. nchunks + nfin) are free for
// the bands; group_done[nchunks - 1] marks the last chunk.
// mk: a masked call's mask, written over each band behind its last kernel (the apply pass, R rows ahead, has read those rows).
static int pp_finish_bands(s2sr_handle* h, hipStream_t st, uint8_t* d_img_out, uint8_t* out_u8, int OH, size_t row_b, int fin_rows, int nfin,
                           int nchunks, const MaskDev& mk) {
    int rc;
    // LUTs, then every finishing band's kernels (in place: a band's rows are rewritten only after the apply pass, which
    // runs R rows ahead, has read them), an event behind each; the copies follow band by band on the copy stream
    const bool timing = getenv("S2SR_JOB_TIMING") != nullptr;     // diagnostic: stage times of the finish on stderr
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_enq = now(), t_compute = 0, t_first = 0;
    if ((rc = pp_band_lut_locked(h, st))) return rc;
    for (int b = 0; b < nfin; ++b) {
        const int y0 = b * fin_rows, y1 = y0 + fin_rows < OH ? y0 + fin_rows : OH;
        if ((rc = pp_band_rows_locked(h, d_img_out, y0, y1, d_img_out, st))) return rc;
        if ((rc = mask_rows(h, st, mk, d_img_out, y0, y1))) return rc;
        HIPCHK(h, ev_record(h, h->group_done[nchunks + b], st, SITE_PP_BAND_D2H));
    }
    if (timing) {
        HIPCHK(h, ev_host_wait(h, h->group_done[nchunks - 1], SITE_CHUNK_BAND_D2H));
        t_compute = now();
    }
    for (int b = 0; b < nfin; ++b) {
        const int y0 = b * fin_rows, y1 = y0 + fin_rows < OH ? y0 + fin_rows : OH;
        HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->group_done[nchunks + b], SITE_PP_BAND_D2H));
        if ((rc = d2h_staged(h, out_u8 + (size_t)y0 * row_b, d_img_out + (size_t)y0 * row_b, (size_t)(y1 - y0) * row_b,
                             false))) return rc;
        if (timing && b == 0) t_first = now();
    }
    if (timing)
        fprintf(stderr, "[s2sr job] finish: %d bands of %d rows; last chunk done %.2f ms after the finish was queued, first band on the host "
                "+%.2f ms, all bands +%.2f ms\n", nfin, fin_rows, t_compute - t_enq, t_first - t_compute, now() - t_compute);
    return S2SR_OK;
}

// What a whole-image call asks for is one s2sr_enhance_args (include/s2sr.h: the fields and what each means), read by everything from
// here to enhance_door.  check_call is the single statement of which records exist: every refusal before the device is touched.
// required: the door's words for a call without image, sizes or output (none: the bare code).
static int check_call(s2sr_handle* h, const s2sr_enhance_args& c, const char* required) {
    if (c.size != sizeof(s2sr_enhance_args)) return fail(h, S2SR_E_INVALID, "s2sr_enhance_args: size must be sizeof(s2sr_enhance_args)");
    if (c.bits != 8 && c.bits != 16) return fail(h, S2SR_E_INVALID, "s2sr_enhance_args: bits must be 8 or 16");
    const bool in16 = c.bits == 16;
    if (!c.img || (!c.out && !c.out_f32) || c.H <= 0 || c.W <= 0 || c.tile <= 0 || c.pad < 0)
        return required ? fail(h, S2SR_E_INVALID, required) : S2SR_E_INVALID;
    if (in16 && (c.prm || c.swap_rb)) return fail(h, S2SR_E_INVALID, "s2sr_enhance_args: prm and swap_rb belong to 8-bit images (bits 16 has no post-process)");
    if (c.force_tiled && (in16 || c.out || c.prm || c.swap_rb || c.blend || c.mask || c.consistency))
        return fail(h, S2SR_E_INVALID, "s2sr_enhance_args: force_tiled is s2sr_tile_process_f32: an 8-bit image, out_f32 alone, every option off");
    if (!in16 && c.out && c.out_f32 && !c.blend) return fail(h, S2SR_E_INVALID, "s2sr_enhance_args: an 8-bit call for out and out_f32 together needs blend");
    if (!in16 && c.out_f32 && (c.prm || c.swap_rb))
        return fail(h, S2SR_E_INVALID, "s2sr_enhance_blend_u8: the float image is the net's own output: not with a post-process or swap_rb");
    if (c.mask) {
        if (const char* why = mask_error(c.mask->valid, c.mask->radius, c.mask->out_nodata, in16)) return fail(h, S2SR_E_INVALID, why);
        if (c.out_f32) return fail(h, S2SR_E_INVALID, "nodata: the float image is the net's own output and is never masked");
    }
    if (c.consistency) {
        if (c.consistency != S2SR_CONSISTENCY_EXACT && c.consistency != S2SR_CONSISTENCY_SMOOTH) return fail(h, S2SR_E_INVALID, kConsMode);
        if (c.out_f32) return fail(h, S2SR_E_INVALID, "consistency: the float image is the net's own output and is never corrected");
    }
    if (in16)
        if (int rc = check_u16(h, c.lo, c.hi)) return rc;
    if (c.prm)                                               // before the net runs, not behind it
        if (const char* why = pp_params_error(*c.prm)) return fail(h, S2SR_E_INVALID, why);
    return S2SR_OK;
}

// Everything about a call that is host arithmetic (the one HIP call in here is plan_chunk_rows' CU count).  Scale 2, odd H or W:
// the job runs on the padded PH x PW image and the paste crops to the output.
struct EnhancePlan {
    int PH = 0, PW = 0;
    bool tiled = false;                       // RealESRGAN.enhance's whole / tiled switch
    bool blend = false;                       // the seam-blended paste: asked for, tiled, and a ramp exists
    WindowJob job;
    std::vector<int32_t> rows, cols;          // blend: the tables (blend_plan.h), 6 ints per output row / column of the padded image, as the kernel reads them
    Mosaic mo;                                // ONE plan for the job: every chunk runs in its workspace geometry
    std::vector<int> chunk_r0, band_end;      // the chunks of window rows (plan_chunk_rows) and the band of output rows each makes final (plan_bands)
    int max_rows = 0;                         // window rows of the largest chunk
};

static int plan_enhance(s2sr_handle* h, const s2sr_enhance_args& c, EnhancePlan& p) {
    int rc;
    if ((rc = plan_dims(h, c.H, c.W, c.tile, &p.PH, &p.PW))) return rc;
    const int scale = h->cfg.scale;
    p.tiled = c.force_tiled || (long long)p.PH * p.PW > (long long)c.tile * c.tile * 4;   // strict '>' (:226)
    WindowJob& job = p.job;
    if ((rc = plan_window_job(p.PH, p.PW, c.tile, c.pad, scale, p.tiled, job))) return fail(h, rc, kBadPlan);
    if (c.blend && p.tiled) {
        p.rows.resize((size_t)kBlendStride * p.PH * scale); p.cols.resize((size_t)kBlendStride * p.PW * scale);
        const char* why = blend_plan_axis(job.rm.data(), (int64_t)p.PH * scale, job.ny, job.wh * scale, c.pad * scale, p.rows.data());
        if (!why) why = blend_plan_axis(job.cm.data(), (int64_t)p.PW * scale, job.nx, job.ww * scale, c.pad * scale, p.cols.data());
        if (why) return fail(h, S2SR_E_INVALID, why);
        for (size_t i = 4; i < p.rows.size() && !p.blend; i += kBlendStride) p.blend = p.rows[i] != 0;
        for (size_t i = 4; i < p.cols.size() && !p.blend; i += kBlendStride) p.blend = p.cols[i] != 0;
    }
    if (p.tiled) p.mo = pick_mosaic(h, job.nx * job.ny, job.wh, job.ww);
    // one chunk for the untiled image, and with out_f32: the fp32 image is pasted from all the tiles at the end
    p.chunk_r0 = p.tiled && !c.out_f32 ? plan_chunk_rows(h, job, p.mo) : std::vector<int>{0, job.ny};
    const int nchunks = (int)p.chunk_r0.size() - 1;
    // a row is final once the last window row it reads is done: the window row that owns it (the paste map), or the later of a ramp's two
    p.band_end.resize(nchunks);
    plan_bands(p.chunk_r0.data(), nchunks, job.ny, c.H * scale, p.blend ? p.rows.data() + 2 : job.rm.data(), p.blend ? kBlendStride : 2, p.band_end.data());
    for (int k = 0; k < nchunks; ++k) {
        const int r0 = p.chunk_r0[k], r1 = p.chunk_r0[k + 1];
        if (r1 - r0 > p.max_rows) p.max_rows = r1 - r0;
        // blend: every row reads window rows its chunk's buffer holds (its own, and the one carried in front)
        if (p.blend)
            if (const char* why = blend_check_band(p.rows.data(), k ? p.band_end[k - 1] : 0, p.band_end[k], r0 - (k > 0), r1)) return fail(h, S2SR_E_INVALID, why);
    }
    if (p.blend) { blend_device_axis(p.rows.data(), (int64_t)p.PH * scale); blend_device_axis(p.cols.data(), (int64_t)p.PW * scale); }
    return S2SR_OK;
}

// RealESRGAN.enhance (cnn_super_resolution.py:217-234) incl. _tile_process (:236-280), behind every door; the caller holds h->mu.
// Upload, gather the windows (SL_SRC -> SL_MID), the chunk loop -- forward a chunk of window rows, paste the band of output rows it
// made final into the image (SL_DST), copy the band out under the next chunk -- and the tail.  Only the paste varies:
//   overwrite (8-bit in): the net writes u8 (or NCHW fp32) tiles of the WHOLE image into SL_CHUNK, each chunk at its own offset, and
//     launch_stitch pastes.  The untiled image is one window: the net writes it straight into SL_DST, or (fp32, or the padded
//     image of an odd scale-2 one) into SL_MID and an identity map crops it.  A job's R / B exchange follows each band;
//   quantise (16-bit in): every chunk's windows leave the net as fp32 tiles into ONE chunk-sized buffer (SL_CHUNK; the same
//     pointers for every chunk, so the chunks' graphs hit) and launch_stitch_quant_u16 pastes and quantises from it;
//   blend: as quantise, for both inputs, and launch_stitch_blend cross-fades inside the ramps.  A row ramp reads the last window
//     row of one chunk and the first of the next, so the buffer has one window row in front of the chunk's, filled from the chunk
//     before by one device-to-device copy.
// A post-process is image-global through CLAHE's grid (wow_sr.py:191-192): in bands it counts every band into the histograms as it
// is pasted (under the compute of the chunks still to come), builds the LUTs behind the last band and finishes the image in row
// bands, each followed by its copy out; a single chunk of the overwrite paste runs it on the whole image instead.
// The fp32 image (one chunk) is pasted from the chunk's tiles behind the loop, and both images leave behind that.
// A consistency pass sits between the paste and everything else: it trails the paste by whole block rows, and the
// exchange back, the histograms, the mask and the copies follow its bands instead of the paste's (ConsRun, cons_out_end).
static int enhance_locked(s2sr_handle* h, const s2sr_enhance_args& c) {
    EnhancePlan p;
    int rc = plan_enhance(h, c, p);
    if (rc) return rc;
    const bool in16 = c.bits == 16, over = !p.blend && !in16;
    if (over && c.out && c.out_f32) {   // a blend call left whole or without a ramp: u8 and fp32 tiles are two forwards of the net
        s2sr_enhance_args f = c, q = c;
        f.blend = q.blend = 0; f.out = nullptr; q.out_f32 = nullptr;
        return (rc = enhance_locked(h, f)) ? rc : enhance_locked(h, q);
    }
    hipStream_t st = h->stream;
    const WindowJob& job = p.job;
    const int H = c.H, W = c.W, scale = h->cfg.scale, OH = H * scale, OW = W * scale, esz = in16 ? 2 : 1;
    const int nx = job.nx, ny = job.ny, wh = job.wh, ww = job.ww, oth = wh * scale, otw = ww * scale;
    const int nchunks = (int)p.chunk_r0.size() - 1, carry = p.blend && nchunks > 1 ? 1 : 0;
    const bool reflect = p.PH != H || p.PW != W;
    const bool direct = over && !p.tiled && !c.out_f32 && !reflect;     // the net writes the image itself: no tiles, no tables, no paste
    const bool banded = c.prm && (p.blend || nchunks > 1);              // the post-process runs in bands (else, if any, on the whole image)
    const size_t ipx = (size_t)H * W * 3, opx = (size_t)OH * OW * 3;
    const size_t win_in = (size_t)wh * ww * 3, win_out = win_in * scale * scale;      // samples per window, in and out
    const size_t row_b = (size_t)OW * 3 * esz;                                         // bytes of one output row
    // ---- staging.  SL_DST: the quantised image, then the fp32 image (the overwrite paste makes one of them per call)
    const size_t f_off = over ? 0 : up256(opx * esz);
    const Slot tslot = over && !p.tiled ? SL_MID : SL_CHUNK;
    const size_t tile_b = over ? (size_t)nx * ny * win_out * (c.out_f32 ? 4 : 1) : (size_t)(p.max_rows + carry) * nx * win_out * sizeof(float);
    if ((rc = ensure_scratch(h, {{SL_SRC, ipx * esz}, {SL_DST, c.out_f32 ? f_off + opx * 4 : over ? opx : f_off},
                                 {SL_MID, (size_t)nx * ny * win_in * esz, p.tiled}, {tslot, tile_b, !direct}, {SL_VALID, (size_t)H * W, c.mask != nullptr},
                                 {SL_CONS, cons_scratch_bytes(c.consistency, H, W), c.consistency != 0}}))) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), c.img, ipx * esz, hipMemcpyHostToDevice, st));
    MaskDev mk;                                        // masked: the fill in front of everything that reads the image, the mask at each exit of a quantised band
    if (c.mask) {
        if ((rc = fill_locked(h, st, c.mask->valid, H, W, c.mask->radius, in16, scratch(h, SL_SRC)))) return rc;
        mk.d_valid = scratch<const uint8_t>(h, SL_VALID); mk.H = H; mk.W = W; mk.scale = scale; mk.out_nodata = c.mask->out_nodata; mk.u16 = in16;
    }
    if (c.swap_rb) HIPCHK(h, launch_swap_rb_u8(scratch<const uint8_t>(h, SL_SRC), (size_t)H * W, scratch<uint8_t>(h, SL_SRC), st));
    int32_t* d_tab[3] = {nullptr, nullptr, nullptr};   // rectangles, row table, column table
    if (!direct && (rc = upload_tables(h, st, job.rects, p.blend ? p.rows : job.rm, p.blend ? p.cols : job.cm, d_tab))) return rc;
    if (p.tiled) {
        if (in16) HIPCHK(h, launch_gather_windows(scratch<const uint16_t>(h, SL_SRC), H, W, d_tab[0], nx * ny, wh, ww, scratch<uint16_t>(h, SL_MID), st));
        else HIPCHK(h, launch_gather_windows(scratch<const uint8_t>(h, SL_SRC), H, W, d_tab[0], nx * ny, wh, ww, reflect, scratch<uint8_t>(h, SL_MID), st));
    }
    const char* d_win = scratch<const char>(h, p.tiled ? SL_MID : SL_SRC);
    uint8_t* d_q = scratch<uint8_t>(h, SL_DST);
    float* d_f = (float*)(d_q + f_off);
    void* d_buf = direct ? (void*)d_q : scratch(h, tslot);      // blend: [carry window row | the chunk's window rows]
    float* d_tiles = (float*)d_buf + (size_t)carry * nx * win_out;
    int fin_rows = 0, nfin = 0;          // finishing bands of the post-process: ~48 MB each, whole 32-row tile rows
    if (banded) {
        fin_rows = (int)(((size_t)48 << 20) / row_b) & ~31;
        if (fin_rows < 64) fin_rows = 64;
        nfin = (OH + fin_rows - 1) / fin_rows;
        if ((rc = pp_band_begin_locked(h, OH, OW, c.prm, c.swap_rb ? 3 : 0, st))) return rc;
    }
    // this call's run took SL_PP from whatever run a caller had open there: it ends with the call on every way out, so that
    // caller's next hist / lut / rows is refused
    struct CloseRun { s2sr_handle* h; ~CloseRun() { if (h) h->scratch.run_open = false; } } close_run{banded ? h : nullptr};
    if ((rc = ensure_group_events(h, nchunks + nfin + 1))) return rc;
    // consistency: the pass trails the paste (whole block rows; mode 2 one more), and everything behind the paste follows the pass's
    // bands -- the R / B exchange back, the histograms of a banded post-process, the mask, the copy out.  SL_SRC holds the image
    // the net saw (filled, exchanged) for the whole call.  The 8-bit blend paste of a job without post-process has exchanged R and
    // B already: image channel c is then input channel 2 - c.
    ConsRun cr;
    std::vector<int> out_end = p.band_end;
    if (c.consistency) {
        cr.mode = c.consistency; cr.H = H; cr.W = W; cr.S = scale; cr.u16 = in16;
        if (in16) { cr.lo = c.lo; cr.hi = c.hi; }
        cr.swap = !over && !in16 && c.swap_rb && !c.prm;
        cr.d_lr = scratch(h, SL_SRC); cr.d_img = d_q;
        for (int k = 0; k < nchunks; ++k) out_end[k] = cons_out_end(cr.mode, scale, H, p.band_end[k], k == nchunks - 1);
        if ((rc = cons_begin(h, st, cr))) return rc;
    }
    // ---- the chunk loop
    int prev_n = 0;                                              // windows of the chunk before
    auto forward = [&](int t0, int n) -> int {
        if (carry && t0 > 0)   // the last window row of the chunk before, to the front of the buffer (its band is pasted: same stream)
            HIPCHK(h, hipMemcpyAsync(d_buf, d_tiles + (size_t)(prev_n - nx) * win_out, (size_t)nx * win_out * sizeof(float), hipMemcpyDeviceToDevice, st));
        prev_n = n;
        const TileIn in = in16 ? TileIn::u16((const uint16_t*)d_win + (size_t)t0 * win_in, c.lo, c.hi)
                               : TileIn::u8((const uint8_t*)d_win + (size_t)t0 * win_in, p.tiled ? wh : H, p.tiled ? ww : W);
        TileOut out;
        if (!over) out.f32 = d_tiles;
        else if (c.out_f32) out.f32 = (float*)d_buf + (size_t)t0 * win_out;
        else out.u8 = (uint8_t*)d_buf + (size_t)t0 * win_out;
        return forward_dev(h, st, in, n, wh, ww, out, p.mo.on() ? &p.mo : nullptr);
    };
    // rows [pyb, pye) into the quantised image, and what follows the paste on rows [yb, ye) (the same rows, unless a consistency pass
    // trails); t0: the chunk's first window (the one-chunk buffers start at window t0 - carry * nx)
    auto finish = [&](int t0, int pyb, int pye, int yb, int ye) -> int {
        if (!c.out) return S2SR_OK;
        uint8_t* dst = d_q + (size_t)pyb * row_b;
        if (pye <= pyb) {                                        // (nothing new is final: only the trailing pass moves)
        } else if (over) {
            if (!direct) HIPCHK(h, launch_stitch((const uint8_t*)d_buf, nx, oth, otw, d_tab[1] + 2 * pyb, d_tab[2], pye - pyb, OW, dst, st));
        } else {
            Scope sc(h, st, F_MISC, 0.0, (double)(pye - pyb) * OW * 3.0 * (4.0 + esz));
            const int32_t* r = d_tab[1] + (size_t)kBlendStride * pyb;
            if (!p.blend) HIPCHK(h, launch_stitch_quant_u16(d_tiles, nx, t0, oth, otw, d_tab[1] + 2 * pyb, d_tab[2], pye - pyb, OW, c.lo, c.hi, (uint16_t*)dst, st));
            else if (in16) HIPCHK(h, launch_stitch_blend((const float*)d_buf, nx, t0 - carry * nx, oth, otw, r, d_tab[2], pye - pyb, OW, c.lo, c.hi, (uint16_t*)dst, st));
            else HIPCHK(h, launch_stitch_blend((const float*)d_buf, nx, t0 - carry * nx, oth, otw, r, d_tab[2], pye - pyb, OW, c.swap_rb && !c.prm, dst, st));
        }
        if (cr.mode && (rc = cons_advance(h, st, cr, pye, ye))) return rc;
        if (ye <= yb) return S2SR_OK;
        if (over && c.swap_rb && !banded) {                      // (a banded post-process exchanges R and B itself)
            uint8_t* band = d_q + (size_t)yb * row_b;
            HIPCHK(h, launch_swap_rb_u8(band, (size_t)(ye - yb) * OW, band, st));
        }
        if (banded) return pp_band_hist_locked(h, d_q, yb, ye, st);
        return c.prm ? S2SR_OK : mask_rows(h, st, mk, d_q, yb, ye);       // (a post-process reads the filled image: its exits mask)
    };
    // with a post-process or the fp32 image no band is copied here: they leave through the tail below
    if ((rc = run_chunks(h, st, nx, p.chunk_r0, p.band_end, out_end, forward, finish, (uint8_t*)c.out, d_q, row_b, c.out && !c.prm && !c.out_f32))) return rc;
    // ---- the tail
    hipEvent_t tail_done = h->group_done[nchunks + nfin];
    if (banded && (rc = pp_finish_bands(h, st, d_q, (uint8_t*)c.out, OH, row_b, fin_rows, nfin, nchunks, mk))) return rc;
    if (c.prm && !banded) {
        // the windows' output buffer is free again once the stitch has read it; the untiled image gets a buffer of its own
        if ((rc = ensure_scratch(h, SL_CHUNK, opx))) return rc;
        if ((rc = postprocess_dev_locked(h, d_q, 1, OH, OW, c.prm, scratch(h, SL_CHUNK), st))) return rc;
        if ((rc = mask_rows(h, st, mk, scratch(h, SL_CHUNK), 0, OH))) return rc;
        HIPCHK(h, ev_record(h, tail_done, st, SITE_TAIL_D2H));
        HIPCHK(h, ev_stream_wait(h, h->copy_stream, tail_done, SITE_TAIL_D2H));
        if ((rc = d2h_staged(h, (uint8_t*)c.out, scratch<const uint8_t>(h, SL_CHUNK), opx, true))) return rc;
    }
    if (c.out_f32) {
        if (p.blend) HIPCHK(h, launch_stitch_blend((const float*)d_buf, nx, 0, oth, otw, d_tab[1], d_tab[2], OH, OW, d_f, st));
        else HIPCHK(h, launch_stitch((const float*)d_buf, nx, oth, otw, d_tab[1], d_tab[2], OH, OW, d_f, st));
        HIPCHK(h, ev_record(h, tail_done, st, SITE_TAIL_D2H));
        if (c.out) {
            HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->group_done[nchunks - 1], SITE_CHUNK_BAND_D2H));
            if ((rc = d2h_staged(h, (uint8_t*)c.out, d_q, OH * row_b, true))) return rc;
        }
        HIPCHK(h, ev_stream_wait(h, h->copy_stream, tail_done, SITE_TAIL_D2H));
        if ((rc = d2h_staged(h, (uint8_t*)c.out_f32, (const uint8_t*)d_f, opx * 4, true))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    HIPCHK(h, hipStreamSynchronize(st));
    if (cr.mode && (rc = cons_counts(h, st, c.inexact))) return rc;
    if (cr.mode && c.inexact && c.swap_rb && !cr.swap) {       // the pass saw B, G, R: the counts go by the channels of the call's images
        const uint64_t b = c.inexact[0];
        c.inexact[0] = c.inexact[2]; c.inexact[2] = b;
    }
    if (in16 && c.out) h->scratch.keep(KEPT_U16, SL_DST, OH, OW);                // the x4 image also stays on the device, for s2sr_display_*_u16
    return S2SR_OK;
}

// ONE lock scope per call, from the checks to the last synchronise (as s2sr_postprocess_u8): the scratch areas belong to the handle
static int enhance_call(s2sr_handle* h, const s2sr_enhance_args* a, const char* required) {
    if (!h || !a) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_call(h, *a, required)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    return enhance_locked(h, *a);
}

// The entry behind s2sr_enhance and every form of it: one recovery around the one lock scope.
static int enhance_door(s2sr_handle* h, const s2sr_enhance_args* a, const char* required) {
    RUN_WITH_STREAM_RECOVERY(h, enhance_call(h, a, required));
}

int s2sr_enhance(s2sr_handle* h, const s2sr_enhance_args* a) {
    return enhance_door(h, a, "s2sr_enhance: an image, positive sizes and at least one output are required");
}

// ---- the forms (include/s2sr.h: the table under s2sr_enhance).  Each builds the record its signature spells and enters enhance_door
// with its own words; what only a signature can get wrong (no image for a blend, no mask, mode 0) it refuses itself.
static s2sr_enhance_args form(int bits, const void* img, int H, int W, int tile, int pad, void* out, float* out_f32) {
    s2sr_enhance_args a = {};
    a.size = sizeof a; a.bits = bits; a.img = img; a.H = H; a.W = W; a.tile = tile; a.pad = pad; a.out = out; a.out_f32 = out_f32;
    return a;
}
static int form_refusal(s2sr_handle* h, const char* why) { return h ? fail(h, S2SR_E_INVALID, why) : S2SR_E_INVALID; }

int s2sr_enhance_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, uint8_t* out) {
    const s2sr_enhance_args a = form(8, img, H, W, tile, pad, out, nullptr);
    return enhance_door(h, &a, nullptr);
}

int s2sr_enhance_job_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, int32_t tile, int32_t pad, const s2sr_pp_params* prm,
                        uint8_t* out_rgb) {
    s2sr_enhance_args a = form(8, rgb, H, W, tile, pad, out_rgb, nullptr);
    a.swap_rb = 1; a.prm = prm;
    return enhance_door(h, &a, nullptr);
}

int s2sr_enhance_f32(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, float* out) {
    const s2sr_enhance_args a = form(8, img, H, W, tile, pad, nullptr, out);
    return enhance_door(h, &a, nullptr);
}

int s2sr_tile_process_f32(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, float* out) {
    s2sr_enhance_args a = form(8, img, H, W, tile, pad, nullptr, out);
    a.force_tiled = 1;
    return enhance_door(h, &a, nullptr);
}

int s2sr_enhance_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo, int32_t hi,
                     uint16_t* out_u16, float* out_f32) {
    s2sr_enhance_args a = form(16, img, H, W, tile, pad, out_u16, out_f32);
    a.lo = lo; a.hi = hi;
    return enhance_door(h, &a, "s2sr_enhance_u16: an image, positive sizes and at least one output are required");
}

int s2sr_enhance_blend_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, const s2sr_pp_params* prm,
                          int32_t swap_rb, uint8_t* out_u8, float* out_f32) {
    s2sr_enhance_args a = form(8, img, H, W, tile, pad, out_u8, out_f32);
    a.blend = 1; a.prm = prm; a.swap_rb = swap_rb;
    if (!img) return form_refusal(h, "s2sr_enhance_blend_u8: an image is required");
    return enhance_door(h, &a, "s2sr_enhance_blend: an image, positive sizes and at least one output are required");
}

int s2sr_enhance_blend_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo, int32_t hi,
                           uint16_t* out_u16, float* out_f32) {
    s2sr_enhance_args a = form(16, img, H, W, tile, pad, out_u16, out_f32);
    a.lo = lo; a.hi = hi; a.blend = 1;
    if (!img) return form_refusal(h, "s2sr_enhance_blend_u16: an image is required");
    return enhance_door(h, &a, "s2sr_enhance_blend: an image, positive sizes and at least one output are required");
}

int s2sr_enhance_masked_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, const s2sr_pp_params* prm,
                           int32_t swap_rb, int32_t blend, const s2sr_mask* m, uint8_t* out_u8) {
    s2sr_enhance_args a = form(8, img, H, W, tile, pad, out_u8, nullptr);
    a.prm = prm; a.swap_rb = swap_rb; a.blend = blend; a.mask = m;
    if (!m) return form_refusal(h, "s2sr_enhance_masked_u8: a mask is required (m == NULL)");
    return enhance_door(h, &a, "s2sr_enhance_masked_u8: an image, positive sizes and out_u8 are required");
}

int s2sr_enhance_masked_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo, int32_t hi,
                            int32_t blend, const s2sr_mask* m, uint16_t* out_u16) {
    s2sr_enhance_args a = form(16, img, H, W, tile, pad, out_u16, nullptr);
    a.lo = lo; a.hi = hi; a.blend = blend; a.mask = m;
    if (!m) return form_refusal(h, "s2sr_enhance_masked_u16: a mask is required (m == NULL)");
    return enhance_door(h, &a, "s2sr_enhance_masked_u16: an image, positive sizes and out_u16 are required");
}

int s2sr_enhance_consistent_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, const s2sr_pp_params* prm,
                               int32_t swap_rb, int32_t blend, const s2sr_mask* m, int32_t mode, uint8_t* out_u8, uint64_t* inexact) {
    s2sr_enhance_args a = form(8, img, H, W, tile, pad, out_u8, nullptr);
    a.prm = prm; a.swap_rb = swap_rb; a.blend = blend; a.mask = m; a.consistency = mode; a.inexact = inexact;
    if (mode != S2SR_CONSISTENCY_EXACT && mode != S2SR_CONSISTENCY_SMOOTH) return form_refusal(h, kConsMode);   // (0 is "off" in the record)
    return enhance_door(h, &a, "s2sr_enhance_consistent_u8: an image, positive sizes and out_u8 are required");
}

int s2sr_enhance_consistent_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo, int32_t hi,
                                int32_t blend, const s2sr_mask* m, int32_t mode, uint16_t* out_u16, uint64_t* inexact) {
    s2sr_enhance_args a = form(16, img, H, W, tile, pad, out_u16, nullptr);
    a.lo = lo; a.hi = hi; a.blend = blend; a.mask = m; a.consistency = mode; a.inexact = inexact;
    if (mode != S2SR_CONSISTENCY_EXACT && mode != S2SR_CONSISTENCY_SMOOTH) return form_refusal(h, kConsMode);
    return enhance_door(h, &a, "s2sr_enhance_consistent_u16: an image, positive sizes and out_u16 are required");
}

// The pass alone: host images in, host image out (out may be sr).  No weights needed.  ONE lock scope, as s2sr_postprocess_u8.
// The image goes up, through the pass and out again in bands of band_rows output rows on one stream: a band's rows are final once
// it is uploaded, the pass trails as it does behind a paste (cons_out_end), and what it has finished leaves.
static int consistency_impl(s2sr_handle* h, const void* sr, const void* img, int H, int W, int S, int lo, int hi, int mode, int band_rows,
                            bool u16, void* out, uint64_t* inexact) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!sr || !img || !out || H <= 0 || W <= 0) return fail(h, S2SR_E_INVALID, "s2sr_consistency: the two images, positive sizes and an output are required");
    if (S != 2 && S != 4) return fail(h, S2SR_E_INVALID, "s2sr_consistency: S must be 2 or 4");
    if (mode != S2SR_CONSISTENCY_EXACT && mode != S2SR_CONSISTENCY_SMOOTH) return fail(h, S2SR_E_INVALID, kConsMode);
    if (band_rows < 0) return fail(h, S2SR_E_INVALID, "s2sr_consistency: band_rows must be >= 0");
    if (u16 && !(0 <= lo && lo < hi && hi <= 65535)) return fail(h, S2SR_E_INVALID, "s2sr_consistency_u16: need 0 <= lo < hi <= 65535");
    if ((long long)H * S > 0x3fffffffLL || (long long)W * S * 3 > 0x3fffffffLL) return fail(h, S2SR_E_INVALID, "s2sr_consistency: the image is too large");
    const int esz = u16 ? 2 : 1, OH = H * S;
    const size_t row_b = (size_t)W * S * 3 * esz, ipx = (size_t)H * W * 3;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    hipStream_t st = h->stream;
    int rc = ensure_scratch(h, {{SL_SRC, ipx * esz}, {SL_DST, row_b * OH}, {SL_CONS, cons_scratch_bytes(mode, H, W)}});
    if (rc) return rc;
    const size_t rows = band_of(band_rows, OH, row_b, (size_t)32 << 20);               // the library's choice: ~32 MB
    ConsRun cr;
    cr.mode = mode; cr.H = H; cr.W = W; cr.S = S; cr.u16 = u16;
    if (u16) { cr.lo = lo; cr.hi = hi; }
    cr.d_lr = scratch(h, SL_SRC); cr.d_img = scratch(h, SL_DST);
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), img, ipx * esz, hipMemcpyHostToDevice, st));
    if ((rc = cons_begin(h, st, cr))) return rc;
    uint8_t* d_img = scratch<uint8_t>(h, SL_DST);
    int left = 0;                                                                       // rows that have left
    for (const RowBand b : row_bands(OH, rows)) {
        const int y1 = (int)b.y1;
        HIPCHK(h, hipMemcpyAsync(d_img + b.y0 * row_b, (const uint8_t*)sr + b.y0 * row_b, b.rows() * row_b, hipMemcpyHostToDevice, st));
        const int oe = cons_out_end(mode, S, H, y1, b.last);
        if ((rc = cons_advance(h, st, cr, y1, oe))) return rc;
        if (oe > left) HIPCHK(h, hipMemcpyAsync((uint8_t*)out + (size_t)left * row_b, d_img + (size_t)left * row_b, (size_t)(oe - left) * row_b, hipMemcpyDeviceToHost, st));
        if (oe > left) left = oe;
    }
    return cons_counts(h, st, inexact);
}

int s2sr_consistency_u8(s2sr_handle* h, const uint8_t* sr, const uint8_t* img, int32_t H, int32_t W, int32_t S, int32_t mode, int32_t band_rows,
                        uint8_t* out, uint64_t* inexact) {
    RUN_WITH_STREAM_RECOVERY(h, consistency_impl(h, sr, img, H, W, S, 0, 255, mode, band_rows, false, out, inexact));
}

int s2sr_consistency_u16(s2sr_handle* h, const uint16_t* sr, const uint16_t* img, int32_t H, int32_t W, int32_t S, int32_t lo, int32_t hi,
                         int32_t mode, int32_t band_rows, uint16_t* out, uint64_t* inexact) {
    RUN_WITH_STREAM_RECOVERY(h, consistency_impl(h, sr, img, H, W, S, lo, hi, mode, band_rows, true, out, inexact));
}

// The fill alone: host image and mask in, filled host image out.  No weights needed.  ONE lock scope, as s2sr_postprocess_u8.
static int fill_nodata_impl(s2sr_handle* h, const void* img, const uint8_t* valid, int H, int W, int radius, bool u16, void* out) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!img || !out || H <= 0 || W <= 0) return fail(h, S2SR_E_INVALID, "s2sr_fill_nodata: an image, positive sizes and an output are required");
    if (const char* why = mask_error(valid, radius, 0, u16)) return fail(h, S2SR_E_INVALID, why);
    const size_t nb = (size_t)H * W * 3 * (u16 ? 2 : 1);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, h->stream);
    int rc = ensure_scratch(h, {{SL_SRC, nb}, {SL_VALID, (size_t)H * W}});
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(scratch(h, SL_SRC), img, nb, hipMemcpyHostToDevice, h->stream));
    if ((rc = fill_locked(h, h->stream, valid, H, W, radius, u16, scratch(h, SL_SRC)))) return rc;
    HIPCHK(h, hipMemcpyAsync(out, scratch(h, SL_SRC), nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return S2SR_OK;
}

int s2sr_fill_nodata_u8(s2sr_handle* h, const uint8_t* img, const uint8_t* valid, int32_t H, int32_t W, int32_t radius, uint8_t* out) {
    return fill_nodata_impl(h, img, valid, H, W, radius, false, out);
}

int s2sr_fill_nodata_u16(s2sr_handle* h, const uint16_t* img, const uint8_t* valid, int32_t H, int32_t W, int32_t radius, uint16_t* out) {
    return fill_nodata_impl(h, img, valid, H, W, radius, true, out);
}

// The blend tables of a PH x PW image's window job (pure host arithmetic, for the CPU tests): six ints per output row / column,
// {a, ia, b, ib, num, den}; window indices are those of s2sr_debug_plan_windows.
int s2sr_debug_plan_blend(int32_t PH, int32_t PW, int32_t tile, int32_t pad, int32_t scale, int32_t tiled, int32_t* rows, int32_t* cols) {
    if (!rows || !cols || PH <= 0 || PW <= 0 || tile <= 0 || pad < 0 || scale <= 0) return S2SR_E_INVALID;
    WindowJob job;
    if (int rc = plan_window_job(PH, PW, tile, pad, scale, tiled != 0, job)) return rc;
    if (blend_plan_axis(job.rm.data(), (int64_t)PH * scale, job.ny, job.wh * scale, pad * scale, rows)) return S2SR_E_INVALID;
    if (blend_plan_axis(job.cm.data(), (int64_t)PW * scale, job.nx, job.ww * scale, pad * scale, cols)) return S2SR_E_INVALID;
    return S2SR_OK;
}

int s2sr_cut_windows_u8_dev(s2sr_handle* h, const void* d_img, int32_t H, int32_t W, int32_t tile, int32_t pad,
                            int32_t first, int32_t count, void* d_tiles, void* stream) {
    if (!h || !d_img || !d_tiles || H <= 0 || W <= 0 || tile <= 0 || pad < 0 || first < 0 || count <= 0) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, as everywhere in HIP
    DOOR_ENTER(h, st);
    int PH, PW;
    int rc = plan_dims(h, H, W, tile, &PH, &PW);
    if (rc) return rc;
    TilePlan p;                                                         // the reference's plan: s2sr/dist.py indexes windows by plan position
    if ((rc = plan_windows(PH, PW, tile, pad, h->cfg.scale, p))) return fail(h, rc, kBadPlan);
    if (first + count > (int)p.wins.size()) return fail(h, S2SR_E_INVALID, "window range exceeds the plan");
    const int wh = p.wh, ww = p.ww;
    std::vector<int32_t> rects(4 * (size_t)count);
    for (int t = 0; t < count; ++t) {
        const s2sr_window& w = p.wins[first + t];
        rects[4 * t] = w.y1; rects[4 * t + 1] = w.y2; rects[4 * t + 2] = w.x1; rects[4 * t + 3] = w.x2;
    }
    int32_t* d_tab[3];
    if ((rc = upload_tables(h, st, rects, {}, {}, d_tab))) return rc;
    const hipError_t eg = launch_gather_windows((const uint8_t*)d_img, H, W, d_tab[0], count, wh, ww, PH != H || PW != W, (uint8_t*)d_tiles, st);
    rc = door_leave(h, st, S2SR_OK);
    if (eg != hipSuccess) return fail(h, S2SR_E_HIP, std::string("launch_gather_windows failed: ") + hipGetErrorString(eg));
    return rc;
}

int s2sr_stitch_rows_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t oy0, int32_t oy1,
                            void* d_out, void* stream) {
    if (!h || !d_tiles || !d_out || H <= 0 || W <= 0 || tile <= 0 || pad < 0 || oy0 < 0 || oy1 > h->cfg.scale * H || oy0 > oy1) return S2SR_E_INVALID;
    if (oy0 == oy1) return S2SR_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, as everywhere in HIP
    DOOR_ENTER(h, st);
    const int S = h->cfg.scale;
    int PH, PW;
    int rc = plan_dims(h, H, W, tile, &PH, &PW);
    if (rc) return rc;
    TilePlan p;                                              // the reference's plan, as s2sr_cut_windows_u8_dev cuts it
    if ((rc = plan_windows(PH, PW, tile, pad, S, p))) return fail(h, rc, kBadPlan);
    const int nx = p.nx, wh = p.wh, ww = p.ww;
    const size_t nrm = 2 * (size_t)(S * PH), ncm = 2 * (size_t)(S * PW);   // maps of the padded image; the stitch reads S H x S W
    // the plan's paste maps: from the handle's LRU of map sets, or built and uploaded now.  A NEW set costs an allocation and a
    // blocking upload on the handle's own stream -- nothing the caller has queued on ITS stream is waited for (r04: any key change
    // synchronised the device under the process-wide gate, so the first band's stitch drained every compute chunk already queued
    // and stalled the captures of other handles).  Only when all four sets are taken is the least recently used one recycled, and
    // only then is the device synchronised: a stitch that still reads it may be in flight on a stream this library does not know.
    const int key[4] = {H, W, tile, pad + 1};
    s2sr_handle::StitchMaps* ms = nullptr;
    for (auto& m : h->stitch_sets)
        if (m.d && m.key[0] == key[0] && m.key[1] == key[1] && m.key[2] == key[2] && m.key[3] == key[3]) ms = &m;
    if (!ms) {
        for (auto& m : h->stitch_sets)
            if (!m.d) { ms = &m; break; }
        if (!ms) {
            ms = &h->stitch_sets[0];
            for (auto& m : h->stitch_sets)
                if (m.last_use < ms->last_use) ms = &m;
            HIPCHK(h, dev_sync());
            if (ms->cap < (nrm + ncm) * 4) {
                HIPCHK(h, dev_free(ms->d));
                ms->d = nullptr; ms->cap = 0;
            }
        }
        ms->key[0] = 0;                       // (invalid until the upload is through)
        if (!ms->d) {
            HIPCHK(h, dev_malloc(&ms->d, (nrm + ncm) * 4));
            ms->cap = (nrm + ncm) * 4;
        }
        std::vector<int32_t> rm, cm;
        build_stitch_maps(p, S * PH, S * PW, rm, cm);
        HIPCHK(h, copy_blocking(h, ms->d, rm.data(), nrm * 4, hipMemcpyHostToDevice));
        HIPCHK(h, copy_blocking(h, ms->d + nrm, cm.data(), ncm * 4, hipMemcpyHostToDevice));
        for (int i = 0; i < 4; ++i) ms->key[i] = key[i];
    }
    ms->last_use = ++h->stitch_clock;
    const int32_t* d_rm = ms->d;
    const int32_t* d_cm = d_rm + nrm;
    const hipError_t es = launch_stitch((const uint8_t*)d_tiles, nx, wh * S, ww * S, d_rm + 2 * (size_t)oy0, d_cm, oy1 - oy0, S * W,
                                        (uint8_t*)d_out + (size_t)oy0 * S * W * 3, st);
    rc = door_leave(h, st, S2SR_OK);
    if (es != hipSuccess) return fail(h, S2SR_E_HIP, std::string("launch_stitch failed: ") + hipGetErrorString(es));
    return rc;
}

int s2sr_stitch_windows_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t H, int32_t W, int32_t tile, int32_t pad,
                               void* d_out, void* stream) {
    if (!h) return S2SR_E_INVALID;
    return s2sr_stitch_rows_u8_dev(h, d_tiles, H, W, tile, pad, 0, h->cfg.scale * H, d_out, stream);
}

// Device -> host for callers that hold device buffers (s2sr/dist.py's consuming rank): `bytes` from d_src into dst once
// everything enqueued on `stream` so far is done; returns when the bytes are in dst.  A destination from s2sr_host_alloc is
// filled by one DMA, a pageable one through the pinned staging slices (d2h_staged) -- never the runtime's copy kernels, which
// take CUs from the conv workgroups of whatever computes meanwhile.
int s2sr_copy_to_host(s2sr_handle* h, void* dst, const void* d_src, size_t bytes, void* stream) {
    if (!h || !dst || !d_src) return S2SR_E_INVALID;
    if (bytes == 0) return S2SR_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DOOR_ENTER(h, (hipStream_t)stream);
    if (!h->host_copy_ev) HIPCHK(h, hipEventCreateWithFlags(&h->host_copy_ev, hipEventDisableTiming));
    HIPCHK(h, ev_record(h, h->host_copy_ev, (hipStream_t)stream, SITE_COPY_TO_HOST));
    HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->host_copy_ev, SITE_COPY_TO_HOST));
    return d2h_staged(h, (uint8_t*)dst, (const uint8_t*)d_src, bytes, false);
}

}  // extern "C"
