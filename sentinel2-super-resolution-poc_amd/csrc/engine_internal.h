// Internal to the engine's translation units (engine.hip, engine_aoi.hip, engine_tiles.hip, engine_display.hip, engine_bands.hip, engine_index.hip, engine_zones.hip, engine_fields.hip, engine_fields_split.hip, engine_mzones.hip, engine_debug.hip): the handle behind
// the C ABI of include/s2sr.h, the types it is made of, and the helpers that more than one of those files uses.  What a single
// file uses stays static or anonymous in that file.
#pragma once
#include <stdio.h>

#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "row_bands.h"
#include "s2sr_internal.h"
#include "scratch.h"

namespace s2sr::engine {

// The handle's scratch slots (grown on demand, shared by every door; the book-keeping is csrc/scratch.h).  The numbers are debug ABI
// (include/s2sr.h: scratch_peek, redzone_poke, the mask of poison_scratch).  THE table of what each holds, door family by family:
enum Slot : int {
    SL_SRC = 0,   // 0 and 1: a call's source and its result: the upload and the image / tiles / level that leave.  Along a chain of
    SL_DST,       //   pyramid or display calls the roles swap: the source is where the call before kept its result, the result other() of it;
                  //   slot 1 also holds the label raster s2sr_zones_rasterize_u16 makes (kept by nobody: it leaves for the host in bands);
                  //   s2sr_fields_segment_i16: slot 0 the int16 index raster, slot 1 the uint16 labels;
                  //   s2sr_zones_kmeans_i16: slot 0 the D int16 index rasters, slot 1 the uint16 labels;
                  //   s2sr_fields_split_i16: as s2sr_fields_segment_i16; until the labels are written slot 1 holds the uint16 distance plane D2
    SL_MID,       // what lies between: gathered windows (the untiled image's tiles), the 16-bit batch's quantised tiles, the resample
                  //   intermediate, the PNG writer's statistics, the band s2sr_carry_band_u16 carries, plane b of s2sr_index_nd_u16,
                  //   one of the two uint8 mask planes of s2sr_fields_segment_i16 (the morphology passes ping-pong between this one and SL_CHUNK),
                  //   one of the two uint8 zone rasters of s2sr_zones_kmeans_i16 (the mode filter ping-pongs between this one and SL_CHUNK);
                  //   s2sr_fields_split_i16: of this one and SL_CHUNK, one ends as the mask m and the other takes the interior I
    SL_TABLES,    // tables and plans: paste / blend tables, warp grid, footprint and tap tables, PNG plans, display histogram + LUT, an index pass's LUT, counter,
                  //   histogram and zonal sums; a zone rasterisation's xy, ring_start, feat_start, label, tile bins (starts, features) and area;
                  //   a segmentation's chunk sums (uint32 per 1024 pixels), found (uint64) and fields (uint64 [Z + 1][6]);
                  //   a k-means' per-field count, minima, maxima, status, rank map, centres, ranked centres, changed flag and sums / table;
                  //   a split's tables are a segmentation's with the growth's changed counter (uint32) and two planes of tile marks (uint8 per 64 x 64 tile) between found and fields
    SL_CHUNK,     // a chunk's tile outputs, the unbanded post-process's image, the PNG streams of even groups; a segmentation's other mask plane; a k-means' other zone raster
    SL_PP,        // the post-process work area, where a banded run lives while it is open; the PNG streams of odd groups (the level the
                  //   writer reads is in 0 / 1, so while it runs 2 .. 5 are free); a segmentation's parent plane (int32 per pixel: the local root,
                  //   then the root; -1 background); a split's growth words (uint64 per pixel: steps << 32 | owner key, all ones = unreached)
    SL_VALID,     // the device copy of a masked call's `valid` (nodata.hip; the masked warp of tiles.hip); an index pass's `valid` and, behind it, its zone labels;
                  //   a split's vertical distances g (uint8 per pixel) and, behind the distance pass, its core plane (uint8)
    SL_CONS,      // a consistency pass's inexact counters (uint64[3], the first 256 bytes) and, in mode 2, its residual plane (consistency.hip);
                  //   a carried band's inexact counter (uint64, the first 256 bytes) and its coefficient planes A, C (bands.hip);
                  //   a segmentation's size plane (uint32 per pixel: a local component's pixels at its local root, the sum at the root, then the root's rank);
                  //   a split's parent plane (int32 per pixel) and, behind it, its size plane (also the components' largest D2 and the owners' keys)
};
static_assert(SL_CONS + 1 == slots::kSlots, "one enumerator per slot");
inline Slot other(Slot s) { return s == SL_DST ? SL_SRC : SL_DST; }            // of the 0 / 1 pair
inline Slot png_stream_slot(int group) { return group & 1 ? SL_PP : SL_CHUNK; }   // tiles_write_png_locked: the streams ping-pong
using slots::KEPT_RASTER; using slots::KEPT_LEVEL; using slots::KEPT_U16;

// The net, layer by layer, in the order of the weight blob: the one place a layer or a model is declared.  layer_table() builds
// it from the config; the blob sizes of the C ABI, the loader (load_weights_locked: one case per role) and the schedules
// (run_net, run_net_compact, through s2sr_handle::conv) all read it.
enum Role {
    L_FIRST,        // RRDB nets: conv_first (scale 2: on the 12 channels of pixel_unshuffle(x, 2))
    L_RDB14,        // conv1..4 of a ResidualDenseBlock
    L_RDB5,         // its conv5 ...
    L_RDB5_RRDB,    // ... and the conv5 that closes an RRDB (third RDB: the RRDB skip in its epilogue)
    L_BODY, L_UP1, L_UP2, L_HR, L_LAST,
    L_CFIRST, L_CBODY, L_CLAST,   // SRVGGNetCompact: first conv, PReLU body convs, the last conv with the pixel-shuffle tail
};
constexpr int kRoles = L_CLAST + 1;
inline bool is_rdb(Role r) { return r == L_RDB14 || r == L_RDB5 || r == L_RDB5_RRDB; }

// Launch order.  Every conv kernel walks its patches image-major, front to back, or mirrored (ConvParams::dbg bit 0).
// The schedules keep one direction and turn it round in front of the launches whose bit is set in s2sr_handle::serpentine: bit `role`
// for a layer of that Role, bits 12..15 for conv1..4 of an RDB (L_RDB14 itself has none), bit 16 for the second row-parity launch of an
// up-conv.  A turned launch meets the planes the launch before it touched last.  The rule is static, so a captured graph replays one order.
inline int serp_bit(Role r, int k = 0) { return r == L_RDB14 ? 12 + (k - 1) : (int)r; }
constexpr int kSerpUpSecond = 16;
// Default: every launch of the RRDB nets walks opposite to the one in front of it (profiles/serpentine_bench.txt: the gain is the trunk's,
// conv2..5 meeting the planes of the launch before; the tail neither gains nor loses).  The compact nets were not measured and keep one direction.
constexpr int kSerpentineDefault = 0x1F1FC;
struct Layer {
    Role role;
    int cin, cout, extra;      // extra: floats behind the bias (the 64 PReLU slopes of a compact conv, 0 otherwise)
    size_t floats() const { return (size_t)cin * cout * 9 + cout + extra; }
};
std::vector<Layer> layer_table(int arch, int num_block, int scale);   // arch: S2SR_ARCH_*; compact: num_block carries num_conv
size_t table_floats(const std::vector<Layer>& table);

struct ConvW {
    Role role = L_FIRST;
    ConvForm form = CF_NONE;            // its launch_conv form; CF_NONE: the RDB convs (conv_trunk.hip) and the up-convs (launch_conv_phase)
    int cin = 0, cout = 0, nstage = 0, ct = 0;
    int seg_len = 0, seg_lo_mask = 0;   // split-operand convs (precision S2SR_PREC_F16_HP), see ConvParams
    bool split = false;                 // hp mode, cin 64: fp16 main term + e4m3 correction planes in (pack_conv_weights_f8hp, ..._phase_f8hp)
    void* d_wphase[2] = {nullptr, nullptr};   // up-convs: the 2x2 sub-pixel kernels per output row parity (pack_conv_weights_phase_f8hp)
    void* d_wpack = nullptr;
    float* d_bias = nullptr;
    // fp8 trunk mode (S2SR_PREC_FP8), the 345 RDB convs: e4m3 weight planes (pack_conv_weights_f8; nstage = planes padded
    // to even, seg_len = real planes) + per-output-channel E8M0 scale bytes
    int32_t* d_wscale = nullptr;
    bool pooled = false;                // d_wpack / d_wscale point into the handle's pools
    float* d_slope = nullptr;           // SRVGGNetCompact: the 64 PReLU slopes behind this conv (in pool_b, next to the bias)
};

// kernel families for the HIP-event statistics
enum Fam { F_PACK, F_FIRST, F_RDB14, F_RDB5, F_BODY, F_UP, F_HR, F_LAST, F_POST, F_MISC, F_CFIRST, F_CBODY, F_CLAST, F_DHIST, F_DAPPLY, F_NFILL, F_NMASK, F_CONS, F_BANDS, F_INDEX, F_COUNT };
inline constexpr const char* kFamName[F_COUNT] = {"pack_u8",   "conv_first", "rdb_conv1-4", "rdb_conv5",   "conv_body",
                                 "conv_up",   "conv_hr",    "conv_last",   "postprocess", "misc",
                                 "compact_first", "compact_body", "compact_last", "display_hist", "display_apply",
                                 "nodata_fill", "nodata_mask", "consistency", "bands", "index"};

inline constexpr int kRoleFam[kRoles] = {F_FIRST, F_RDB14, F_RDB5, F_RDB5, F_BODY, F_UP, F_UP, F_HR, F_LAST, F_CFIRST, F_CBODY, F_CLAST};   // by Role

struct Workspace {
    int G = 0, H = 0, W = 0;   // capacity (images) and logical LR dims
    char* base = nullptr;
    size_t bytes = 0;
    // LR tensors (blocked-16 fp16 / blocked-8 fp32, see s2sr_internal.h)
    char *P0 = nullptr;                  // input, 1 block
    char *D[3] = {nullptr, nullptr, nullptr};   // dense-block tensors, 12 blocks: [x(4) | x1 | x2 | x3 | x4]; three of them rotate
                                         // through an RRDB (rdb k reads D[k], writes the next x into D[(k+1)%3]), so the
                                         // RRDB's input D[0] is still there when rdb3's conv5 needs it as the skip
    char *U0 = nullptr;                  // 4 blocks
    char *T = nullptr;                   // trunk lo as fp16 (4 blocks): conv_first writes it, the trunk's lo planes are made from it (Tr[0])
    char *Tr[3] = {nullptr, nullptr, nullptr};  // one-wave-per-SIMD path: trunk lo of D[0..2] as e4m3(lo * 2^lo_exp), 2 planes of 32 channels
    float *R = nullptr, *F = nullptr;    // fp32 RRDB skip / global skip (8 blocks of 8)
    // 2x and 4x tensors, 4 blocks each
    char *U1 = nullptr, *U2 = nullptr, *U3 = nullptr;
    // split-operand mode only: e4m3 correction planes of U0..U3 and of the trunk, 4 planes of 32 B per
    // pixel each ([lo*2^11 p0, p1, hi p0, p1]) -- the size of a 4-block fp16 tensor
    char *U0lo = nullptr, *U1lo = nullptr, *U2lo = nullptr, *U3lo = nullptr, *T8 = nullptr;
    // fp8 trunk mode only: the dense-block tensors as e4m3 planes of 32 channels [x(2) | x1 | x2 | x3 | x4], the trunk x in
    // fp16 (three rotating buffers: an RRDB's input stays readable until its last conv5 has used it as the skip), and
    // an all-zero "trunk lo" for conv_body's split-operand path
    char *D8[2] = {nullptr, nullptr};
    char *Xh[3] = {nullptr, nullptr, nullptr};
    char *Tz = nullptr;
    bool hp = false, fp8 = false;
    int mos_py = 0, mos_px = 0;          // separator periods of the window mosaic these planes were zeroed for (0: plain images)
    int Hp = 0, Wp = 0, Hp2 = 0, Wp2 = 0, Hp4 = 0, Wp4 = 0;
    size_t blk1 = 0, blk2 = 0, blk4 = 0;   // bytes of one block plane at 1x / 2x / 4x
};

struct EvRec {
    int fam;
    hipEvent_t e0, e1;
    double flops, bytes;
    int n = 1;           // launches between the two events (a span of consecutive launches of one family)
};

// Window mosaic geometry of one forward (see ConvParams::mos_*): kx x ky windows of wh x ww per image, `count` windows in all.
inline int mosaic_extent(int k, int w) { return k * (w + 1) - 1; }   // rows / columns of k windows of w with their separators
struct Mosaic {
    int kx = 1, ky = 1, wh = 0, ww = 0, count = 0;
    bool on() const { return wh > 0; }
    // per launch image, for windows of th x tw on the trunk grid: windows, rows, columns, 32 x 32 patches.  A mosaic that is on was
    // picked for these very windows (pick_mosaic sets wh x ww = th x tw), so it answers from its own wh x ww; th, tw serve the plain image.
    int per() const { return on() ? kx * ky : 1; }
    int image_h(int th) const { return on() ? mosaic_extent(ky, wh) : th; }
    int image_w(int tw) const { return on() ? mosaic_extent(kx, ww) : tw; }
    long patches(int th, int tw) const { return (long)((image_h(th) + 31) / 32) * ((image_w(tw) + 31) / 32); }
};

// What a forward writes, either or both (device): u8 [B,S th,S tw,3], f32 [B,3,S th,S tw], S = cfg.scale.  What it reads is a
// TileIn (s2sr_internal.h).
struct TileOut {
    uint8_t* u8 = nullptr;
    float* f32 = nullptr;
    TileOut from(size_t px) const { return TileOut{u8 ? u8 + px : nullptr, f32 ? f32 + px : nullptr}; }   // px samples further on
    bool operator==(const TileOut& o) const { return u8 == o.u8 && f32 == o.f32; }
};

// One captured group (pack + the whole layer schedule) for fixed shapes and buffers.  A net is
// 351 dependent launches; small groups are launch-bound (~15 us per launch against a few us of
// work), so the second time the same (shape, buffers) group shows up it is captured into a
// hipGraph and replayed from then on.  GraphKey: everything a replay must have in common with the captured group.
struct GraphKey {
    int n = 0, th = 0, tw = 0;
    int mos_kx = 0, mos_ky = 0, mos_count = 0;
    // the group's input: kind, pointer, the rows / columns as stored, and for 16-bit tiles the value range (the packer's constants
    // and conv_first's in_scale are baked into the captured launches, and the host entries reuse one scratch pointer for every range)
    TileIn in;
    TileOut out;
    hipStream_t st = nullptr;
    bool operator==(const GraphKey& o) const {
        return n == o.n && th == o.th && tw == o.tw && mos_kx == o.mos_kx && mos_ky == o.mos_ky && mos_count == o.mos_count && in == o.in &&
               out == o.out && st == o.st;
    }
};
struct GraphEntry {
    GraphKey key;
    hipGraphExec_t exec = nullptr;   // null until captured
    bool refused = false;            // capture failed once: stay on direct launches
    uint64_t last_use = 0;
};

// s2sr_debug_trunk_taps while its batch runs: the RDB range whose fields run_net copies out (trunk_tap) and where the form
// records of the range's conv launches go
struct TrunkTap {
    int first = 0, count = 0;
    s2sr_debug_trunk_fields* t = nullptr;
    s2sr_debug_trunk_form spare[5];     // the records of RDBs outside the range
    s2sr_debug_trunk_form* forms(int g) { return t->form && g >= first && g < first + count ? t->form + 5 * (g - first) : spare; }
};

// s2sr_debug_compact_taps while its batch runs: run_net_compact copies the chosen layers' activations out
struct CompactTap {
    s2sr_debug_compact_fields* t = nullptr;
};

// What the N stages of a raster pass's last profiled call took (StageMarks::close writes it, stage_times_out reads it)
template <int N>
struct StageTimes { double ms[N] = {}; int32_t launches[N] = {}; };

}  // namespace s2sr::engine

// A device buffer added to this struct is also added to for_each_device_buffer below.
struct s2sr_handle {
    s2sr_config cfg{};
    // RealESRGAN_x2plus (cfg.scale 2) runs pixel_unshuffle(x, 2) and then the x4 net on the half grid.  Every entry takes input
    // sizes: the trunk (workspace, mosaic, launch groups, graphs) is input / unshuffle(), the output input * cfg.scale.
    int unshuffle() const { return cfg.scale == 2 ? 2 : 1; }
    bool compact() const { return cfg.arch == S2SR_ARCH_COMPACT; }   // SRVGGNetCompact: cfg.num_block carries num_conv
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    // split-operand ("hp") head / tail convs: S2SR_PREC_F16_HP, or the fp8 trunk with S2SR_FP8_TAIL=hp
    bool hp() const { return cfg.precision == S2SR_PREC_F16_HP || (cfg.precision == S2SR_PREC_FP8 && fp8_hp_tail); }
    std::vector<s2sr::engine::ConvW> convs;      // one per entry of layer_table(cfg), in its order
    int at[s2sr::engine::kRoles] = {};             // where each role's first conv sits in convs (the loader fills it)
    const s2sr::engine::ConvW& conv(s2sr::engine::Role r, int k = 0) const { return convs[at[r] + k]; }   // the k-th conv from there on
    // conv_first of the 16-bit door (x4 RRDB nets): the same conv on a cin-6 weight set, w6[:, c] = w6[:, c + 3] = w[:, c], for
    // the (d & 255, d & 0xff00) channel pairs pack_u16 writes; built next to conv_first, sharing its bias (d_wpack null: not built)
    s2sr::engine::ConvW first16;
    // the packed weights of the 345 RDB convs, their fp8 scales and every conv's bias live in three pooled allocations
    // (ConvW pointers point into them); only the six head/tail convs own separate buffers (pooled == false)
    char* pool_w = nullptr;
    int32_t* pool_s = nullptr;
    float* pool_b = nullptr;
    bool has_weights = false;
    char* d_trash = nullptr;      // parking area for out-of-image epilogue stores
    s2sr::engine::Workspace ws;
    // the scratch slots (enum Slot), what the last call kept in one of them for the next (the pyramid calls a raster or a level, the
    // 16-bit enhance doors and the display calls a uint16 image), and whether a banded post-process run is open in SL_PP
    s2sr::slots::Book scratch{s2sr::engine::SL_PP};
    int capture_failures = 0;            // captures voided by a device-wide call of another runtime user; 3 -> graphs off
    // profiling
    int prof = 0;                 // 0 off, N>=1: bracket every N-th launch of each family with events
    bool span_on = false;         // a sampled span of consecutive launches of ONE family is open (span_begin / span_end): its launches
    s2sr::engine::EvRec span;     // add their work to it instead of recording events of their own.  Two marker packets between two
    int64_t span_count = 0;       // kernels cost ~2 us of a 70-us launch (r03: 71.6 us by events against 69.0 by rocprofv3); one pair around
                                  // the four conv1-4 launches of an RDB spreads that over four
    int64_t fam_count[s2sr::engine::F_COUNT] = {0};
    std::vector<s2sr::engine::EvRec> evs;
    std::vector<hipEvent_t> ev_pool;
    s2sr_kstat stats[s2sr::engine::F_COUNT];
    hipStream_t copy_stream = nullptr;          // device-to-host copies behind the compute stream
    std::vector<hipEvent_t> group_done;
    void* stage_buf[2] = {nullptr, nullptr};    // pinned staging slices of the device-to-host path (d2h_staged)
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    bool d2h_staged_on = true;                  // S2SR_D2H_STAGED=0: hipMemcpyAsync straight into the caller's (pageable) buffer
    float* d_calib = nullptr;     // fp8 calibration: [0] max |x| of the trunk, [1] max |x_k| of the growth planes (device)
    bool fp8_hp_tail = false;     // S2SR_PREC_FP8: the six head / tail convs in plain fp16 (their ~2e-3 is below the trunk's e4m3
                                  // error) unless S2SR_FP8_TAIL=hp asks for the split-operand forms
    int lo_exp = 12;              // fp16 modes, one-wave-per-SIMD trunk: the trunk's lo half as e4m3(lo * 2^lo_exp): exact to 4 bits for
                                  // |x| < 2^(20 - lo_exp) = 256, clamped beyond (S2SR_LO_EXP)
    int fp8_x_exp = 3, fp8_g_exp = 5;   // S2SR_PREC_FP8 activation scales 2^e of the x / growth planes (S2SR_FP8_XEXP, S2SR_FP8_GEXP); calibrated
                                        // on the synthetic set: profiles/r02_fp8_scale_sweep.txt (|x| up to 56, |x_k| up to 14 before clipping)
    int fp8_x_exp0 = 3, fp8_g_exp0 = 5; // ... as s2sr_create left them: every weight load starts from these again (a calibration belongs to the weights it saw)
    bool graphs_on = true;        // S2SR_GRAPH=0 turns it off
    int64_t ws_allocs = 0;        // workspace (re)allocations since s2sr_create (s2sr_debug_get_config reserved[5])
    bool last_fold = true;        // S2SR_LAST_FOLD=0: conv_last (hp) reads all four e4m3 planes (8 stages) instead of folding w_lo into idle couts
    bool f16_full = true;         // S2SR_F16_FULL=0: fp16 conv1-4 never take the whole-patch form (no px_live arithmetic in the epilogue) on 32-multiple launches
    int serpentine = s2sr::engine::kSerpentineDefault;   // S2SR_SERPENTINE=0: every launch walks its patches front to back; otherwise the flip mask of run_net's launch order
    bool small8 = true;          // S2SR_SMALL8=0: single tiles keep the 16x32-patch form of fp16 conv1-4 (default: 8x32 patches, 256 per 256x256 tile)
    s2sr::FormSwitches form_switches() const { return s2sr::FormSwitches{small8, f16_full}; }   // what the conv launchers' picks read (conv_forms.h)
    bool mosaic_on = true;        // S2SR_MOSAIC=0: windows that are no multiple of the 32-pixel patch travel one per image (ConvParams::mos_*)
    // paste maps of the window plan last stitched through s2sr_stitch_rows_u8_dev (row map, column map), kept on the device:
    // an AOI is stitched band by band, the maps are uploaded once per (H, W, tile, pad)
    // (a small LRU of map sets: a service that alternates AOI sizes neither re-uploads nor synchronises the device per job)
    struct StitchMaps { int key[4] = {0, 0, 0, 0}; int32_t* d = nullptr; size_t cap = 0; uint64_t last_use = 0; };
    StitchMaps stitch_sets[4];
    uint64_t stitch_clock = 0;
    hipEvent_t host_copy_ev = nullptr;          // s2sr_copy_to_host: orders the copy stream behind the caller's stream
    // The last call that returned with work still queued (a *_dev door): the event behind its last enqueue and the stream it went to.
    // A later call on ANOTHER stream makes that stream wait for it first (door_enter): the workspace and the scratch slots are the
    // handle's, and the mutex only orders the enqueues.  Never cleared: a wait for an event that has fired costs nothing on the device.
    hipEvent_t order_ev = nullptr;
    hipStream_t order_stream = nullptr;
    bool order_pending = false;
    void* host_arena = nullptr;                 // page-locked host block of the tile-PNG stage (stats back, plan up): grown on demand, kept
    size_t host_arena_bytes = 0;
    // the banded post-process in progress on this handle (s2sr_pp_band_*_dev, or a whole-image job: enhance_locked): geometry, channel order, how far the
    // CLAHE'd rows and the finished rows reach
    struct PPBand {
        bool lut = false;             // (whether the run is open: scratch.run_open)
        int H = 0, W = 0, bgr = 0, swap_out = 0, radius = 0;
        int applied_end = 0, rows_end = 0;
        s2sr_pp_params prm{};
    } ppb;
    // hipGraph replay of repeated groups
    std::vector<s2sr::engine::GraphEntry> graphs;
    uint64_t graph_clock = 0;
    int64_t graph_replays = 0, graph_captures = 0;
    // where the last run_net left the trunk output conv_body reads (it differs between the fp16 and the fp8 trunk);
    // read by s2sr_debug_forward_taps only
    struct TrunkRec { const char* hi = nullptr; uint64_t hi_img = 0; const char* lo = nullptr; uint64_t lo_img = 0; int lo_exp = -1; } trunk_rec;
    // The last s2sr_fields_segment_i16, s2sr_zones_kmeans_i16 and s2sr_fields_split_i16 with profiling on: the event time and the
    // bracketed launches, stage by stage (S2SR_FIELDS_STAGE_*, S2SR_MZONES_*, S2SR_FSPLIT_*; written by StageMarks::close); and the
    // rounds the split's two growths took (always)
    s2sr::engine::StageTimes<S2SR_FIELDS_STAGES> fields_stages;
    s2sr::engine::StageTimes<S2SR_MZONES_STAGES> mzones_stages;
    s2sr::engine::StageTimes<S2SR_FSPLIT_STAGES> fsplit_stages;
    int32_t fsplit_rounds[2] = {};
    s2sr::engine::TrunkTap* ttap = nullptr;     // s2sr_debug_trunk_taps' batch is running (run_net taps the trunk at its RDB boundaries); null otherwise
    s2sr::engine::CompactTap* ctap = nullptr;   // s2sr_debug_compact_taps' batch is running
};

namespace s2sr::engine {

// ---- engine.hip (each is described at its definition)
int fail(s2sr_handle* h, int code, const std::string& msg);

#define HIPCHK(h, expr)                                                                        \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            char b__[512];                                                                     \
            snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return fail(h, S2SR_E_HIP, b__);                                                   \
        }                                                                                      \
    } while (0)

bool recover_stream(s2sr_handle* h);
#define RUN_WITH_STREAM_RECOVERY(h, call)            \
    do {                                             \
        int rc_ = (call);                            \
        if (rc_ != S2SR_OK && (h) && recover_stream(h)) rc_ = (call); \
        return rc_;                                  \
    } while (0)

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }   // the next multiple of 256: where the next table or plane starts
constexpr size_t kRasterBandBytes = (size_t)64 << 20;   // the raster passes' rasters come and go in row bands of about this size (band_of: row_bands.h)

constexpr size_t kTrashBytes = 8192;   // s2sr_handle::d_trash
// Every device allocation the handle owns, each once: s2sr_destroy frees them, s2sr_debug_redzone_check counts the zoned ones.
template <class F>
void for_each_device_buffer(s2sr_handle* h, F f) {
    f(h->d_trash); f(h->pool_w); f(h->pool_s); f(h->pool_b); f(h->first16.d_wpack); f(h->ws.base);
    for (const ConvW& c : h->convs) {
        if (!c.pooled) f(c.d_wpack);
        f(c.d_wphase[0]); f(c.d_wphase[1]);
    }
    for (void* p : h->scratch.ptr) f(p);
    for (const auto& m : h->stitch_sets) f(m.d);
}

// Scratch requests, in the order written; `on` false: this one is skipped.  Any request voids what the last call kept (slots::Book::drop).
struct Want { Slot slot; size_t bytes; bool on = true; };
int ensure_scratch(s2sr_handle* h, std::initializer_list<Want> wants);
inline int ensure_scratch(s2sr_handle* h, Slot slot, size_t bytes) { return ensure_scratch(h, {{slot, bytes}}); }
template <class T = void>
T* scratch(s2sr_handle* h, Slot s) { return (T*)h->scratch.ptr[s]; }
// The source of a door that may read what the last call kept: SL_SRC for a host buffer, or the slot take() finds.  The slot is
// guarded against regrowth while the door runs; keep() at the door's successful end says what it leaves.
struct KeptInput {
    s2sr_handle* h;
    Slot slot = SL_SRC;
    explicit KeptInput(s2sr_handle* h_) : h(h_) {}
    ~KeptInput() { h->scratch.release(); }
    bool take(slots::Kind kind, int a, int b) {
        const int s = h->scratch.take(kind, a, b);
        if (s >= 0) slot = (Slot)s;
        return s >= 0;
    }
};
hipError_t copy_blocking(s2sr_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
hipError_t fill_blocking(s2sr_handle* h, void* dst, int value, size_t bytes);
// H rows of row_bytes each from src to dst in bands of `rows` rows, queued on st: a raster comes in or leaves
hipError_t copy_rows(s2sr_handle* h, void* dst, const void* src, size_t H, size_t row_bytes, size_t rows, hipMemcpyKind kind, hipStream_t st);

// the plane decoders of the test hooks
typedef _Float16 hf16;
float e4m3_to_f32(uint8_t b);
int fetch_planes(s2sr_handle* h, std::vector<uint8_t>& buf, const char* src, uint64_t img, int n, int nb, size_t blk);
int decode_f16_planes(s2sr_handle* h, float* dst, const char* src, uint64_t img, int n, int nb, size_t blk);
int decode_e4m3_planes(s2sr_handle* h, float* dst, const char* src, uint64_t img, int n, int nb, size_t blk, const float* scale);

hipEvent_t get_event(s2sr_handle* h);
int ensure_group_events(s2sr_handle* h, int n);

// ---- ordering events (stall.hip) ---------------------------------------------------------------------------------
// Every event that ORDERS two streams, or a stream and the host, goes through ev_record / ev_stream_wait / ev_host_wait with the
// Site that names its producer / consumer pair; hipEventRecord, hipStreamWaitEvent and hipEventSynchronize appear nowhere else in
// csrc/ except at the timing events (Scope, span_begin / span_end, the e0 / e1 pairs of engine_debug.hip), which order nothing
// (tests/test_stall_cpu.py scans for that).  With the stall mode off a wrapper is the call it wraps plus one relaxed atomic load.
enum Site {
    SITE_BATCH_GROUP_D2H,       // forward_batch_u8_once: group g's tiles leave on the copy stream under group g + 1's forward
    SITE_BATCH_U16_D2H,         // forward_batch_u16_once: the quantised and / or fp32 tiles leave behind the quantiser
    SITE_CHUNK_BAND_D2H,        // run_chunks / enhance_locked: band c - 1 leaves under chunk c; the whole quantised image next to an fp32 one
    SITE_PP_BAND_D2H,           // pp_finish_bands: a finished band of a banded post-process leaves
    SITE_TAIL_D2H,              // enhance_locked: the unbanded post-process's image, the fp32 image
    SITE_DISPLAY_UPLOAD,        // display_hist_impl / display_apply_impl: band i + 1 uploads on the copy stream under band i's kernel
    SITE_DISPLAY_BAND_D2H,      // display_apply_impl: band i - 1 leaves under band i's kernel (two ping-pong events)
    SITE_COPY_TO_HOST,          // s2sr_copy_to_host: the copy stream behind the caller's stream
    SITE_STAGE_SLICE,           // d2h_staged: a page-locked slice is full (host wait)
    SITE_PNG_STATS,             // tiles_write_png_locked: a group's statistics are on the host (host wait)
    SITE_PNG_EMIT,              // ... its streams are emitted: the copy stream may read them (host wait)
    SITE_PNG_BATCH,             // ... a batch of streams sits in its staging buffer (host wait)
    SITE_HANDLE_ORDER,          // door_enter / door_leave: a call on one stream behind the unfinished call on another
    SITE_COUNT
};
// The negative control (s2sr_debug_delay_drop) may skip the stream-waits of these sites and no others.  At each of them the waiting
// stream is the copy stream and what it runs next is a device-to-host hipMemcpyAsync of finished pixel bytes, with source, size and
// destination computed on the host before the wait: a wait that is missing lets the copy read pixels too early and nothing else.
//   SITE_BATCH_GROUP_D2H   d2h_staged of SL_DST [g0 tout, n tout): u8 tiles; no kernel runs on the copy stream
//   SITE_CHUNK_BAND_D2H    d2h_staged of rows [prev_yb, prev_ye) of the quantised image (SL_DST): pixels; as above
//   SITE_DISPLAY_BAND_D2H  d2h_staged of bytes [pb0, pb1) of the 8-bit image (SL_SRC / SL_DST); the NEXT upload on the copy stream
//                          writes the uint16 image in the other slot, which this wait never guarded
//   SITE_COPY_TO_HOST      d2h_staged of the caller's [d_src, d_src + bytes)
// Never droppable: SITE_DISPLAY_UPLOAD (a kernel consumes it), SITE_HANDLE_ORDER (tables, plans and LUTs of the call before live in
// the scratch it guards), the host waits (the host reads statistics, offsets and plans behind them), and the rest, which no control needs.
inline constexpr int kDroppableSites[] = {SITE_BATCH_GROUP_D2H, SITE_CHUNK_BAND_D2H, SITE_DISPLAY_BAND_D2H, SITE_COPY_TO_HOST};

extern std::atomic<int> g_delay_mode;      // s2sr_debug_delay: bit 1 the compute side, bit 2 the copy side; 0 off
extern std::atomic<int> g_delay_drop;      // s2sr_debug_delay_drop: the Site whose stream-waits are skipped, -1 none
hipError_t delay_stall(s2sr_handle* h, hipStream_t st);   // one stall on st when its side's bit is set and st is not capturing
inline hipError_t ev_record(s2sr_handle* h, hipEvent_t ev, hipStream_t st, Site) {
    const hipError_t e = hipEventRecord(ev, st);
    return e == hipSuccess && g_delay_mode.load(std::memory_order_relaxed) ? delay_stall(h, st) : e;
}
inline hipError_t ev_stream_wait(s2sr_handle* h, hipStream_t st, hipEvent_t ev, Site site) {
    const bool on = g_delay_mode.load(std::memory_order_relaxed) != 0;
    if (on && g_delay_drop.load(std::memory_order_relaxed) == (int)site) return delay_stall(h, st);
    const hipError_t e = hipStreamWaitEvent(st, ev, 0);
    return e == hipSuccess && on ? delay_stall(h, st) : e;
}
inline hipError_t ev_host_wait(s2sr_handle*, hipEvent_t ev, Site) { return hipEventSynchronize(ev); }
// The first and last line of a door behind hipSetDevice.  door_enter: st (and, for a door on the handle's own stream, the copy
// stream) waits for the unfinished call on another stream, then the mode's entry stalls.  door_leave: a *_dev door returns with
// work queued on the caller's stream: the event behind it.  rc is passed through.
int door_enter(s2sr_handle* h, hipStream_t st);
int door_leave(s2sr_handle* h, hipStream_t st, int rc);
#define DOOR_ENTER(h, st)                                    \
    do {                                                     \
        if (int rc__ = door_enter((h), (st))) return rc__;   \
    } while (0)

struct Scope {   // brackets one launch with events when profiling is on
    s2sr_handle* h;
    hipStream_t st;
    EvRec r;
    bool on;
    Scope(s2sr_handle* h_, hipStream_t st_, int fam, double flops, double bytes) : h(h_), st(st_), on(false) {
        if (h->prof <= 0) return;
        if (h->span_on && h->span.fam == fam) { h->span.flops += flops; h->span.bytes += bytes; h->span.n += 1; return; }
        on = (h->fam_count[fam]++ % h->prof) == 0;
        if (!on) return;
        r.fam = fam; r.flops = flops; r.bytes = bytes;
        r.e0 = get_event(h); r.e1 = get_event(h);
        hipEventRecord(r.e0, st);
    }
    ~Scope() {
        if (!on) return;
        hipEventRecord(r.e1, st);
        h->evs.push_back(r);
    }
};

// The stage book of one call of a raster pass.  With profiling on every launch's event pair (Scope) is also booked to the stage it
// belongs to: [from, to) of h->evs per stage.  next() ends a stage; close(), at the call's successful end only, writes what each
// stage took to the handle, so a call that fails midway leaves the times of the call before.  The events stay where they are: the
// family's statistics read them later.  An unprofiled call records no event and leaves zeros.
constexpr int kMaxStages = 8;
struct StageMarks {
    s2sr_handle* h;
    int stage = 0;
    size_t mark[kMaxStages + 1];
    explicit StageMarks(s2sr_handle* h_) : h(h_) { mark[0] = h->evs.size(); }
    void next() { if (stage++ < kMaxStages) mark[stage] = h->evs.size(); }   // one too many is counted, not stored: close refuses
    template <int N>
    int close(StageTimes<N>& t) {
        static_assert(N <= kMaxStages, "a book of more stages needs a larger kMaxStages");
        if (stage != N) return fail(h, S2SR_E_HIP, "stage book: " + std::to_string(stage) + " stages were ended where the pass has " + std::to_string(N));
        for (int k = 0; k < N; ++k) {
            t.ms[k] = 0.0;
            t.launches[k] = 0;
            for (size_t i = mark[k]; i < mark[k + 1] && i < h->evs.size(); ++i) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, h->evs[i].e0, h->evs[i].e1) != hipSuccess) continue;
                t.ms[k] += ms;
                t.launches[k] += h->evs[i].n;
            }
        }
        return S2SR_OK;
    }
};
// The body of the s2sr_debug_*_stage_ms hooks: the book of the last call copied out under the lock.  given: every array the hook
// requires is there (`refusal` otherwise); rounds: the split's hook also hands out fsplit_rounds.
template <int N>
int stage_times_out(s2sr_handle* h, StageTimes<N> s2sr_handle::*book, bool given, const char* refusal, double* ms, int32_t* launches,
                    int32_t* rounds = nullptr) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!given) return fail(h, S2SR_E_INVALID, refusal);
    for (int k = 0; k < N; ++k) {
        ms[k] = (h->*book).ms[k];
        launches[k] = (h->*book).launches[k];
    }
    if (rounds) rounds[0] = h->fsplit_rounds[0], rounds[1] = h->fsplit_rounds[1];
    return S2SR_OK;
}

int group_size(const s2sr_handle* h, int B, int H, int W);
int group_windows(const s2sr_handle* h, const Mosaic& mo, int T, int th, int tw);
void mosaic_remainder(int rem, int kx, int ky, int* rkx, int* rky);
long mosaic_patches(int B, int th, int tw, int kx, int ky);
Mosaic pick_mosaic_cfg(bool mosaic_on, int B, int th, int tw);
Mosaic pick_mosaic(const s2sr_handle* h, int B, int th, int tw);
int forward_dev(s2sr_handle* h, hipStream_t st, TileIn in, int B, int th, int tw, const TileOut& out, const Mosaic* plan = nullptr);
int check_u16(s2sr_handle* h, int lo, int hi);

// ---- engine_aoi.hip
constexpr size_t kStageBytes = 32u << 20;   // one pinned staging slice (s2sr_handle::stage_buf)
int d2h_staged(s2sr_handle* h, uint8_t* dst, const uint8_t* src, size_t bytes, bool exposed);
void plan_chunk_sizes(int units, int u_max, long unit_windows, int per, long pimg, int ncu, std::vector<int>& sizes);
// The windows a whole-image call runs the net on: ny rows of nx distinct windows of wh x ww, their rectangles (y1, y2, x1, x2 each,
// row-major; empty for the untiled image, which is its own window) and the paste maps of the scale PH x scale PW output: per output
// row (column) the window row (column) it comes from and the row (column) inside that window's output.
struct WindowJob {
    int nx = 1, ny = 1, wh = 0, ww = 0;
    std::vector<int32_t> rects, rm, cm;
};
int plan_window_job(int PH, int PW, int tile, int pad, int scale, bool tiled, WindowJob& job);

// ---- engine_fields.hip: the stages s2sr_fields_segment_i16 and s2sr_fields_split_i16 (engine_fields_split.hip) share
// The refusals of both doors, in order, under the door's own prefix `what`; S2SR_OK when none applies.
int fields_check_args(s2sr_handle* h, const char* what, const void* idx, const void* labels, int H, int W, int lo, int hi, int r_open, int r_close,
                      int conn, int64_t min_pixels, int Z);
// min_pixels as the kernels take it, and SL_TABLES: the chunk sums, found (at o_found), `between` bytes of the door's own (at
// o_between; a multiple of 256), the fields table (fields_b bytes at o_fields); bytes: the slot's request.
struct FieldsPlan { uint32_t minpx; size_t o_found, o_between, o_fields, fields_b, bytes; };
FieldsPlan fields_plan(int H, int W, int64_t min_pixels, int Z, size_t between = 0);
// The index -> the mask: lo..hi, opened and closed, nodata taken out again behind a morphology.  *cur: the plane of d_m that holds it.
int fields_mask(s2sr_handle* h, hipStream_t st, const int16_t* d_idx, uint8_t* const d_m[2], int H, int W, int lo, int hi, int r_open, int r_close,
                int* cur);
// A plane's connected components (local, border, flatten: parent = the root) and the numbering (count, scan, apply, labels).
// book: the plain segmentation ends a stage behind every launch; the split books them in groups and passes none.
int fields_components(s2sr_handle* h, hipStream_t st, const uint8_t* plane, int* d_parent, uint32_t* d_size, int H, int W, int conn, StageMarks* book);
int fields_numbering(s2sr_handle* h, hipStream_t st, int* d_parent, uint32_t* d_size, int H, int W, uint32_t minpx, int Z, uint32_t* d_sums,
                     unsigned long long* d_found, unsigned long long* d_fields, uint16_t* d_labels, StageMarks* book);

}  // namespace s2sr::engine
