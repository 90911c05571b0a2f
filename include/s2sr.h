/*
 * s2sr.h -- C ABI of libs2sr.so, the MI355X (gfx950) Real-ESRGAN x4 (and x2plus, and SRVGGNetCompact x4) inference path.
 *
 * The reference (fieldin/sentinel2-super-resolution-poc) has no FFI layer: its seam is the
 * Python class `RealESRGAN` (server/app/cnn_super_resolution.py:161-280) plus the free
 * functions `_enhance_for_crops` (server/app/wow_sr.py:187-209) and the farm variants
 * (server/app/farm_sr.py:61-108).  This header is the native boundary a replacement of that
 * seam binds; the ctypes stub that sits on it is in INTEGRATION.md and
 * in sentinel2-super-resolution-poc_amd/s2sr/native.py.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * S2SR_E_* code; no exception crosses the boundary; outputs are caller-allocated; the last
 * error text is handle-scoped (s2sr_last_error).  A handle serialises its own calls
 * (internal mutex), so it may be shared by the reference's worker threads
 * (server/app/main.py:247-368 run jobs from a thread pool).
 *
 * Pointers named `d_*` are DEVICE pointers (HIP), everything else is host memory.
 */
#ifndef S2SR_H
#define S2SR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2SR_OK            0
#define S2SR_E_INVALID    -1   /* bad argument */
#define S2SR_E_HIP        -2   /* HIP runtime error (text in s2sr_last_error) */
#define S2SR_E_NOWEIGHTS  -3   /* forward called before s2sr_load_weights */
#define S2SR_E_BADBLOB    -4   /* weight blob size does not match the configured net */
#define S2SR_E_NODEVICE   -5   /* no gfx950 device visible: there is NO CPU fallback */
#define S2SR_E_CAPACITY   -6   /* caller buffer too small */
#define S2SR_E_IO         -7   /* a file could not be written (errno holds the reason) */

/* arithmetic of the conv stack */
#define S2SR_PREC_F16  0   /* fp16 operands, fp32 accumulate on MFMA; fp32 residual trunk  */
#define S2SR_PREC_F16_HP 1 /* same, plus the six convs outside the RRDB trunk (conv_first, conv_body, up1, up2,
                            * hr, last) computed with split fp16 operands (x_hi,w_hi)+(x_lo,w_hi)+(x_hi,w_lo):
                            * fp32-class head/tail, ~1e-4 of the fp32 reference at ~1.2x the time            */

#define S2SR_PREC_FP8 2    /* the 345 RDB convs on e4m3 operands (block-scaled fp8 MFMA, K = 64; per-output-channel weight
                            * scales, per-tensor-kind activation scales, fp16 trunk); the six head / tail convs in PLAIN fp16 (as S2SR_PREC_F16;
                            * their ~2e-3 is below the trunk's e4m3 error) unless S2SR_FP8_TAIL=hp selects the split-operand forms.
                            * BASELINE.json configs[4] (the /api/sr variant).  NOT within the 1e-3 tolerance: e4m3 keeps
                            * 3 mantissa bits; measured max-abs in tests/test_gpu_net.py (test_fp8_mode_*)             */

/* network family (s2sr_config.arch) */
#define S2SR_ARCH_RRDB    0   /* RRDBNet: realesrgan_x4, realesrgan_anime, RealESRGAN_x2plus */
#define S2SR_ARCH_COMPACT 1   /* SRVGGNetCompact(num_feat=64, num_conv, upscale=4, act_type="prelu"): realesr-general-x4v3,
                               * realesr-general-wdn-x4v3 (num_conv 32), realesr-animevideov3 (16):
                               *   h = PReLU(conv3x3(x, 3->64)); num_conv x h = PReLU(conv3x3(h, 64->64)); y = conv3x3(h, 64->48);
                               *   out = pixel_shuffle(y, 4) + nearest_upsample(x, 4)
                               * Arithmetic: fp16 operands, fp32 accumulate, fp16 activations between layers, fp32 bias / slope /
                               * base add.  S2SR_PREC_F16 and S2SR_PREC_F16_HP run this SAME arithmetic on this arch (there is no
                               * split-operand form of it); S2SR_PREC_FP8 is S2SR_E_INVALID (s2sr_create, s2sr_calibrate_fp8). */

typedef struct s2sr_handle s2sr_handle;

/* Mirrors the constructor arguments of the reference net
 * `RRDBNet(num_in_ch=3,num_out_ch=3,num_feat,num_block,num_grow_ch=32,scale)`
 * (cnn_super_resolution.py:113-121,196-203) plus device-side knobs. */
typedef struct s2sr_config {
    int32_t num_block;   /* 23 (realesrgan_x4) or 6 (realesrgan_anime), cnn_super_resolution.py:28-45 */
    int32_t num_feat;    /* must be 64 */
    int32_t num_grow;    /* must be 32 */
    int32_t scale;       /* 4, or 2 = RealESRGAN_x2plus: F.pixel_unshuffle(x, 2), a 12-channel conv_first, then the x4 body and
                          * tail on the half-resolution grid (basicsr RRDBNet(num_in_ch=3, scale=2)); output 2H x 2W.  Scale 2
                          * network-level entries (forward_batch_u8, forward_f32, calibrate_fp8, forward_part_u8_dev, the debug
                          * hooks) take even th, tw (S2SR_E_INVALID otherwise); the image entries (enhance_*, tile_process, cut /
                          * stitch) take any H, W >= 2 and an even tile, reflect-pad an odd H or W by one row / column at the
                          * bottom / right (RealESRGANer's mod-2 rule), plan the windows on the padded image at scale 2 and crop
                          * the output to 2H x 2W. */
    int32_t precision;   /* S2SR_PREC_* */
    int32_t device;      /* HIP device ordinal */
    int32_t group;       /* images pushed through the trunk together (0 = default) */
    int32_t arch;        /* S2SR_ARCH_* (the field was `reserved`: callers that zeroed it get S2SR_ARCH_RRDB; any other value is
                          * S2SR_E_INVALID).  S2SR_ARCH_COMPACT: num_block carries num_conv (16 or 32), num_feat 64, num_grow is
                          * ignored, scale 4 only. */
} s2sr_config;

/* One window of RealESRGAN._tile_process (cnn_super_resolution.py:244-278). */
typedef struct s2sr_window {
    int32_t y1, y2, x1, x2;             /* input rectangle, LR pixels                          */
    int32_t crop_top, crop_bottom, crop_left, crop_right;   /* output pixels dropped           */
    int32_t oy1, oy2, ox1, ox2;         /* paste rectangle in the output image                 */
} s2sr_window;

/* Constants of the crop-visibility post-process (wow_sr.py:187-209 / farm_sr.py:61-108,170-178).
 * Supported range: clahe_grid 1..64; with the unsharp stage (bit1) 0 < blur_sigma < 2.75.  OpenCV's kernel for sigma is
 * cvRound(6 sigma + 1) | 1 taps wide and the device's holds 17; a wider one is not cut short: every entry that takes these
 * parameters (s2sr_postprocess_u8, s2sr_postprocess_batch_u8_dev, s2sr_pp_band_begin_dev, s2sr_enhance_job_u8) returns
 * S2SR_E_INVALID, s2sr_last_error names the limit, and nothing is computed.  A sigma below 1/12 gives the 1-tap kernel: the blur is
 * the image and the weighted sum img * (w_img + w_blur) is still taken, as addWeighted does.  clahe_clip <= 0 turns clipping off. */
typedef struct s2sr_pp_params {
    float   clahe_clip;      /* cv2.createCLAHE clipLimit: 2.5                     */
    int32_t clahe_grid;      /* tileGridSize (g,g): 8; 1..64                       */
    float   blur_sigma;      /* GaussianBlur sigma: 1.2 (wow) / 1.5 (farm); < 2.75 */
    float   w_img;           /* addWeighted alpha: 1.4 (wow) / 2.2 (farm)          */
    float   w_blur;          /* addWeighted beta: -0.4 (wow) / -1.2 (farm)         */
    int32_t hue_lo, hue_hi;  /* exclusive hue bounds of the green mask: 35, 85     */
    float   sat_gain;        /* 1.2 (wow) / 1.3 (farm)                             */
    int32_t stages;          /* bit0 CLAHE, bit1 unsharp, bit2 vegetation; 7 = all */
} s2sr_pp_params;

/* per-kernel-family timing collected with HIP events on the handle's stream */
typedef struct s2sr_kstat {
    char     name[48];
    int64_t  launches;
    double   total_ms;
    double   flops;          /* algorithmic FLOP summed over those launches  */
    double   bytes;          /* algorithmic HBM bytes summed over those launches */
} s2sr_kstat;

const char* s2sr_version(void);
int  s2sr_device_count(void);      /* number of HIP devices (0 when there is no GPU) */

/* replaces RealESRGAN.__init__'s model construction (cnn_super_resolution.py:196-203) */
int  s2sr_create(const s2sr_config* cfg, s2sr_handle** out);
void s2sr_destroy(s2sr_handle* h);
const char* s2sr_last_error(const s2sr_handle* h);   /* h may be NULL: last create() error */

/* Page-locked host memory for images that cross PCIe.  The reference returns `output.cpu().numpy()` (cnn_super_resolution.py:231-233),
 * a pageable array; a destination from s2sr_host_alloc lets s2sr_enhance_u8 / s2sr_forward_batch_u8 land their bands with the DMA
 * engines (no staging copy, no first-touch page faults: 805 MB in 20 ms instead of 130).  Any host pointer stays valid as a
 * destination; the library detects page-locked ones (hipPointerGetAttributes).  Not tied to a handle or device. */
int  s2sr_host_alloc(size_t bytes, void** out);
int  s2sr_host_free(void* p);

/* replaces load_state_dict (cnn_super_resolution.py:205-213).  `blob`: for every conv in
 * registration order (conv_first, body.{b}.rdb{1..3}.conv{1..5}, conv_body, conv_up1,
 * conv_up2, conv_hr, conv_last): weight[Cout][Cin][3][3] then bias[Cout], fp32. */
int  s2sr_load_weights(s2sr_handle* h, const float* blob, size_t n_floats);
/* floats of the blob of a scale-4 net (conv_first 3 -> 64) */
size_t s2sr_expected_blob_floats(int32_t num_block);
/* ... of a net of `scale` 4 or 2 (scale 2: conv_first 12 -> 64, 5184 floats more); 0 for any other scale.  A blob of the other
 * scale is S2SR_E_BADBLOB in s2sr_load_weights. */
size_t s2sr_expected_blob_floats_scale(int32_t num_block, int32_t scale);
/* ... of the net a config describes, either arch; 0 for a config s2sr_create would refuse for its shape.  S2SR_ARCH_COMPACT: the
 * blob is the state dict's flat `body` list in order, fp32 -- body.0.weight [64][3][3][3], body.0.bias [64], body.1.weight (64
 * PReLU slopes), then conv weight / bias / slopes alternating, last body.{2 num_conv + 2}.weight [48][64][3][3] and .bias [48]
 * (1,213,296 floats at num_conv 32).  The blob stays in state-dict order: the row permutation of the last conv that the
 * pixel-shuffle epilogue wants is a property of the packed weights only. */
size_t s2sr_expected_blob_floats_cfg(const s2sr_config* cfg);
/* same blob, DEVICE-resident (e.g. the receive buffer of the RCCL weight broadcast); `stream`
 * is the stream the blob was produced on (a hipStream_t; NULL = default stream).  Returns when loaded.  The RDB convs are
 * repacked on the device; only the six head/tail convs' weights (0.9 MB) pass through host memory. */
int  s2sr_load_weights_dev(s2sr_handle* h, const void* d_blob, size_t n_floats, void* stream);

/* S2SR_PREC_FP8 only: choose the two activation scales of the fp8 trunk from data.  Runs one forward of `tiles`
 * ([B,th,tw,3] u8, host) with wide scales, takes the largest |x| of the trunk and |x_k| of the growth features over all
 * RDBs, and sets the exponents so that headroom x those maxima stays below e4m3's 448 (headroom >= 1; 2 is a sane
 * default: e4m3 is a floating format, so a wider scale costs precision only at its subnormal end).  The defaults (3 / 5) come from the synthetic calibration set, profiles/r02_fp8_scale_sweep.txt; a deployment
 * with real checkpoints calls this once after s2sr_load_weights with a few representative tiles. */
int  s2sr_calibrate_fp8(s2sr_handle* h, const uint8_t* tiles, int32_t B, int32_t th, int32_t tw, float headroom,
                        int32_t* x_exp, int32_t* g_exp);

/* pure host function = the index math of _tile_process (cnn_super_resolution.py:244-278) */
int  s2sr_plan_tiles(int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t scale,
                     s2sr_window* out, int32_t cap, int32_t* n);

/* replaces RRDBNet.forward + the u8 quantisation of enhance() on a batch of equal-size tiles
 * (cnn_super_resolution.py:140-158,220-222,231-232): [B,h,w,3] u8 -> [B,S h,S w,3] u8, S = s2sr_config.scale (scale 2: even h,
 * w).  Every output shape below that says 4 is S on a scale-2 handle. */
int  s2sr_forward_batch_u8(s2sr_handle* h, const uint8_t* tiles, int32_t B, int32_t th, int32_t tw,
                           uint8_t* out);
/* same with device-resident input/output, asynchronous on `stream` (a hipStream_t; NULL = the
 * default stream, ordered with the caller's other default-stream work).
 * STREAMS, for this and every other *_dev entry (forward_batch_u16, forward_part, cut_windows, stitch_windows / stitch_rows,
 * postprocess_batch, pp_band_*): the call returns while its work is queued on `stream`.
 *   The library orders by itself: everything it enqueues for the call behind what `stream` already holds (so behind the work
 *   that produces the input); the call behind an earlier call on the same handle that is still running on ANOTHER stream --
 *   the handle records an event behind each *_dev call's last enqueue, and the next call on a different stream (a caller's, or
 *   the handle's own for the host-facing entries) makes that stream wait for it before it touches the workspace, the scratch
 *   slots or a graph; and its own copy stream against the compute stream.
 *   Left to the caller: its own buffers.  The input must not be overwritten, nor the output read, on another stream before
 *   `stream` has passed the call (synchronise it, or record an event behind the call and wait for that); a buffer handed to
 *   two calls on two streams is the caller's race.  A stream must stay alive until its work is done. */
int  s2sr_forward_batch_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw,
                               void* d_out, void* stream);
/* unquantised net output for parity tests: x [N,3,H,W] fp32 in [0,1] -> y [N,3,4H,4W] fp32 (scale 2: even H, W -> [N,3,2H,2W]).
 * The entry quantises its input to fp16(fp32(255 x)): exact for x = u / 255 (what the u8 entries feed), up to 0.0625 / 255 = 2.5e-4
 * off for other x above 0.5.  SRVGGNetCompact adds that input to its output (the nearest-x4 base); measured on uniform random
 * floats against a float64 net fed the same floats: 5.0e-4 max-abs at num_conv 16, 3.4e-4 at 32 (fed the quantised input: 3.1e-4 /
 * 1.3e-4); tests/test_gpu_compact_insitu.py holds both to 1e-3. */
int  s2sr_forward_f32(s2sr_handle* h, const float* x, int32_t N, int32_t H, int32_t W, float* y);

/* s2sr_enhance_args.bits == 16, and the 16-bit tile entries.
 * The 16-bit door: uint16 samples in, uint16 x4 out, no 8-bit squeeze (upstream RealESRGANer's max_range = 65535 branch; the
 * reference quantises its rasters to 8 bits first, so there is no reference to be byte-equal to here).  A call carries a value
 * range lo, hi (0 <= lo < hi <= 65535; 0, 65535 is upstream's rule):
 *   in :  d = clamp(v, lo, hi) - lo, the net sees x = d / (hi - lo) -- exactly: d reaches conv_first as two exact fp16 integers
 *         (d & 255, d & 0xff00) against a doubled weight set, the 1 / (hi - lo) lives in conv_first as the u8 door's 1 / 255 does
 *   out:  q = lo + rint(clamp(y, 0, 1) * (hi - lo)), the product taken in fp32 and rounded once, rint to nearest even; numpy:
 *         lo + np.rint(np.clip(y, 0, 1).astype(np.float32) * np.float32(hi - lo)).astype(np.int64).  (Rounds, where the u8 door
 *         truncates: truncation is the reference's quirk and stays with the u8 door.)
 * For data with d < 256 the float output is bit-identical to the u8 door's on the same values.  x4 RRDB handles of every
 * precision; S2SR_E_INVALID (text in s2sr_last_error) for a bad range, a scale-2 handle or an S2SR_ARCH_COMPACT handle,
 * S2SR_E_NOWEIGHTS before weights are loaded.  The u8 door is untouched and may be mixed freely with this one on one handle.
 *
 * s2sr_forward_batch_u16: [B,th,tw,3] u16 -> out_u16 [B,4th,4tw,3] u16 and / or out_f32 [B,3,4th,4tw] fp32 (the unquantised net
 * output); at least one of the two. */
int  s2sr_forward_batch_u16(s2sr_handle* h, const uint16_t* tiles, int32_t B, int32_t th, int32_t tw, int32_t lo, int32_t hi,
                            uint16_t* out_u16 /* [B,4th,4tw,3] or NULL */, float* out_f32 /* [B,3,4th,4tw] or NULL */);
/* same with device-resident input / output, asynchronous on `stream` (NULL = the default stream).  The fp32 tiles between the
 * net and the quantiser live in a scratch buffer of the handle: 48 B per output pixel, regrown when a larger batch arrives.
 * d_out_u16 must be 8-byte aligned (the quantiser stores four samples at a time; S2SR_E_HIP before anything is written to it). */
int  s2sr_forward_batch_u16_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw, int32_t lo, int32_t hi,
                                void* d_out_u16, void* stream);

/* s2sr_enhance_args.blend.
 * The seam-blended stitch, opt-in: the windows, forwards and whole / tiled switch of s2sr_enhance_u8 / s2sr_enhance_u16 with
 * another paste.  The overwrite paste crops every window hard, so where two windows disagree in their overlap (the net sees far
 * beyond the pad) the output steps along every tile line.  Here, per axis: owner(o) is the window the overwrite paste takes output
 * coordinate o from; a seam S is a coordinate whose owner is another rectangle than owner(S - 1); around it lies a ramp of
 * half-width r = min(pad * scale, half the way to the previous seam or the axis start, half the way to the next seam or the axis
 * end).  For o in [S - r, S + r) the output cross-fades from a = owner(S - 1) to b = owner(S), b weighing
 * w = fp32(2 (o - S + r) + 1) / fp32(4 r); where a row ramp meets a column ramp four windows take part:
 *     top = A + wx (B - A),  bot = C + wx (D - C),  v = top + wy (bot - top)       A = (a_y, a_x), B = (a_y, b_x), C = (b_y, a_x), D = (b_y, b_x)
 * in fp32, every product and sum rounded on its own, terms of weight 0 left out.  Outside every ramp v is the overwrite paste's
 * value, bit for bit.  The windows leave the net as fp32 tiles (the 16-bit door's route) and one kernel pastes, blends and
 * quantises each chunk's band of final rows; a row ramp reads the last window row of the chunk before, which is carried along.
 * An image the switch leaves whole, or a plan without ramps (pad 0), runs through the default doors as it is.  A plan whose ramps
 * would leave their windows, or that leaves output pixels uncovered (pad > tile / 2 on an image shorter than two pads), is refused
 * with S2SR_E_INVALID and a text before the device is touched.
 * 8 bits: out [S H, S W, 3] = trunc(clip(v * 255, 0, 255)) and / or out_f32 [S H, S W, 3] = v; at least one.
 * 16 bits: the 16-bit door's contract and refusals (x4 RRDB nets only), out = lo + rint(clip(v, 0, 1) * (hi - lo)). */

/* s2sr_enhance_args.mask.
 * Nodata-aware enhance, opt-in: pixels that were never measured (a clipped AOI, a swath edge, a cloud mask) are
 * kept out of the net's way and come out as nodata again.  valid is uint8 [H, W], nonzero = valid.  Integers throughout:
 *   fill (in front of the net, of the R / B exchange and of the window gather): a valid pixel is unchanged; an invalid pixel
 *     (y, x) takes all three samples of the valid pixel (qy, qx) that minimises (d2, qy, qx) lexicographically,
 *     d2 = (qy - y)^2 + (qx - x)^2, among those with d2 <= radius^2; none: it keeps its samples.  The image edge is not
 *     replicated.  radius 1..64 (the app's default of 32 is policy, not a measurement).
 *   mask (behind the paste and the post-process, before a byte leaves the device): output pixel (Y, X) is invalid iff input pixel
 *     (Y / S, X / S) is, S = s2sr_config.scale; an invalid output pixel gets out_nodata in all three samples, a valid one is the
 *     unmasked call's byte (also where it happens to equal out_nodata: the mask is the truth, the value only the file convention).
 *   The post-process runs on the filled image: its CLAHE sees extrapolated ground, not a black plane.
 * So a masked call's bytes are mask(unmasked door(fill(img))), and a mask that is valid everywhere gives the unmasked door's bytes.
 * The uint16 image a masked call leaves on the device for s2sr_display_*_u16 is the masked one.  The fp32 images are the net's own
 * output and are not offered with a mask.
 * s2sr_fill_nodata_u8 / _u16: the fill alone, host image in, filled host image out (out may be img); no weights needed.
 * S2SR_E_INVALID with a text, before the device is touched: m or m->valid NULL, radius outside 1..64, out_nodata outside 0..255
 * (0..65535 for uint16).  The handle keeps working afterwards. */
typedef struct s2sr_mask {
    const uint8_t* valid;    /* [H, W], nonzero = valid */
    int32_t radius;          /* fill radius, 1..64 */
    int32_t out_nodata;      /* the value invalid output pixels get: 0..255, or 0..65535 */
} s2sr_mask;
int  s2sr_fill_nodata_u8(s2sr_handle* h, const uint8_t* img, const uint8_t* valid, int32_t H, int32_t W, int32_t radius, uint8_t* out);
int  s2sr_fill_nodata_u16(s2sr_handle* h, const uint16_t* img, const uint8_t* valid, int32_t H, int32_t W, int32_t radius, uint16_t* out);

/* s2sr_enhance_args.consistency.
 * Radiometric consistency, opt-in: one back-projection step against the box-average sensor model, so that the mean
 * of the S x S output samples over an input pixel is that input pixel again.  Integers throughout, per channel: S = 2 or 4,
 * n = S S; q the door's quantised image [S H, S W, 3]; v = clamp(img, lo, hi) the input the net saw (8 bits: 0, 255; 16 bits: the
 * call's range); sum[y, x] the sum of q over block [S y, S y + S) x [S x, S x + S); e = n v - sum.
 *   exact step:  k = floor(e / n), r = e - n k (0..n-1); block sample (i, j) gets d = k + (rank[i][j] < r), rank the 4 x 4 Bayer
 *     order [[0,8,2,10],[12,4,14,6],[3,11,1,9],[15,7,13,5]] (S = 2: [[0,2],[3,1]]); q' = clip(q + d, lo, hi).  Where no sample of a
 *     block clips, sum' = n v exactly.
 *   smooth step: e interpolated bilinearly between input-pixel centres, edges replicated.  Output row Y = S y + i: t = 2 i + 1 - S,
 *     neighbour row clamp(y + sign(t), 0, H - 1), weights w1 = |t| (neighbour) and w0 = 2 S - w1 (y); columns alike; num = the sum
 *     of wy wx e over the four pairs, den = 4 S S n, d = floor((num + den / 2) / den), q' = clip(q + d, lo, hi).
 *   S2SR_CONSISTENCY_EXACT: the exact step.  S2SR_CONSISTENCY_SMOOTH: the smooth step, the block sums again on its result, the
 *     exact step on what remains: most of the correction then lies in a field without steps along the block grid.
 *   inexact[c] = the blocks of channel c whose final sum differs from n v (a sample clipped); every block of the image counts,
 *     filled ones included; c is a channel of the call's images as given (a swap_rb job: R, G, B).
 * In a whole-image call the pass runs on the quantised image on the device behind the paste (overwrite, quantise or blend, and
 * the untiled image) and in front of the R / B exchange back, the post-process, the mask and the copy out: a masked call is
 * mask(pp(consistency(door(fill(img)), fill(img)))).  With a post-process the product is consistent BEFORE it: the crop-visibility
 * step changes radiometry on purpose.  The uint16 image left on the device for s2sr_display_*_u16 is the consistent one.  The
 * result does not depend on the chunk plan.  The fp32 images are the net's own output and are not offered; s2sr/dist.py's cut /
 * stitch entries do not run the pass; a saturated block stays inexact (no redistribution among its unclipped samples).
 * s2sr_consistency_u8 / _u16: the pass alone, host images in and out (out may be sr), no weights needed; band_rows (0: the library's
 *   choice, ~32 MB) sets the bands of output rows it works in, and the result does not depend on it.
 * Every handle takes the pass: x4, x2plus (odd H or W too) and compact.
 * S2SR_E_INVALID with a text, before the device is touched: a mode outside 1..2, S outside {2, 4}, band_rows < 0, a NULL image or
 * output, a bad range.  The handle keeps working afterwards. */
#define S2SR_CONSISTENCY_EXACT  1
#define S2SR_CONSISTENCY_SMOOTH 2
int  s2sr_consistency_u8(s2sr_handle* h, const uint8_t* sr /* [S H, S W, 3] */, const uint8_t* img /* [H, W, 3] */, int32_t H, int32_t W,
                         int32_t S, int32_t mode, int32_t band_rows, uint8_t* out, uint64_t* inexact /* [3] or NULL */);
int  s2sr_consistency_u16(s2sr_handle* h, const uint16_t* sr, const uint16_t* img, int32_t H, int32_t W, int32_t S, int32_t lo, int32_t hi,
                          int32_t mode, int32_t band_rows, uint16_t* out, uint64_t* inexact /* [3] or NULL */);

/* ---- The whole-image door.  ONE record describes a call and s2sr_enhance runs it: RealESRGAN.enhance incl. the whole / tiled
 * switch and _tile_process (cnn_super_resolution.py:217-280) with the options that are on.  Every option is a field; its contract
 * stands once, at the field or in the block above that the field names.  With every option on a call's bytes are
 * mask(pp(consistency(door(fill(img))))): fill, R / B exchange, the net and the paste, the consistency pass, the exchange back, the
 * post-process, the mask.  Which records exist is stated in one place (engine_aoi.hip check_call), each refusal S2SR_E_INVALID with a
 * text in s2sr_last_error before the device is touched, and the handle keeps working afterwards:
 *   size != sizeof(s2sr_enhance_args); bits not 8 or 16; no image, no output at all, H, W, tile <= 0 or pad < 0;
 *   bits 16 with prm or swap_rb; bits 16 on a scale-2 or S2SR_ARCH_COMPACT handle, or with a bad range;
 *   force_tiled with anything but an 8-bit image, out_f32 alone and every option off;
 *   bits 8 with out and out_f32 both and blend == 0;
 *   out_f32 with prm, swap_rb, mask or consistency (the float image is the net's own output);
 *   a mask with valid NULL, radius outside 1..64 or out_nodata outside the sample range; a consistency outside 0..2; bad prm.
 * Everything else is a union of independent options and runs, also where no form below spells it (prm without swap_rb, blend, mask
 * or consistency: the post-process on the plain door's image in the order given). */
typedef struct s2sr_enhance_args {
    uint32_t size;              /* sizeof(s2sr_enhance_args); anything else is refused */
    int32_t  bits;              /* 8: img is uint8 [H,W,3] -> out uint8 [S H, S W, 3], S = s2sr_config.scale, channel order as given,
                                 * quantised by the reference's truncation.  Scale 2: H, W >= 2, even tile; the whole / tiled
                                 * switch compares the padded size.
                                 * 16: img is uint16 [H,W,3] -> out uint16 [4H,4W,3] and / or out_f32 (the 16-bit rule above): the
                                 * whole / tiled switch, the window plan and the paste order of 8 bits.  The windows leave the net as
                                 * fp32 tiles (12 B per output pixel written and read again, against 3), one chunk of window rows
                                 * at a time; a fused crop + paste + quantise kernel writes each chunk's band of final rows. */
    const void* img;
    int32_t  H, W, tile, pad;
    int32_t  lo, hi;            /* bits 16: the value range; bits 8: ignored */
    const s2sr_pp_params* prm;  /* or NULL.  bits 8: the crop-visibility post-process on the stitched image, in the order given */
    int32_t  swap_rb;           /* != 0, bits 8: the device work of one /api/wow or /api/sr job (apply_wow_sr, wow_sr.py:85-110;
                                 * apply_farm_sr, farm_sr.py:156-178): RGB image in -> cvtColor RGB2BGR -> RealESRGAN.enhance ->
                                 * BGR2RGB -> the crop-visibility post-process (prm; NULL: none) -> RGB image out.  Same bytes as the
                                 * plain call on the swapped image followed by s2sr_postprocess_u8; one upload and one download
                                 * instead of three round trips and two host-side channel flips of the 16x image. */
    int32_t  blend;             /* != 0: the seam-blended paste (above) */
    int32_t  force_tiled;       /* != 0: RealESRGAN._tile_process alone (cnn_super_resolution.py:236-280): always the window plan,
                                 * whatever the image size; HWC fp32 out (unquantised) */
    const s2sr_mask* mask;      /* or NULL: not masked.  Fill before the net, out_nodata behind everything (above) */
    int32_t  consistency;       /* 0: off, S2SR_CONSISTENCY_* (above) */
    void*    out;               /* the quantised image (uint8 / uint16 [S H, S W, 3]) or NULL */
    float*   out_f32;           /* the float image before quantisation (HWC fp32 [S H, S W, 3]) or NULL */
    uint64_t* inexact;          /* [3] or NULL; read only when consistency != 0 */
} s2sr_enhance_args;
int  s2sr_enhance(s2sr_handle* h, const s2sr_enhance_args* a);

/* The forms: the signatures from before the record, kept for callers that bind them.  Each builds the record below (what it does not
 * name is 0 / NULL) and runs s2sr_enhance's code, with its own words for a missing image, size or output.
 *   s2sr_enhance_u8             bits 8, out
 *   s2sr_enhance_job_u8         bits 8, out, swap_rb 1, prm
 *   s2sr_enhance_f32            bits 8, out_f32
 *   s2sr_tile_process_f32       bits 8, out_f32, force_tiled 1
 *   s2sr_enhance_u16            bits 16, lo, hi, out and / or out_f32
 *   s2sr_enhance_blend_u8       bits 8, blend 1, prm, swap_rb, out and / or out_f32; img NULL is refused by name
 *   s2sr_enhance_blend_u16      bits 16, lo, hi, blend 1, out and / or out_f32; img NULL is refused by name
 *   s2sr_enhance_masked_u8      bits 8, prm, swap_rb, blend, mask m, out; m NULL is refused
 *   s2sr_enhance_masked_u16     bits 16, lo, hi, blend, mask m, out; m NULL is refused
 *   s2sr_enhance_consistent_u8  bits 8, prm, swap_rb, blend, mask m (or NULL), consistency mode, out, inexact; a mode outside 1..2 is refused
 *   s2sr_enhance_consistent_u16 bits 16, lo, hi, blend, mask m (or NULL), consistency mode, out, inexact; a mode outside 1..2 is refused */
int  s2sr_enhance_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, uint8_t* out);
int  s2sr_enhance_job_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, int32_t tile, int32_t pad,
                         const s2sr_pp_params* prm, uint8_t* out_rgb);
int  s2sr_enhance_f32(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, float* out);
int  s2sr_tile_process_f32(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, float* out);
int  s2sr_enhance_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo, int32_t hi,
                      uint16_t* out_u16 /* or NULL */, float* out_f32 /* or NULL */);
int  s2sr_enhance_blend_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad,
                           const s2sr_pp_params* prm /* or NULL */, int32_t swap_rb, uint8_t* out_u8 /* or NULL */,
                           float* out_f32 /* or NULL */);
int  s2sr_enhance_blend_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo,
                            int32_t hi, uint16_t* out_u16 /* or NULL */, float* out_f32 /* or NULL */);
int  s2sr_enhance_masked_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad,
                            const s2sr_pp_params* prm /* or NULL */, int32_t swap_rb, int32_t blend, const s2sr_mask* m, uint8_t* out_u8);
int  s2sr_enhance_masked_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo,
                             int32_t hi, int32_t blend, const s2sr_mask* m, uint16_t* out_u16);
int  s2sr_enhance_consistent_u8(s2sr_handle* h, const uint8_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad,
                                const s2sr_pp_params* prm /* or NULL */, int32_t swap_rb, int32_t blend, const s2sr_mask* m /* or NULL */,
                                int32_t mode, uint8_t* out_u8, uint64_t* inexact /* [3] or NULL */);
int  s2sr_enhance_consistent_u16(s2sr_handle* h, const uint16_t* img, int32_t H, int32_t W, int32_t tile, int32_t pad, int32_t lo,
                                 int32_t hi, int32_t blend, const s2sr_mask* m /* or NULL */, int32_t mode, uint16_t* out_u16,
                                 uint64_t* inexact /* [3] or NULL */);

/* Display rendering of a 16-bit image: the two passes over a uint16 [H, W, 3] interleaved image that reduce it to
 * the 8-bit image the PNG writer, the warp, the pyramid and the post-process take.  Neither entry needs weights.  What lies between
 * them -- percentile limits from the histogram, the stretch LUT -- is the caller's (s2sr/display.py).
 * hist:  hist[c][v] = the exact number of samples of channel c with value v, the samples equal to nodata (0..65535; -1: none)
 *   left out.
 * apply: out[y, x, c] = lut[c][img[y, x, c]], lut = uint8 [3][65536].
 * img == NULL in either entry: the uint16 image of exactly H x W that the previous call on this handle left on the device -- the
 *   uploaded copy of a host-image display call, or the x4 image of s2sr_enhance_u16 / s2sr_enhance_blend_u16 called with out_u16
 *   (pass their 4H, 4W).  Any other call on the handle in between invalidates the copy.
 * band_rows (0: the library's choice, ~32 MB) sets the row bands the passes work in; for a host image band i + 1 uploads under
 *   band i's kernel and band i's output leaves under band i + 1's.  The result does not depend on it.
 * Limits: a row holds at most 2^30 samples (W <= 357913941); counts are 64 bits wide and exact for every image.
 * S2SR_E_INVALID with a text, before the device is touched: nodata outside -1..65535, non-positive H or W, band_rows < 0, a NULL
 * hist / lut / out, and img == NULL without a device image of that size. */
int  s2sr_display_hist_u16(s2sr_handle* h, const uint16_t* img /* or NULL */, int32_t H, int32_t W, int32_t nodata, int32_t band_rows,
                           uint64_t* hist /* [3][65536] */);
int  s2sr_display_apply_u16(s2sr_handle* h, const uint16_t* img /* or NULL */, int32_t H, int32_t W, const uint8_t* lut /* [3][65536] */,
                            int32_t band_rows, uint8_t* out /* [H,W,3] */);

/* Carrying an extra band to the SR grid: a uint16 band [H, W] the net never saw (NIR, red edge) is upsampled S
 * times against the uint16 image [S H, S W, 3] a 16-bit door produced, by a local linear model (the fast guided filter), and one
 * back-projection step then makes every block mean the measured band value again.  Integers throughout; no weights needed.
 * n = S S; q the guide; w the guide weights (0..255 each, Wt their sum, >= 1); p = clamp(band, lo, hi), lo < hi the band's own range.
 *   guide:  I[Y, X] = floor((w0 q0 + w1 q1 + w2 q2) / Wt) over the guide's channels as stored; G[y, x] = floor(blocksum(I) / n).
 *   coefficients, one pair per valid input pixel, from sums over the valid pixels of the window [y - r, y + r] x [x - r, x + r] cut
 *     at the image border: N (their number), SG, Sp, SGG, SGp; cov = N SGp - SG Sp, var = N SGG - SG SG;
 *     A = clamp(floor((cov << 16) / (var + N N eps)), -(4 << 16), 4 << 16) (Q16, gain limit 4); C = floor(((Sp << 16) - A SG) / N).
 *   apply:  A and C interpolated bilinearly between input-pixel centres with the consistency pass's weights (above), an invalid
 *     neighbour replaced by the pixel itself; Abar, Cbar the undivided weighted sums, den = 4 S S;
 *     g0 = floor((Abar I + Cbar + (den << 15)) / (den << 16)), g = clamp(g0, lo, hi).
 *   exact step: the consistency pass's, towards n p: e = n p - blocksum(g), k = floor(e / n), rr = e - n k, sample (i, j) gets
 *     k + (rank[i][j] < rr), clamped to [lo, hi].
 *   valid (uint8 [H, W], nonzero = valid; NULL: every pixel): invalid pixels take no part in any sum, their blocks are written `fill`.
 *   inexact = the valid blocks whose final sum differs from n p (a sample clipped at lo or hi).
 * sr == NULL: the uint16 image of exactly S H x S W that the previous call on this handle left on the device (s2sr_enhance_u16 and
 *   its kin, a display call, another carried band).  The call leaves that image intact and names it kept again at its end, a host
 *   sr's upload likewise: several bands, and a display call afterwards, read one copy.
 * band_rows (0: the library's choice, ~32 MB of guide) sets the bands of guide rows the call works in; the coefficients trail the
 *   upload by r input rows, the output the coefficients by one more.  The result does not depend on it.
 * S2SR_E_INVALID with a text, before the device is touched: S outside {2, 4}, r outside 1..4, eps < 1, a range that is not
 * 0 <= lo < hi <= 65535, a weight outside 0..255 or all weights zero, fill outside 0..65535, band_rows < 0, a NULL band or out,
 * non-positive H or W, and sr == NULL without a device image of that size.  The handle keeps working afterwards. */
int  s2sr_carry_band_u16(s2sr_handle* h, const uint16_t* sr /* [S H, S W, 3] or NULL */, const uint16_t* band /* [H, W] */, int32_t H, int32_t W,
                         int32_t S, int32_t lo, int32_t hi, const int32_t* w /* [3] */, int32_t r, int32_t eps,
                         const uint8_t* valid /* [H, W] or NULL */, int32_t fill, int32_t band_rows, uint16_t* out /* [S H, S W] */,
                         uint64_t* inexact /* or NULL */);

/* Normalised-difference indices on one grid: NDVI, NDWI, NDRE, SAVI and their kin from two uint16 planes, with the
 * rendering, the histogram and per-zone sums out of the same read.  Integers throughout; no weights needed.
 *   a' = max(a - offset, 0), b' = max(b - offset, 0), n = a' - b', d = a' + b' + L
 *   v  = sign(n) floor((2 |n| K + d) / (2 d)) for d > 0 (round half away from zero; |v| <= K), -32768 (nodata) for d == 0
 *   offset 0..65535 (the DN offset of both planes), L 0..65535 (the soil term in DN), K 1..16383 (the output scale).
 * a, b: uint16 [H, W, ac] / [H, W, bc] with ac, bc 1 or 3; ca, cb the channel read.  a == NULL: channel ca of the uint16 image of
 *   exactly H x W x 3 that the previous call on this handle left on the device (as s2sr_carry_band_u16 takes sr == NULL); the call
 *   leaves that image intact and names it kept again at its end.
 * valid: uint8 [ceil(H / valid_scale)][ceil(W / valid_scale)] or NULL; a pixel whose cell is 0 gets -32768.
 * undefined: the unmasked pixels with d == 0.
 * out_i16: int16 [H, W].  hist: uint64 [2 K + 1], hist[v + K] = the pixels of value v, nodata left out.
 * rgba: uint8 [H, W, 4] = lut[(uint16)(v + 32768)], lut uint8 [65536][4]; a nodata pixel is 0, 0, 0, 0 whatever the LUT holds.
 * zones: uint16 labels [ceil(H / zone_scale)][ceil(W / zone_scale)], 0 = no zone, 1..Z (Z <= 65535; a label above Z counts as 0);
 *   zonal: int64 [Z + 1][3] = count, sum v, sum v^2 over the defined pixels of each label, row 0 the pixels without a zone.
 * Every output may be NULL, not all of them.  band_rows (0: the library's choice) sets the row bands; the result does not depend on it.
 * S2SR_E_INVALID with a text, before the device is touched: K, L, offset or Z out of range, ac or bc not 1 or 3, a channel outside
 * its image, valid_scale or zone_scale < 1, zonal without zones or zones without zonal, rgba without lut, every output NULL, a NULL
 * b, non-positive H or W, H W >= 2^31, band_rows < 0, and a == NULL without a device image of that size.  The handle keeps working. */
int  s2sr_index_nd_u16(s2sr_handle* h, const uint16_t* a /* [H, W, ac] or NULL */, int32_t ac, int32_t ca, const uint16_t* b /* [H, W, bc] */,
                       int32_t bc, int32_t cb, int32_t H, int32_t W, int32_t offset, int32_t L, int32_t K, const uint8_t* valid /* or NULL */,
                       int32_t valid_scale, const uint16_t* zones /* or NULL */, int32_t zone_scale, int32_t Z,
                       const uint8_t* lut /* [65536][4] or NULL */, int32_t band_rows, int16_t* out_i16 /* or NULL */,
                       uint64_t* hist /* or NULL */, int64_t* zonal /* or NULL */, uint8_t* rgba /* or NULL */, uint64_t* undefined /* or NULL */);
/* The same mapping for an index raster that already exists: rgba[y, x] = lut[(uint16)(idx[y, x] + 32768)], -32768 -> 0, 0, 0, 0. */
int  s2sr_index_render_i16(s2sr_handle* h, const int16_t* idx /* [H, W] */, int32_t H, int32_t W, const uint8_t* lut /* [65536][4] */,
                           int32_t band_rows, uint8_t* rgba /* [H, W, 4] */);

/* Polygons to zone labels: the label raster the `zones` of s2sr_index_nd_u16 takes, rasterised from features made
 * of rings.  Integers throughout; no weights needed.
 *   The label grid is H x W.  Coordinates are int32 in 1/256 of a label pixel, x along columns, y along rows, from the grid's
 *   top-left corner, |x|, |y| <= 2^29 (every product below then fits int64); the centre of pixel (r, c) is
 *   (cx, cy) = (256 c + 128, 256 r + 128).
 *   A feature is a list of rings, a ring a closed list of at least 3 vertices (the edge last -> first is implied).  Holes, the
 *   parts of a MultiPolygon and self-intersections need no special case, and winding does not matter:
 *   an edge, its endpoints exchanged so that ya < yb (ya == yb: it never counts), counts for a centre iff
 *     ya <= cy < yb  and  (cx - xa) (yb - ya) < (xb - xa) (cy - ya)
 *   (the row test is half-open, the centre lies strictly left of the crossing), and a centre is inside a feature iff the count
 *   over all edges of all its rings is odd.  Per row: with dy = yb - ya and N = (xb - xa) (cy - ya) + (xa - 128) dy the edge
 *   toggles exactly the columns c < k, k = clamp(ceil(N / (256 dy)), 0, W).
 *   Feature f carries label[f] in 1..Z; several may share one.  Where several features hold a centre the one latest in the list
 *   wins (burn order); a pixel no feature holds is 0.
 * xy: int32 [V][2] (x, y); ring_start: int32 [R + 1] into xy; feat_start: int32 [F + 1] into the rings (R = feat_start[F],
 *   V = ring_start[R]); label: uint16 [F].
 * out: uint16 [H, W].  area: uint64 [Z + 1] or NULL: the pixels per label, row 0 the unlabelled ones; its sum is H W.
 * band_rows (0: the library's choice) sets the row bands the labels leave in; the result does not depend on it, nor on the number
 *   of workgroups or on which stream runs first.
 * The call requests scratch, so it voids whatever the call before it kept on the device (a uint16 image, a raster, a level), and it
 *   keeps nothing itself: the labels go to the host, and s2sr_index_nd_u16 takes them from there.  A job calls it in front of the net.
 * S2SR_E_INVALID with a text, before the device is touched: non-positive H or W, H W >= 2^31, F < 1, Z outside 1..65535, a label
 * of 0 or above Z, start tables that are not non-decreasing from 0, a ring of fewer than 3 vertices, a coordinate outside +-2^29, a
 * NULL table or out, band_rows < 0, and features that meet more than 2^31 - 1 tiles of 64 x 64 pixels in all.  The handle keeps working. */
int  s2sr_zones_rasterize_u16(s2sr_handle* h, const int32_t* xy /* [V][2] */, const int32_t* ring_start /* [R + 1], into xy */,
                              const int32_t* feat_start /* [F + 1], into the rings */, const uint16_t* label /* [F] */, int32_t F, int32_t Z,
                              int32_t H, int32_t W, int32_t band_rows, uint16_t* out /* [H, W] */, uint64_t* area /* [Z + 1] or NULL */);

/* Fields from the image: the inverse of s2sr_zones_rasterize_u16.  An index raster is thresholded, cleaned and
 * split into connected components; the components are the zone labels.  Integers throughout; no weights needed.
 *   idx: int16 [H, W], -32768 = nodata: the raster s2sr_index_nd_u16 writes.  H W < 2^31.
 *   1. mask        m0 = idx != -32768 and lo <= idx <= hi          (lo <= hi, both in -32767..32767)
 *   2. morphology  binary, the (2 r + 1) x (2 r + 1) square as the element (r_open, r_close in 0..8).  Erode is the AND, dilate the
 *                  OR over the neighbours that lie INSIDE the image: out-of-image neighbours take no part, so a field at the
 *                  raster's edge does not shrink.  open = dilate(erode(m0, r_open), r_open), close = erode(dilate(open, r_close),
 *                  r_close), m = close and idx != -32768: a label never lies on a nodata pixel.  r = 0: the identity.
 *   3. components  of m under conn (4 or 8).  A component's key is the smallest linear index y W + x among its pixels, its size its
 *                  pixel count.  Components smaller than min_pixels (>= 1) become 0; the rest are numbered 1, 2, ... by ascending
 *                  key; found is how many remain.  A component whose number exceeds Z (1..65535) is written as 0; found still
 *                  counts it, so the caller can tell.
 *   labels: uint16 [H, W].  fields: int64 [Z + 1][6] = pixels, key, x0, y0, x1, y1 (the bounding box, half-open); row 0 holds the
 *   unlabelled pixel count and zeros; rows above min(found, Z) are zero; the pixels column sums to H W.
 * Nothing depends on the order of atomics, on the row bands the rasters travel in, on the number of workgroups or on which stream
 * runs first.
 * The call requests scratch, so it voids whatever the call before it kept on the device (a uint16 image, a raster, a level), and it
 *   keeps nothing itself: labels and fields go to the host, and s2sr_index_nd_u16 takes the labels from there.
 * S2SR_E_INVALID with a text, before the device is touched: lo > hi or either outside -32767..32767, a radius outside 0..8, conn
 * other than 4 or 8, min_pixels < 1, Z outside 1..65535, a NULL idx or labels, non-positive H or W, H W >= 2^31.  The handle keeps
 * working. */
int  s2sr_fields_segment_i16(s2sr_handle* h, const int16_t* idx /* [H, W] */, int32_t H, int32_t W, int32_t lo, int32_t hi, int32_t r_open,
                             int32_t r_close, int32_t conn, int64_t min_pixels, int32_t Z, uint16_t* labels /* [H, W] */,
                             int64_t* fields /* [Z + 1][6] or NULL */, uint64_t* found /* or NULL */);
/* Labels to rings (host code: csrc/ring_trace.h): the polygons around the labels 1..Z of a uint16 raster, in pixel corners (pixel
 * (r, c) covers x in [c, c + 1], y in [r, r + 1]).
 *   The boundary of label l is the set of unit pixel edges between a pixel of l and anything else; the image border counts as
 *   anything else.  Each edge is directed so that l's pixel lies on its left as seen on screen: exterior rings run counterclockwise
 *   on a north-up map (RFC 7946), holes clockwise.  At a corner with two ways on the walk turns left: pixels of l that touch only
 *   diagonally get rings of their own that touch.  By the same rule everything else is 8-connected, so a ring MAY TOUCH ITSELF at
 *   a corner: two holes of one label that meet at a corner are ONE ring that passes through that corner twice, and a hole that
 *   meets the outside at a corner is a notch of the exterior ring, which touches itself there.  No ring crosses itself or runs
 *   along itself, every ring turns at every vertex, and under the even-odd rule of s2sr_zones_rasterize_u16 the rings of a label
 *   burn back to exactly its pixels.  A caller that needs OGC-simple rings splits a ring at its repeated vertices.
 *   Collinear vertices are dropped; a ring starts at its smallest (y, x) vertex (never a touching corner) and is not closed (the edge last -> first is implied, as s2sr_zones_rasterize_u16 takes it); rings are ordered by label,
 *   then by start vertex.  Label 0 and labels above Z are not traced.
 * counts: uint64 [2] = vertices, rings: always filled.  xy: int32 [xy_cap][2] (x, y); ring_start: int32 [ring_cap + 1] into xy;
 * ring_label: uint16 [ring_cap].  The tables are written only if both capacities suffice (and none is NULL), so a caller sizes them
 * with a first call at capacity 0.  S2SR_E_INVALID: a NULL labels or counts, non-positive H or W, H W >= 2^31, Z outside 1..65535,
 * more than 2^31 - 1 vertices.  Touches no device. */
int  s2sr_labels_trace_u16(s2sr_handle* h, const uint16_t* labels /* [H, W] */, int32_t H, int32_t W, int32_t Z, uint64_t xy_cap, uint64_t ring_cap,
                           int32_t* xy, int32_t* ring_start, uint16_t* ring_label, uint64_t* counts /* [2] */);
/* test hook: what the stages of the last s2sr_fields_segment_i16 on this handle took by HIP events.  The pass's launches share the
 * statistics family "index"; with profiling on (s2sr_set_profiling(h, 1): every launch bracketed) each launch's event pair is also
 * booked to its stage.  ms, launches: S2SR_FIELDS_STAGES entries, in the order of the S2SR_FIELDS_STAGE_* below; all zero when the
 * last call ran with profiling off (with every_n > 1 only the sampled launches count).  Touches no device beyond reading event times. */
#define S2SR_FIELDS_STAGES 8
#define S2SR_FIELDS_STAGE_MASK 0      /* the mask, the morphology's passes, the nodata mask behind them */
#define S2SR_FIELDS_STAGE_LOCAL 1     /* the tiles' union-find */
#define S2SR_FIELDS_STAGE_BORDER 2    /* the unions across the tile lines */
#define S2SR_FIELDS_STAGE_FLATTEN 3   /* parents to roots, sizes to roots */
#define S2SR_FIELDS_STAGE_COUNT 4     /* numbering: the chunks' flags */
#define S2SR_FIELDS_STAGE_SCAN 5      /* numbering: the one-workgroup scan of the chunk sums */
#define S2SR_FIELDS_STAGE_APPLY 6     /* numbering: ranks to the roots, pixels and key to fields */
#define S2SR_FIELDS_STAGE_LABELS 7    /* labels and boxes */
int  s2sr_debug_fields_stage_ms(s2sr_handle* h, double* ms /* [S2SR_FIELDS_STAGES] */, int32_t* launches /* [S2SR_FIELDS_STAGES] */);

/* Touching fields split: s2sr_fields_segment_i16 with the blobs of several parcels cut apart.  Two vegetated
 * parcels with no bare pixel between them, or joined by a bridge the close built, are one component of the mask; here every
 * component is split around the cores of its distance transform, optionally after field boundaries found as a gradient ridge of
 * the index were taken out.  Integers throughout, order-free; no weights needed.  All arguments up to Z are s2sr_fields_segment_i16's.
 *   1. mask      m: steps 1 and 2 of s2sr_fields_segment_i16, unchanged.
 *   2. interior  I = m when edge == 0.  Otherwise, for every pixel p that is not nodata: B(p) is the sum over the (2 edge_r + 1)^2 box
 *                around p of idx[q], where a q outside the image or a nodata q contributes idx[p] instead; gx and gy are the
 *                unnormalised 3 x 3 Sobel sums of B, where a neighbour outside the image or a nodata neighbour contributes B(p); p is
 *                an edge pixel iff gx^2 + gy^2 > (8 n T)^2 with n = (2 edge_r + 1)^2 and T = edge, in index units (of 1 / K) per
 *                pixel.  int64 arithmetic: everything stays below 2^50.  I = m minus the edge pixels.
 *   3. distance  for p in I, D2(p) = min(255^2, min |p - q|^2 over the pixels q of the image that are not in I); elsewhere D2 = 0: the
 *                exact squared Euclidean distance, capped.  Pixels beyond the image take no part, as in the morphology: a field on
 *                the raster's edge does not thin out there.
 *   4. cores     take the components of I under conn; Dmax2 is the largest D2 in a component.  A pixel of I is a core pixel iff
 *                Dmax2 < core_px^2 (the whole component is then one core), or else iff D2 >= core_px^2 and
 *                1000000 D2 >= core_q^2 Dmax2.  Every component of I therefore holds a core.
 *   5. markers   the components of the core pixels under conn.  A marker's key is its smallest linear index y W + x.
 *   6. growth inside I         every pixel of I goes to the marker with the smallest pair (number of conn-steps of the shortest path
 *                inside I, marker key).
 *   7. growth over the edges   every pixel of m \ I goes to the owner with the smallest pair (steps of the shortest path that runs
 *                through m \ I and starts on any pixel of I, marker key of that pixel's owner); a pixel of I from which several
 *                paths start counts with its own owner.  A pixel of m \ I that no such path reaches gets label 0.
 *   8. fields    a field is the set of pixels of one owner.  Its key is the smallest linear index among ITS pixels (not the
 *                marker's).  Size, min_pixels, numbering by ascending key, Z, found and the fields table are exactly as in step 3 of
 *                s2sr_fields_segment_i16.
 *   labels, fields, found: as s2sr_fields_segment_i16.  dist2: uint16 [H, W] or NULL, receives D2.  cores: uint8 [H, W] or NULL,
 *   receives 1 on core pixels and 0 elsewhere.
 * split == NULL gives the bytes of s2sr_fields_segment_i16 (dist2 and cores are then left alone); so does {core_q 1, core_px 0,
 * edge 0}, because every pixel of m is then a core.  Nothing depends on the order of atomics, on the row bands the rasters travel in,
 * on the number of workgroups or on which stream runs first.
 * The call requests scratch, so it voids whatever the call before it kept on the device, and it keeps nothing itself.
 * S2SR_E_INVALID with a text, before the device is touched: every refusal of s2sr_fields_segment_i16, core_q outside 1..1000,
 * core_px outside 0..255, edge outside 0..32767, edge_r outside 0..4.  The handle keeps working. */
typedef struct s2sr_fields_split {
    int32_t core_q;    /* 1..1000: a core pixel lies at >= core_q / 1000 of its interior component's largest distance */
    int32_t core_px;   /* 0..255: and at >= core_px pixels from the interior's outside */
    int32_t edge;      /* 0: no edge test; 1..32767: T, index units (of 1 / K) per pixel */
    int32_t edge_r;    /* 0..4: radius of the box sum in front of the Sobel */
} s2sr_fields_split;
int  s2sr_fields_split_i16(s2sr_handle* h, const int16_t* idx /* [H, W] */, int32_t H, int32_t W, int32_t lo, int32_t hi, int32_t r_open,
                           int32_t r_close, int32_t conn, int64_t min_pixels, int32_t Z,
                           const s2sr_fields_split* split /* NULL: exactly s2sr_fields_segment_i16 */, uint16_t* labels /* [H, W] */,
                           int64_t* fields /* [Z + 1][6] or NULL */, uint64_t* found /* or NULL */, uint16_t* dist2 /* [H, W] or NULL */,
                           uint8_t* cores /* [H, W] or NULL */);
/* test hook: what the stages of the last s2sr_fields_split_i16 with a split on this handle took by HIP events, as
 * s2sr_debug_fields_stage_ms does for the plain segmentation (which keeps its own hook): S2SR_FSPLIT_STAGES entries in the order
 * below, all zero when the last call ran with profiling off.  rounds: int32 [2], the launches the growth inside I and the growth
 * over the edge pixels took until one changed nothing (the last one included; 0 for a growth that did not run), filled always. */
#define S2SR_FSPLIT_STAGES 7
#define S2SR_FSPLIT_EDGE 0            /* the mask and its morphology, the edge test: the interior */
#define S2SR_FSPLIT_DISTANCE 1        /* the column pass and the row pass */
#define S2SR_FSPLIT_CORES 2           /* components of the interior, maxima, the core test, components of the cores, the seeds */
#define S2SR_FSPLIT_GROW_INTERIOR 3   /* the rounds of the growth inside I */
#define S2SR_FSPLIT_GROW_EDGES 4      /* the restart and the rounds of the growth over the edge pixels */
#define S2SR_FSPLIT_REMAP 5           /* field keys, parents and sizes */
#define S2SR_FSPLIT_NUMBERING 6       /* count, scan, apply, labels */
int  s2sr_debug_fields_split_stage_ms(s2sr_handle* h, double* ms /* [S2SR_FSPLIT_STAGES] */, int32_t* launches /* [S2SR_FSPLIT_STAGES] */,
                                      int32_t* rounds /* [2] */);

/* Management zones: integer k-means inside every field.  The pixels of each label of a uint16 raster are split
 * into k classes by their values in D index rasters; the classes are ranked by the first raster, so zone 1 is the lowest.  Integers
 * throughout; no weights needed.
 *   feat: int16 [D][H][W], -32768 = nodata, D in 1..4 (the rasters s2sr_index_nd_u16 writes).  labels: uint16 [H][W], 0 = no field,
 *   1..Z (Z in 1..65535), a label above Z counts as 0.  H W < 2^31.  k in 2..8, iters in 1..64, min_per_zone >= 1, smooth in 0..4.
 *   1. members     a pixel is a member of field l if its label is l in 1..Z and none of its D values is -32768.  Every other pixel
 *                  gets zone 0 and is counted nowhere.
 *   2. statistics  per field the member count n_l and per feature the member minimum lo_d and maximum hi_d.  A field with
 *                  n_l < k min_per_zone is SKIPPED: its pixels get zone 0, its status is 1, its table and centre rows are zero.
 *   3. start       c[j][d] = lo_d + ((2 j + 1) (hi_d - lo_d)) / (2 k), j = 0..k-1: on the diagonal of the field's bounding box.
 *   4. iteration   each member goes to the j with the smallest sum_d (v_d - c[j][d])^2 (exact: a term is below 2^32, the sum below
 *                  2^35), a tie to the smallest j.  Per (field, j) the count n and the sums s_d are taken in int64.  A cluster
 *                  with n > 0 gets the centre sign(s_d) ((2 |s_d| + n) / (2 n)): rounded half away from zero.  An empty cluster
 *                  keeps its centre.
 *   5. the run     iters iterations.  An iteration that changes no centre of any field is a fixed point; the library stops there,
 *                  because the bytes are the same.  iterations is the number of the first such iteration, counted from 1, or iters
 *                  if none came: a defined output.
 *   6. zones       the members are assigned once more to the final centres.  A field's clusters are ranked by (c[j][0], j)
 *                  ascending; the zone id is 1 + rank.  An empty cluster keeps its rank: a zone id may have no pixel.  A field
 *                  whose values are all equal ends with every member in zone 1.
 *   7. smoothing   smooth Jacobi passes, each reading the previous raster.  For a pixel of zone > 0 the zone ids are counted among
 *                  the at most 9 pixels of its 3 x 3 neighbourhood that lie inside the image, carry the same label and have
 *                  zone > 0 (itself included).  The new zone is the id with the most votes; the pixel keeps its own id if that is
 *                  among the tied, otherwise it takes the smallest tied id.  Zone 0 stays 0.
 *   zone: uint8 [H][W].  table: int64 [Z + 1][k][1 + 2 D], row [l][z - 1] = the pixels of zone z of field l in the FINAL raster
 *   (after smoothing), then per feature the sum of v_d and the sum of v_d^2 (pixels, s_0, q_0, s_1, q_1, ...); row 0 and the rows of
 *   skipped or absent fields are zero.  centres: int32 [Z + 1][k][D], the final centres in zone order, zero for skipped or absent
 *   fields.  status: uint8 [Z + 1]: 0 absent (no member), 1 skipped, 2 zoned.  iterations: see 5.
 *   band_rows: the rows per band the rasters travel and the pixel passes run in (0: the library's choice).
 * Nothing depends on the order of atomics, on the row bands or on the number of workgroups: every sum is an integer add, every
 * statistic an integer minimum or maximum.
 * The call requests scratch, so it voids whatever the call before it kept on the device (a uint16 image, a raster, a level), and it
 *   keeps nothing itself.
 * S2SR_E_INVALID with a text, before the device is touched: D outside 1..4, k outside 2..8, iters outside 1..64, smooth outside
 * 0..4, Z outside 1..65535, min_per_zone < 1, a NULL feat, labels or zone, non-positive H or W, H W >= 2^31, band_rows < 0.  The
 * handle keeps working. */
int  s2sr_zones_kmeans_i16(s2sr_handle* h, const int16_t* feat /* [D][H][W] */, int32_t D, int32_t H, int32_t W,
                           const uint16_t* labels /* [H][W] */, int32_t Z, int32_t k, int32_t iters, int64_t min_per_zone, int32_t smooth,
                           int32_t band_rows, uint8_t* zone /* [H][W] */, int64_t* table /* [Z+1][k][1+2D] or NULL */,
                           int32_t* centres /* [Z+1][k][D] or NULL */, uint8_t* status /* [Z+1] or NULL */, uint32_t* iterations /* or NULL */);
/* test hook: what the stages of the last s2sr_zones_kmeans_i16 on this handle took by HIP events, as s2sr_debug_fields_stage_ms
 * does for the segmentation: S2SR_MZONES_STAGES entries in the order below, all zero when the last call ran with profiling off. */
#define S2SR_MZONES_STAGES 5
#define S2SR_MZONES_STATISTICS 0      /* the tables cleared, the statistics band by band, status and the start centres */
#define S2SR_MZONES_ITERATIONS 1      /* assign-and-accumulate and the centre update, once per iteration run */
#define S2SR_MZONES_ASSIGN 2          /* the rank map and the final assignment */
#define S2SR_MZONES_SMOOTHING 3       /* the mode filter's passes */
#define S2SR_MZONES_TABLE 4           /* the sums of the final raster */
int  s2sr_debug_mzones_stage_ms(s2sr_handle* h, double* ms /* [S2SR_MZONES_STAGES] */, int32_t* launches /* [S2SR_MZONES_STAGES] */);

/* Multi-GPU building blocks of _tile_process (cnn_super_resolution.py:244-278), device-resident:
 * cut windows [first, first+count) of the plan into d_tiles [count, wh, ww, 3] (wh/ww = the
 * plan's common window size), and paste ALL T windows' outputs d_tiles [T, 4wh, 4ww, 3] into
 * d_out [4H, 4W, 3] with the reference's crop + overwrite order.  Scale 2: the plan of the padded image at scale 2 (odd H or W:
 * the cut reads the reflect row / column by index), [T, 2wh, 2ww, 3] into [2H, 2W, 3].  Between the two a rank runs
 * s2sr_forward_batch_u8_dev on its share and the ranks all-gather (RCCL) the outputs. */
int  s2sr_cut_windows_u8_dev(s2sr_handle* h, const void* d_img, int32_t H, int32_t W, int32_t tile, int32_t pad,
                             int32_t first, int32_t count, void* d_tiles, void* stream);
int  s2sr_stitch_windows_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t H, int32_t W, int32_t tile, int32_t pad,
                                void* d_out, void* stream);
/* The same paste for output rows [oy0, oy1) only (d_out is still the whole [4H, 4W, 3] image): a rank that receives the windows
 * chunk by chunk stitches every band as soon as the window rows that own it have arrived, and copies it out under the next
 * chunk's compute.  The plan's paste maps stay on the device between calls with the same (H, W, tile, pad). */
int  s2sr_stitch_rows_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t H, int32_t W, int32_t tile, int32_t pad,
                             int32_t oy0, int32_t oy1, void* d_out, void* stream);
/* s2sr_forward_batch_u8_dev for a PART of a job of `job_windows` (>= B) equal windows: the window mosaic and the workspace are
 * planned for the whole job, so its parts (the chunks a rank's share of an AOI is cut into) share one workspace and their
 * hipGraphs.  Same bytes as any other split. */
int  s2sr_forward_part_u8_dev(s2sr_handle* h, const void* d_tiles, int32_t B, int32_t th, int32_t tw, int32_t job_windows,
                              void* d_out, void* stream);
/* Device -> host: `bytes` from d_src into dst once everything enqueued on `stream` so far has run; returns when they are there.
 * Replaces the reference's `output.cpu()` (cnn_super_resolution.py:231) for callers that hold device buffers: a destination
 * from s2sr_host_alloc takes one DMA, a pageable one goes through pinned staging slices. */
int  s2sr_copy_to_host(s2sr_handle* h, void* dst, const void* d_src, size_t bytes, void* stream);

/* replaces _enhance_for_crops (wow_sr.py:187-209) and enhance_local_contrast /
 * apply_unsharp_mask / enhance_vegetation (farm_sr.py:61-108): HxWx3 u8 RGB -> same. */
int  s2sr_postprocess_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W,
                         const s2sr_pp_params* prm, uint8_t* out);
int  s2sr_postprocess_batch_u8_dev(s2sr_handle* h, const void* d_rgb, int32_t B, int32_t H, int32_t W,
                                   const s2sr_pp_params* prm, void* d_out, void* stream);

/* The same post-process over ONE device-resident image in row bands, for callers whose image becomes complete band by band (an
 * AOI's mosaic: the chunks of s2sr_enhance_u8, the gathers of s2sr/dist.py).  CLAHE's 8x8 grid spans the whole image
 * (wow_sr.py:191-192), so no output row exists before every input row has been counted; the split lets the counting run under
 * the compute of the windows still to come and the finishing overlap the copy out:
 *   begin  geometry, constants and channel order of the image; zeroes the histograms (allocates: call it before queueing work)
 *   hist   counts rows [y0, y1) of d_img ([H, W, 3] u8) -- any order, every row exactly once
 *   lut    clip / redistribute / CDF once all rows are counted
 *   rows   finishes rows [y0, y1) into the same rows of d_out ([H, W, 3]); bands follow each other from row 0; d_out may be d_img
 *          (a band is rewritten only after the CLAHE pass, which runs a blur radius ahead, has read it)
 * Same bytes as s2sr_postprocess_batch_u8_dev on the whole image.  order: S2SR_PP_ORDER_BGR = the bytes are B,G,R (what
 * RealESRGAN.enhance handles, wow_sr.py:85,94; the colour math is always RGB's); S2SR_PP_ORDER_SWAP_OUT = R and B exchanged in
 * the rows written (the job's cvtColor BGR2RGB, wow_sr.py:103, folded into the last pass).
 * One banded run per handle at a time, and the handle enforces it: the run's histograms, LUTs and CLAHE'd rows live in a scratch area
 * that s2sr_postprocess_u8, s2sr_postprocess_batch_u8_dev, an s2sr_enhance_job_u8 with post-process parameters, a multi-group
 * s2sr_tiles_write_png and another begin also use.  Any of them on the same handle between begin and the last rows band ends the
 * run: its next hist / lut / rows returns S2SR_E_INVALID and launches nothing (begin again). */
#define S2SR_PP_ORDER_BGR      1
#define S2SR_PP_ORDER_SWAP_OUT 2
int  s2sr_pp_band_begin_dev(s2sr_handle* h, int32_t H, int32_t W, const s2sr_pp_params* prm, int32_t order, void* stream);
int  s2sr_pp_band_hist_dev(s2sr_handle* h, const void* d_img, int32_t y0, int32_t y1, void* stream);
int  s2sr_pp_band_lut_dev(s2sr_handle* h, void* stream);
int  s2sr_pp_band_rows_dev(s2sr_handle* h, const void* d_img, int32_t y0, int32_t y1, void* d_out, void* stream);

/* ---- XYZ tile pyramid: the step after the path (reference server/app/tiling.py:102-186 shells out to
 * `gdalwarp -t_srs EPSG:3857 -r bilinear` and `gdal2tiles.py --xyz --resampling average`).  The geometry
 * (projection, tile bounds, footprints) is resolved by the caller into tables; tile arrays are
 * [rows north to south][columns][256][256][4] RGBA u8, alpha 0 = no data.
 * warp: grid = float32 [gh][gw][2], the source (column, row) in pixel-centre coordinates at every
 *   `step`-th output pixel (step a power of two, (gh-1)*step >= OH-1); bilinear with edge replication,
 *   alpha = 255 inside the source raster.
 * base: tile pixel = rounded mean of the source pixels with alpha > 0 in columns col_lo..col_hi and
 *   rows row_lo..row_hi (tables of nx*256 and ny*256 entries, lo > hi = empty).  rgba == NULL: the raster is the H x W output the
 *   previous call on this handle -- s2sr_warp_bilinear_u8 -- produced, taken from its device copy (any other call in between
 *   invalidates the copy -> S2SR_E_INVALID).
 * overview: parent pixel = rounded mean of the valid pixels of its 2x2 group in the child array;
 *   (ox, oy) = child-array tile coordinates of the first parent tile's north-west child (may be -1).
 *   child == NULL: the children are the level the previous base / overview call on this handle produced, taken from the
 *   device copy (cnx, cny must match it; any other call on the handle in between invalidates the copy -> S2SR_E_INVALID). */
int  s2sr_warp_bilinear_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, const float* grid, int32_t gh, int32_t gw,
                           int32_t step, int32_t OH, int32_t OW, uint8_t* out_rgba);
/* The warp in front of a nodata-transparent pyramid.  valid = uint8 [ceil(H / valid_scale)][ceil(W / valid_scale)], nonzero = valid:
 * source pixel (y, x) is valid iff valid[y / valid_scale][x / valid_scale] != 0 (the convention of s2sr_mask).  Coordinates, coverage
 * and taps are the plain call's.  All four taps valid: the plain call's bytes.  No tap valid: (0,0,0,0).  Otherwise the valid taps'
 * bilinear weights are summed to ws; ws < 0.5: (0,0,0,0); else colour = (sum of w * p over the valid taps) / ws rounded half up,
 * alpha 255 (fp32, every operation rounded on its own, fixed order).  Alpha is 0 or 255 and colour is 0 wherever alpha is 0; the
 * bytes of an invalid source pixel never reach the output.  Refused with S2SR_E_INVALID: valid == NULL, valid_scale < 1, and what
 * the plain call refuses.  Leaves its raster on the device exactly as the plain call does. */
int  s2sr_warp_bilinear_masked_u8(s2sr_handle* h, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* valid, int32_t valid_scale,
                                  const float* grid, int32_t gh, int32_t gw, int32_t step, int32_t OH, int32_t OW, uint8_t* out_rgba);
int  s2sr_tiles_base_u8(s2sr_handle* h, const uint8_t* rgba, int32_t H, int32_t W, const int32_t* col_lo, const int32_t* col_hi,
                        const int32_t* row_lo, const int32_t* row_hi, int32_t nx, int32_t ny, uint8_t* out);
int  s2sr_tiles_overview_u8(s2sr_handle* h, const uint8_t* child, int32_t cnx, int32_t cny, int32_t ox, int32_t oy, int32_t pnx,
                            int32_t pny, uint8_t* out);
/* resample: a level through a separable filter given as tap tables -- the other form of base (source: a raster) and of overview
 * (source: the level below, crossing its tile borders).  The entry knows no filter: Lanczos, cubic and bilinear are tables.
 * Column sample j of nx*256 reads source columns col_first[j] .. col_first[j] + col_count[j] - 1 with the integer coefficients
 * col_coef[j][0 .. Kx) (22 fractional bits; count 0 = the sample misses the source); rows alike.  Pixels are RGBA u8, not
 * premultiplied; the arithmetic is Pillow's Image.resize: premultiply on load (c' = ((m >> 8) + m) >> 8, m = c * a + 128),
 * horizontal pass clip((2^21 + sum coef * px) >> 22, 0, 255) per channel stored as 8 bits, the same down the columns,
 * un-premultiply on store (alpha 0 / 255: copy; else min(255, 255 * c' / a)).
 * Refused with S2SR_E_INVALID before the device is touched: K outside 1..S2SR_RESAMPLE_MAX_TAPS, a count outside 0..K, taps that
 * leave the source (first < 0 or first + count > its extent), a sample with 255 * sum|coef| + 2^21 >= 2^31, and src == NULL when
 * the previous call on the handle left no raster / level of the stated size.  out == NULL: the level stays on the device, for
 * s2sr_tiles_write_png and as the source of the next overview or resample call, exactly like base / overview. */
#define S2SR_TILES_SRC_RASTER 0   /* src: [sa = H, sb = W, 4] u8;  NULL: the raster s2sr_warp_bilinear_u8 left on the device */
#define S2SR_TILES_SRC_LEVEL  1   /* src: [sa = cny, sb = cnx] tiles; NULL: the level the previous tiles call left on the device */
#define S2SR_RESAMPLE_MAX_TAPS 64
int  s2sr_tiles_resample_u8(s2sr_handle* h, const uint8_t* src, int32_t src_kind, int32_t sa, int32_t sb,
                            const int32_t* col_first, const int32_t* col_count, const int32_t* col_coef, int32_t Kx,
                            const int32_t* row_first, const int32_t* row_count, const int32_t* row_coef, int32_t Ky,
                            int32_t nx, int32_t ny, uint8_t* out /* NULL: the level stays on the device */);
/* base / overview with out == NULL: the level is computed and stays on the device (for s2sr_tiles_write_png and as the next
 * overview's children).
 * write_png: the PNG files (8-bit RGBA, what s2sr_png_encode writes up to the tokenisation: runs do not cross rows) of the level the
 * previous base / overview call produced, encoded on the device: token statistics and bit emission are kernels, the Huffman codes
 * come from the host between them, only compressed bytes cross PCIe.  paths: nx * ny entries, row-major like the tile array, NULL =
 * skip; flags: S2SR_PNG_SKIP_TRANSPARENT = no file for a tile whose alpha is 0 everywhere, S2SR_PNG_HOST_ENCODER = every tile
 * through the host encoder (the route a tile takes by itself when stored blocks would be smaller; a diagnostic); written
 * (optional): 1 per file written.  Missing parent directories are created. */
#define S2SR_PNG_SKIP_TRANSPARENT 1
#define S2SR_PNG_HOST_ENCODER     2
#define S2SR_PNG_ROW_THREADS      4   /* the first form of the two kernels (one thread walks one row): same bytes, kept as the check */
#define S2SR_PNG_SMALL_GROUPS     8   /* the level goes through in groups of 3 tiles instead of ~2048 (the device phases of a group run under
                                         the host phases of its neighbours): same files; lets a test drive the pipeline on a small level */
int  s2sr_tiles_write_png(s2sr_handle* h, int32_t nx, int32_t ny, const char* const* paths, int32_t flags, int32_t* written);
/* the same for the XYZ layout gdal2tiles writes (tiling.py:138-186): tile (row j, column i) of the level goes to
 * <dir>/<zoom>/<x0 + i>/<y_rows[j]>.png -- the caller hands over ny row numbers instead of nx * ny path strings */
int  s2sr_tiles_write_png_xyz(s2sr_handle* h, int32_t nx, int32_t ny, const char* dir, int32_t zoom, int32_t x0, const int32_t* y_rows,
                              int32_t flags, int32_t* written);

/* measurement: HIP-event timing per kernel family on the launch stream.  on = 0: off;
 * on = N >= 1: every N-th launch of each family is bracketed by a hipEvent pair (N > 1 keeps
 * the event overhead out of a timed region; stats then cover the sampled launches only). */
int  s2sr_set_profiling(s2sr_handle* h, int32_t on);
int  s2sr_get_kernel_stats(s2sr_handle* h, s2sr_kstat* out, int32_t cap, int32_t* n);
int  s2sr_reset_kernel_stats(s2sr_handle* h);
int  s2sr_synchronize(s2sr_handle* h);
/* A group (pack + 351 dependent launches) seen twice with the same shapes, buffers and stream
 * is captured into a hipGraph and replayed afterwards (S2SR_GRAPH=0 disables; the legacy null
 * stream and profiling runs use direct launches).  Counters since s2sr_create. */
int  s2sr_graph_stats(s2sr_handle* h, int64_t* captures, int64_t* replays);

/* host-only codec for the file glue around the path (reference reads LZW GeoTIFFs through rasterio,
 * server/app/wow_sr.py:59-79): TIFF-flavoured LZW (MSB-first 9..12-bit codes, early change).  Decodes
 * at most `cap` bytes into dst, *out_n = bytes produced. */
int  s2sr_tiff_lzw_decode(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_n);
/* the encoder for one strip (writes compress="lzw" GeoTIFFs, wow_sr.py:138-151); cap >= n*3/2 + 16 is always enough */
int  s2sr_tiff_lzw_encode(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_n);

/* host-only PNG encoder for what the path writes (the reference calls cv2.imwrite(path, img) bare, server/app/wow_sr.py:156,163,
 * and hands the tile pyramid to gdal2tiles, server/app/tiling.py:138-186): 8-bit RGB (channels 3) or RGBA (4), filter Sub on
 * every row, deflate with distance-1 matches and dynamic Huffman blocks (cv2's Z_RLE / Z_BEST_SPEED settings, 3-4x zlib's speed).
 * `px`: rows of `width * channels` bytes, `row_stride` bytes apart.  s2sr_png_bound() is always enough for `cap`. */
size_t s2sr_png_bound(int32_t width, int32_t rows, int32_t channels);
/* a complete PNG file (signature, IHDR, one IDAT, IEND) */
int  s2sr_png_encode(const uint8_t* px, int32_t width, int32_t height, int32_t channels, size_t row_stride, uint8_t* out, size_t cap,
                     size_t* out_n);
/* one band of a big image as a complete IDAT chunk, so bands encode on parallel threads: `first` puts the zlib header in front,
 * every band but the `last` ends on a sync flush (byte aligned), the last one on the final block.  The caller writes signature +
 * IHDR, the bands' chunks in order, one more IDAT chunk holding the 4 bytes of the stream's Adler-32 (big endian; combine the
 * per-band values `*adler` over `*raw_n` filtered bytes with adler32_combine), and IEND. */
int  s2sr_png_idat_band(const uint8_t* px, int32_t width, int32_t rows, int32_t channels, size_t row_stride, int32_t first, int32_t last,
                        uint8_t* out, size_t cap, size_t* out_n, uint32_t* adler, size_t* raw_n);
/* `count` square tiles of `size` x `size` pixels, `tile_stride` bytes apart, each written to paths[t] as a PNG file (missing
 * parent directories are created; paths[t] == NULL skips the tile).  skip_transparent: an RGBA tile whose alpha is 0 everywhere is
 * not written (gdal2tiles writes no file for tiles outside the raster, reference server/app/tiling.py:138-186).  written[t]
 * (optional) = 1 for the files written.  One call per tile row keeps the interpreter out of the 12.8k-tile loop of a pyramid. */
int  s2sr_png_write_tiles(const uint8_t* tiles, int32_t count, int32_t size, int32_t channels, size_t tile_stride,
                          const char* const* paths, int32_t skip_transparent, int32_t* written);

/* test hook (host only, no GPU): the OCP e4m3fn encoder the weight packer uses for the fp8
 * correction stages -- round to nearest even, saturating at +-448, NaN -> 0x7f. */
uint8_t s2sr_debug_f32_to_e4m3(float v);
/* test hook (host only): the fp8-trunk weight packer (S2SR_PREC_FP8).  w = [cout][cin][3][3] fp32 -> e4m3 planes of 32 input
 * channels, padded to an even plane count with an all-zero plane: out[plane][tap][ct][16-B half][cout row 0..31][16 bytes] =
 * e4m3(w * 2^k_co); wscale[co] (64 entries) = the E8M0 byte 127 - k_co the MFMA's scale_a operand takes. */
size_t s2sr_debug_pack_f8_bytes(int32_t cin, int32_t cout);
int  s2sr_debug_pack_f8(const float* w, int32_t cin, int32_t cout, uint8_t* out, int32_t* wscale);

/* test hook: one 3x3 conv layer on NCHW fp32 host tensors through the generic fp16 form of conv3x3.hip (the EPI_DEBUG
 * instantiations: plain fp16 operands, no split-operand stages, no sub-pixel or whole-patch forms, none of the head / tail
 * epilogues -- no launch of the net runs this form; s2sr_debug_forward_taps checks what does).
 * upsample != 0 -> nearest-2x on load.  act: 0 none, 1 LeakyReLU(0.2); + 0x100: the launch walks its patches back to front (same bytes). */
int  s2sr_debug_conv(s2sr_handle* h, const float* x, int32_t N, int32_t Cin, int32_t H, int32_t W,
                     const float* weight, const float* bias, int32_t Cout, int32_t upsample,
                     int32_t act, float* y);

/* test hook: what s2sr_create read from the environment (every kernel-form / scale switch is fixed at creation), so a
 * test that sets S2SR_* can assert the switch took on the handle it then creates. */
typedef struct s2sr_debug_config {
    int32_t precision;      /* S2SR_PREC_* */
    int32_t group;          /* cfg.group as given (0 = default) */
    int32_t trunk_w4;       /* always 1: RDB convs on the one-wave-per-SIMD kernels (conv_trunk.hip) */
    int32_t lo_exp;         /* trunk lo half as e4m3(lo * 2^lo_exp) (S2SR_LO_EXP) */
    int32_t fp8_form;       /* the launch-order mask (S2SR_SERPENTINE; 0 = every launch walks its patches front to back).  The form this slot named was removed */
    int32_t fp8_x_exp, fp8_g_exp;   /* fp8 trunk activation scales (S2SR_FP8_XEXP / _GEXP or s2sr_calibrate_fp8) */
    int32_t fp8_hp_tail;    /* S2SR_FP8_TAIL=hp */
    int32_t graphs_on;      /* S2SR_GRAPH */
    int32_t trunk_wino;     /* always 0 (the row-Winograd form was removed) */
    int32_t reserved[6];    /* [0]: window mosaics on (S2SR_MOSAIC); [1]: always 0; [2]: conv_last folded 6-stage form (S2SR_LAST_FOLD); [3]: always 0; [4]: whole-patch fp16 conv1-4 forms allowed (S2SR_F16_FULL); [5]: workspace allocations since s2sr_create */
} s2sr_debug_config;
int  s2sr_debug_get_config(s2sr_handle* h, s2sr_debug_config* out);

/* How `B` equal windows of th x tw travel through the net: kx x ky per launch image with one zero row / column between neighbours
 * (1 x 1: one window per image -- sizes that are multiples of the 32-pixel patch gain nothing); the windows past the last full
 * mosaic travel as ONE smaller mosaic.  Chosen for the fewest launched patches.  Host arithmetic only. */
int  s2sr_debug_pick_mosaic(int32_t B, int32_t th, int32_t tw, int32_t* kx, int32_t* ky);
/* ... and what that choice LAUNCHES: 32 x 32 patches of floor(B / (kx*ky)) full mosaics plus the remainder's smaller mosaic
 * (`launched`), next to B plain images (`plain`).  The engine only takes a mosaic when launched <= 0.98 plain.  Host arithmetic only. */
int  s2sr_debug_mosaic_patches(int32_t B, int32_t th, int32_t tw, int64_t* launched, int64_t* plain);
/* The chunk plan of a tiled s2sr_enhance_u8 (host arithmetic only, no device needed): `units` row units of `unit_windows` windows
 * each, at most `u_max` units per chunk, `per` windows per launch image (mosaic), `pimg` 32x32 patches per launch image, `ncu`
 * workgroups.  Writes the chunk sizes front to back; *n = their number (cap 0: count only). */
int  s2sr_debug_plan_chunks(int32_t units, int32_t u_max, int32_t unit_windows, int32_t per, int32_t pimg, int32_t ncu,
                            int32_t* sizes, int32_t cap, int32_t* n);
/* The window job of s2sr_enhance_u8 / s2sr_enhance_u16 on a PH x PW image (for scale 2: already padded to even sizes); host
 * arithmetic only, no device needed.  dims = {nx, ny, wh, ww}: ny rows of nx DISTINCT windows of wh x ww (window rows / columns of
 * the reference's plan that coincide run once).  rects: y1, y2, x1, x2 per window, row-major, `cap` windows of room
 * (ceil(PH / tile) * ceil(PW / tile) always suffice); none for tiled == 0, where the image is its own window.  rm (2 * scale * PH
 * entries) and cm (2 * scale * PW): per output row / column the window row / column that is pasted there and the row / column
 * inside that window's output. */
int  s2sr_debug_plan_windows(int32_t PH, int32_t PW, int32_t tile, int32_t pad, int32_t scale, int32_t tiled, int32_t* dims,
                             int32_t* rects, int32_t cap, int32_t* rm, int32_t* cm);
/* The blend tables of s2sr_enhance_blend_* for that window job (host arithmetic only): rows (6 * scale * PH ints) and cols
 * (6 * scale * PW), per output row / column {a, ia, b, ib, num, den}: the two windows (indices of s2sr_debug_plan_windows'
 * distinct window rows / columns), the row / column inside each one's output, and the weight of b, w = num / den; outside every
 * ramp a == b, ia == ib, num = 0, den = 1. */
int  s2sr_debug_plan_blend(int32_t PH, int32_t PW, int32_t tile, int32_t pad, int32_t scale, int32_t tiled, int32_t* rows,
                           int32_t* cols);
/* The bands of a chunked whole-image call (host arithmetic only): chunk_r0[0 .. nchunks] = the first window row of each chunk,
 * ascending from 0, then ny; last_row[OH] = per output row the last window row it reads (s2sr_debug_plan_windows' rm[:, 0], or
 * column 2 of s2sr_debug_plan_blend's rows), monotone.  bands[2 k], bands[2 k + 1] = the output rows [yb, ye) chunk k makes final. */
int  s2sr_debug_plan_bands(const int32_t* chunk_r0, int32_t nchunks, int32_t ny, int32_t OH, const int32_t* last_row, int32_t* bands);

/* test hook: ONE RDB-shaped conv through the TRUNK kernels (conv_trunk.hip: conv_trunk_f16 / conv_trunk_f8), host tensors in
 * NCHW fp32 -- the per-layer parity check of the kernels that carry 84 % of a step (s2sr_debug_conv goes through conv3x3.hip).
 *   kind 0: fp16 conv1-4 form   y = lrelu(conv(x) + b)                        Cin in {64,96,128,160}, Cout 32, y = the fp16 plane written
 *   kind 1: fp16 conv5 form     y = 0.2*(conv(x) + b) + (x[:, :64] + lo)     Cin 192, Cout 64, y = hi + lo of the (fp16, e4m3) pair written
 *   kind 2: fp16 conv5 of rdb3  y = 0.2*(kind 1) + skip
 *   kind 3: fp8 conv1-4 form    y = e4m3(lrelu(conv + b) * 2^g_exp) / 2^g_exp  (x planes at 2^x_exp, growth planes at 2^g_exp)
 *   kind 4: fp8 conv5 form      y = fp16(0.2*(conv + b) + x[:, :64]); y_aux = its e4m3(* 2^x_exp) image
 *   kind 5: fp8 conv5 of rdb3   y = fp16(0.2*(kind 4 value) + skip)
 * x is rounded to the operand format on the way in (fp16, or e4m3 at the handle's scales), so callers pass representable
 * values; `lo` ([N,64,H,W], kinds 1-2, may be NULL) is stored as e4m3(lo * 2^lo_exp); `skip` ([N,64,H,W]) as the
 * (fp16 hi, e4m3 lo) pair (kind 2) or fp16 (kind 5).  form: kind 0: 0 auto, 1 = 16x32 patches, 2 = 32x32 patches,
 * 5 = 8x32 patches (single tiles), 6 / 7 / 8 = the whole-patch forms of 2 / 1 / 5, 10 = 8x32 patches with two planes per pipeline
 * stage; kinds 1-2: 0 auto, 1 = 16x32 patches, 5 = 8x32 patches, 10 = 8x32 patches with two planes per stage; kind 3: 0.  The removed
 * forms (kind 0: 3, 4, 9, 11; kinds 1-2: 2; kind 3: anything but 0) are refused (S2SR_E_HIP, not supported).  Kinds 1-2 refuse
 * every number conv5 has no form for in the same way: they answer to 0, 1, 5 and 10 only.
 * form + 0x100 (every kind): the launch walks its patches back to front (same bytes). */
typedef struct s2sr_debug_trunk_args {
    int32_t kind, form;
    int32_t N, Cin, H, W;
    const float* x;
    const float* weight;    /* [Cout,Cin,3,3] */
    const float* bias;      /* [Cout] */
    const float* lo;
    const float* skip;
    float* y;               /* [N,Cout,H,W] */
    float* y_aux;           /* kinds 4-5: [N,64,H,W], may be NULL */
} s2sr_debug_trunk_args;
int  s2sr_debug_conv_trunk(s2sr_handle* h, const s2sr_debug_trunk_args* a);

/* test hook: ONE batch through the production forward (the launch schedule of s2sr_forward_batch_u8 / s2sr_forward_f32, with the
 * handle's weights and switches; run eagerly, never from a captured graph), then every tensor the six head / tail convs read or
 * write, decoded on the host to fp32 over the PADDED extent [n, C, Hp, Wp] of the launch images (halo and round-up slack
 * included).  Input: `tiles` [B, th, tw, 3] u8, or `x` [B, 3, th, tw] fp32 in [0, 1] (exactly one of them); `job_windows`
 * (>= B, 0 = B) sizes the window mosaic as s2sr_forward_part_u8_dev does.  A batch that needs more than one launch group or more
 * than one mosaic segment is refused (S2SR_E_INVALID); after the call the workspace holds exactly this batch.
 * The geometry fields are always filled; the batch runs only when at least one buffer is given.  Buffers (NULL: skip):
 *   tap[S2SR_TAP_P0]       16 ch  the packed input (fp16)
 *   tap[S2SR_TAP_F]        64 ch  conv_first's fp32 output (the global skip)
 *   tap[S2SR_TAP_TRUNK_HI] 64 ch  the trunk output conv_body reads: fp16 hi
 *   tap[S2SR_TAP_TRUNK_LO] 64 ch  ... its lo as stored: fp16, or e4m3(lo * 2^trunk_lo_exp) (the value lo is returned)
 *   tap[S2SR_TAP_T8]      128 ch  conv_body's e4m3 operand planes: ch 0-63 the lo8 bytes' values * 2^-11, ch 64-127 the hi8 values
 *   tap[S2SR_TAP_U0 + k]   64 ch  conv_body (k 0), up1, up2, hr outputs: fp16 hi (U1 at 2x, U2 and U3 at 4x)
 *   tap[S2SR_TAP_U0LO + k] 128 ch their e4m3 planes as T8 (split-operand tail only; hi8 planes that are not written read as 0)
 *   out_f32 [B, 3, 4th, 4tw], out_u8 [B, 4th, 4tw, 3]: the outputs of the same run.
 * `avail` bit t: tap t exists in this mode.
 * Scale 2: th, tw even; every tap is on the th/2 x tw/2 trunk grid (P0 = the unshuffled input, channels 12-15 zero), mos_wh /
 * mos_ww are trunk sizes, and the outputs are [B, 3, 2th, 2tw] / [B, 2th, 2tw, 3]. */
enum { S2SR_TAP_P0 = 0, S2SR_TAP_F, S2SR_TAP_TRUNK_HI, S2SR_TAP_TRUNK_LO, S2SR_TAP_T8, S2SR_TAP_U0, S2SR_TAP_U1, S2SR_TAP_U2,
       S2SR_TAP_U3, S2SR_TAP_U0LO, S2SR_TAP_U1LO, S2SR_TAP_U2LO, S2SR_TAP_U3LO, S2SR_TAP_COUNT };
typedef struct s2sr_debug_taps {
    int32_t n;                          /* out: launch images */
    int32_t H[3], W[3], Hp[3], Wp[3];   /* out: per scale 1x / 2x / 4x: live extent of a launch image, padded plane dims */
    int32_t mos_kx, mos_ky, mos_wh, mos_ww, mos_count;   /* out: window mosaic of the launch (all 0: one window per image) */
    int32_t trunk_lo_exp;               /* out: -1 trunk lo stored as fp16, else as e4m3 at 2^trunk_lo_exp */
    int32_t avail;                      /* out: bit t = tap t exists */
    int32_t reserved[4];
    float* tap[S2SR_TAP_COUNT];         /* in */
    float* out_f32;                     /* in */
    uint8_t* out_u8;                    /* in */
} s2sr_debug_taps;
int  s2sr_debug_forward_taps(s2sr_handle* h, const uint8_t* tiles, const float* x, int32_t B, int32_t th, int32_t tw,
                             int32_t job_windows, s2sr_debug_taps* t);

/* The trunk kernel instantiation one RDB conv launch took (launch_conv_trunk / launch_conv_trunk_f8 report it).
 * kernel: 1 conv_trunk_f16, 2 conv_trunk_f8, 0 nothing recorded.
 * rows: patch rows (the patch is rows x 32 pixels); ring: slab ring depth; full: the FULL template argument (0 generic px_live
 * test, 1 whole patches, 2 mosaics of 276-pixel windows, 3 the extent test alone); pl: planes per pipeline stage; prod: a
 * load-only wave (conv_trunk_f8 conv1-4); wgl: always 0; loe: 1, conv5's short lo encoding; wv: MFMA waves (4); npl: fp8 weights
 * resident in LDS (planes; 0 = streamed); epi: the epilogue (0 conv1-4 LeakyReLU, 1 conv5 of rdb1 / rdb2, 2 conv5 of rdb3 with the
 * RRDB skip). */
typedef struct s2sr_debug_trunk_form {
    int32_t kernel, ct, rows, ring, full, pl, prod, wgl, loe, wv, npl, epi;
} s2sr_debug_trunk_form;

/* test hook: ONE batch through the production forward, exactly as s2sr_debug_forward_taps runs it (same input rules, same
 * refusals, graphs off, buffers of its own; also refused while s2sr_calibrate_fp8 runs),
 * with the trunk fields of the RDBs [first, first + count) (global RDB index: 3 * block + rdb, < 3 * num_block) copied out at
 * every RDB boundary and decoded to fp32 over the PADDED extent [n, C, Hp, Wp] (halo and round-up slack included):
 *   x_hi   [count + 1][n][64][Hp][Wp]  the trunk x at boundary j (the input of RDB first + j): fp16 hi (fp8 path: the fp16 Xh)
 *   x_lo   [count + 1][n][64][Hp][Wp]  fp16 path: its lo as stored, e4m3 planes at 2^lo_exp (the value lo is returned);
 *                                      fp8 path: the e4m3 x planes of D8 at 2^x_exp (the value x is returned)
 *   growth [count][n][128][Hp][Wp]     x1..x4 of each RDB: fp16, or (fp8 path) e4m3 planes at 2^g_exp (value returned)
 *   skip_hi, skip_lo [count][n][64][Hp][Wp]  the RRDB skip a rdb3 reads (its RRDB's input: fp16 hi, or Xh; lo as x_lo, fp16
 *                                      path only); left untouched for rdb1 / rdb2
 *   entry_lo [n][64][Hp][Wp]           first == 0, fp16 path: conv_first's fp16 lo (T) that xh_to_fp8 turns into boundary 0's lo
 *   form   [count][5]                  the instantiation conv1..conv5 of each RDB ran on
 *   out_f32 / out_u8                   the outputs of the same run, as s2sr_debug_forward_taps.
 * The geometry fields are always filled; the batch runs only when at least one buffer is given. */
typedef struct s2sr_debug_trunk_fields {
    int32_t first, count;               /* in */
    int32_t n, H, W, Hp, Wp;            /* out: launch images, live extent of one, padded plane dims */
    int32_t mos_kx, mos_ky, mos_wh, mos_ww, mos_count;   /* out: window mosaic of the launch (all 0: one window per image) */
    int32_t fp8;                        /* out: 1 = the fp8 trunk path, 0 = the fp16 one */
    int32_t lo_exp, x_exp, g_exp;       /* out: the scales of the path (-1 where the path has none) */
    int32_t reserved[4];
    float *x_hi, *x_lo, *growth, *skip_hi, *skip_lo, *entry_lo;   /* in (NULL: skip) */
    s2sr_debug_trunk_form* form;        /* in */
    float* out_f32;                     /* in */
    uint8_t* out_u8;                    /* in */
} s2sr_debug_trunk_fields;
/* (scale-4 handles only: S2SR_E_INVALID on a scale-2 handle, whose trunk is the same schedule on the half grid) */
int  s2sr_debug_trunk_taps(s2sr_handle* h, const uint8_t* tiles, const float* x, int32_t B, int32_t th, int32_t tw,
                           int32_t job_windows, s2sr_debug_trunk_fields* t);

/* diagnostic: time one RDB-shaped conv (cin in {64,96,128,160,192}; cout 32 -> conv1..4 form,
 * cout 64 -> conv5 form) over N images of HxW, `iters` launches; avg_us = mean launch time from
 * HIP events.  If trace != NULL, one extra launch of the stamped diagnostic build fills
 * trace[wg*24 + k] with s_memtime ticks for the first trace_wgs workgroups. */
int  s2sr_debug_bench_conv(s2sr_handle* h, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout,
                           int32_t iters, float* avg_us, uint64_t* trace, int32_t trace_wgs);

/* diagnostic: what the matrix pipe sustains on THIS part at its power cap, for the roofline claim of the fp16 trunk kernel
 * (csrc/ceiling.hip).  mode 0: a bare v_mfma_f32_32x32x16_f16 loop, operands in registers; 1: the same loop with its operands
 * re-read from LDS at conv_trunk_f16's 0.75 KiB per MFMA; 2: + the LDS ring refilled by LDS-DMA at the kernel's 48 KiB per 288
 * MFMAs from a 336-MB buffer (3-deep ring, counted vmcnt, one barrier per stage); 3: as 2 with half the fill (24 KiB); 4: as 2 from
 * an 8-MB source that stays in L2 / MALL (the fill without the HBM side); 5: the kernel's own mix -- 36 KiB streamed from HBM, 12 KiB
 * from the cached source (the weights), 8 KiB stored per stage (its output); 6: conv5's mix -- 384 MFMAs per stage (64 output channels),
 * 0.44 LDS reads per MFMA, 32 KiB streamed, 16 KiB cached, 12 KiB stored; 7 / 8: as 2 from a 100-MB / 200-MB source (past the L2s, inside
 * the Infinity Cache: the dense tensor of a launch group of 4 / 8 images).  One workgroup per CU, random fp16 operands;
 * `launches` back-to-back launches of `stages` stages per workgroup behind launches / 4 + 1 untimed ones; *ms_total = their
 * time by HIP events, *flop_per_launch / *dma_bytes_per_launch = the work of one (28 stages = one conv1-4 launch of 16 images). */
int  s2sr_debug_mfma_ceiling(s2sr_handle* h, int32_t mode, int32_t stages, int32_t launches, double* flop_per_launch,
                             double* dma_bytes_per_launch, float* ms_total);

/* diagnostic prototype (csrc/persist.hip; nothing of the product calls it): what would a trunk schedule sustain whose workgroups stay across the
 * layers of the RDBs, planes handed to the neighbours through flags, on a launch group small enough for the Infinity Cache?  `grid` workgroups
 * (at most one per CU, on an otherwise idle device: they must all be resident) of `P` = 2..4 patches each run `rdbs` RDB-shaped rounds per launch
 * (per patch 28 stages of 288 MFMAs + 12 of 576, 48 KiB of LDS-DMA per stage, the layer's planes stored behind each patch; working set
 * grid x P x 512 KiB); variant bit 0: plane loads with sc1, plane stores with sc0 sc1; bit 1: the same work on 32-KiB stages in a 4-deep ring
 * (three stages of look-ahead instead of two); variant 4 / 5: variant 0 / 1 with the hand-over CHECKED -- the plane stores carry (layer count,
 * writer) and every landed piece is compared: mismatches[0] = halo pieces (written by a workgroup on another XCD), mismatches[1] = own pieces.
 * *timeouts: dependency waits that ran into their bound (must be 0 for the timing to mean anything). */
int  s2sr_debug_rdb_persistent(s2sr_handle* h, int32_t variant, int32_t grid, int32_t P, int32_t rdbs, int32_t launches, double* flop_per_launch,
                               float* ms_total, int32_t* timeouts, int32_t* mismatches);

/* test hook (S2SR_ARCH_COMPACT handles only; the RRDB-only hooks above -- s2sr_debug_conv_trunk, s2sr_debug_forward_taps,
 * s2sr_debug_trunk_taps, s2sr_debug_rdb_persistent -- answer S2SR_E_INVALID on such a handle): ONE batch through the production
 * forward exactly as s2sr_debug_forward_taps runs it (same input rules and refusals, graphs off), with the fp16 activation
 * copied out after the layers of the caller's choice and decoded to fp32 over the PADDED extent [n, 64, Hp, Wp] of the launch
 * images.  Layer 0 is the first conv (after its PReLU), layer k in 1..num_conv body conv k (after its PReLU).  The geometry
 * fields are always filled; the batch runs only when at least one buffer is given. */
#define S2SR_COMPACT_TAPS_MAX 8
typedef struct s2sr_debug_compact_fields {
    int32_t nlayers;                        /* in: entries of layers / act in use (<= S2SR_COMPACT_TAPS_MAX) */
    int32_t layers[S2SR_COMPACT_TAPS_MAX];  /* in: ascending, each in [0, num_conv] */
    int32_t n, H, W, Hp, Wp;                /* out: launch images, live extent of one, padded plane dims */
    int32_t mos_kx, mos_ky, mos_wh, mos_ww, mos_count;   /* out: window mosaic of the launch (all 0: one window per image) */
    int32_t reserved[4];
    float* act[S2SR_COMPACT_TAPS_MAX];      /* in (NULL: skip): [n][64][Hp][Wp] */
    float* p0;                              /* in (NULL: skip): the packed input, [n][16][Hp][Wp] (channels 0..2 = exact 0..255) */
    float* out_f32;                         /* in: [B, 3, 4th, 4tw] */
    uint8_t* out_u8;                        /* in: [B, 4th, 4tw, 3] */
} s2sr_debug_compact_fields;
int  s2sr_debug_compact_taps(s2sr_handle* h, const uint8_t* tiles, const float* x, int32_t B, int32_t th, int32_t tw,
                             int32_t job_windows, s2sr_debug_compact_fields* t);

/* test hooks: red zones around the library's device allocations (csrc/redzone.h).  A diagnostic for stores that land in front
 * of or behind the buffer they belong to -- allocator slack, a neighbouring workspace plane -- where no output comparison
 * looks.  Reads past a buffer are not detected.  Process-wide; off by default, and then every allocation, pointer and byte is
 * what it is without these entries.  The environment variable S2SR_REDZONE=<bytes>, read once when the library is loaded,
 * sets the initial zone size (a value that is no number, or no multiple of 4096, is reported on stderr and leaves the mode
 * off); with it set the process prints "s2sr redzones: <n> allocations checked, <m> damaged" to stderr when it exits.  That
 * line counts what was checked at a free or by s2sr_debug_redzone_check: a buffer still live at exit -- a handle that was
 * never destroyed -- is NOT read then, so call s2sr_debug_redzone_check (or destroy the handles) before the process ends.
 *
 * s2sr_debug_redzone: device allocations made FROM NOW ON get `bytes` of patterned memory in front and behind (and every
 *   plane carved out of a handle's workspace a zone behind it); 0 turns the mode off.  Existing allocations keep what they
 *   have: handles created before the switch have no zones until a buffer of theirs regrows.  S2SR_E_INVALID unless bytes is 0
 *   or a positive multiple of 4096 (pointers keep their alignment).  When a zoned buffer is freed, its zones are checked and
 *   damage is remembered for the next s2sr_debug_redzone_check.
 * s2sr_debug_redzone_check: waits for the handle's streams (work a caller put on a stream of its own: synchronise it first),
 *   then checks the zones of EVERY live zoned allocation of the process.  *damaged = zones found damaged now + zones found
 *   damaged at a free since the last check; *allocations = the zoned allocations this handle owns (workspace planes count
 *   one each).  With damage, s2sr_last_error(h) describes the first: "redzone: allocation of <user bytes> bytes, <front|back>
 *   zone damaged at offset <byte offset from the zone's start>: found 0x.., expected 0x..".  Damaged zones are patterned
 *   again and the remembered damage is cleared: the next check is clean.
 * s2sr_debug_redzone_poke: the negative control.  Writes one wrong byte into the back zone of scratch buffer `slot` (0..5),
 *   `offset` bytes behind its last byte (offset >= 0), or into its front zone, -offset bytes in front of its first byte
 *   (offset < 0; offset -1 is the zone's last byte).  The byte lies inside the library's own allocation.  S2SR_E_INVALID when
 *   the slot has no zones or the offset is not inside the zone. */
int  s2sr_debug_redzone(int64_t bytes);
int64_t s2sr_debug_redzone_bytes(void);       /* the zone size in force (0: off), for callers that switch it and put it back */
int  s2sr_debug_redzone_check(s2sr_handle* h, int64_t* allocations, int64_t* damaged);
int  s2sr_debug_redzone_poke(s2sr_handle* h, int32_t slot, int64_t offset);

/* test hooks: poisoned device memory (csrc/redzone.h, namespace poison).  The red zones catch a store outside a buffer; this catches
 * a LOAD of in-bounds bytes that nobody wrote in this call -- a histogram without its memset, a stream assembled with atomicOr,
 * a scratch slot that still holds the previous call's bytes.  Fresh device memory reads as zeros in practice and the scratch slots
 * of a handle grow and are never cleared, so such a load returns a plausible value in a fresh process and something else in a
 * long-lived one.  Process-wide; off by default, and then every allocation, pointer and byte is what it is without these entries.
 * Works with and without red zones.  The environment variable S2SR_POISON=<1|2>, read once when the library is loaded, sets the
 * initial pattern (another value is reported on stderr and leaves the mode off).
 *
 * s2sr_debug_poison: every device and page-locked host allocation the library makes FROM NOW ON is filled with the pattern before
 *   anybody sees it; 0 turns the mode off.  Pattern 1: every byte 0xFF (a NaN as fp32, fp16 and e4m3, -1 as an int32, 255 as a
 *   u8); pattern 2: a non-zero byte that depends on its position (the red zones' front pattern).  The workspace is still zeroed
 *   after the fill: its zero halos are the convs' padding, part of the contract and no leftover.  S2SR_E_INVALID for any other
 *   value.  Existing allocations keep their bytes.
 * s2sr_debug_poison_scratch: waits for the handle's streams (work a caller put on a stream of its own: synchronise it first),
 *   then fills every allocated scratch slot over its whole capacity, and the trash page, with the pattern in force, and forgets
 *   what a call left in scratch for the next one (the tile level, the warped raster, the 16-bit image, an open banded
 *   post-process) exactly as a call that takes scratch does.  Nothing is moved or freed: captured graphs stay valid and replay
 *   on the poisoned bytes.  *slots: bit i set = slot i was filled; bytes[i] (S2SR_SCRATCH_SLOTS entries): its capacity, 0 when
 *   the slot is not allocated.  S2SR_E_INVALID when the mode is off.
 * s2sr_debug_scratch_peek: copies n bytes at `offset` of scratch slot `slot` (-1: the trash page, S2SR_TRASH_BYTES long) to `out`,
 *   after waiting for the handle's streams.  S2SR_E_INVALID when the range is not inside the slot's capacity.  Works in either mode. */
#define S2SR_SCRATCH_SLOTS 8
#define S2SR_TRASH_BYTES 8192
int  s2sr_debug_poison(int32_t pattern);
int32_t s2sr_debug_poison_pattern(void);      /* the pattern in force (0: off), for callers that switch it and put it back */
int  s2sr_debug_poison_scratch(s2sr_handle* h, int64_t* slots, int64_t* bytes);
int  s2sr_debug_scratch_peek(s2sr_handle* h, int32_t slot, int64_t offset, int64_t n, uint8_t* out);

/* test hooks: stalled streams (csrc/stall.hip, csrc/engine_internal.h "ordering events").  The red zones catch a store outside a
 * buffer, poison a load of bytes nobody wrote; this catches a CONSUMER THAT DOES NOT WAIT for its producer on another stream -- a
 * missing or mis-indexed event wait between the compute stream (the handle's, or the one a *_dev door was given) and the handle's
 * copy stream, which changes no byte as long as the producer happens to be done in time.  A stall is a one-wave kernel that reads
 * the constant-rate counter until the time has passed; it touches no memory and ends after a fixed number of iterations whatever
 * the counter does.  Process-wide; off by default, and then the library enqueues nothing it would not enqueue without these entries.
 *
 * s2sr_debug_delay: mode bit 1 stalls the compute side, bit 2 the copy side, for `usec` microseconds (1 .. S2SR_DEBUG_STALL_MAX_USEC)
 *   at the head of every stream segment: at the entry of every door on each stream it uses, behind every ordering event recorded
 *   on that side's stream and behind every wait of that stream.  Never on a stream that is capturing (no captured region holds an
 *   ordering event, and a door's entry stall precedes its capture).  Mode 0 (usec 0) turns it off.  S2SR_E_INVALID otherwise.
 * s2sr_debug_delay_drop: the negative control.  While the mode is on, the stream-waits of ordering site `site` are skipped (-1:
 *   none).  Only the S2SR_SITE_* below are accepted: the waits behind which the copy stream copies finished pixels to the host and
 *   does nothing else, so a dropped wait yields early pixels and cannot send a load or a store anywhere (engine_internal.h says
 *   why, site by site).  S2SR_E_INVALID for every other site.
 * s2sr_debug_stall: one stall of `usec` on the handle's stream (which 0), its copy stream (1) or `stream` (2), in either mode.
 * s2sr_debug_stream_touch: 64 bytes of the handle's trash page set to zero on that stream (which as above); wait != 0: returns
 *   when that stream is idle.  With s2sr_debug_stall on another stream it shows whether two streams run side by side. */
#define S2SR_DEBUG_STALL_MAX_USEC 20000
#define S2SR_SITE_BATCH_GROUP_D2H 0     /* s2sr_forward_batch_u8: a group's tiles leave under the next group's forward */
#define S2SR_SITE_CHUNK_BAND_D2H 2      /* the whole-image doors: a band leaves under the next chunk */
#define S2SR_SITE_DISPLAY_BAND_D2H 6    /* s2sr_display_apply_u16: a band leaves under the next band's kernel */
#define S2SR_SITE_COPY_TO_HOST 7        /* s2sr_copy_to_host: the copy stream behind the caller's stream */
int  s2sr_debug_delay(int32_t mode, int32_t usec);
int32_t s2sr_debug_delay_mode(void);          /* the mode in force (0: off), for callers that switch it and put it back */
int32_t s2sr_debug_delay_usec(void);
int  s2sr_debug_delay_drop(int32_t site);
int32_t s2sr_debug_delay_dropped(void);       /* the site being dropped, -1: none */
int  s2sr_debug_stall(s2sr_handle* h, int32_t which, void* stream, int32_t usec);
int  s2sr_debug_stream_touch(s2sr_handle* h, int32_t which, void* stream, int32_t wait);

/* test hooks: capped grids (csrc/gridcap.hip, csrc/s2sr_internal.h capped_grid).  The fourth question to the doors: does any byte
 * depend on HOW THE WORK WAS DEALT OUT TO WORKGROUPS?  Every hot kernel is a loop over work items (patches, tiles, blocks' worth of
 * elements) inside a workgroup that stays; on a 256-CU part a small image gives every workgroup one item, and the second trip
 * through the loop never runs.  With a cap in force every launch whose kernel loops over its grid takes at most `workgroups`
 * workgroups (the conv kernels, whose grids stay a positive multiple of 8: max(8, workgroups & ~7)), so small shapes make many
 * trips.  No kernel changes, and every byte must be what it is without the cap.  Launches where a workgroup IS the work item (the
 * PNG kernels, the CLAHE histogram / LUT and the blur tile grids) and the diagnostic kernels (ceiling, persist, stall) are never
 * capped.  Process-wide; off by default, and then every launch has the grid it has without these entries (one relaxed atomic load
 * per launch).  Not for production: a capped launch leaves most of the device idle.  The environment variable
 * S2SR_GRID_CAP=<workgroups>, read once when the library is loaded, sets the initial cap (a value that is no number in
 * 0 .. S2SR_DEBUG_GRID_CAP_MAX is reported on stderr and leaves the mode off).
 *
 * The contract: the cap is read when a launch is ENQUEUED.  A captured graph keeps the grids it was captured with, whatever the
 * cap is when it replays; so a caller that wants capped replays creates its handle, or at least captures, under the cap (handles
 * cache their graphs per shape).
 *
 * s2sr_debug_grid_cap: 0 turns the mode off; 1 .. S2SR_DEBUG_GRID_CAP_MAX the cap.  S2SR_E_INVALID otherwise, and the cap stays
 *   what it was.
 * s2sr_debug_grid_cap_stats: the precondition of a test that relies on the cap.  Per launcher family i (names:
 *   s2sr_debug_grid_cap_family(i), NULL past the last) launches[i] = the launches the cap made smaller since the last reset, and
 *   max_trips[i] = the largest ceil(work items / workgroups) among them -- how often the busiest workgroup went through its loop.
 *   Host arithmetic at enqueue time; a replayed graph counts nothing.  `cap` entries of room, at least S2SR_GRID_CAP_FAMILIES;
 *   *n = the number written. */
#define S2SR_DEBUG_GRID_CAP_MAX 1048576
#define S2SR_GRID_CAP_FAMILIES 11
int  s2sr_debug_grid_cap(int32_t workgroups);
int32_t s2sr_debug_grid_cap_workgroups(void); /* the cap in force (0: off), for callers that switch it and put it back */
int  s2sr_debug_grid_cap_stats(int64_t* launches, int64_t* max_trips, int32_t cap, int32_t* n);
void s2sr_debug_grid_cap_stats_reset(void);
const char* s2sr_debug_grid_cap_family(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* S2SR_H */
