// Data-movement kernels around the conv stack: HBM-bound byte work, one element per thread,
// coalesced on the side that moves the most bytes.
//   pack_tiles         : [N,H,W,3] u8 -> one fp16 blocked-16 plane with zero halo; replaces
//                        `img.astype(float32)/255` + permute (cnn_super_resolution.py:220-222);
//                        values stay the exact integers 0..255, the 1/255 lives in conv_first.
//                        One pixel template over what is read (u8, u16 with a range, u8 / f32 unshuffled by 2) and where it
//                        lands (image or mosaic cell), one kernel per built pair, one host entry.
//   gather_windows     : cut the _tile_process windows (cnn_super_resolution.py:249-256)
//   stitch             : crop + paste with the reference's overwrite order (:259-278)
#include "s2sr_internal.h"

namespace s2sr {

typedef _Float16 f16;
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x8 __attribute__((ext_vector_type(8)));

// blocks of 256 threads for a grid-stride loop over `total` elements, at most `cap` of them
static inline int grid_for(size_t total, int most) { return stride_grid(total, most, GF_PACK); }   // under the diagnostic grid cap (s2sr_internal.h)

// ------------------------------------------------------------------------------------------
// The tile packers: B tiles -> the one-block input plane, one thread per plane pixel, consecutive lanes along a row.
// Where pixel (ly, lx) of tile t lands:
//   Plain : image t, pixel (ly, lx).
//   Cells : a window mosaic, B windows of h x w into ceil(B / (kx*ky)) images of (ky*(h+1)-1) x (kx*(w+1)-1), window t at grid
//           cell (t % (kx*ky)) / kx, % kx of image t / (kx*ky); separator rows / columns are never written.
// What is read (a source: its sample type, its constants, and get() = the channels of one plane pixel, stored as they come):
//   SrcU8          : [B,h,w,3] u8 as the exact integers 0..255, one 8-byte store (one 16-channel block per image; channels
//                    4..15 stay zero from the allocation memset).
//   SrcU16         : the 16-bit door, see split_u16; one 16-byte store.  SrcU8's 8-byte store leaves channels 4..5 of a plane
//                    this source wrote as they are (finite values); the u8 conv_first weights of those channels are zero.
//   SrcU8Unshuffle, SrcF32Unshuffle : RealESRGAN_x2plus (s2sr_config.scale 2), F.pixel_unshuffle(x, 2) in front of conv_first:
//                    the input at full resolution, the plane at half resolution (the trunk grid h x w).  Channel c*4 + i*2 + j of
//                    trunk pixel (y, x) is input channel c at (2y+i, 2x+j) (torch's order); all 16 channels (12..15 zero) leave
//                    as two 16-byte stores.
// ------------------------------------------------------------------------------------------
struct Plain {
    __device__ void move(int&, int&, int&, int, int) const {}
};
struct Cells {   // (tile, ly, lx) of an h x w window -> (image, y, x) of its mosaic
    int kx, ky;
    __device__ void move(int& n, int& y, int& x, int h, int w) const {
        const int t = n;
        n = t / (kx * ky);
        const int slot = t - n * (kx * ky);
        const int wy = slot / kx, wx = slot - wy * kx;
        y += wy * (h + 1);
        x += wx * (w + 1);
    }
};
template <class V>
struct Channels {   // the first channels of a plane pixel as one vector
    V v;
    __device__ void store(char* dst) const { *(V*)dst = v; }
};

struct SrcU8 {
    typedef uint8_t sample;
    __device__ Channels<f16x4> get(const uint8_t* in, size_t i, int, int, int, int, int) const {
        const uint8_t* s = in + i * 3;
        f16x4 v;
        v[0] = (f16)(float)s[0];
        v[1] = (f16)(float)s[1];
        v[2] = (f16)(float)s[2];
        v[3] = (f16)0.f;
        return {v};
    }
};

// uint16 samples with a value range [lo, hi] (s2sr_forward_batch_u16 / s2sr_enhance_u16):
//   in : d = clamp(v, lo, hi) - lo (0..65535) travels as TWO exact fp16 integers, d = 256 * dh + dl: channels 0..2 of the
//        one-block input plane carry dl (0..255), channels 3..5 carry 256 * dh (0..65280: 8 significant bits, below fp16's
//        65504).  conv_first runs on a cin-6 weight set with w6[:, c] = w6[:, c + 3] = w[:, c] and in_scale 1 / (hi - lo), so
//        its accumulator sums w * d exactly as it sums w * u for u8 input.
//   out: q = lo + rint(clamp(y, 0, 1) * (hi - lo)), the product in fp32 rounded once, rint to nearest even (upstream
//        RealESRGANer's 16-bit branch rounds; the u8 door's truncation is the reference's quirk and stays there).
__device__ inline f16x8 split_u16(const uint16_t* s, int lo, int hi) {
    f16x8 v;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int d = (int)s[c];
        d = (d < lo ? lo : (d > hi ? hi : d)) - lo;
        v[c] = (f16)(float)(d & 0xff);
        v[3 + c] = (f16)(float)(d & 0xff00);
    }
    v[6] = (f16)0.f;
    v[7] = (f16)0.f;
    return v;
}

struct SrcU16 {
    typedef uint16_t sample;
    int lo, hi;
    __device__ Channels<f16x8> get(const uint16_t* in, size_t i, int, int, int, int, int) const { return {split_u16(in + i * 3, lo, hi)}; }
};

struct Unshuffled {   // channels 0..11 of a plane pixel; 12..15 are zero
    float v[12];
    __device__ void store(char* dst) const {
        f16x8 a, b;
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = (f16)v[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) { b[k] = (f16)v[8 + k]; b[4 + k] = (f16)0.f; }
        *(f16x8*)dst = a;
        *(f16x8*)(dst + 16) = b;
    }
};

// u8 images of H x W as stored: H is 2h or, for an odd image, 2h - 1.  A row / column 2y+i that is not stored is the one-pixel
// reflect pad of RealESRGANer's mod-2 rule (torch 'reflect': row H reads row H - 2), read by index -- there is no padded copy.
struct SrcU8Unshuffle {
    typedef uint8_t sample;
    int H, W;
    __device__ Unshuffled get(const uint8_t* in, size_t, int t, int ly, int lx, int, int) const {
        const uint8_t* img = in + (size_t)t * H * W * 3;
        Unshuffled p;
#pragma unroll
        for (int di = 0; di < 2; ++di) {
            const int sy0 = 2 * ly + di, sy = sy0 < H ? sy0 : 2 * H - 2 - sy0;
#pragma unroll
            for (int dj = 0; dj < 2; ++dj) {
                const int sx0 = 2 * lx + dj, sx = sx0 < W ? sx0 : 2 * W - 2 - sx0;
                const uint8_t* s = img + ((size_t)sy * W + sx) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) p.v[c * 4 + di * 2 + dj] = (float)s[c];
            }
        }
        return p;
    }
};

// [B,3,2h,2w] fp32 (plane = 2h * 2w samples per colour), values x * scale (255: the f32 entries feed [0,1] floats)
struct SrcF32Unshuffle {
    typedef float sample;
    float scale;
    size_t plane;
    __device__ Unshuffled get(const float* x, size_t, int n, int y, int xx, int, int w) const {
        Unshuffled p;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int di = 0; di < 2; ++di)
#pragma unroll
                for (int dj = 0; dj < 2; ++dj)
                    p.v[c * 4 + di * 2 + dj] = x[((size_t)n * 3 + c) * plane + (size_t)(2 * y + di) * (2 * w) + 2 * xx + dj] * scale;
        return p;
    }
};

// plane pixel i of B tiles of h x w: where it lands, then the source reads and stores it
template <class Src, class Place>
__device__ inline void pack_pixel(size_t i, const typename Src::sample* in, int h, int w, Place at, Src src, char* blk, int Hp, int Wp) {
    const int lx = (int)(i % w);
    const size_t r = i / w;
    const int ly = (int)(r % h);
    const int t = (int)(r / h);
    int n = t, y = ly, x = lx;
    at.move(n, y, x, h, w);
    src.get(in, i, t, ly, lx, h, w).store(blk + (((size_t)n * Hp + y + 1) * Wp + x + 1) * 32);
}

// The kernels: one per built pair of source and placement, each the grid-stride loop around pack_pixel.  They are not one kernel
// template: each takes the scalars it uses, as scalars and in this order, because handed over as structs they arrive through other
// scalar loads, and with the loop inside a __device__ function blockDim.x keeps the device library's partial-block select -- either
// way the registers of the whole loop come out renamed.  So a new input kind costs a source struct, a kernel of four lines here and
// a branch in launch_pack_tiles.
__global__ void pack_u8_kernel(const uint8_t* __restrict__ in, int N, int H, int W, char* __restrict__ blk, int Hp, int Wp) {
    const size_t total = (size_t)N * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        pack_pixel(i, in, H, W, Plain{}, SrcU8{}, blk, Hp, Wp);
}
__global__ void pack_u8_mosaic_kernel(const uint8_t* __restrict__ in, int B, int h, int w, int kx, int ky, char* __restrict__ blk, int Hp, int Wp) {
    const size_t total = (size_t)B * h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        pack_pixel(i, in, h, w, Cells{kx, ky}, SrcU8{}, blk, Hp, Wp);
}
__global__ void pack_u16_kernel(const uint16_t* __restrict__ in, int N, int H, int W, int lo, int hi, char* __restrict__ blk, int Hp, int Wp) {
    const size_t total = (size_t)N * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        pack_pixel(i, in, H, W, Plain{}, SrcU16{lo, hi}, blk, Hp, Wp);
}
__global__ void pack_u16_mosaic_kernel(const uint16_t* __restrict__ in, int B, int h, int w, int kx, int ky, int lo, int hi, char* __restrict__ blk, int Hp, int Wp) {
    const size_t total = (size_t)B * h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        pack_pixel(i, in, h, w, Cells{kx, ky}, SrcU16{lo, hi}, blk, Hp, Wp);
}
__global__ void pack_u8_unshuffle_kernel(const uint8_t* __restrict__ in, int N, int H, int W, int h, int w, char* __restrict__ blk, int Hp, int Wp) {
    const size_t total = (size_t)N * h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        pack_pixel(i, in, h, w, Plain{}, SrcU8Unshuffle{H, W}, blk, Hp, Wp);
}
__global__ void pack_u8_unshuffle_mosaic_kernel(const uint8_t* __restrict__ in, int B, int h, int w, int kx, int ky, char* __restrict__ blk, int Hp, int Wp) {
    const size_t total = (size_t)B * h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        // pack_pixel with the read of whole 2h x 2w tiles (no reflect) written out: behind get() the compiler shares the address
        // arithmetic of the two columns before it unrolls, and the loop comes out with other registers and waits
        const int lx = (int)(i % w);
        const size_t r = i / w;
        const int ly = (int)(r % h);
        const int t = (int)(r / h);
        int n = t, y = ly, x = lx;
        Cells{kx, ky}.move(n, y, x, h, w);
        const uint8_t* img = in + (size_t)t * (4 * h) * w * 3;
        Unshuffled p;
#pragma unroll
        for (int di = 0; di < 2; ++di)
#pragma unroll
            for (int dj = 0; dj < 2; ++dj) {
                const uint8_t* s = img + ((size_t)(2 * ly + di) * (2 * w) + 2 * lx + dj) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) p.v[c * 4 + di * 2 + dj] = (float)s[c];
            }
        p.store(blk + (((size_t)n * Hp + y + 1) * Wp + x + 1) * 32);
    }
}
__global__ void pack_f32_nchw_unshuffle_kernel(const float* __restrict__ x, int N, int h, int w, float scale, char* __restrict__ blk, int Hp, int Wp) {
    const size_t total = (size_t)N * h * w;
    const size_t plane = (size_t)(2 * h) * (2 * w);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        pack_pixel(i, x, h, w, Plain{}, SrcF32Unshuffle{scale, plane}, blk, Hp, Wp);
}

hipError_t launch_pack_tiles(const TileIn& in, int unshuffle, float f32_scale, int B, int h, int w, int kx, int ky, char* blk, int Hp, int Wp,
                             hipStream_t st) {
    const bool mosaic = kx > 0;
    const dim3 grid(grid_for((size_t)B * h * w, 4096)), block(256);
    const uint8_t* u8 = (const uint8_t*)in.p;
    const uint16_t* u16 = (const uint16_t*)in.p;
    if (in.kind == TILE_F32 && !mosaic) {
        if (unshuffle == 2) hipLaunchKernelGGL(pack_f32_nchw_unshuffle_kernel, grid, block, 0, st, (const float*)in.p, B, h, w, f32_scale, blk, Hp, Wp);
        else return launch_pack_f32_nchw((const float*)in.p, B, 3, h, w, f32_scale, blk, 1, Hp, Wp, st);
    } else if (in.kind == TILE_U8 && unshuffle == 2) {
        if (mosaic) hipLaunchKernelGGL(pack_u8_unshuffle_mosaic_kernel, grid, block, 0, st, u8, B, h, w, kx, ky, blk, Hp, Wp);
        else hipLaunchKernelGGL(pack_u8_unshuffle_kernel, grid, block, 0, st, u8, B, in.src_h, in.src_w, h, w, blk, Hp, Wp);
    } else if (in.kind == TILE_U8 && unshuffle == 1) {
        if (mosaic) hipLaunchKernelGGL(pack_u8_mosaic_kernel, grid, block, 0, st, u8, B, h, w, kx, ky, blk, Hp, Wp);
        else hipLaunchKernelGGL(pack_u8_kernel, grid, block, 0, st, u8, B, h, w, blk, Hp, Wp);
    } else if (in.kind == TILE_U16 && unshuffle == 1) {
        if (mosaic) hipLaunchKernelGGL(pack_u16_mosaic_kernel, grid, block, 0, st, u16, B, h, w, kx, ky, in.lo, in.hi, blk, Hp, Wp);
        else hipLaunchKernelGGL(pack_u16_kernel, grid, block, 0, st, u16, B, h, w, in.lo, in.hi, blk, Hp, Wp);
    } else {
        return hipErrorInvalidValue;   // not built: f32 mosaics; u16 at scale 2 (24 unshuffled channels need a second input block)
    }
    return hipGetLastError();
}

__global__ void pack_f32_nchw_kernel(const float* __restrict__ x, int N, int C, int H, int W, float scale,
                                     char* __restrict__ blk, int NB, int Hp, int Wp) {
    const size_t total = (size_t)N * C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % W);
        size_t r = i / W;
        const int y = (int)(r % H);
        r /= H;
        const int c = (int)(r % C);
        const int n = (int)(r / C);
        f16* d = (f16*)(blk + ((((size_t)n * NB + (c >> 4)) * Hp + y + 1) * Wp + xx + 1) * 32) + (c & 15);
        // fp16(fp32(x * scale)): the product rounded to fp32, then to fp16, as pack_f32_nchw_unshuffle_kernel's v_mul_f32 +
        // v_cvt_pk_f16_f32 do.  Left to itself the compiler selects one v_fma_mixlo_f16 for (f16)(x[i] * scale) (__fmul_rn does
        // not stop it), which rounds the exact product once: an fp16 ulp apart wherever the fp32 product lands on an fp16 tie
        // (x = 0.21868873f: 55.78125 against 55.75).  The empty asm keeps the fp32 product in a register.
        float v = x[i] * scale;
        asm volatile("" : "+v"(v));
        *d = (f16)v;
    }
}

hipError_t launch_pack_f32_nchw(const float* d_x, int N, int C, int H, int W, float scale, char* blk, int NB, int Hp,
                                int Wp, hipStream_t st) {
    hipLaunchKernelGGL(pack_f32_nchw_kernel, dim3(grid_for((size_t)N * C * H * W, 4096)), dim3(256), 0, st, d_x, N, C, H, W, scale, blk, NB, Hp, Wp);
    return hipGetLastError();
}

// one pixel of two fp16 blocks of 16 channels (ppx * 32 bytes apart) x scale -> 32 e4m3 bytes, saturating at +-448
struct E4m3Pixel { uint4 a, b; };
__device__ inline E4m3Pixel f16_pixel_to_e4m3(const char* src, size_t ppx, float scale) {
    uint32_t o[8];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const f16* v = (const f16*)(src + (size_t)b * ppx * 32);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float f[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = __builtin_amdgcn_fmed3f((float)v[4 * q + k] * scale, -448.0f, 448.0f);
            int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
            w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true);
            o[4 * b + q] = (uint32_t)w;
        }
    }
    return E4m3Pixel{make_uint4(o[0], o[1], o[2], o[3]), make_uint4(o[4], o[5], o[6], o[7])};
}

// conv_body's correction operands (S2SR_PREC_F16_HP): the trunk arrives as an fp16 pair (hi = dense
// blocks 0..3, lo = the trunk-lo tensor); the split-operand kernel wants e4m3 planes of 32 channels
// [lo*2^11 plane 0, plane 1, hi plane 0, plane 1] in the same padded geometry (halo pixels are zero
// in both inputs, so the whole padded tensor is converted).  One thread = one pixel of one plane.
// lo_e4m3_exp >= 0: the lo half arrives as e4m3(lo * 2^lo_e4m3_exp) planes already (the one-wave-per-SIMD trunk keeps it so);
// it is rescaled to the 2^11 the split-operand kernel expects.
__global__ void trunk_to_fp8_kernel(const char* __restrict__ hi, size_t hi_img, const char* __restrict__ lo, size_t lo_img,
                                    int lo_e4m3_exp, int N, size_t ppx, char* __restrict__ out) {
    const size_t total = (size_t)N * 4 * ppx;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i % ppx;
        const int plane = (int)((i / ppx) & 3);
        const int n = (int)(i / (4 * ppx));
        const bool is_hi = plane >= 2;
        if (!is_hi && lo_e4m3_exp >= 0) {
            const uint32_t* v = (const uint32_t*)(lo + (size_t)n * lo_img + (size_t)plane * ppx * 32 + pix * 32);
            const float rs = ldexpf(1.0f, 11 - lo_e4m3_exp);
            uint32_t o8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int w0 = (int)v[q];
                const float f0 = __builtin_amdgcn_fmed3f(__builtin_amdgcn_cvt_f32_fp8(w0, 0) * rs, -448.0f, 448.0f);
                const float f1 = __builtin_amdgcn_fmed3f(__builtin_amdgcn_cvt_f32_fp8(w0, 1) * rs, -448.0f, 448.0f);
                const float f2 = __builtin_amdgcn_fmed3f(__builtin_amdgcn_cvt_f32_fp8(w0, 2) * rs, -448.0f, 448.0f);
                const float f3 = __builtin_amdgcn_fmed3f(__builtin_amdgcn_cvt_f32_fp8(w0, 3) * rs, -448.0f, 448.0f);
                int w = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
                w = __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, w, true);
                o8[q] = (uint32_t)w;
            }
            uint4* d8 = (uint4*)(out + ((size_t)n * 4 + plane) * ppx * 32 + pix * 32);
            d8[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
            d8[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
            continue;
        }
        const char* src = (is_hi ? hi + (size_t)n * hi_img : lo + (size_t)n * lo_img) + (size_t)(2 * (plane & 1)) * ppx * 32 + pix * 32;
        *(E4m3Pixel*)(out + ((size_t)n * 4 + plane) * ppx * 32 + pix * 32) = f16_pixel_to_e4m3(src, ppx, is_hi ? 1.0f : 2048.0f);
    }
}

hipError_t launch_trunk_to_fp8(const char* hi, size_t hi_img, const char* lo, size_t lo_img, int lo_e4m3_exp, int N, int Hp, int Wp, char* out,
                               hipStream_t st) {
    const size_t ppx = (size_t)Hp * Wp, total = (size_t)N * 4 * ppx;
    hipLaunchKernelGGL(trunk_to_fp8_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, st, hi, hi_img, lo, lo_img, lo_e4m3_exp, N, ppx, out);
    return hipGetLastError();
}

// fp8 trunk mode: the trunk x (fp16, 4 blocks of 16 channels) -> the two e4m3 planes e4m3(x * 2^x_exp) the RDB convs
// read (whole padded tensor: halo zeros stay zeros).  One thread = one pixel of one plane.
__global__ void xh_to_fp8_kernel(const char* __restrict__ xh, size_t xh_img, int N, size_t ppx, float scale, char* __restrict__ out,
                                 size_t out_img) {
    const size_t total = (size_t)N * 2 * ppx;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i % ppx;
        const int plane = (int)((i / ppx) & 1);
        const int n = (int)(i / (2 * ppx));
        *(E4m3Pixel*)(out + (size_t)n * out_img + (size_t)plane * ppx * 32 + pix * 32) =
            f16_pixel_to_e4m3(xh + (size_t)n * xh_img + (size_t)(2 * plane) * ppx * 32 + pix * 32, ppx, scale);
    }
}

hipError_t launch_xh_to_fp8(const char* xh, size_t xh_img, int N, int Hp, int Wp, int x_exp, char* out, size_t out_img, hipStream_t st) {
    const size_t ppx = (size_t)Hp * Wp, total = (size_t)N * 2 * ppx;
    hipLaunchKernelGGL(xh_to_fp8_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, st, xh, xh_img, N, ppx, ldexpf(1.0f, x_exp), out, out_img);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Device-side weight repack for the 345 RDB convs (the receive buffer of the RCCL weight broadcast goes straight into MFMA
// fragment order: no host copy of the 67 MB blob).  Same layouts, same roundings as the host packers in conv3x3.hip /
// conv_trunk.hip (pack_conv_weights nseg = 1, pack_conv_weights_f8), which stay for the six head/tail convs and the test hooks.
// ------------------------------------------------------------------------------------------
// fp16 trunk: out[stage][tap][ct][lane][8] = fp16(W[co = ct*32 + (lane&31)][ci = stage*16 + 8*(lane>>5) + j][tap])
__global__ void pack_trunk_f16_kernel(const float* __restrict__ w, int cin, int cout, int ns, int CT, f16* __restrict__ out) {
    const size_t total = (size_t)ns * 9 * CT * 64 * 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7), l = (int)((i >> 3) & 63);
        size_t r = i >> 9;
        const int ct = (int)(r % CT); r /= CT;
        const int t = (int)(r % 9);
        const int st = (int)(r / 9);
        const int co = ct * 32 + (l & 31), ci = st * 16 + 8 * (l >> 5) + j;
        out[i] = (co < cout && ci < cin) ? (f16)w[((size_t)co * cin + ci) * 9 + t] : (f16)0.f;
    }
}

hipError_t launch_pack_trunk_f16(const float* d_w, int cin, int cout, void* d_out, hipStream_t st) {
    const int ns = (cin + 15) / 16, CT = (cout + 31) / 32;
    const size_t total = (size_t)ns * 9 * CT * 512;
    hipLaunchKernelGGL(pack_trunk_f16_kernel, dim3((unsigned)grid_for(total, 0x7fffffff)), dim3(256), 0, st, d_w, cin, cout, ns, CT, (f16*)d_out);
    return hipGetLastError();
}

// fp8 trunk, pass 1: per output channel the largest k with max|w_co| * 2^k < 448; wscale[co] = 127 - k (64 entries)
__global__ void f8_scale_kernel(const float* __restrict__ w, int cin, int cout, int32_t* __restrict__ wscale) {
    __shared__ float red[256];
    const int co = blockIdx.x;
    float m = 0.f;
    if (co < cout)
        for (int i = threadIdx.x; i < cin * 9; i += 256) m = fmaxf(m, fabsf(w[(size_t)co * cin * 9 + i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if ((int)threadIdx.x < s2) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s2]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int k = 0;
        m = red[0];
        if (m > 0.f) {
            int e;
            const float f = frexpf(m, &e);            // m = f * 2^e, f in [0.5, 1); 448 = 0.875 * 2^9
            k = (f < 0.875f ? 9 : 8) - e;
        }
        k = k > 100 ? 100 : (k < -100 ? -100 : k);
        wscale[co] = 127 - k;
    }
}

// pass 2: out[plane][tap][ct][16-B half][cout row][16] = e4m3(W * 2^k_co), phantom plane (odd plane counts) all zero
__global__ void pack_trunk_f8_kernel(const float* __restrict__ w, int cin, int cout, int nreal, int npad, int CT,
                                     const int32_t* __restrict__ wscale, uint8_t* __restrict__ out) {
    const size_t total4 = (size_t)npad * 9 * CT * 256;          // groups of 4 bytes
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const int j4 = (int)(i & 3), row = (int)((i >> 2) & 31), h16 = (int)((i >> 7) & 1);
        size_t r = i >> 8;
        const int ct = (int)(r % CT); r /= CT;
        const int t = (int)(r % 9);
        const int pl = (int)(r / 9);
        const int co = ct * 32 + row;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (pl < nreal && co < cout) {
            const float sc = ldexpf(1.0f, 127 - wscale[co]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ci = 32 * pl + 16 * h16 + 4 * j4 + q;
                if (ci < cin) v[q] = w[((size_t)co * cin + ci) * 9 + t] * sc;     // |v| < 448 by construction of k_co
            }
        }
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], pk, true);
        ((uint32_t*)out)[i] = (uint32_t)pk;
    }
}

hipError_t launch_pack_trunk_f8(const float* d_w, int cin, int cout, void* d_out, int32_t* d_wscale, hipStream_t st) {
    const int nreal = (cin + 31) / 32, npad = (nreal + 1) & ~1, CT = (cout + 31) / 32;
    hipLaunchKernelGGL(f8_scale_kernel, dim3(64), dim3(256), 0, st, d_w, cin, cout, d_wscale);
    const size_t total4 = (size_t)npad * 9 * CT * 256;
    hipLaunchKernelGGL(pack_trunk_f8_kernel, dim3((unsigned)grid_for(total4, 0x7fffffff)), dim3(256), 0, st, d_w, cin, cout, nreal, npad, CT, d_wscale,
                       (uint8_t*)d_out);
    return hipGetLastError();
}

// biases of all convs: blob offsets -> [nconv][64] fp32, zero padded
__global__ void gather_bias_kernel(const float* __restrict__ blob, const uint64_t* __restrict__ off, const int32_t* __restrict__ cout,
                                   int nconv, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nconv * 64) return;
    const int c = i >> 6, k = i & 63;
    out[i] = k < cout[c] ? blob[off[c] + k] : 0.f;
}

hipError_t launch_gather_bias(const float* d_blob, const uint64_t* d_off, const int32_t* d_cout, int nconv, float* d_out, hipStream_t st) {
    hipLaunchKernelGGL(gather_bias_kernel, dim3((nconv * 64 + 255) / 256), dim3(256), 0, st, d_blob, d_off, d_cout, nconv, d_out);
    return hipGetLastError();
}

// fp8 calibration: running max |v| of an fp16 blocked tensor / of an e4m3 plane tensor (whole padded extent: halos are
// zero) into one float (bit pattern compared as unsigned: valid for non-negative floats)
__global__ void absmax_f16_kernel(const f16* __restrict__ v, size_t n, float* __restrict__ out) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float a = fabsf((float)v[i]);
        m = (a == a && a > m) ? a : m;
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)out, __float_as_uint(m));
}
__global__ void absmax_e4m3_kernel(const uint8_t* __restrict__ v, size_t n, float scale_inv, float* __restrict__ out) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int b = v[i] & 0x7f;
        if (b == 0x7f) continue;                                  // NaN code (never stored: producers clamp)
        const int e = b >> 3, mm = b & 7;
        const float a = e == 0 ? (float)mm * 0.001953125f : ldexpf((float)(8 + mm), e - 10);
        m = fmaxf(m, a);
    }
    m *= scale_inv;
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax((unsigned int*)out, __float_as_uint(m));
}
hipError_t launch_absmax_f16(const void* d, size_t n_halves, float* d_out, hipStream_t st) {
    hipLaunchKernelGGL(absmax_f16_kernel, dim3((unsigned)capped_grid(1024, (long long)((n_halves + 255) / 256), GF_PACK)), dim3(256), 0, st, (const f16*)d, n_halves, d_out);
    return hipGetLastError();
}
hipError_t launch_absmax_e4m3(const void* d, size_t n_bytes, int exp2, float* d_out, hipStream_t st) {
    hipLaunchKernelGGL(absmax_e4m3_kernel, dim3((unsigned)capped_grid(1024, (long long)((n_bytes + 255) / 256), GF_PACK)), dim3(256), 0, st, (const uint8_t*)d, n_bytes, ldexpf(1.0f, -exp2), d_out);
    return hipGetLastError();
}

// R <-> B of a u8 HWC image, in place or into another buffer: the reference feeds the net BGR and turns its output back
// (cv2.cvtColor RGB2BGR / BGR2RGB, wow_sr.py:85,103)
__global__ void swap_rb_kernel(const uint8_t* __restrict__ in, size_t npx, uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        const uint8_t r = in[3 * i], g = in[3 * i + 1], b = in[3 * i + 2];
        out[3 * i] = b; out[3 * i + 1] = g; out[3 * i + 2] = r;
    }
}

hipError_t launch_swap_rb_u8(const uint8_t* d_in, size_t npx, uint8_t* d_out, hipStream_t st) {
    const int grid = grid_for(npx, 8192);
    hipLaunchKernelGGL(swap_rb_kernel, dim3(grid ? grid : 1), dim3(256), 0, st, d_in, npx, d_out);
    return hipGetLastError();
}

// T windows of wh x ww out of an H x W image of 1- or 2-byte samples.  REFLECT (scale 2 with an odd H or W): the windows are planned
// on the reflect-padded image (one row / column more); that row / column is read by index (row H = row H - 2, as torch's 'reflect').
template <class S, bool REFLECT>
__global__ void gather_windows_kernel(const S* __restrict__ img, int H, int W, const int32_t* __restrict__ rects,
                                      int T, int wh, int ww, S* __restrict__ tiles) {
    const size_t total = (size_t)T * wh * ww * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        size_t r = i / 3;
        const int x = (int)(r % ww);
        r /= ww;
        const int y = (int)(r % wh);
        const int t = (int)(r / wh);
        int sy = rects[t * 4 + 0] + y, sx = rects[t * 4 + 2] + x;
        if constexpr (REFLECT) { sy = sy < H ? sy : 2 * H - 2 - sy; sx = sx < W ? sx : 2 * W - 2 - sx; }
        tiles[i] = img[((size_t)sy * W + sx) * 3 + c];
    }
}

template <class S, bool REFLECT>
static hipError_t gather_windows(const S* d_img, int H, int W, const int32_t* d_rects, int T, int wh, int ww, S* d_tiles, hipStream_t st) {
    hipLaunchKernelGGL((gather_windows_kernel<S, REFLECT>), dim3(grid_for((size_t)T * wh * ww * 3, 8192)), dim3(256), 0, st, d_img, H, W, d_rects,
                       T, wh, ww, d_tiles);
    return hipGetLastError();
}
hipError_t launch_gather_windows(const uint8_t* d_img, int H, int W, const int32_t* d_rects, int T, int wh, int ww, bool reflect,
                                 uint8_t* d_tiles, hipStream_t st) {
    return reflect ? gather_windows<uint8_t, true>(d_img, H, W, d_rects, T, wh, ww, d_tiles, st)
                   : gather_windows<uint8_t, false>(d_img, H, W, d_rects, T, wh, ww, d_tiles, st);
}
hipError_t launch_gather_windows(const uint16_t* d_img, int H, int W, const int32_t* d_rects, int T, int wh, int ww, uint16_t* d_tiles,
                                 hipStream_t st) {
    return gather_windows<uint16_t, false>(d_img, H, W, d_rects, T, wh, ww, d_tiles, st);
}

// rowmap[2*oy] = window-row index ty (or -1: not covered), rowmap[2*oy+1] = row inside that
// window's output; colmap likewise with tx.
// "Later windows overwrite" (cnn_super_resolution.py:278) == the LAST (ty, tx) in loop order
// whose paste rectangle contains the pixel; paste rectangles are row-range x column-range
// products, so that is (last covering ty, last covering tx) -- resolved on the host into
// these maps, which makes the paste race-free and order-independent.
// PLANAR: the tiles are [T,3,oth,otw] (the net's fp32 output), else [T,oth,otw,3]; the output is HWC either way.
template <class E, bool PLANAR>
__global__ void stitch_kernel(const E* __restrict__ tiles, int oth, int otw, const int32_t* __restrict__ rowmap,
                              const int32_t* __restrict__ colmap, int tilesX, int OH, int OW, E* __restrict__ out) {
    const size_t total = (size_t)OH * OW * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        const size_t r = i / 3;
        const int ox = (int)(r % OW);
        const int oy = (int)(r / OW);
        const int ty = rowmap[2 * oy], sy = rowmap[2 * oy + 1];
        const int tx = colmap[2 * ox], sx = colmap[2 * ox + 1];
        E v = 0;   // reference output starts as zeros (cnn_super_resolution.py:242)
        if (ty >= 0 && tx >= 0)
            v = PLANAR ? tiles[(((size_t)(ty * tilesX + tx) * 3 + c) * oth + sy) * otw + sx]
                       : tiles[(((size_t)(ty * tilesX + tx) * oth + sy) * otw + sx) * 3 + c];
        out[i] = v;
    }
}

template <class E, bool PLANAR>
static hipError_t stitch(const E* d_tiles, int tilesX, int oth, int otw, const int32_t* d_rowmap, const int32_t* d_colmap, int OH, int OW,
                         E* d_out, hipStream_t st) {
    hipLaunchKernelGGL((stitch_kernel<E, PLANAR>), dim3(grid_for((size_t)OH * OW * 3, 8192)), dim3(256), 0, st, d_tiles, oth, otw, d_rowmap,
                       d_colmap, tilesX, OH, OW, d_out);
    return hipGetLastError();
}
hipError_t launch_stitch(const uint8_t* d_tiles, int tilesX, int oth, int otw, const int32_t* d_rowmap, const int32_t* d_colmap, int OH,
                         int OW, uint8_t* d_out, hipStream_t st) {
    return stitch<uint8_t, false>(d_tiles, tilesX, oth, otw, d_rowmap, d_colmap, OH, OW, d_out, st);
}
hipError_t launch_stitch(const float* d_tiles, int tilesX, int oth, int otw, const int32_t* d_rowmap, const int32_t* d_colmap, int OH,
                         int OW, float* d_out, hipStream_t st) {
    return stitch<float, true>(d_tiles, tilesX, oth, otw, d_rowmap, d_colmap, OH, OW, d_out, st);
}

__device__ inline uint32_t quant_u16(float y, float range, int lo) {
    const float c = fminf(fmaxf(y, 0.f), 1.f);
    return (uint32_t)(lo + (int)rintf(__fmul_rn(c, range)));   // a lone fp32 product: nothing here to fuse it with
}

// Crop + paste + quantise: planar fp32 tiles [.., 3, oth, otw] -> rows [0, OH) of an HWC u16 image through the paste maps, as
// stitch_kernel<float, true> reads them (rowmap already offset to the band's first row; window (ty, tx) is tile ty * tilesX + tx - tile0
// of `tiles`, so a chunk's buffer holds only its own window rows).  rowmap == nullptr: a plain batch, row oy of the output is row
// oy % oth of tile oy / oth.  One thread = 4 consecutive output pixels (OW is a multiple of 4: the x4 net): paste rectangles
// start and end on multiples of 4 on both sides, so the 4 pixels are one float4 per colour plane (checked, with a scalar
// route), and leave as 24 contiguous bytes.
__global__ void stitch_quant_u16_kernel(const float* __restrict__ tiles, int oth, int otw, const int32_t* __restrict__ rowmap,
                                        const int32_t* __restrict__ colmap, int tilesX, int tile0, int OH, int OW, int lo, int hi,
                                        uint16_t* __restrict__ out) {
    const int gw = OW >> 2;
    const size_t total = (size_t)OH * gw;
    const float range = (float)(hi - lo);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % gw) << 2;
        const int oy = (int)(i / gw);
        int ty, sy;
        if (rowmap) { ty = rowmap[2 * oy]; sy = rowmap[2 * oy + 1]; }
        else { ty = oy / oth; sy = oy - ty * oth; }
        float v[3][4];
        int tx[4], sx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (colmap) { tx[k] = colmap[2 * (ox + k)]; sx[k] = colmap[2 * (ox + k) + 1]; }
            else { tx[k] = 0; sx[k] = ox + k; }
        }
        const bool vec = ty >= 0 && tx[0] >= 0 && tx[1] == tx[0] && tx[2] == tx[0] && tx[3] == tx[0] && sx[1] == sx[0] + 1 &&
                         sx[2] == sx[0] + 2 && sx[3] == sx[0] + 3 && (sx[0] & 3) == 0 && (otw & 3) == 0;
        if (vec) {
            const float* p = tiles + (((size_t)(ty * tilesX + tx[0] - tile0) * 3) * oth + sy) * otw + sx[0];
            const size_t plane = (size_t)oth * otw;
            if (((uintptr_t)p & 15) == 0 && (plane & 3) == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 f = *(const float4*)(p + c * plane);
                    v[c][0] = f.x; v[c][1] = f.y; v[c][2] = f.z; v[c][3] = f.w;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[c][k] = p[c * plane + k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    v[c][k] = (ty >= 0 && tx[k] >= 0) ? tiles[(((size_t)(ty * tilesX + tx[k] - tile0) * 3 + c) * oth + sy) * otw + sx[k]] : 0.f;
        }
        uint32_t q[12];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) q[3 * k + c] = quant_u16(v[c][k], range, lo);
        // (oy * OW + ox) * 6 bytes: a multiple of 24, so the three 8-byte stores are aligned
        uint2* d = (uint2*)(out + ((size_t)oy * OW + ox) * 3);
        d[0] = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
        d[1] = make_uint2(q[4] | (q[5] << 16), q[6] | (q[7] << 16));
        d[2] = make_uint2(q[8] | (q[9] << 16), q[10] | (q[11] << 16));
    }
}

hipError_t launch_stitch_quant_u16(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rowmap,
                                   const int32_t* d_colmap, int OH, int OW, int lo, int hi, uint16_t* d_out, hipStream_t st) {
    if (OH <= 0 || OW <= 0 || (OW & 3) || ((uintptr_t)d_out & 7)) return hipErrorInvalidValue;
    const size_t total = (size_t)OH * (OW >> 2);
    hipLaunchKernelGGL(stitch_quant_u16_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, st, d_tiles, oth, otw, d_rowmap, d_colmap, tilesX, tile0, OH, OW,
                       lo, hi, d_out);
    return hipGetLastError();
}

// ---- the seam-blended stitch (s2sr_enhance_blend_*) ---------------------------------------------------------------------------
// Planar fp32 tiles [.., 3, oth, otw] -> rows [0, OH) of an HWC image, cross-faded inside the ramps of the blend plan
// (blend_plan.h).  rows / cols: six ints per output row / column, {a, ia, b, ib, bits of the fp32 weight of b, 0}: the two windows
// (window (ty, tx) is tile ty * tilesX + tx - tile0 of `tiles`), the offsets inside their outputs, and w = 0 outside every ramp,
// where a == b.  With A = (a_y, a_x), B = (a_y, b_x), C = (b_y, a_x), D = (b_y, b_x):
//     top = A + wx (B - A),  bot = C + wx (D - C),  v = top + wy (bot - top)
// each product and sum rounded on its own (no FMA), and a term whose weight is 0 neither read nor computed (A + 0 * x is not A
// for A = -0 or an infinite x).  The output: u8 trunc(clip(v * 255, 0, 255)) as conv_last's epilogue, u16 quant_u16, or v itself.
struct BlendQ { int lo; float range; };
__device__ inline uint32_t blend_quant(float v, uint8_t, const BlendQ&) { return (uint32_t)(int)fminf(fmaxf(__fmul_rn(v, 255.0f), 0.f), 255.f); }
__device__ inline uint32_t blend_quant(float v, uint16_t, const BlendQ& q) { return quant_u16(v, q.range, q.lo); }
__device__ inline uint32_t blend_quant(float v, float, const BlendQ&) { return __float_as_uint(v); }

// a + w (b - a), the difference, the product and the sum each rounded to fp32.  This file is compiled with contraction on, and
// __fmul_rn / __fadd_rn are header functions whose operators carry that setting with them when inlined (conv3x3.hip, where the
// epilogues use them, is built with -ffp-contract=off): the pragma on plain operators is what keeps the product and the sum apart.
__device__ inline float blend_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
    const float d = b - a;
    const float p = w * d;
    return a + p;
}

// One thread = 4 consecutive output pixels of a row.  Where the 4 share their windows (a ramp edge does not split them: edges of
// shortened ramps fall on any column) and the offsets are consecutive and 16-byte aligned, each sample row is one float4 per colour
// plane; else pixel by pixel.  The stores are 12 (u8) / 24 (u16) / 48 (fp32) contiguous bytes when OW is a multiple of 4 (every x4
// net), element by element otherwise (the x2 net on an odd width).  swap: R and B exchanged in the pixels written.
template <class O>
__global__ void stitch_blend_kernel(const float* __restrict__ tiles, int oth, int otw, const int32_t* __restrict__ rows,
                                    const int32_t* __restrict__ cols, int tilesX, int tile0, int OH, int OW, int swap, BlendQ q,
                                    O* __restrict__ out) {
    const int gw = (OW + 3) >> 2;
    const size_t total = (size_t)OH * gw;
    const size_t plane = (size_t)oth * otw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % gw) << 2;
        const int oy = (int)(i / gw);
        const int npx = OW - ox < 4 ? OW - ox : 4;
        const int32_t* re = rows + 6 * (size_t)oy;
        const int ya = re[0], iya = re[1], yb = re[2], iyb = re[3];
        const float wy = __int_as_float(re[4]);
        int xa[4], ixa[4], xb[4], ixb[4];
        float wx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int32_t* ce = cols + 6 * (size_t)(ox + (k < npx ? k : 0));
            xa[k] = ce[0]; ixa[k] = ce[1]; xb[k] = ce[2]; ixb[k] = ce[3]; wx[k] = __int_as_float(ce[4]);
        }
        // start of the planes of window (ty, tx), row sy
        auto at = [&](int ty, int sy, int tx) { return tiles + (((size_t)(ty * tilesX + tx - tile0) * 3) * oth + sy) * otw; };
        bool vec = npx == 4 && (otw & 3) == 0 && (plane & 3) == 0 && ((uintptr_t)tiles & 15) == 0 && (ixa[0] & 3) == 0 && (ixb[0] & 3) == 0;
#pragma unroll
        for (int k = 1; k < 4; ++k)
            vec = vec && xa[k] == xa[0] && xb[k] == xb[0] && ixa[k] == ixa[0] + k && ixb[k] == ixb[0] + k && (wx[k] != 0.f) == (wx[0] != 0.f);
        float v[3][4];
        if (vec) {
            const bool fx = wx[0] != 0.f, fy = wy != 0.f;
            const float* pA = at(ya, iya, xa[0]) + ixa[0];
            const float* pB = at(ya, iya, xb[0]) + ixb[0];
            const float* pC = at(yb, iyb, xa[0]) + ixa[0];
            const float* pD = at(yb, iyb, xb[0]) + ixb[0];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t[4];
                const float4 A = *(const float4*)(pA + c * plane);
                t[0] = A.x; t[1] = A.y; t[2] = A.z; t[3] = A.w;
                if (fx) {
                    const float4 B = *(const float4*)(pB + c * plane);
                    t[0] = blend_lerp(t[0], B.x, wx[0]); t[1] = blend_lerp(t[1], B.y, wx[1]);
                    t[2] = blend_lerp(t[2], B.z, wx[2]); t[3] = blend_lerp(t[3], B.w, wx[3]);
                }
                if (fy) {
                    float u[4];
                    const float4 Cc = *(const float4*)(pC + c * plane);
                    u[0] = Cc.x; u[1] = Cc.y; u[2] = Cc.z; u[3] = Cc.w;
                    if (fx) {
                        const float4 D = *(const float4*)(pD + c * plane);
                        u[0] = blend_lerp(u[0], D.x, wx[0]); u[1] = blend_lerp(u[1], D.y, wx[1]);
                        u[2] = blend_lerp(u[2], D.z, wx[2]); u[3] = blend_lerp(u[3], D.w, wx[3]);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) t[k] = blend_lerp(t[k], u[k], wy);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) v[c][k] = t[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool fx = wx[k] != 0.f, fy = wy != 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float t = 0.f;
                    if (k < npx) {
                        t = at(ya, iya, xa[k])[c * plane + ixa[k]];
                        if (fx) t = blend_lerp(t, at(ya, iya, xb[k])[c * plane + ixb[k]], wx[k]);
                        if (fy) {
                            float u = at(yb, iyb, xa[k])[c * plane + ixa[k]];
                            if (fx) u = blend_lerp(u, at(yb, iyb, xb[k])[c * plane + ixb[k]], wx[k]);
                            t = blend_lerp(t, u, wy);
                        }
                    }
                    v[c][k] = t;
                }
            }
        }
        uint32_t e[12];                                   // the 4 pixels in output order, quantised (fp32: the value's bits)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) e[3 * k + c] = blend_quant(v[swap ? 2 - c : c][k], O(), q);
        O* d = out + ((size_t)oy * OW + ox) * 3;
        if ((OW & 3) == 0) {   // (oy * OW + ox) * 3 elements: a multiple of 12, so the stores below are aligned (the launcher checks `out`)
            if constexpr (sizeof(O) == 1) {
                uint32_t* d4 = (uint32_t*)d;
#pragma unroll
                for (int j = 0; j < 3; ++j) d4[j] = e[4 * j] | (e[4 * j + 1] << 8) | (e[4 * j + 2] << 16) | (e[4 * j + 3] << 24);
            } else if constexpr (sizeof(O) == 2) {
                uint2* d8 = (uint2*)d;
#pragma unroll
                for (int j = 0; j < 3; ++j) d8[j] = make_uint2(e[4 * j] | (e[4 * j + 1] << 16), e[4 * j + 2] | (e[4 * j + 3] << 16));
            } else {
                uint4* d16 = (uint4*)d;
#pragma unroll
                for (int j = 0; j < 3; ++j) d16[j] = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if (j < 3 * npx) {
                    if constexpr (sizeof(O) == 4) d[j] = __uint_as_float(e[j]);
                    else d[j] = (O)e[j];
                }
        }
    }
}

template <class O>
static hipError_t stitch_blend(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rows, const int32_t* d_cols,
                               int OH, int OW, bool swap_rb, BlendQ q, O* d_out, hipStream_t st) {
    if (OH <= 0 || OW <= 0 || !d_tiles || !d_rows || !d_cols || !d_out) return hipErrorInvalidValue;
    if ((uintptr_t)d_out & ((OW & 3) ? sizeof(O) - 1 : 4 * sizeof(O) - 1)) return hipErrorInvalidValue;   // the kernel's 4-pixel stores
    const size_t total = (size_t)OH * ((OW + 3) >> 2);
    hipLaunchKernelGGL((stitch_blend_kernel<O>), dim3(grid_for(total, 8192)), dim3(256), 0, st, d_tiles, oth, otw, d_rows, d_cols, tilesX, tile0,
                       OH, OW, swap_rb ? 1 : 0, q, d_out);
    return hipGetLastError();
}
hipError_t launch_stitch_blend(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rows, const int32_t* d_cols,
                               int OH, int OW, bool swap_rb, uint8_t* d_out, hipStream_t st) {
    return stitch_blend(d_tiles, tilesX, tile0, oth, otw, d_rows, d_cols, OH, OW, swap_rb, BlendQ{0, 255.f}, d_out, st);
}
hipError_t launch_stitch_blend(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rows, const int32_t* d_cols,
                               int OH, int OW, int lo, int hi, uint16_t* d_out, hipStream_t st) {
    return stitch_blend(d_tiles, tilesX, tile0, oth, otw, d_rows, d_cols, OH, OW, false, BlendQ{lo, (float)(hi - lo)}, d_out, st);
}
hipError_t launch_stitch_blend(const float* d_tiles, int tilesX, int tile0, int oth, int otw, const int32_t* d_rows, const int32_t* d_cols,
                               int OH, int OW, float* d_out, hipStream_t st) {
    return stitch_blend(d_tiles, tilesX, tile0, oth, otw, d_rows, d_cols, OH, OW, false, BlendQ{0, 1.f}, d_out, st);
}

}  // namespace s2sr
