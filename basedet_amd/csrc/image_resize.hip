// Raw-image input on the device: a packed batch of uint8 HWC images, each with its own size -> the stem's input layout, in one pass.
// Per image: bilinear resize to (dst_h, dst_w), optional horizontal flip, zero-pad to (Hp, Wp), (x - mean) / std -- what
// data/transforms.py (ShortestEdgeResize, RandomHorizontalFlip), data/collators.py and bd_pad_normalize produce together, bit for bit.
//
// The resize restates transforms.resize_bilinear operation by operation: source coordinate in float64, floor, fraction cast to fp32,
// neighbours clamped, three fp32 blends of two products each, rint, clamp to a byte.  Every step is one IEEE operation in numpy, so it
// must be one here: multiply-add contraction is OFF in this file (the pragma below and the per-file flag of build.py); a contracted
// a * (1 - fx) + b * fx differs from numpy's in the last bit, and that bit decides rint at a tie.
//
// HBM-bound on the 8 bytes per output pixel.  One lane owns two neighbouring output pixels and stores them with one 16-byte access (row
// pitch and halo width are even, so a pair never straddles the halo edge; an odd dst_w leaves the pair's second pixel in the pad
// region).  A source pixel is three bytes: each of the four taps is ONE unaligned dword load (the fourth byte is ignored), except where
// that dword would end past the packed buffer, which reads the three bytes singly.  Neighbouring lanes share taps; the reuse is left to
// the vector L1 / L2 (the source footprint of an output tile is unbounded under downscaling: no LDS staging).
#include "common.h"

namespace {

constexpr int HALO_Y = 3, HALO_X = 4;
constexpr int GROUP = 32;          // descriptors per launch, passed by value: 32 x 32 bytes of kernel argument

static_assert(sizeof(bd_image_desc) == 32, "bd_image_desc is 32 bytes");
struct ImageGroup { bd_image_desc d[GROUP]; };

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

struct Tap { int i0, i1; float f; };

// output index o of a resize src -> dst: the two clamped source indices and the fp32 fraction between them
__device__ __forceinline__ Tap tap_of(int o, int src, int dst) {
#pragma clang fp contract(off)
    const double c = ((double)o + 0.5) * ((double)src / (double)dst) - 0.5;
    const double fl = floor(c);
    const int i = (int)fl;
    Tap t;
    t.f = (float)(c - fl);
    t.i0 = min(max(i, 0), src - 1);
    t.i1 = min(max(i + 1, 0), src - 1);
    return t;
}

// bytes 0..2 of the result = the pixel's three channels
__device__ __forceinline__ uint32_t load_px(const uint8_t* __restrict__ packed, long long at, long long packed_bytes) {
    if (at + 4 <= packed_bytes) return *reinterpret_cast<const u32_unaligned*>(packed + at);
    return (uint32_t)packed[at] | ((uint32_t)packed[at + 1] << 8) | ((uint32_t)packed[at + 2] << 16);
}

__device__ __forceinline__ float blend(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int ch, float fx, float fy) {
#pragma clang fp contract(off)
    const float fa = (float)((a >> (8 * ch)) & 0xffu), fb = (float)((b >> (8 * ch)) & 0xffu);
    const float fc = (float)((c >> (8 * ch)) & 0xffu), fd = (float)((d >> (8 * ch)) & 0xffu);
    const float top = fa * (1.f - fx) + fb * fx;
    const float bot = fc * (1.f - fx) + fd * fx;
    const float out = top * (1.f - fy) + bot * fy;
    return fminf(fmaxf(rintf(out), 0.f), 255.f);
}

__global__ __launch_bounds__(256) void resize_pad_normalize_kernel(const uint8_t* __restrict__ packed, long long packed_bytes,
                                                                   const ImageGroup g, int Hp, int Wp, float m0, float m1, float m2,
                                                                   float s0, float s1, float s2, bf16_raw* __restrict__ out) {
    const int Wb = Wp + 2 * HALO_X;
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (2 * pair >= Wb) return;
    const int yb = blockIdx.y, n = blockIdx.z;
    const bd_image_desc& d = g.d[n];
    const int y = yb - HALO_Y, x = 2 * pair - HALO_X;
    u32x4_t o = {0u, 0u, 0u, 0u};
    if (y >= 0 && y < Hp && x >= 0 && x < Wp) {
        const uint32_t pad01 = pack_bf2((0.f - m0) / s0, (0.f - m1) / s1), pad2 = pack_bf2((0.f - m2) / s2, 0.f);
        o[0] = o[2] = pad01;
        o[1] = o[3] = pad2;
        if (y < d.dst_h && x < d.dst_w) {
            const Tap ty = tap_of(y, d.src_h, d.dst_h);
            const long long row0 = d.offset + (long long)ty.i0 * d.src_w * 3, row1 = d.offset + (long long)ty.i1 * d.src_w * 3;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (x + k < d.dst_w) {
                    // resize, then flip (Compose's order): output column x is column dst_w - 1 - x of the resized image
                    const Tap tx = tap_of(d.flip ? d.dst_w - 1 - (x + k) : x + k, d.src_w, d.dst_w);
                    const uint32_t a = load_px(packed, row0 + 3ll * tx.i0, packed_bytes), b = load_px(packed, row0 + 3ll * tx.i1, packed_bytes);
                    const uint32_t c = load_px(packed, row1 + 3ll * tx.i0, packed_bytes), e = load_px(packed, row1 + 3ll * tx.i1, packed_bytes);
                    o[2 * k] = pack_bf2((blend(a, b, c, e, 0, tx.f, ty.f) - m0) / s0, (blend(a, b, c, e, 1, tx.f, ty.f) - m1) / s1);
                    o[2 * k + 1] = pack_bf2((blend(a, b, c, e, 2, tx.f, ty.f) - m2) / s2, 0.f);
                }
            }
        }
    }
    const long long px = ((long long)n * gridDim.y + yb) * Wb + 2 * pair;
    *reinterpret_cast<u32x4_t*>(out + px * 4) = o;
}

// ---- bd_resize_bilinear_normalize: a dense fp32 NCHW batch resized to one size (YOLOX's multi-scale pre_process) ------------------------
// The sampling rule of torch.nn.functional.interpolate(mode="bilinear", align_corners=False), which is MegEngine's
// F.vision.interpolate: src = max(0, (dst + 0.5) * in / out - 0.5), neighbours floor(src) and min(floor(src) + 1, in - 1).  The source
// coordinate is float64 (in fp32 its rounding alone, ~800 * 2^-24 of a pixel, would move a blend of bytes by 1e-2); the fraction is cast
// to fp32 once, and a blend is a + f (b - a) written as two explicit FMAs, fma(f, b, fma(-f, a, a)): two roundings per blend instead of the
// four of a (1 - f) + b f, exact (= a) at f = 0 -- which makes dst == (H, W) bd_pad_normalize's bits.  Error against the float64 rule, for
// values in [0, 255] (one rounding there is at most 2^-17): per blend the fraction's cast (255 * 2^-25) and two roundings, so 3 * 2^-17
// after the horizontal pass and 6 * 2^-17 after the vertical one, under 4 * 2^-24 * 255.
//
// HBM-bound: 8 bytes written per output pixel, and the source is read once when upscaling (neighbouring lanes share taps in L1 / L2).  One
// lane owns one output pixel of the halo buffer: its two column taps and two row taps are computed once and serve the three planes; a
// wave reads runs of neighbouring columns of one source row per tap (coalesced up to the scale factor).
struct LinTap { int i0, i1; float f; };

__device__ __forceinline__ LinTap lin_tap(int o, double scale, int src) {
    double c = ((double)o + 0.5) * scale - 0.5;
    c = c < 0.0 ? 0.0 : c;
    const double fl = floor(c);
    LinTap t;
    t.i0 = min((int)fl, src - 1);
    t.i1 = min(t.i0 + 1, src - 1);
    t.f = (float)(c - fl);
    return t;
}

__device__ __forceinline__ float lerp_fma(float a, float b, float f) { return fmaf(f, b, fmaf(-f, a, a)); }

__global__ __launch_bounds__(256) void resize_bilinear_normalize_kernel(const float* __restrict__ in, int H, int W, int dst_h, int dst_w,
                                                                        int Hp, int Wp, double sy, double sx, float m0, float m1, float m2,
                                                                        float s0, float s1, float s2, bf16_raw* __restrict__ out) {
    const int Wb = Wp + 2 * HALO_X;
    const int xb = blockIdx.x * 256 + threadIdx.x;
    if (xb >= Wb) return;
    const int yb = blockIdx.y, n = blockIdx.z;
    const int y = yb - HALO_Y, x = xb - HALO_X;
    u32x2_t o = {0u, 0u};
    if (y >= 0 && y < Hp && x >= 0 && x < Wp) {
        float v[3] = {0.f, 0.f, 0.f};          // beyond (dst_h, dst_w): the zero pad, normalised like bd_pad_normalize's
        if (y < dst_h && x < dst_w) {
            const LinTap ty = lin_tap(y, sy, H), tx = lin_tap(x, sx, W);
            const long long plane = (long long)H * W, r0 = (long long)ty.i0 * W, r1 = (long long)ty.i1 * W;
            const float* __restrict__ p = in + (long long)n * 3 * plane;
#pragma unroll
            for (int c = 0; c < 3; ++c, p += plane)
                v[c] = lerp_fma(lerp_fma(p[r0 + tx.i0], p[r0 + tx.i1], tx.f), lerp_fma(p[r1 + tx.i0], p[r1 + tx.i1], tx.f), ty.f);
        }
        o[0] = pack_bf2((v[0] - m0) / s0, (v[1] - m1) / s1);
        o[1] = pack_bf2((v[2] - m2) / s2, 0.f);
    }
    const long long px = ((long long)n * gridDim.y + yb) * Wb + xb;
    *reinterpret_cast<u32x2_t*>(out + px * 4) = o;
}

}  // namespace

extern "C" int bd_resize_pad_normalize(const uint8_t* packed_dev, int64_t packed_bytes, const bd_image_desc* descs_host, int N, int Hp,
                                       int Wp, const float* mean3, const float* std3, void* x_halo, bd_stream_t stream) {
    BD_REQUIRE(packed_dev && descs_host && mean3 && std3 && x_halo, "resize_pad_normalize: null pointer");
    BD_REQUIRE(N > 0 && packed_bytes > 0, "resize_pad_normalize: N=%d images in %lld bytes", N, (long long)packed_bytes);
    BD_REQUIRE(Hp > 0 && Wp > 0 && Hp % 32 == 0 && Wp % 32 == 0 && Hp + 2 * HALO_Y <= 65535,
               "resize_pad_normalize: padded size %d x %d must be positive multiples of 32 (at most 65504 rows)", Hp, Wp);
    for (int i = 0; i < N; ++i) {
        const bd_image_desc& d = descs_host[i];
        BD_REQUIRE(d.src_h > 0 && d.src_w > 0 && d.dst_h > 0 && d.dst_w > 0, "resize_pad_normalize: image %d: %d x %d -> %d x %d", i, d.src_h,
                   d.src_w, d.dst_h, d.dst_w);
        BD_REQUIRE(d.offset >= 0 && d.offset <= packed_bytes && (int64_t)d.src_h * d.src_w * 3 <= packed_bytes - d.offset,
                   "resize_pad_normalize: image %d: %d x %d x 3 bytes at offset %lld end past the %lld packed bytes", i, d.src_h, d.src_w,
                   (long long)d.offset, (long long)packed_bytes);
        BD_REQUIRE(d.dst_h <= Hp && d.dst_w <= Wp, "resize_pad_normalize: image %d: resized %d x %d exceeds the padded %d x %d", i, d.dst_h,
                   d.dst_w, Hp, Wp);
    }
    const int Hb = Hp + 2 * HALO_Y, Wb = Wp + 2 * HALO_X;
    for (int g0 = 0; g0 < N; g0 += GROUP) {
        const int cnt = N - g0 < GROUP ? N - g0 : GROUP;
        ImageGroup g = {};
        for (int i = 0; i < cnt; ++i) g.d[i] = descs_host[g0 + i];
        hipLaunchKernelGGL(resize_pad_normalize_kernel, dim3(cdiv(Wb / 2, 256), Hb, cnt), dim3(256), 0, (hipStream_t)stream, packed_dev,
                           (long long)packed_bytes, g, Hp, Wp, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                           (bf16_raw*)x_halo + (long long)g0 * Hb * Wb * 4);
        BD_CHECK_LAUNCH("bd_resize_pad_normalize");
    }
    return BD_OK;
}

extern "C" int bd_resize_bilinear_normalize(const float* in, int N, int H, int W, int dst_h, int dst_w, int Hp, int Wp, const float* mean3,
                                            const float* std3, void* x_halo, bd_stream_t stream) {
    BD_REQUIRE(in && mean3 && std3 && x_halo, "resize_bilinear_normalize: null pointer");
    BD_REQUIRE((uintptr_t)in % 4 == 0 && (uintptr_t)x_halo % 8 == 0, "resize_bilinear_normalize: in must be 4-byte and x_halo 8-byte aligned");
    BD_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && dst_h > 0 && dst_w > 0, "resize_bilinear_normalize: N=%d, %d x %d -> %d x %d", N, H, W,
               dst_h, dst_w);
    BD_REQUIRE(Hp > 0 && Wp > 0 && Hp % 32 == 0 && Wp % 32 == 0 && Hp + 2 * HALO_Y <= 65535,
               "resize_bilinear_normalize: padded size %d x %d must be positive multiples of 32 (at most 65504 rows)", Hp, Wp);
    BD_REQUIRE(dst_h <= Hp && dst_w <= Wp, "resize_bilinear_normalize: resized %d x %d exceeds the padded %d x %d", dst_h, dst_w, Hp, Wp);
    const int Hb = Hp + 2 * HALO_Y, Wb = Wp + 2 * HALO_X;
    hipLaunchKernelGGL(resize_bilinear_normalize_kernel, dim3(cdiv(Wb, 256), Hb, N), dim3(256), 0, (hipStream_t)stream, in, H, W, dst_h, dst_w,
                       Hp, Wp, (double)H / (double)dst_h, (double)W / (double)dst_w, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                       (bf16_raw*)x_halo);
    BD_CHECK_LAUNCH("bd_resize_bilinear_normalize");
    return BD_OK;
}
