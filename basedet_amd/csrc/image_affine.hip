// CenterNet's training input on the device (CenterNetConfig.AUG.TRAIN_VALUE): a packed batch of raw uint8 HWC images -> the stem's input
// layout.  Per image: CenterAffine's warp into (out_h, out_w), horizontal flip, brightness, contrast, saturation, lighting, then
// (x - mean) / std -- bit for bit what tests/center_affine_oracle.py computes.
//
// The warp is cv2.warpAffine(INTER_LINEAR, constant border 0) in its fixed-point form: source coordinates in 1/1024 pixel from two
// separately rounded float64 terms (one per column, one per row), reduced to 1/32 pixel; the four bilinear weights are
// 32 (32 - fx)(32 - fy) ... -- the 32 x 32 table's entries are exact integers that sum to 32768, so no table is kept; the blend is
// (sum w p + 16384) >> 15.  Integer work: nothing to round differently.  The colour stages are fp32 expressions of one IEEE operation per
// numpy operation: multiply-add contraction is OFF in this file (the pragmas below and the per-file flag of build.py).  Every colour
// stage reads bytes and writes bytes.
//
// The contrast stage blends with the mean grey level of the whole image as it stands after brightness: the one reduction of the
// pipeline.  Launch 1 (warp, flip, brightness) writes the intermediate pixels to the workspace, one dword each, and adds the three
// channel sums of every image into 64-bit counters: exact integers, so the order of the atomics cannot change the result.  Launch 2
// (contrast, saturation, lighting, normalise) reads them.  A batch in which no image has contrast enabled runs launch 2 alone, with the
// warp inside it, and touches no workspace.
//
// HBM-bound: launch 1 writes 4 bytes per pixel, launch 2 reads them and writes 8.  One lane owns two neighbouring output pixels (one
// 16-byte store in launch 2).  The source taps are unaligned dword loads left to the vector L1 / L2, as in image_resize.hip.
#include "common.h"

namespace {

constexpr int HALO_Y = 3, HALO_X = 4;
constexpr int GROUP = 32;          // descriptors per launch, passed by value: 32 x 96 bytes of kernel argument
constexpr int AB_BITS = 10, INTER_BITS = 5, INTER_TAB = 1 << INTER_BITS;      // cv2: 1/1024 pixel coordinates, 1/32 pixel weights

static_assert(sizeof(bd_affine_desc) == 96, "bd_affine_desc is 96 bytes");
struct AffineGroup { bd_affine_desc d[GROUP]; };

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

// bytes 0..2 of the result = the pixel's three channels; a tap outside the image is 0 (constant border)
__device__ __forceinline__ uint32_t load_tap(const uint8_t* __restrict__ packed, long long packed_bytes, const bd_affine_desc& d, int sx,
                                             int sy) {
    if (sx < 0 || sy < 0 || sx >= d.src_w || sy >= d.src_h) return 0u;
    const long long at = d.offset + ((long long)sy * d.src_w + sx) * 3;
    if (at + 4 <= packed_bytes) return *reinterpret_cast<const u32_unaligned*>(packed + at) & 0xffffffu;
    return (uint32_t)packed[at] | ((uint32_t)packed[at + 1] << 8) | ((uint32_t)packed[at + 2] << 16);
}

__device__ __forceinline__ uint32_t to_byte(float v) { return (uint32_t)(int)fminf(fmaxf(v, 0.f), 255.f); }      // clip, then truncate

// The row terms of the source coordinate of output row y: round((m1 y + m2) 1024) + 16 and the same for the second row of the map
__device__ __forceinline__ void row_terms(const bd_affine_desc& d, int y, int* X0, int* Y0) {
#pragma clang fp contract(off)
    const double fy = (double)y;
    *X0 = (int)rint((d.inv[1] * fy + d.inv[2]) * 1024.0) + (1 << (AB_BITS - INTER_BITS - 1));
    *Y0 = (int)rint((d.inv[4] * fy + d.inv[5]) * 1024.0) + (1 << (AB_BITS - INTER_BITS - 1));
}

// Launch 1's work for output pixel (x, y): the warped pixel of column x (column out_w - 1 - x when flipped), after brightness
__device__ __forceinline__ uint32_t warp_flip_brightness(const uint8_t* __restrict__ packed, long long packed_bytes, const bd_affine_desc& d,
                                                         int X0, int Y0, int x, int out_w) {
#pragma clang fp contract(off)
    const double fx = (double)(d.flip ? out_w - 1 - x : x);
    const int X = (X0 + (int)rint(d.inv[0] * fx * 1024.0)) >> (AB_BITS - INTER_BITS);
    const int Y = (Y0 + (int)rint(d.inv[3] * fx * 1024.0)) >> (AB_BITS - INTER_BITS);
    const int sx = X >> INTER_BITS, sy = Y >> INTER_BITS, ax = X & (INTER_TAB - 1), ay = Y & (INTER_TAB - 1);
    const uint32_t a = load_tap(packed, packed_bytes, d, sx, sy), b = load_tap(packed, packed_bytes, d, sx + 1, sy);
    const uint32_t c = load_tap(packed, packed_bytes, d, sx, sy + 1), e = load_tap(packed, packed_bytes, d, sx + 1, sy + 1);
    const int w00 = (INTER_TAB - ax) * (INTER_TAB - ay) * 32, w01 = ax * (INTER_TAB - ay) * 32;
    const int w10 = (INTER_TAB - ax) * ay * 32, w11 = ax * ay * 32;
    uint32_t px = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int sh = 8 * ch;
        const int acc = w00 * (int)((a >> sh) & 0xffu) + w01 * (int)((b >> sh) & 0xffu) + w10 * (int)((c >> sh) & 0xffu) +
                        w11 * (int)((e >> sh) & 0xffu);
        uint32_t v = (uint32_t)((acc + (1 << 14)) >> 15);
        if (d.stages & BD_AFFINE_BRIGHTNESS) v = to_byte((float)v * d.alpha_brightness);
        px |= v << sh;
    }
    return px;
}

// Launch 2's colour stages on one pixel (bytes 0..2 of px); gmean: the image's mean grey level (read only under BD_AFFINE_CONTRAST)
__device__ __forceinline__ uint32_t contrast_saturation_lighting(uint32_t px, const bd_affine_desc& d, float gmean) {
#pragma clang fp contract(off)
    uint32_t p[3] = {px & 0xffu, (px >> 8) & 0xffu, (px >> 16) & 0xffu};
    if (d.stages & BD_AFFINE_CONTRAST) {
        const float al = d.alpha_contrast, t = gmean * (1.f - al);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) p[ch] = to_byte((float)p[ch] * al + t);
    }
    if (d.stages & BD_AFFINE_SATURATION) {
        const float al = d.alpha_saturation;
        const float grey = 0.114f * (float)p[0] + 0.587f * (float)p[1] + 0.299f * (float)p[2];
        const float t = grey * (1.f - al);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) p[ch] = to_byte((float)p[ch] * al + t);
    }
    if (d.stages & BD_AFFINE_LIGHTING) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) p[ch] = to_byte((float)p[ch] + d.delta[ch]);
    }
    return p[0] | (p[1] << 8) | (p[2] << 16);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// Launch 1.  Lane = WARP_PER pairs of neighbouring pixels of one image (blockIdx.y), a block apart from each other; mid [cnt][H][W]
// dwords; sums [cnt][3] 64-bit counters, zeroed by the entry.  A wave adds at most WARP_PER x 128 x 255 per channel: 32 bits hold it.
// (Atomics on one address serialise in L2: WARP_PER pairs per lane keep them at 256 per counter for a 512 x 512 image.)
constexpr int WARP_PER = 8;
__global__ __launch_bounds__(256) void affine_warp_kernel(const uint8_t* __restrict__ packed, long long packed_bytes, const AffineGroup g,
                                                          int H, int W, uint32_t* __restrict__ mid, unsigned long long* __restrict__ sums) {
    const int n = blockIdx.y;
    const bd_affine_desc& d = g.d[n];
    const int half_w = W / 2;
    uint32_t s0 = 0u, s1 = 0u, s2 = 0u;
#pragma unroll 2
    for (int k = 0; k < WARP_PER; ++k) {
        const int pair = (blockIdx.x * WARP_PER + k) * 256 + threadIdx.x;
        if (pair < H * half_w) {
            const int y = pair / half_w, x = 2 * (pair - y * half_w);
            int X0, Y0;
            row_terms(d, y, &X0, &Y0);
            const uint32_t p0 = warp_flip_brightness(packed, packed_bytes, d, X0, Y0, x, W);
            const uint32_t p1 = warp_flip_brightness(packed, packed_bytes, d, X0, Y0, x + 1, W);
            *reinterpret_cast<u32x2_t*>(mid + ((long long)n * H + y) * W + x) = (u32x2_t){p0, p1};
            s0 += (p0 & 0xffu) + (p1 & 0xffu);
            s1 += ((p0 >> 8) & 0xffu) + ((p1 >> 8) & 0xffu);
            s2 += (p0 >> 16) + (p1 >> 16);
        }
    }
    s0 = wave_sum_u32(s0);
    s1 = wave_sum_u32(s1);
    s2 = wave_sum_u32(s2);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(sums + 3 * n + 0, (unsigned long long)s0);
        atomicAdd(sums + 3 * n + 1, (unsigned long long)s1);
        atomicAdd(sums + 3 * n + 2, (unsigned long long)s2);
    }
}

// Launch 2 (FUSED: the whole pipeline; no image of the batch has contrast enabled).  Lane = two neighbouring elements of one row of the
// haloed output; the halo is written as zeros.
template <bool FUSED>
__global__ __launch_bounds__(256) void affine_colour_normalize_kernel(const uint8_t* __restrict__ packed, long long packed_bytes,
                                                                      const AffineGroup g, int H, int W, const uint32_t* __restrict__ mid,
                                                                      const unsigned long long* __restrict__ sums, float m0, float m1,
                                                                      float m2, float s0, float s1, float s2, bf16_raw* __restrict__ out,
                                                                      uint8_t* __restrict__ u8_out) {
#pragma clang fp contract(off)
    const int Hb = H + 2 * HALO_Y, half_wb = (W + 2 * HALO_X) / 2;
    const int pair = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (pair >= Hb * half_wb) return;
    const bd_affine_desc& d = g.d[n];
    const int yb = pair / half_wb, xb = 2 * (pair - yb * half_wb);
    const int y = yb - HALO_Y, x = xb - HALO_X;
    u32x4_t o = {0u, 0u, 0u, 0u};
    if (y >= 0 && y < H && x >= 0 && x < W) {
        uint32_t p[2];
        if (FUSED) {
            int X0, Y0;
            row_terms(d, y, &X0, &Y0);
            p[0] = warp_flip_brightness(packed, packed_bytes, d, X0, Y0, x, W);
            p[1] = warp_flip_brightness(packed, packed_bytes, d, X0, Y0, x + 1, W);
        } else {
            const u32x2_t v = *reinterpret_cast<const u32x2_t*>(mid + ((long long)n * H + y) * W + x);
            p[0] = v[0];
            p[1] = v[1];
        }
        float gmean = 0.f;
        if (!FUSED && (d.stages & BD_AFFINE_CONTRAST)) {
            // exact integer sums, combined in float64 and rounded once: every lane of every launch gets the same fp32
            const double grey = (double)0.114f * (double)sums[3 * n] + (double)0.587f * (double)sums[3 * n + 1] +
                                (double)0.299f * (double)sums[3 * n + 2];
            gmean = (float)(grey / ((double)H * (double)W));
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t q = contrast_saturation_lighting(p[k], d, gmean);
            const float c0 = (float)(q & 0xffu), c1 = (float)((q >> 8) & 0xffu), c2 = (float)(q >> 16);
            o[2 * k] = pack_bf2((c0 - m0) / s0, (c1 - m1) / s1);
            o[2 * k + 1] = pack_bf2((c2 - m2) / s2, 0.f);
            p[k] = q;
        }
        if (u8_out != nullptr) {
            // six bytes at an even offset (x is even): three 16-bit stores
            uint16_t* u = reinterpret_cast<uint16_t*>(u8_out + (((long long)n * H + y) * W + x) * 3);
            u[0] = (uint16_t)(p[0] & 0xffffu);
            u[1] = (uint16_t)((p[0] >> 16) | ((p[1] & 0xffu) << 8));
            u[2] = (uint16_t)(p[1] >> 8);
        }
    }
    *reinterpret_cast<u32x4_t*>(out + (((long long)n * Hb + yb) * (2 * half_wb) + xb) * 4) = o;
}

constexpr size_t SUMS_ALIGN = 256;
size_t sums_bytes(int N) { return ((size_t)N * 3 * sizeof(unsigned long long) + SUMS_ALIGN - 1) / SUMS_ALIGN * SUMS_ALIGN; }

bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" size_t bd_affine_jitter_workspace_bytes(int N, int out_h, int out_w) {
    if (N <= 0 || out_h <= 0 || out_w <= 0) return 0;
    return sums_bytes(N) + (size_t)N * out_h * out_w * sizeof(uint32_t);
}

extern "C" int bd_affine_jitter_normalize(const uint8_t* packed_dev, int64_t packed_bytes, const bd_affine_desc* descs_host, int N, int out_h,
                                          int out_w, const float* mean3, const float* std3, void* x_halo, uint8_t* u8_out, void* ws,
                                          size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(packed_dev && descs_host && mean3 && std3 && x_halo, "affine_jitter_normalize: null pointer");
    BD_REQUIRE(N > 0 && packed_bytes > 0, "affine_jitter_normalize: N=%d images in %lld bytes", N, (long long)packed_bytes);
    BD_REQUIRE(out_h > 0 && out_w > 0 && out_h % 32 == 0 && out_w % 32 == 0 && out_h <= 16384 && out_w <= 16384,
               "affine_jitter_normalize: output size %d x %d must be positive multiples of 32 (at most 16384)", out_h, out_w);
    bool contrast = false;
    const double reach = (double)(out_h > out_w ? out_h : out_w);
    for (int i = 0; i < N; ++i) {
        const bd_affine_desc& d = descs_host[i];
        BD_REQUIRE(d.src_h > 0 && d.src_w > 0 && d.src_h <= 32767 && d.src_w <= 32767, "affine_jitter_normalize: image %d: source %d x %d", i,
                   d.src_h, d.src_w);
        BD_REQUIRE(d.offset >= 0 && d.offset <= packed_bytes && (int64_t)d.src_h * d.src_w * 3 <= packed_bytes - d.offset,
                   "affine_jitter_normalize: image %d: %d x %d x 3 bytes at offset %lld end past the %lld packed bytes", i, d.src_h, d.src_w,
                   (long long)d.offset, (long long)packed_bytes);
        // every fixed-point term stays below 2^29 in magnitude (|m| x 1024 x the output's extent), so their sums fit 32 bits
        for (int k = 0; k < 6; ++k) {
            const double lim = (k == 2 || k == 5) ? 524288.0 / 2 : 524288.0 / 2 / reach;
            BD_REQUIRE(d.inv[k] == d.inv[k] && d.inv[k] <= lim && d.inv[k] >= -lim,
                       "affine_jitter_normalize: image %d: entry %d of the inverse map (%g) is not finite or too large", i, k, d.inv[k]);
        }
        BD_REQUIRE(d.inv[0] * d.inv[4] - d.inv[1] * d.inv[3] != 0.0, "affine_jitter_normalize: image %d: the map is singular", i);
        BD_REQUIRE((d.stages & ~(uint32_t)BD_AFFINE_ALL) == 0, "affine_jitter_normalize: image %d: unknown stage bits %#x", i, d.stages);
        BD_REQUIRE(finite_f(d.alpha_brightness) && finite_f(d.alpha_contrast) && finite_f(d.alpha_saturation) && finite_f(d.delta[0]) &&
                       finite_f(d.delta[1]) && finite_f(d.delta[2]),
                   "affine_jitter_normalize: image %d: a colour parameter is not finite", i);
        contrast = contrast || (d.stages & BD_AFFINE_CONTRAST);
    }
    const size_t need = contrast ? bd_affine_jitter_workspace_bytes(N, out_h, out_w) : 0;
    BD_REQUIRE(!contrast || (ws && ws_bytes >= need && (uintptr_t)ws % 8 == 0),
               "affine_jitter_normalize: the contrast stage needs an 8-byte aligned workspace of %zu bytes (got %zu)", need, ws_bytes);
    const hipStream_t st = (hipStream_t)stream;
    const int Hb = out_h + 2 * HALO_Y, Wb = out_w + 2 * HALO_X;
    unsigned long long* sums = (unsigned long long*)ws;
    uint32_t* mid = contrast ? (uint32_t*)((char*)ws + sums_bytes(N)) : nullptr;
    if (contrast && hipMemsetAsync(sums, 0, (size_t)N * 3 * sizeof(unsigned long long), st) != hipSuccess) {
        bd_set_error("affine_jitter_normalize: memset failed");
        return BD_ELAUNCH;
    }
    for (int g0 = 0; g0 < N; g0 += GROUP) {
        const int cnt = N - g0 < GROUP ? N - g0 : GROUP;
        AffineGroup g = {};
        for (int i = 0; i < cnt; ++i) g.d[i] = descs_host[g0 + i];
        const long long px0 = (long long)g0 * out_h * out_w;
        bf16_raw* out = (bf16_raw*)x_halo + (long long)g0 * Hb * Wb * 4;
        uint8_t* u8 = u8_out ? u8_out + px0 * 3 : nullptr;
        const dim3 grid2(cdiv(Hb * (Wb / 2), 256), cnt);
        if (contrast) {
            hipLaunchKernelGGL(affine_warp_kernel, dim3(cdiv(out_h * (out_w / 2), 256 * WARP_PER), cnt), dim3(256), 0, st, packed_dev,
                               (long long)packed_bytes, g, out_h, out_w, mid + px0, sums + 3 * g0);
            BD_CHECK_LAUNCH("bd_affine_jitter_normalize (warp)");
            hipLaunchKernelGGL(affine_colour_normalize_kernel<false>, grid2, dim3(256), 0, st, packed_dev, (long long)packed_bytes, g, out_h,
                               out_w, mid + px0, sums + 3 * g0, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out, u8);
        } else {
            hipLaunchKernelGGL(affine_colour_normalize_kernel<true>, grid2, dim3(256), 0, st, packed_dev, (long long)packed_bytes, g, out_h,
                               out_w, mid, sums, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out, u8);
        }
        BD_CHECK_LAUNCH("bd_affine_jitter_normalize");
    }
    return BD_OK;
}
