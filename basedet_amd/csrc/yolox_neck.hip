// The memory-bound glue between the convolutions of CSPDarknet and YOLOPAFPN (layers/yolox_blocks.py): the SPP max-pools and their
// adjoint, the channel concatenation (with PAFPN's nearest 2x upsample folded into its first operand) and its split, and Focus's
// space-to-depth of the normalised image.  Operands are bf16 pixel-major [rows][C], C % 8 == 0, every global access a 16-byte vector
// of 8 channels.  No atomics anywhere: every output has the same bits on every run.
//
// bd_spp_fwd -- one workgroup per (image, group of 8 channels) holds that plane in LDS (two 16-byte-per-pixel buffers).  maxpool5 is a
// row pass (A -> B) and a column pass (B -> A) over windows clipped to the image, so padding never takes part; maxpool9 is maxpool5 of
// maxpool5 and maxpool13 one more (the clipped windows compose exactly), so the three pools are three rounds over the same two buffers,
// each written to its channel block of `cat` from the column pass.  max selects one of its operands: the bits are the input's.
//
// bd_spp_bwd -- gather form.  Same workgroup shape.  For k = 5, 9, 13 in turn the FIRST maximum in row-major order of every clipped k x k
// window is found separably: the row pass keeps, per pixel and channel, the maximum of the row segment and the first column that reaches
// it (strict > while walking left to right); the column pass walks the rows of the window top to bottom with strict > over those row
// maxima, so the row it stops at is the first row holding the window's maximum and that row's recorded column is the first position.
// The position is kept as one byte per channel ((ay - (cy - r)) * k + (ax - (cx - r)) < 169).  Each pixel then visits the windows that
// contain it, window centres in row-major order, and adds the window's gradient where the recorded position is its own.  The
// accumulator is fp32 and lives in registers across the three rounds: identity term first, then k = 5, 9, 13; one rounding.
// LDS per pixel: 16 B (the plane; its first half becomes the position bytes after the row pass) + 16 B (row maxima) + 4 B (row columns,
// a nibble per channel) = 36 B, so the 64 x 64 plane limit takes 147456 B of the 160 KiB.
//
// bd_cat2_fwd / bd_cat2_bwd and bd_focus_fwd are grid-stride element-wise kernels, one 16-byte vector (cat2) or one output pixel
// (focus) per thread and step.
#include "common.h"

namespace {

constexpr int SPP_MAX_PLANE = 4096;          // pixels of one image plane a workgroup holds (64 x 64)
constexpr int SPP_BWD_PPT = 4;               // pixels per thread of the backward (their accumulators live in registers)

// per-channel maximum of two vectors of 8 bf16; the result's bits are an operand's (a where equal)
__device__ __forceinline__ u32x4_t max8(u32x4_t a, u32x4_t b) {
    u32x4_t o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lo = bf_lo(b[k]) > bf_lo(a[k]) ? b[k] : a[k];
        const uint32_t hi = bf_hi(b[k]) > bf_hi(a[k]) ? b[k] : a[k];
        o[k] = (lo & 0xffffu) | (hi & 0xffff0000u);
    }
    return o;
}

__global__ __launch_bounds__(1024) void spp_fwd_kernel(const bf16_raw* __restrict__ x, bf16_raw* __restrict__ cat, int H, int W, int C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spp_smem[];
    const int HW = H * W, groups = C >> 3;
    const int n = blockIdx.x / groups, cg = blockIdx.x % groups;
    u32x4_t* A = reinterpret_cast<u32x4_t*>(spp_smem);
    u32x4_t* B = A + HW;
    const bf16_raw* xin = x + (long long)n * HW * C + cg * 8;
    bf16_raw* out = cat + (long long)n * HW * 4 * C + cg * 8;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(xin + (long long)p * C);
        A[p] = v;
        *reinterpret_cast<u32x4_t*>(out + (long long)p * 4 * C) = v;
    }
    __syncthreads();
    for (int round = 1; round <= 3; ++round) {
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int y = p / W, xx = p - y * W;
            const int x0 = xx - 2 < 0 ? 0 : xx - 2, x1 = xx + 2 > W - 1 ? W - 1 : xx + 2;
            u32x4_t m = A[y * W + x0];
            for (int e = x0 + 1; e <= x1; ++e) m = max8(m, A[y * W + e]);
            B[p] = m;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int y = p / W, xx = p - y * W;
            const int y0 = y - 2 < 0 ? 0 : y - 2, y1 = y + 2 > H - 1 ? H - 1 : y + 2;
            u32x4_t m = B[y0 * W + xx];
            for (int e = y0 + 1; e <= y1; ++e) m = max8(m, B[e * W + xx]);
            A[p] = m;
            *reinterpret_cast<u32x4_t*>(out + ((long long)p * 4 + round) * C) = m;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void unpack8(u32x4_t v, float* f) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[2 * k] = bf_lo(v[k]); f[2 * k + 1] = bf_hi(v[k]); }
}

__global__ __launch_bounds__(1024) void spp_bwd_kernel(const bf16_raw* __restrict__ g_cat, const bf16_raw* __restrict__ x,
                                                       bf16_raw* __restrict__ d_x, int H, int W, int C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spp_smem[];
    const int HW = H * W, groups = C >> 3;
    const int n = blockIdx.x / groups, cg = blockIdx.x % groups;
    u32x4_t* A = reinterpret_cast<u32x4_t*>(spp_smem);                 // the plane during a row pass ...
    u32x2_t* ARG = reinterpret_cast<u32x2_t*>(spp_smem);               // ... the windows' first-maximum positions after it
    u32x4_t* RMAX = A + HW;
    uint32_t* RCOL = reinterpret_cast<uint32_t*>(RMAX + HW);
    const bf16_raw* xin = x + (long long)n * HW * C + cg * 8;
    const bf16_raw* gin = g_cat + (long long)n * HW * 4 * C + cg * 8;
    bf16_raw* out = d_x + (long long)n * HW * C + cg * 8;

    u32x4_t xr[SPP_BWD_PPT];
    float acc[SPP_BWD_PPT][8];
#pragma unroll
    for (int i = 0; i < SPP_BWD_PPT; ++i) {
        const int p = threadIdx.x + i * blockDim.x;
        if (p < HW) {
            xr[i] = *reinterpret_cast<const u32x4_t*>(xin + (long long)p * C);
            unpack8(*reinterpret_cast<const u32x4_t*>(gin + (long long)p * 4 * C), acc[i]);          // the identity term
        }
    }
    for (int round = 1; round <= 3; ++round) {
        const int r = 2 * round, k = 2 * r + 1;          // k = 5, 9, 13
        if (round > 1) __syncthreads();          // the previous round's gather has read ARG
#pragma unroll
        for (int i = 0; i < SPP_BWD_PPT; ++i) {
            const int p = threadIdx.x + i * blockDim.x;
            if (p < HW) A[p] = xr[i];
        }
        __syncthreads();
        // row pass: maximum of the clipped row segment and the first column (relative to x - r) that reaches it
#pragma unroll 1
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int y = p / W, xx = p - y * W;
            const int x0 = xx - r < 0 ? 0 : xx - r, x1 = xx + r > W - 1 ? W - 1 : xx + r;
            float m[8];
            uint32_t col = 0;
            u32x4_t mraw = A[y * W + x0];
            unpack8(mraw, m);
#pragma unroll
            for (int c = 0; c < 8; ++c) col |= (uint32_t)(x0 - (xx - r)) << (4 * c);
            for (int e = x0 + 1; e <= x1; ++e) {
                const u32x4_t vraw = A[y * W + e];
                float v[8];
                unpack8(vraw, v);
                const uint32_t rel = (uint32_t)(e - (xx - r));
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (v[c] > m[c]) { m[c] = v[c]; col = (col & ~(0xfu << (4 * c))) | (rel << (4 * c)); }
            }
            u32x4_t o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = (__float_as_uint(m[2 * c]) >> 16) | (__float_as_uint(m[2 * c + 1]) & 0xffff0000u);
            RMAX[p] = o;
            RCOL[p] = col;
        }
        __syncthreads();          // (also: every row pass has read A before ARG overwrites it)
        // column pass: the first row of the clipped window that holds its maximum, and that row's first column
#pragma unroll 1
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            const int y = p / W, xx = p - y * W;
            const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > H - 1 ? H - 1 : y + r;
            float m[8];
            uint32_t pos[8];
            {
                unpack8(RMAX[y0 * W + xx], m);
                const uint32_t col = RCOL[y0 * W + xx], base = (uint32_t)(y0 - (y - r)) * k;
#pragma unroll
                for (int c = 0; c < 8; ++c) pos[c] = base + ((col >> (4 * c)) & 0xfu);
            }
            for (int e = y0 + 1; e <= y1; ++e) {
                float v[8];
                unpack8(RMAX[e * W + xx], v);
                const uint32_t col = RCOL[e * W + xx], base = (uint32_t)(e - (y - r)) * k;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (v[c] > m[c]) { m[c] = v[c]; pos[c] = base + ((col >> (4 * c)) & 0xfu); }
            }
            u32x2_t o;
            o[0] = pos[0] | (pos[1] << 8) | (pos[2] << 16) | (pos[3] << 24);
            o[1] = pos[4] | (pos[5] << 8) | (pos[6] << 16) | (pos[7] << 24);
            ARG[p] = o;
        }
        __syncthreads();
        // gather: the windows that contain this pixel, centres in row-major order
#pragma unroll
        for (int i = 0; i < SPP_BWD_PPT; ++i) {
            const int p = threadIdx.x + i * blockDim.x;
            if (p < HW) {
                const int y = p / W, xx = p - y * W;
                const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > H - 1 ? H - 1 : y + r;
                const int x0 = xx - r < 0 ? 0 : xx - r, x1 = xx + r > W - 1 ? W - 1 : xx + r;
                for (int cy = y0; cy <= y1; ++cy)
                    for (int cx = x0; cx <= x1; ++cx) {
                        const uint32_t mine = (uint32_t)((y - cy + r) * k + (xx - cx + r)) * 0x01010101u;
                        const u32x2_t a = ARG[cy * W + cx];
                        const uint32_t d0 = a[0] ^ mine, d1 = a[1] ^ mine;          // a zero byte: this pixel is that channel's first maximum
                        const uint32_t z0 = (d0 - 0x01010101u) & ~d0 & 0x80808080u, z1 = (d1 - 0x01010101u) & ~d1 & 0x80808080u;
                        if (z0 | z1) {
                            float g[8];
                            unpack8(*reinterpret_cast<const u32x4_t*>(gin + ((long long)(cy * W + cx) * 4 + round) * C), g);
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                if (((d0 >> (8 * c)) & 0xffu) == 0) acc[i][c] += g[c];
                                if (((d1 >> (8 * c)) & 0xffu) == 0) acc[i][4 + c] += g[4 + c];
                            }
                        }
                    }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < SPP_BWD_PPT; ++i) {
        const int p = threadIdx.x + i * blockDim.x;
        if (p < HW) {
            u32x4_t o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = pack_bf2(acc[i][2 * c], acc[i][2 * c + 1]);
            *reinterpret_cast<u32x4_t*>(out + (long long)p * C) = o;
        }
    }
}

// ---- concatenation / split ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cat2_fwd_kernel(const bf16_raw* __restrict__ a, const bf16_raw* __restrict__ b, bf16_raw* __restrict__ out,
                                                       long long M, int Ga, int Gb, int up, int H, int W) {
    const int G = Ga + Gb;
    const long long total = M * G;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / G;
        const int g = (int)(i - row * G);
        const bf16_raw* src;
        if (g >= Ga) {
            src = b + (row * Gb + (g - Ga)) * 8;
        } else {
            long long ra = row;
            if (up) {
                const int xx = (int)(row % W);
                const long long t = row / W;
                const int y = (int)(t % H);
                const long long n = t / H;
                ra = (n * (H >> 1) + (y >> 1)) * (W >> 1) + (xx >> 1);
            }
            src = a + (ra * Ga + g) * 8;
        }
        *reinterpret_cast<u32x4_t*>(out + i * 8) = *reinterpret_cast<const u32x4_t*>(src);
    }
}

__global__ __launch_bounds__(256) void cat2_bwd_kernel(const bf16_raw* __restrict__ g, bf16_raw* __restrict__ d_a, bf16_raw* __restrict__ d_b,
                                                       long long M, long long Ma, int Ga, int Gb, int up, int H, int W, int acc_a, int acc_b) {
    const int G = Ga + Gb;
    const long long na = Ma * Ga, total = na + M * Gb;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float s[8];
        bf16_raw* dst;
        int acc;
        if (i >= na) {
            const long long j = i - na, row = j / Gb;
            const int c = (int)(j - row * Gb);
            unpack8(*reinterpret_cast<const u32x4_t*>(g + (row * G + Ga + c) * 8), s);
            dst = d_b + j * 8;
            acc = acc_b;
        } else {
            const long long row = i / Ga;
            const int c = (int)(i - row * Ga);
            if (up) {
                const int Wa = W >> 1, Ha = H >> 1;
                const int xx = (int)(row % Wa);
                const long long t = row / Wa;
                const int y = (int)(t % Ha);
                const long long n = t / Ha;
                const long long r00 = (n * H + 2 * y) * W + 2 * xx;
                float v[8];
                unpack8(*reinterpret_cast<const u32x4_t*>(g + (r00 * G + c) * 8), s);
                unpack8(*reinterpret_cast<const u32x4_t*>(g + ((r00 + 1) * G + c) * 8), v);
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] += v[k];
                unpack8(*reinterpret_cast<const u32x4_t*>(g + ((r00 + W) * G + c) * 8), v);
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] += v[k];
                unpack8(*reinterpret_cast<const u32x4_t*>(g + ((r00 + W + 1) * G + c) * 8), v);
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] += v[k];
            } else {
                unpack8(*reinterpret_cast<const u32x4_t*>(g + (row * G + c) * 8), s);
            }
            dst = d_a + i * 8;
            acc = acc_a;
        }
        if (acc) {
            float old[8];
            unpack8(*reinterpret_cast<const u32x4_t*>(dst), old);
#pragma unroll
            for (int k = 0; k < 8; ++k) s[k] += old[k];
        }
        u32x4_t o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = pack_bf2(s[2 * k], s[2 * k + 1]);
        *reinterpret_cast<u32x4_t*>(dst) = o;
    }
}

// ---- Focus -------------------------------------------------------------------------------------------------------------------------------
// One thread per output pixel: the two 16-byte pixel pairs (rows 2y, 2y + 1; columns 2x, 2x + 1; 4 channels each) -> 12 channels + 4 zeros.
__global__ __launch_bounds__(256) void focus_fwd_kernel(const bf16_raw* __restrict__ x_halo, bf16_raw* __restrict__ out, int N, int H, int W) {
    const int Ho = H >> 1, Wo = W >> 1;
    const long long pitch = (long long)(W + 8) * 4, img = (long long)(H + 6) * pitch;
    const long long total = (long long)N * Ho * Wo;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int xo = (int)(i % Wo);
        const long long t = i / Wo;
        const int yo = (int)(t % Ho);
        const long long n = t / Ho;
        const bf16_raw* src = x_halo + n * img + (long long)(3 + 2 * yo) * pitch + (long long)(4 + 2 * xo) * 4;
        const u32x4_t T = *reinterpret_cast<const u32x4_t*>(src);                  // (top-left c0 c1 | c2 0 | top-right c0 c1 | c2 0)
        const u32x4_t B = *reinterpret_cast<const u32x4_t*>(src + pitch);          // (bottom-left ... | bottom-right ...)
        u32x4_t o0, o1;
        o0[0] = T[0];                                          // tl0 tl1
        o0[1] = (T[1] & 0xffffu) | (B[0] << 16);               // tl2 bl0
        o0[2] = (B[0] >> 16) | (B[1] << 16);                   // bl1 bl2
        o0[3] = T[2];                                          // tr0 tr1
        o1[0] = (T[3] & 0xffffu) | (B[2] << 16);               // tr2 br0
        o1[1] = (B[2] >> 16) | (B[3] << 16);                   // br1 br2
        o1[2] = 0u;
        o1[3] = 0u;
        *reinterpret_cast<u32x4_t*>(out + i * 16) = o0;
        *reinterpret_cast<u32x4_t*>(out + i * 16 + 8) = o1;
    }
}

int spp_check(const char* name, const void* p0, const void* p1, const void* p2, int N, int H, int W, int C) {
    BD_REQUIRE(p0 && p1 && p2, "%s: null pointer", name);
    BD_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad shape N=%d H=%d W=%d", name, N, H, W);
    BD_REQUIRE(C > 0 && C % 8 == 0, "%s: C=%d must be a multiple of 8", name, C);
    BD_REQUIRE((long long)H * W <= SPP_MAX_PLANE, "%s: a %d x %d plane exceeds the %d pixels a workgroup holds", name, H, W, SPP_MAX_PLANE);
    BD_REQUIRE((long long)N * (C / 8) <= 0x7fffffffll, "%s: too many planes", name);
    return BD_OK;
}

int cat2_check(const char* name, int64_t M, int Ca, int Cb, int up, int N, int H, int W) {
    BD_REQUIRE(M > 0, "%s: M=%lld", name, (long long)M);
    BD_REQUIRE(Ca > 0 && Cb > 0 && Ca % 8 == 0 && Cb % 8 == 0, "%s: Ca=%d and Cb=%d must be positive multiples of 8", name, Ca, Cb);
    if (up) {
        BD_REQUIRE(N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "%s: up needs even H and W (N=%d H=%d W=%d)", name, N, H, W);
        BD_REQUIRE((int64_t)N * H * W == M, "%s: M=%lld is not N * H * W", name, (long long)M);
    }
    return BD_OK;
}

}  // namespace

extern "C" int bd_spp_fwd(const void* x, int N, int H, int W, int C, void* cat, bd_stream_t stream) {
    const int rc = spp_check("spp_fwd", x, cat, cat, N, H, W, C);
    if (rc != BD_OK) return rc;
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)spp_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SPP_MAX_PLANE * 32));
    const int HW = H * W;
    hipLaunchKernelGGL(spp_fwd_kernel, dim3(N * (C / 8)), dim3(HW <= 1024 ? 256 : 1024), (size_t)HW * 32, (hipStream_t)stream,
                       (const bf16_raw*)x, (bf16_raw*)cat, H, W, C);
    BD_CHECK_LAUNCH("bd_spp_fwd");
    return BD_OK;
}

extern "C" int bd_spp_bwd(const void* g_cat, const void* x, int N, int H, int W, int C, void* d_x, bd_stream_t stream) {
    const int rc = spp_check("spp_bwd", g_cat, x, d_x, N, H, W, C);
    if (rc != BD_OK) return rc;
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)spp_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SPP_MAX_PLANE * 36));
    const int HW = H * W;
    // SPP_BWD_PPT pixels per thread: 256 threads cover 1024 pixels, 1024 threads the limit
    hipLaunchKernelGGL(spp_bwd_kernel, dim3(N * (C / 8)), dim3(HW <= 256 * SPP_BWD_PPT ? 256 : 1024), (size_t)HW * 36, (hipStream_t)stream,
                       (const bf16_raw*)g_cat, (const bf16_raw*)x, (bf16_raw*)d_x, H, W, C);
    BD_CHECK_LAUNCH("bd_spp_bwd");
    return BD_OK;
}

extern "C" int bd_cat2_fwd(const void* a, const void* b, int64_t M, int Ca, int Cb, int up, int N, int H, int W, void* out, bd_stream_t stream) {
    BD_REQUIRE(a && b && out, "cat2_fwd: null pointer");
    const int rc = cat2_check("cat2_fwd", M, Ca, Cb, up, N, H, W);
    if (rc != BD_OK) return rc;
    const long long total = (long long)M * ((Ca + Cb) / 8);
    hipLaunchKernelGGL(cat2_fwd_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)a,
                       (const bf16_raw*)b, (bf16_raw*)out, (long long)M, Ca / 8, Cb / 8, up ? 1 : 0, H, W);
    BD_CHECK_LAUNCH("bd_cat2_fwd");
    return BD_OK;
}

extern "C" int bd_cat2_bwd(const void* g, int64_t M, int Ca, int Cb, int up, int N, int H, int W, void* d_a, int acc_a, void* d_b, int acc_b,
                           bd_stream_t stream) {
    BD_REQUIRE(g && d_a && d_b, "cat2_bwd: null pointer");
    const int rc = cat2_check("cat2_bwd", M, Ca, Cb, up, N, H, W);
    if (rc != BD_OK) return rc;
    const long long Ma = up ? (long long)M / 4 : (long long)M;
    const long long total = Ma * (Ca / 8) + (long long)M * (Cb / 8);
    hipLaunchKernelGGL(cat2_bwd_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)g,
                       (bf16_raw*)d_a, (bf16_raw*)d_b, (long long)M, Ma, Ca / 8, Cb / 8, up ? 1 : 0, H, W, acc_a ? 1 : 0, acc_b ? 1 : 0);
    BD_CHECK_LAUNCH("bd_cat2_bwd");
    return BD_OK;
}

extern "C" int bd_focus_fwd(const void* x_halo, int N, int H, int W, void* out, bd_stream_t stream) {
    BD_REQUIRE(x_halo && out, "focus_fwd: null pointer");
    BD_REQUIRE(N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "focus_fwd: needs even H and W (N=%d H=%d W=%d)", N, H, W);
    const long long total = (long long)N * (H / 2) * (W / 2);
    hipLaunchKernelGGL(focus_fwd_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)x_halo,
                       (bf16_raw*)out, N, H, W);
    BD_CHECK_LAUNCH("bd_focus_fwd");
    return BD_OK;
}
