// Backward of the ResNet stem (MODEL.BACKBONE.FREEZE_AT = 0: conv1 trains, solver/default_solver.py:83-94): the max-pool's data
// gradient with the stem's ReLU gate folded in, and the 7x7 convolution's weight gradient.  The forward kernels are stem.hip's.
//
// bd_maxpool3x3s2_bwd -- gather form, no atomics.  One thread owns 8 channels of one stem pixel (y, x) and visits the up to four pooling
// windows (kernel 3, stride 2, pad 1) that contain it, in row-major window order (py ascending, then px).  It takes a window's gradient
// iff the pixel is that window's FIRST maximum in row-major order inside the window -- the element M.MaxPool2d's backward routes the
// gradient to (the rule bd_roi_pool_bwd_bf16 follows): its value equals the window's maximum (pool_out) and no earlier in-image position
// of the window holds that value.  Positions outside the image are padding and never win.  The taken gradients are summed in fp32 in that
// window order, gated by stem_out > 0 and rounded once: the result is dL/d(pre-activation) of the stem, bitwise reproducible.
//
// bd_stem_conv7x7_wgrad -- dW[o][ky][kx][c] = row_scale[o] * sum over pixels m = (n, y, x) of g[m][o] * x_halo[n][2y + ky][2x + 1 + kx][c]
// (x_halo's image starts at row 3, column 4: halo column 2x is the forward's zero-weight tap 0).  A skinny GEMM, 64 x 224 with
// K = N * H/2 * W/2: the columns are the forward's K layout, 7 filter rows x (8 taps x 4 channels) = 64 contiguous bytes of x_halo
// per row; tap 0 and channel 3 are computed and never written.  The reduction index is the slow index of both operands, so tiles are
// staged [pixel][column] as they lie in memory and the fragments are fetched with the transposing LDS read, as conv_wgrad.hip does.
// K is split over persistent workgroups (contiguous pixel ranges); each writes its own fp32 slab in the result's order and
// wgrad_batch_reduce_kernel (conv_wgrad.hip) sums the slabs in a fixed order: two runs give the same bits.
#include "common.h"

void bd_wgrad_reduce_launch(const float* slab, int splits, long long n, int row_len, const float* row_scale, float* dw, int accumulate,
                            hipStream_t stream);

namespace {

// ---- max-pool backward ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const bf16_raw* __restrict__ g_pool, const bf16_raw* __restrict__ stem_out,
                                                               const bf16_raw* __restrict__ pool_out, bf16_raw* __restrict__ g_stem,
                                                               int N, int Hs, int Ws, int C) {
    const int Hq = (Hs - 1) / 2 + 1, Wq = (Ws - 1) / 2 + 1;
    const int groups = C >> 3;
    const long long total = (long long)N * Hs * Ws * groups;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % groups);
        long long pix = i / groups;
        const int x = (int)(pix % Ws);
        pix /= Ws;
        const int y = (int)(pix % Hs);
        const long long n = pix / Hs;
        const bf16_raw* img = stem_out + n * Hs * Ws * C + cg * 8;
        const u32x4_t vraw = *reinterpret_cast<const u32x4_t*>(img + ((long long)y * Ws + x) * C);
        float v[8], acc[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[2 * k] = bf_lo(vraw[k]); v[2 * k + 1] = bf_hi(vraw[k]); }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        // windows that contain row y: py = y / 2 for an even y (its middle row), (y - 1) / 2 and (y + 1) / 2 for an odd one
        const int py0 = y >> 1, py1 = (y + 1) >> 1, px0 = x >> 1, px1 = (x + 1) >> 1;
        for (int py = py0; py <= py1 && py < Hq; ++py)
            for (int px = px0; px <= px1 && px < Wq; ++px) {
                const long long q = ((n * Hq + py) * Wq + px) * C + cg * 8;
                const u32x4_t mraw = *reinterpret_cast<const u32x4_t*>(pool_out + q);
                const u32x4_t graw = *reinterpret_cast<const u32x4_t*>(g_pool + q);
                float mx[8];
                bool take[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) { mx[2 * k] = bf_lo(mraw[k]); mx[2 * k + 1] = bf_hi(mraw[k]); }
#pragma unroll
                for (int k = 0; k < 8; ++k) take[k] = v[k] == mx[k];
                // earlier positions of the window, row-major, inside the image
                const int wy0 = 2 * py - 1, wx0 = 2 * px - 1;
                for (int ey = wy0 < 0 ? 0 : wy0; ey <= y; ++ey) {
                    const int ex_end = ey < y ? (wx0 + 3 < Ws ? wx0 + 3 : Ws) : x;
                    for (int ex = wx0 < 0 ? 0 : wx0; ex < ex_end; ++ex) {
                        const u32x4_t eraw = *reinterpret_cast<const u32x4_t*>(img + ((long long)ey * Ws + ex) * C);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            take[2 * k] = take[2 * k] && bf_lo(eraw[k]) != mx[2 * k];
                            take[2 * k + 1] = take[2 * k + 1] && bf_hi(eraw[k]) != mx[2 * k + 1];
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (take[2 * k]) acc[2 * k] += bf_lo(graw[k]);
                    if (take[2 * k + 1]) acc[2 * k + 1] += bf_hi(graw[k]);
                }
            }
        u32x4_t o;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[k] = pack_bf2(v[2 * k] > 0.f ? acc[2 * k] : 0.f, v[2 * k + 1] > 0.f ? acc[2 * k + 1] : 0.f);
        *reinterpret_cast<u32x4_t*>(g_stem + (n * Hs * Ws + (long long)y * Ws + x) * C + cg * 8) = o;
    }
}

// ---- stem weight gradient ------------------------------------------------------------------------------------------------------------
constexpr int SW_BKP = 64;                 // pixels per staged K step (two MFMA k steps)
constexpr int SW_GPITCH = 160;             // bytes per staged gradient row: 64 channels + 32 pad
constexpr int SW_XPITCH = 480;             // bytes per staged patch row: 7 x 64 + 32 pad (both pitches: 8 rows x 32 B cover all 64 banks)
constexpr int SW_BUF = SW_BKP * (SW_GPITCH + SW_XPITCH);
constexpr int SW_WGS = 512;                // K splits aimed at: two workgroups (80 KB of LDS each) per CU
constexpr int SW_DW = 64 * 147;            // floats of the result, [64][7][7][3]

struct StemWgradPlan { int splits, steps_per_split; long long total_steps; };

StemWgradPlan stem_wgrad_plan(int N, int H, int W) {
    StemWgradPlan pl;
    const long long M = (long long)N * (H / 2) * (W / 2);
    pl.total_steps = cdiv64(M, SW_BKP);
    pl.steps_per_split = (int)cdiv64(pl.total_steps, SW_WGS);
    pl.splits = (int)cdiv64(pl.total_steps, pl.steps_per_split);
    return pl;
}

__global__ __launch_bounds__(256) void stem_wgrad_kernel(const bf16_raw* __restrict__ xh, const bf16_raw* __restrict__ g,
                                                         const float* __restrict__ row_scale, float* __restrict__ slab,
                                                         int Hs, int Ws, int M, int steps_per_split) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wo = wave & 1;            // output-channel half (MFMA rows)
    const int wc = wave >> 1;           // column half: tiles 7 wc .. 7 wc + 6 of the 14 (MFMA columns)
    const int Hb = 2 * Hs + 6, Wb = 2 * Ws + 8;
    const int hw = Hs * Ws;

    const long long m_begin = (long long)blockIdx.x * steps_per_split * SW_BKP;       // < M: every split has at least one step
    long long m_end = m_begin + (long long)steps_per_split * SW_BKP;
    if (m_end > M) m_end = M;
    const int nsteps = (int)((m_end - m_begin + SW_BKP - 1) / SW_BKP);

    const int p = tid >> 2, q = tid & 3;           // staging: four threads per pixel row
    u32x4_t rg[2], rx[7];
    auto stage_load = [&](int step) {
        const long long m = m_begin + (long long)step * SW_BKP + p;
        if (m < m_end) {
            const unsigned n = (unsigned)(m / hw), rem = (unsigned)(m - (long long)n * hw);
            const unsigned y = rem / (unsigned)Ws, x = rem - y * (unsigned)Ws;
            const bf16_raw* gp = g + m * 64 + q * 16;
            rg[0] = *reinterpret_cast<const u32x4_t*>(gp);
            rg[1] = *reinterpret_cast<const u32x4_t*>(gp + 8);
            const bf16_raw* xp = xh + (((long long)n * Hb + 2 * y) * Wb + 2 * x) * 4 + q * 8;
#pragma unroll
            for (int r = 0; r < 7; ++r) rx[r] = *reinterpret_cast<const u32x4_t*>(xp + (long long)r * Wb * 4);
        } else {                                   // past the split's last pixel: zero rows add nothing
            rg[0] = rg[1] = (u32x4_t){0u, 0u, 0u, 0u};
#pragma unroll
            for (int r = 0; r < 7; ++r) rx[r] = (u32x4_t){0u, 0u, 0u, 0u};
        }
    };
    auto stage_write = [&](int buf) {
        unsigned char* Gt = smem + buf * SW_BUF;
        unsigned char* Xt = Gt + SW_BKP * SW_GPITCH;
        *reinterpret_cast<u32x4_t*>(Gt + p * SW_GPITCH + q * 32) = rg[0];
        *reinterpret_cast<u32x4_t*>(Gt + p * SW_GPITCH + q * 32 + 16) = rg[1];
#pragma unroll
        for (int r = 0; r < 7; ++r) *reinterpret_cast<u32x4_t*>(Xt + p * SW_XPITCH + r * 64 + q * 16) = rx[r];
    };

    f32x4_t acc[2][7];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // MFMA k index -> pixel of the 32-pixel step, the same permutation for both operands (conv_wgrad.hip): k = 8 g4 + j <-> pixel
    // 16 (g4 >> 1) + 4 (g4 & 1) + (j & 3) + 8 (j >> 2); the transposing read hands lane idx of a 16-lane group column col0 + idx of 4 rows
    const int g4 = lane >> 4, idx = lane & 15;
    const int prow_base = 16 * (g4 >> 1) + 4 * (g4 & 1);
    const int tr_q = idx >> 2, tr_p = idx & 3;
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;
    auto load_frag = [&](const unsigned char* tile, int pitch, int kk, int cbase) -> bf16x8_t {
        const unsigned char* a0 = tile + (kk * 32 + prow_base + tr_q) * pitch + (cbase + 4 * tr_p) * 2;
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(a0));
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(a0 + 8 * pitch));
        const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8_t, v);
    };
    auto compute = [&](int buf) {
        const unsigned char* Gt = smem + buf * SW_BUF;
        const unsigned char* Xt = Gt + SW_BKP * SW_GPITCH;
#pragma unroll
        for (int kk = 0; kk < SW_BKP / 32; ++kk) {
            bf16x8_t a[2], b[7];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = load_frag(Gt, SW_GPITCH, kk, wo * 32 + i * 16);
#pragma unroll
            for (int j = 0; j < 7; ++j) b[j] = load_frag(Xt, SW_XPITCH, kk, (wc * 7 + j) * 16);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 7; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };

    stage_load(0);
    stage_write(0);
    __syncthreads();
    int cur = 0;
    for (int st = 0; st < nsteps; ++st) {
        const bool more = st + 1 < nsteps;
        if (more) stage_load(st + 1);
        compute(cur);
        if (more) stage_write(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // D[row = o][col = t]: this lane holds o = 4 g4 + reg of its row tile and column idx of its column tile; column t = 32 ky + 4 pos + c
    // is tap kx = pos - 1 (pos 0: the forward's zero weight) of channel c (c = 3: the pad channel) -- those are not part of the result
    float* out = slab + (long long)blockIdx.x * SW_DW;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int t = (wc * 7 + j) * 16 + idx;
        const int ky = t >> 5, pos = (t >> 2) & 7, c = t & 3;
        if (pos == 0 || c == 3) continue;
        const int col = ky * 21 + (pos - 1) * 3 + c;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = wo * 32 + i * 16 + g4 * 4 + r;
                out[o * 147 + col] = row_scale ? acc[i][j][r] * row_scale[o] : acc[i][j][r];
            }
    }
}

}  // namespace

extern "C" int bd_maxpool3x3s2_bwd(const void* g_pool, const void* stem_out, const void* pool_out, int N, int Hs, int Ws, int C, void* g_stem,
                                   bd_stream_t stream) {
    BD_REQUIRE(g_pool && stem_out && pool_out && g_stem, "maxpool3x3s2_bwd: null pointer");
    BD_REQUIRE(N > 0 && Hs > 0 && Ws > 0, "maxpool3x3s2_bwd: bad shape N=%d Hs=%d Ws=%d", N, Hs, Ws);
    BD_REQUIRE(C > 0 && C % 8 == 0, "maxpool3x3s2_bwd: C=%d must be a multiple of 8", C);
    BD_REQUIRE((long long)Hs * Ws < 0x7fffffffll, "maxpool3x3s2_bwd: image too large");
    const long long total = (long long)N * Hs * Ws * (C / 8);
    hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)g_pool,
                       (const bf16_raw*)stem_out, (const bf16_raw*)pool_out, (bf16_raw*)g_stem, N, Hs, Ws, C);
    BD_CHECK_LAUNCH("bd_maxpool3x3s2_bwd");
    return BD_OK;
}

extern "C" size_t bd_stem_conv7x7_wgrad_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2) return 0;
    return (size_t)stem_wgrad_plan(N, H, W).splits * SW_DW * sizeof(float);
}

extern "C" int bd_stem_conv7x7_wgrad(int N, int H, int W, const void* x_halo, const void* g_stem, const float* row_scale, float* dw,
                                     int accumulate, void* ws, size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(x_halo && g_stem && dw && ws, "stem_conv7x7_wgrad: null pointer");
    BD_REQUIRE(N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "stem_conv7x7_wgrad: H=%d W=%d must be even", H, W);
    const long long M = (long long)N * (H / 2) * (W / 2);
    BD_REQUIRE(M < 0x7fffffffll, "stem_conv7x7_wgrad: too many output pixels");
    const size_t need = bd_stem_conv7x7_wgrad_workspace_bytes(N, H, W);
    BD_REQUIRE(ws_bytes >= need, "stem_conv7x7_wgrad: workspace %zu < required %zu bytes", ws_bytes, need);
    const StemWgradPlan pl = stem_wgrad_plan(N, H, W);
    const size_t lds = 2 * SW_BUF;
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_wgrad_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(pl.splits), dim3(256), lds, (hipStream_t)stream, (const bf16_raw*)x_halo,
                       (const bf16_raw*)g_stem, row_scale, (float*)ws, H / 2, W / 2, (int)M, pl.steps_per_split);
    BD_CHECK_LAUNCH("bd_stem_conv7x7_wgrad");
    // (the FrozenBN row scale went into the slabs: a row of 147 floats does not end on the reduce's 16-byte elements)
    bd_wgrad_reduce_launch((const float*)ws, pl.splits, SW_DW, 147, nullptr, dw, accumulate, (hipStream_t)stream);
    BD_CHECK_LAUNCH("bd_stem_conv7x7_wgrad(reduce)");
    return BD_OK;
}
