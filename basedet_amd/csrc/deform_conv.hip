// Deformable convolution (DCNv1 / DCNv2; layers/blocks/deformable.py:24-34,52-63 -> M.DeformableConv2d) on CDNA4 MFMA (gfx950), forward and
// backward, for the one configuration the reference instantiates (layers/head/center_head.py:22-30): 3 x 3, stride 1, padding 1,
// dilation 1, one deformable group, with bias.
//
// Tensors (pixel-major NHWC bf16): x [N H W][Cin]; om [N H W][ld], the RAW output of the offset convolution: channel 2k = dy and 2k + 1 = dx
// of tap k = 3 i + j, channel 18 + k = the mask logit of tap k (modulated form, ld >= 27; sigmoid in fp32 here) -- unmodulated: mask = 1,
// ld >= 18.  Channels past 18 / 27 are padding: never read, their gradient is written as +0.
//
// Sampling: output pixel (y, x), tap (i, j) reads h = y - 1 + i + dy, w = x - 1 + j + dx (fp32); val = bilinear(x zero-extended, h, w) with
// h0 = floor(h), w0 = floor(w); the sample and all its gradients are 0 unless -1 < h < H and -1 < w < W; inside that range a corner counts
// only if it lies in the image.  The coordinate gradients are those of the floor formula (the right-hand derivative at an integer).
//   y[p][co] = bias[co] + sum_{k, ci} w[co][k][ci] m[p][k] val[p][k][ci]
//
// Forward: ONE implicit GEMM, K tap-major over 9 Cin (A = bd_weight_pack's forward layout as it stands); the sampled operand never goes to
// HBM: every lane gathers the 16-byte channel runs of the four corners of its pixels with range-checked buffer loads (a corner outside the
// image, a dead sample or a channel past Cin reads zeros through an offset past the buffer), blends them in fp32 with the mask folded into
// the four weights and writes the result into the LDS B tile as a bf16 PAIR (the rounded value and the bf16 of what the rounding dropped:
// two MFMAs per fragment, sampled operand good to 2^-16 -- one bf16 alone is off by up to 2^-8 of a sample, which a sum that one sample
// dominates shows in full; the kernels wait for the gather, not for the matrix pipe).  Tile: (64 MI) output channels x 64 pixels, MI = 1, 2, 4; the four waves split
// the channels and share the pixel tile, so a layer of up to 256 output channels gathers once.  K step 64 channels of one tap, two LDS
// buffers, one barrier per step, 160-byte padded rows (fpn_deconv.hip's scheme).
//
// Weight gradient: dw[co][k][ci] = sum_p dy[p][co] (m val)[p][k][ci]: the same gather feeds a pixel-split GEMM per tap (tile 128 ci x 128 co,
// 64 pixels per step, the same bf16 pair for the sampled operand, transposing LDS reads as in fpn_deconv.hip), fp32 slabs [split][Cout][9][Cin], fixed-order reduce; the bias gradient
// is bd_colsum_bf16.  Both bitwise reproducible.
//
// Data gradient, two stages per chunk of pixel rows: (1) the column gradient gcol [rows][9 Cin] bf16 = dy W is a 1 x 1 convolution
// Cout -> 9 Cin whose forward weight is bd_weight_pack's dgrad layout [Cin][9][Cout] byte for byte (output channel ci 9 + k), run by
// bd_conv2d_fwd; the chunk keeps gcol at <= 64 MB.  (2) deform_bwd_kernel re-reads x and om: a thread owns 8 channels of one pixel (its
// 72 gcol values are 144 contiguous bytes), adds m w_corner gcol into the fp32 [pixels][Cin] scratch with atomics and keeps the 27
// partial sums of d_om, which the workgroup reduces over the pixel's threads in index order through LDS: d_om is bitwise reproducible.
// d_x = bf16(scratch [+ add]) is NOT: the scatter targets depend on the data, so the order of the fp32 additions into one element varies
// from run to run (last-bit differences).
#include "common.h"
#include "wgrad_reduce.h"

void bd_wgrad_reduce_launch(const float* slab, int splits, long long n, int row_len, const float* row_scale, float* dw, int accumulate,
                            hipStream_t stream);

namespace {

constexpr int DF_BN = 64;                  // pixels per forward tile
constexpr int DF_BK = 64;                  // channels per K step
constexpr int DF_STRIDE = 160;             // 128 data bytes + 32 pad per LDS row
constexpr int DF_B_BYTES = DF_BN * DF_STRIDE;
constexpr unsigned DF_NONE = 0x80000000u;  // >= num_records of every buffer: the load returns zeros
constexpr size_t DF_GCOL_BYTES = 64u << 20;    // bound of the column-gradient chunk

// One sampling position: the pixel index of each corner (-1: contributes nothing), the bilinear fractions and the mask
struct DfSample {
    int i00, i01, i10, i11;
    float lh, lw, m;
    bool inside;
};

__device__ __forceinline__ float df_sigmoid(float l) { return 1.f / (1.f + __expf(-l)); }
// sigmoid'(l) = e^-|l| / (1 + e^-|l|)^2: no 1 - sigmoid cancellation, so a saturated mask keeps its (tiny) gradient to fp32 accuracy
__device__ __forceinline__ float df_sigmoid_grad(float l) {
    const float t = __expf(-fabsf(l));
    return t / ((1.f + t) * (1.f + t));
}

__device__ __forceinline__ DfSample df_sample(const bf16_raw* __restrict__ om_row, int modulated, int k, int n, int y, int x, int H, int W) {
    DfSample s;
    const int ti = k / 3, tj = k - 3 * ti;
    const float h = (float)(y - 1 + ti) + bf2f(om_row[2 * k]);
    const float w = (float)(x - 1 + tj) + bf2f(om_row[2 * k + 1]);
    s.m = modulated ? df_sigmoid(bf2f(om_row[18 + k])) : 1.f;
    s.inside = h > -1.f && h < (float)H && w > -1.f && w < (float)W;
    s.i00 = s.i01 = s.i10 = s.i11 = -1;
    s.lh = s.lw = 0.f;
    if (s.inside) {
        const float hf = floorf(h), wf = floorf(w);
        const int h0 = (int)hf, w0 = (int)wf;
        s.lh = h - hf; s.lw = w - wf;
        const bool t = h0 >= 0, b = h0 + 1 < H, l = w0 >= 0, r = w0 + 1 < W;
        const int base = (n * H + h0) * W + w0;
        if (t && l) s.i00 = base;
        if (t && r) s.i01 = base + 1;
        if (b && l) s.i10 = base + W;
        if (b && r) s.i11 = base + W + 1;
    }
    return s;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
struct DfParams {
    const bf16_raw* x;
    const bf16_raw* om;
    const bf16_raw* w;
    const float* bias;
    bf16_raw* y;
    int H, W, Cin, Cout, ld, modulated;
    int M;                 // N * H * W
    int co_tiles;
    unsigned x_bytes, w_bytes;
};

template <int MI>
__global__ __launch_bounds__(256) void deform_fwd_kernel(const DfParams p) {
    constexpr int BM = 64 * MI;
    constexpr int A_PASSES = BM / 32;          // 256 threads x 16 bytes = 32 rows of 64 channels
    constexpr int A_BYTES = BM * DF_STRIDE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int co_tile = blockIdx.x % p.co_tiles, m_tile = blockIdx.x / p.co_tiles;
    const int m0 = m_tile * DF_BN, co0 = co_tile * BM;
    const int Cin = p.Cin, HW = p.H * p.W;

    const int chunk = tid & 7, row0 = tid >> 3;
    int r_n[2], r_y[2], r_x[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + row0 + i * 32;
        r_n[i] = -1; r_y[i] = 0; r_x[i] = 0;
        if (m < p.M) {
            const int n = m / HW, rem = m - n * HW;
            r_n[i] = n; r_y[i] = rem / p.W; r_x[i] = rem - r_y[i] * p.W;
        }
    }
    unsigned a_voff[A_PASSES];
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
        const int co = co0 + row0 + i * 32;
        a_voff[i] = co < p.Cout ? (unsigned)((co * 9 * Cin + chunk * 8) * 2) : DF_NONE;
    }
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(p.w), 0, p.w_bytes, 0x00020000);

    const int kblocks = (Cin + DF_BK - 1) / DF_BK;
    const int nsteps = 9 * kblocks;
    int cur_tap = -1, cur_kb = kblocks;
    unsigned b_voff[2][4];
    float b_wt[2][4];
    u32x4_t ra[A_PASSES], rb[2][4];

    auto stage_load = [&]() {
        if (cur_kb == kblocks) {             // next tap (workgroup-uniform): every staged pixel's sampling position moves
            cur_kb = 0;
            ++cur_tap;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int c = 0; c < 4; ++c) { b_voff[i][c] = DF_NONE; b_wt[i][c] = 0.f; }
                if (r_n[i] >= 0) {
                    const DfSample s = df_sample(p.om + (long long)(m0 + row0 + i * 32) * p.ld, p.modulated, cur_tap, r_n[i], r_y[i], r_x[i],
                                                 p.H, p.W);
                    const int idx[4] = {s.i00, s.i01, s.i10, s.i11};
                    const float wt[4] = {(1.f - s.lh) * (1.f - s.lw), (1.f - s.lh) * s.lw, s.lh * (1.f - s.lw), s.lh * s.lw};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (idx[c] >= 0) {
                            b_voff[i][c] = (unsigned)((idx[c] * Cin + chunk * 8) * 2);
                            b_wt[i][c] = wt[c] * s.m;
                        }
                }
            }
        }
        const bool cok = cur_kb * DF_BK + chunk * 8 < Cin;      // K tail: channels past Cin are zeros in both operands
        int so_a = (cur_tap * Cin + cur_kb * DF_BK) * 2, so_b = cur_kb * DF_BK * 2;
        asm volatile("" : "+s"(so_a), "+s"(so_b));
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, cok ? a_voff[i] : DF_NONE, so_a, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) rb[i][c] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, cok ? b_voff[i][c] : DF_NONE, so_b, 0);
        ++cur_kb;
    };
    auto stage_write = [&](int buf) {
        unsigned char* At = smem + buf * (A_BYTES + 2 * DF_B_BYTES);
        unsigned char* Bt = At + A_BYTES;
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) *reinterpret_cast<u32x4_t*>(At + (row0 + i * 32) * DF_STRIDE + chunk * 16) = ra[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x4_t o, o2;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float lo = 0.f, hi = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    lo += b_wt[i][c] * bf_lo(rb[i][c][q]);
                    hi += b_wt[i][c] * bf_hi(rb[i][c][q]);
                }
                o[q] = pack_bf2(lo, hi);
                o2[q] = pack_bf2(lo - bf_lo(o[q]), hi - bf_hi(o[q]));       // what the bf16 rounding dropped
            }
            *reinterpret_cast<u32x4_t*>(Bt + (row0 + i * 32) * DF_STRIDE + chunk * 16) = o;
            *reinterpret_cast<u32x4_t*>(Bt + DF_B_BYTES + (row0 + i * 32) * DF_STRIDE + chunk * 16) = o2;
        }
    };

    f32x4_t acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int frag_row = lane & 15, frag_chunk = lane >> 4;

    auto compute = [&](int buf) {
        const unsigned char* At = smem + buf * (A_BYTES + 2 * DF_B_BYTES);
        const unsigned char* Bt = At + A_BYTES;
#pragma unroll
        for (int kk = 0; kk < DF_BK / 32; ++kk) {
            bf16x8_t a[MI], b[4], b2[4];
            const int ch = kk * 4 + frag_chunk;
#pragma unroll
            for (int i = 0; i < MI; ++i)
                a[i] = *reinterpret_cast<const bf16x8_t*>(At + (wave * 16 * MI + i * 16 + frag_row) * DF_STRIDE + ch * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                b[j] = *reinterpret_cast<const bf16x8_t*>(Bt + (j * 16 + frag_row) * DF_STRIDE + ch * 16);
                b2[j] = *reinterpret_cast<const bf16x8_t*>(Bt + DF_B_BYTES + (j * 16 + frag_row) * DF_STRIDE + ch * 16);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b2[j], acc[i][j], 0, 0, 0);
                }
        }
    };

    stage_load();
    stage_write(0);
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < nsteps; ++t) {
        const bool more = t + 1 < nsteps;
        if (more) stage_load();
        compute(cur);
        if (more) stage_write(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: lane holds output channels co0 + 16 MI wave + 16 i + 4 (lane >> 4) + r of pixel m0 + 16 j + (lane & 15) ----
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + j * 16 + (lane & 15);
        if (m >= p.M) continue;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int co = co0 + wave * 16 * MI + i * 16 + 4 * (lane >> 4);
            if (co >= p.Cout) continue;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (p.bias) {
                const f32x4_t b = *reinterpret_cast<const f32x4_t*>(p.bias + co);
                v[0] += b[0]; v[1] += b[1]; v[2] += b[2]; v[3] += b[3];
            }
            *reinterpret_cast<u32x2_t*>(p.y + (long long)m * p.Cout + co) = (u32x2_t){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        }
    }
}

// ---- weight gradient: D[ci][co] per tap, reduction over pixels ---------------------------------------------------------------------------
// Tiles staged [pixel][channel] (16-byte writes, 288-byte rows) and read with ds_read_b64_tr_b16 under fpn_deconv.hip's k -> pixel
// permutation.  A = the sampled columns (rows = input channels), B = dy (columns = output channels): a lane ends up with 4 consecutive
// input channels of one output channel = one 16-byte store into the [co][tap][ci] slab of its split.
constexpr int DW_TILE = 128;
constexpr int DW_BKP = 64;                 // pixels per K step
constexpr int DW_PITCH = 288;
constexpr int DW_PASSES = DW_BKP / 16;
constexpr int DW_TILE_BYTES = DW_BKP * DW_PITCH;

struct DwParams {
    const bf16_raw* x;
    const bf16_raw* om;
    const bf16_raw* dy;
    float* slab;            // [splits][Cout][9][Cin]
    int H, W, Cin, Cout, ld, modulated, M;
    int ci_tiles, co_tiles, splits, steps_per_split, total_steps;
};

__global__ __launch_bounds__(256) void deform_wgrad_kernel(const DwParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;     // ci half (MFMA rows), co half (MFMA columns)
    const int tiles_per_tap = p.ci_tiles * p.co_tiles;
    int bid = blockIdx.x;
    const int split = bid / (9 * tiles_per_tap);
    bid -= split * 9 * tiles_per_tap;
    const int tap = bid / tiles_per_tap;
    bid -= tap * tiles_per_tap;
    const int ci_tile = bid / p.co_tiles, co_tile = bid - ci_tile * p.co_tiles;
    const int ci0 = ci_tile * DW_TILE, co0 = co_tile * DW_TILE;
    const int Cin = p.Cin, Cout = p.Cout, HW = p.H * p.W;

    const int step_begin = split * p.steps_per_split;
    const int step_end = min(step_begin + p.steps_per_split, p.total_steps);
    const int chunk = tid & 15, row0 = tid >> 4;
    const bool ci_ok = ci0 + chunk * 8 < Cin, co_ok = co0 + chunk * 8 < Cout;

    u32x4_t rx[DW_PASSES][4], rg[DW_PASSES];
    float wt[DW_PASSES][4];
    auto stage_load = [&](int step) {
#pragma unroll
        for (int i = 0; i < DW_PASSES; ++i) {
            const int m = step * DW_BKP + row0 + i * 16;
            const u32x4_t zero = {0u, 0u, 0u, 0u};
            rg[i] = zero;
#pragma unroll
            for (int c = 0; c < 4; ++c) { rx[i][c] = zero; wt[i][c] = 0.f; }
            if (m < p.M) {
                if (co_ok) rg[i] = *reinterpret_cast<const u32x4_t*>(p.dy + (long long)m * Cout + co0 + chunk * 8);
                if (ci_ok) {
                    const int n = m / HW, rem = m - n * HW;
                    const int y = rem / p.W, x = rem - y * p.W;
                    const DfSample s = df_sample(p.om + (long long)m * p.ld, p.modulated, tap, n, y, x, p.H, p.W);
                    const int idx[4] = {s.i00, s.i01, s.i10, s.i11};
                    const float w4[4] = {(1.f - s.lh) * (1.f - s.lw), (1.f - s.lh) * s.lw, s.lh * (1.f - s.lw), s.lh * s.lw};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (idx[c] >= 0) {
                            rx[i][c] = *reinterpret_cast<const u32x4_t*>(p.x + (long long)idx[c] * Cin + ci0 + chunk * 8);
                            wt[i][c] = w4[c] * s.m;
                        }
                }
            }
        }
    };
    auto stage_write = [&](int buf) {
        unsigned char* Ct = smem + buf * 3 * DW_TILE_BYTES;
        unsigned char* Gt = Ct + 2 * DW_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < DW_PASSES; ++i) {
            const int row = row0 + i * 16;
            u32x4_t o, o2;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float lo = 0.f, hi = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    lo += wt[i][c] * bf_lo(rx[i][c][q]);
                    hi += wt[i][c] * bf_hi(rx[i][c][q]);
                }
                o[q] = pack_bf2(lo, hi);
                o2[q] = pack_bf2(lo - bf_lo(o[q]), hi - bf_hi(o[q]));       // what the bf16 rounding dropped
            }
            *reinterpret_cast<u32x4_t*>(Ct + row * DW_PITCH + chunk * 16) = o;
            *reinterpret_cast<u32x4_t*>(Ct + DW_TILE_BYTES + row * DW_PITCH + chunk * 16) = o2;
            *reinterpret_cast<u32x4_t*>(Gt + row * DW_PITCH + chunk * 16) = rg[i];
        }
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // k -> pixel permutation (identical for A and B): k = 8*g4 + j  <->  pixel 16*(g4>>1) + 4*(g4&1) + (j&3) + 8*(j>>2)
    const int g4 = lane >> 4, idx = lane & 15;
    const int prow_base = 16 * (g4 >> 1) + 4 * (g4 & 1);
    const int tr_q = idx >> 2, tr_p = idx & 3;     // lane 4q+p of the group supplies &tile[row + q][col0 + 4p]
    auto load_frag = [&](const unsigned char* tile, int kk, int cbase) -> bf16x8_t {
        typedef __attribute__((ext_vector_type(8))) short s16x8_t;
        const unsigned char* a0 = tile + (kk * 32 + prow_base + tr_q) * DW_PITCH + (cbase + 4 * tr_p) * 2;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a0));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a0 + 8 * DW_PITCH));
        s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8_t, v);
    };
    auto compute = [&](int buf) {
        const unsigned char* Ct = smem + buf * 3 * DW_TILE_BYTES;
        const unsigned char* Gt = Ct + 2 * DW_TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < DW_BKP / 32; ++kk) {
            bf16x8_t a[4], a2[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = load_frag(Ct, kk, wa * 64 + i * 16);
                a2[i] = load_frag(Ct + DW_TILE_BYTES, kk, wa * 64 + i * 16);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = load_frag(Gt, kk, wb * 64 + j * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2[i], b[j], acc[i][j], 0, 0, 0);
                }
        }
    };

    if (step_begin < step_end) {
        stage_load(step_begin);
        stage_write(0);
    }
    __syncthreads();
    int cur = 0;
    for (int st = step_begin; st < step_end; ++st) {
        const bool more = st + 1 < step_end;
        if (more) stage_load(st + 1);
        compute(cur);
        if (more) stage_write(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // D[row = ci][col = co]: lane holds ci = 4 (lane >> 4) + r (4 consecutive), co = lane & 15
    float* slab = p.slab + (long long)split * 9 * Cout * Cin;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int co = co0 + wb * 64 + j * 16 + idx;
        if (co >= Cout) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ci = ci0 + wa * 64 + i * 16 + g4 * 4;
            if (ci >= Cin) continue;
            *reinterpret_cast<f32x4_t*>(slab + ((long long)co * 9 + tap) * Cin + ci) = acc[i][j];
        }
    }
}

// ---- data gradient, stage 2 ------------------------------------------------------------------------------------------------------------
// Thread (pixel, 8-channel chunk): gcol[row][ci 9 + k] of its chunk = 72 contiguous bf16.  part[thread][3 k + {0: d/dh, 1: d/dw, 2: d/dm}].
struct DbParams {
    const bf16_raw* x;
    const bf16_raw* om;
    const bf16_raw* gcol;   // [rows][9 Cin] of this chunk
    float* dx_ws;           // [M][Cin] fp32
    bf16_raw* d_om;
    int H, W, Cin, ld, modulated;
    int p0, rows;           // first pixel row of the chunk, rows in it
    int CH;                 // Cin / 8
    int CHE;                // threads per pixel: min(CH, 256)
    int PB;                 // pixels per workgroup: 256 / CHE
};

__global__ __launch_bounds__(256) void deform_bwd_kernel(const DbParams p) {
    __shared__ float part[256 * 27];
    const int tid = threadIdx.x;
    const int pl = tid / p.CHE, c0 = tid - pl * p.CHE;
    const int row = blockIdx.x * p.PB + pl;
    const int Cin = p.Cin, HW = p.H * p.W;
    float acc[27];
#pragma unroll
    for (int v = 0; v < 27; ++v) acc[v] = 0.f;

    if (pl < p.PB && row < p.rows) {
        const int m = p.p0 + row;
        const int n = m / HW, rem = m - n * HW;
        const int y = rem / p.W, x = rem - y * p.W;
        const bf16_raw* om_row = p.om + (long long)m * p.ld;
        for (int c = c0; c < p.CH; c += p.CHE) {          // more than one round only past 2048 channels
            u32x4_t g[9];
            const u32x4_t* gp = reinterpret_cast<const u32x4_t*>(p.gcol + ((long long)row * Cin + c * 8) * 9);
#pragma unroll
            for (int q = 0; q < 9; ++q) g[q] = gp[q];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const DfSample s = df_sample(om_row, p.modulated, k, n, y, x, p.H, p.W);
                if (s.inside) {
                    const u32x4_t zero = {0u, 0u, 0u, 0u};
                    u32x4_t v00 = zero, v01 = zero, v10 = zero, v11 = zero;
                    if (s.i00 >= 0) v00 = *reinterpret_cast<const u32x4_t*>(p.x + (long long)s.i00 * Cin + c * 8);
                    if (s.i01 >= 0) v01 = *reinterpret_cast<const u32x4_t*>(p.x + (long long)s.i01 * Cin + c * 8);
                    if (s.i10 >= 0) v10 = *reinterpret_cast<const u32x4_t*>(p.x + (long long)s.i10 * Cin + c * 8);
                    if (s.i11 >= 0) v11 = *reinterpret_cast<const u32x4_t*>(p.x + (long long)s.i11 * Cin + c * 8);
                    const float w00 = (1.f - s.lh) * (1.f - s.lw), w01 = (1.f - s.lh) * s.lw, w10 = s.lh * (1.f - s.lw), w11 = s.lh * s.lw;
                    float dh = 0.f, dw = 0.f, dm = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int gi = e * 9 + k;                      // element of the 72-value run (compile-time after unrolling)
                        const unsigned gw = g[gi >> 3][(gi >> 1) & 3];
                        const float gv = (gi & 1) ? bf_hi(gw) : bf_lo(gw);
                        const int q = e >> 1;
                        const float a00 = (e & 1) ? bf_hi(v00[q]) : bf_lo(v00[q]), a01 = (e & 1) ? bf_hi(v01[q]) : bf_lo(v01[q]);
                        const float a10 = (e & 1) ? bf_hi(v10[q]) : bf_lo(v10[q]), a11 = (e & 1) ? bf_hi(v11[q]) : bf_lo(v11[q]);
                        const float gm = gv * s.m;
                        if (s.i00 >= 0) atomicAdd(p.dx_ws + (long long)s.i00 * Cin + c * 8 + e, w00 * gm);
                        if (s.i01 >= 0) atomicAdd(p.dx_ws + (long long)s.i01 * Cin + c * 8 + e, w01 * gm);
                        if (s.i10 >= 0) atomicAdd(p.dx_ws + (long long)s.i10 * Cin + c * 8 + e, w10 * gm);
                        if (s.i11 >= 0) atomicAdd(p.dx_ws + (long long)s.i11 * Cin + c * 8 + e, w11 * gm);
                        dm += gv * (w00 * a00 + w01 * a01 + w10 * a10 + w11 * a11);
                        dh += gm * ((a10 - a00) * (1.f - s.lw) + (a11 - a01) * s.lw);
                        dw += gm * ((a01 - a00) * (1.f - s.lh) + (a11 - a10) * s.lh);
                    }
                    acc[3 * k] += dh; acc[3 * k + 1] += dw; acc[3 * k + 2] += dm;
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 27; ++v) part[tid * 27 + v] = acc[v];
    __syncthreads();

    // d_om: channel c of pixel pl = the sum of its threads' partials in thread order (fixed: reproducible)
    for (int item = tid; item < p.PB * p.ld; item += 256) {
        const int ql = item / p.ld, c = item - ql * p.ld;
        const int r = blockIdx.x * p.PB + ql;
        if (r >= p.rows) continue;
        const long long m = p.p0 + r;
        float sum = 0.f;
        if (c < 18 || (p.modulated && c < 27)) {
            const int v = c < 18 ? (c >> 1) * 3 + (c & 1) : (c - 18) * 3 + 2;
            for (int j = 0; j < p.CHE; ++j) sum += part[(ql * p.CHE + j) * 27 + v];
            if (c >= 18) sum *= df_sigmoid_grad(bf2f(p.om[m * p.ld + c]));
        }
        p.d_om[m * p.ld + c] = f2bf(sum);
    }
}

// d_x = bf16(scratch [+ add]), 8 elements per thread
__global__ __launch_bounds__(256) void deform_dx_finish_kernel(const float* __restrict__ ws, const bf16_raw* __restrict__ add,
                                                               bf16_raw* __restrict__ dx, long long n8) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(ws + i * 8), b = *reinterpret_cast<const f32x4_t*>(ws + i * 8 + 4);
        float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        if (add) {
            const u32x4_t r = *reinterpret_cast<const u32x4_t*>(add + i * 8);
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[2 * q] += bf_lo(r[q]); v[2 * q + 1] += bf_hi(r[q]); }
        }
        *reinterpret_cast<u32x4_t*>(dx + i * 8) = (u32x4_t){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

int check_config(const char* who, int N, int H, int W, int Cin, int Cout, int ld, int modulated, int kernel_size, int stride, int padding,
                 int dilation, int deformable_groups) {
    BD_REQUIRE(kernel_size == 3 && stride == 1 && padding == 1 && dilation == 1 && deformable_groups == 1,
               "%s: only kernel_size=3, stride=1, padding=1, dilation=1, deformable_groups=1 is built (got %d, %d, %d, %d, %d)", who,
               kernel_size, stride, padding, dilation, deformable_groups);
    BD_REQUIRE(N > 0 && H > 0 && W > 0, "%s: empty input (N=%d, H=%d, W=%d)", who, N, H, W);
    BD_REQUIRE(Cin > 0 && Cin % 8 == 0 && Cout > 0 && Cout % 8 == 0, "%s: Cin=%d and Cout=%d must be positive multiples of 8", who, Cin, Cout);
    BD_REQUIRE(ld % 8 == 0 && ld >= (modulated ? 27 : 18), "%s: ld=%d must be a multiple of 8 and hold the %d offset%s channels", who, ld,
               modulated ? 27 : 18, modulated ? " and mask" : "");
    const long long M = (long long)N * H * W, Cmax = Cin > Cout ? Cin : Cout;
    BD_REQUIRE(M * Cmax * 2 < 0x7fffffffll && M * ld * 2 < 0x7fffffffll && 9ll * Cin * Cout * 2 < 0x7fffffffll,
               "%s: tensors of 2 GB or more are not supported (32-bit buffer offsets)", who);
    return BD_OK;
}
bool config_ok(int N, int H, int W, int Cin, int Cout) {
    return N > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 8 == 0 && Cout > 0 && Cout % 8 == 0 &&
           (long long)N * H * W * (Cin > Cout ? Cin : Cout) * 2 < 0x7fffffffll;
}

template <int MI>
int fwd_launch(const DfParams& p0, hipStream_t stream) {
    DfParams p = p0;
    p.co_tiles = cdiv(p.Cout, 64 * MI);
    const size_t lds = 2 * (size_t)(64 * MI * DF_STRIDE + 2 * DF_B_BYTES);
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&deform_fwd_kernel<MI>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = cdiv(p.M, DF_BN) * p.co_tiles;
    bd_note_kernel("deform_fwd_kernel");
    hipLaunchKernelGGL(deform_fwd_kernel<MI>, dim3(grid), dim3(256), lds, stream, p);
    BD_CHECK_LAUNCH("bd_deform_conv_fwd");
    return BD_OK;
}

struct DwPlan { int ci_tiles, co_tiles, splits, steps_per_split, total_steps; };

DwPlan dw_plan(int N, int H, int W, int Cin, int Cout) {
    DwPlan pl;
    const long long M = (long long)N * H * W;
    pl.ci_tiles = cdiv(Cin, DW_TILE);
    pl.co_tiles = cdiv(Cout, DW_TILE);
    pl.total_steps = (int)cdiv64(M, DW_BKP);
    const int tiles = 9 * pl.ci_tiles * pl.co_tiles;
    int splits = 1024 / tiles;
    if (splits < 1) splits = 1;
    const int max_splits = pl.total_steps / 4 > 0 ? pl.total_steps / 4 : 1;
    if (splits > max_splits) splits = max_splits;
    pl.steps_per_split = cdiv(pl.total_steps, splits);
    pl.splits = cdiv(pl.total_steps, pl.steps_per_split);
    return pl;
}

// pixel rows per column-gradient chunk: gcol [rows][9 Cin] bf16 <= DF_GCOL_BYTES
long long bwd_chunk_rows(long long M, int Cin) {
    long long rows = (long long)(DF_GCOL_BYTES / (18ull * (size_t)Cin));
    if (rows < 1) rows = 1;
    return rows < M ? rows : M;
}

}  // namespace

extern "C" int bd_deform_conv_fwd(const void* x, const void* om, const void* w_fwd, const float* bias, void* y, int N, int H, int W, int Cin,
                                  int Cout, int ld, int modulated, int kernel_size, int stride, int padding, int dilation,
                                  int deformable_groups, bd_stream_t stream) {
    if (int e = check_config("deform_conv_fwd", N, H, W, Cin, Cout, ld, modulated, kernel_size, stride, padding, dilation, deformable_groups))
        return e;
    BD_REQUIRE(x && om && w_fwd && y, "deform_conv_fwd: null pointer");
    DfParams p{};
    p.x = (const bf16_raw*)x; p.om = (const bf16_raw*)om; p.w = (const bf16_raw*)w_fwd; p.bias = bias; p.y = (bf16_raw*)y;
    p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.ld = ld; p.modulated = modulated ? 1 : 0;
    p.M = N * H * W;
    p.x_bytes = (unsigned)((long long)p.M * Cin * 2);
    p.w_bytes = (unsigned)(9ll * Cin * Cout * 2);
    // the widest channel tile that still gives every CU a workgroup: a wider tile gathers the sampled operand fewer times
    const int m_tiles = cdiv(p.M, DF_BN), cus = bd_num_cus();
    int mi = Cout > 128 ? 4 : Cout > 64 ? 2 : 1;
    while (mi > 1 && m_tiles * cdiv(Cout, 64 * mi) < cus) mi >>= 1;
    if (mi == 4) return fwd_launch<4>(p, (hipStream_t)stream);
    if (mi == 2) return fwd_launch<2>(p, (hipStream_t)stream);
    return fwd_launch<1>(p, (hipStream_t)stream);
}

extern "C" size_t bd_deform_conv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
    if (!config_ok(N, H, W, Cin, Cout)) return 0;
    const DwPlan pl = dw_plan(N, H, W, Cin, Cout);
    return align256((size_t)pl.splits * 9 * Cin * Cout * sizeof(float)) + bd_colsum_workspace_bytes(Cout);
}

extern "C" int bd_deform_conv_wgrad(const void* x, const void* om, const void* dy, float* dw, float* dbias, int accumulate, void* ws,
                                    size_t ws_bytes, int N, int H, int W, int Cin, int Cout, int ld, int modulated, int kernel_size, int stride,
                                    int padding, int dilation, int deformable_groups, bd_stream_t stream) {
    if (int e = check_config("deform_conv_wgrad", N, H, W, Cin, Cout, ld, modulated, kernel_size, stride, padding, dilation, deformable_groups))
        return e;
    BD_REQUIRE(x && om && dy && dw && ws, "deform_conv_wgrad: null pointer");
    const size_t need = bd_deform_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout);
    BD_REQUIRE(ws_bytes >= need, "deform_conv_wgrad: workspace %zu < required %zu bytes", ws_bytes, need);
    const DwPlan pl = dw_plan(N, H, W, Cin, Cout);
    DwParams p{};
    p.x = (const bf16_raw*)x; p.om = (const bf16_raw*)om; p.dy = (const bf16_raw*)dy; p.slab = (float*)ws;
    p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.ld = ld; p.modulated = modulated ? 1 : 0; p.M = N * H * W;
    p.ci_tiles = pl.ci_tiles; p.co_tiles = pl.co_tiles; p.splits = pl.splits; p.steps_per_split = pl.steps_per_split;
    p.total_steps = pl.total_steps;
    const size_t lds = 6 * DW_TILE_BYTES;
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&deform_wgrad_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = pl.splits * 9 * pl.ci_tiles * pl.co_tiles;
    bd_note_kernel("deform_wgrad_kernel");
    hipLaunchKernelGGL(deform_wgrad_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
    BD_CHECK_LAUNCH("bd_deform_conv_wgrad");
    bd_wgrad_reduce_launch((const float*)ws, pl.splits, 9ll * Cin * Cout, 9 * Cin, nullptr, dw, accumulate, (hipStream_t)stream);
    BD_CHECK_LAUNCH("bd_deform_conv_wgrad(reduce)");
    if (dbias) {
        void* cs = (char*)ws + align256((size_t)pl.splits * 9 * Cin * Cout * sizeof(float));
        return bd_colsum_bf16(dy, 1, (int64_t)p.M, 0, (int64_t)p.M, Cout, dbias, accumulate, cs, bd_colsum_workspace_bytes(Cout), stream);
    }
    return BD_OK;
}

extern "C" size_t bd_deform_conv_bwd_data_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
    if (!config_ok(N, H, W, Cin, Cout)) return 0;
    const long long M = (long long)N * H * W;
    return align256((size_t)M * Cin * sizeof(float)) + (size_t)bwd_chunk_rows(M, Cin) * 9 * Cin * 2;
}

extern "C" int bd_deform_conv_bwd_data(const void* x, const void* om, const void* dy, const void* w_dgrad, const void* add, void* d_x,
                                       void* d_om, void* ws, size_t ws_bytes, int N, int H, int W, int Cin, int Cout, int ld, int modulated,
                                       int kernel_size, int stride, int padding, int dilation, int deformable_groups, bd_stream_t stream) {
    if (int e = check_config("deform_conv_bwd_data", N, H, W, Cin, Cout, ld, modulated, kernel_size, stride, padding, dilation,
                             deformable_groups))
        return e;
    BD_REQUIRE(x && om && dy && w_dgrad && d_x && d_om && ws, "deform_conv_bwd_data: null pointer");
    const size_t need = bd_deform_conv_bwd_data_workspace_bytes(N, H, W, Cin, Cout);
    BD_REQUIRE(ws_bytes >= need, "deform_conv_bwd_data: workspace %zu < required %zu bytes", ws_bytes, need);
    const long long M = (long long)N * H * W;
    float* dx_ws = (float*)ws;
    bf16_raw* gcol = (bf16_raw*)((char*)ws + align256((size_t)M * Cin * sizeof(float)));
    if (hipMemsetAsync(dx_ws, 0, (size_t)M * Cin * sizeof(float), (hipStream_t)stream) != hipSuccess) {
        bd_set_error("deform_conv_bwd_data: clearing the scratch failed");
        return BD_ELAUNCH;
    }
    const long long chunk = bwd_chunk_rows(M, Cin);
    DbParams p{};
    p.x = (const bf16_raw*)x; p.om = (const bf16_raw*)om; p.gcol = gcol; p.dx_ws = dx_ws; p.d_om = (bf16_raw*)d_om;
    p.H = H; p.W = W; p.Cin = Cin; p.ld = ld; p.modulated = modulated ? 1 : 0;
    p.CH = Cin / 8;
    p.CHE = p.CH < 256 ? p.CH : 256;
    p.PB = 256 / p.CHE;
    for (long long r0 = 0; r0 < M; r0 += chunk) {
        const int rows = (int)(M - r0 < chunk ? M - r0 : chunk);
        // stage 1: gcol = dy W as the 1 x 1 convolution Cout -> 9 Cin over this chunk's pixel rows
        bd_conv_desc d{};
        d.N = 1; d.Cin = Cout; d.Cout = 9 * Cin; d.R = 1; d.S = 1; d.stride = 1; d.pad = 0; d.nseg = 1;
        d.Hi[0] = 1; d.Wi[0] = rows; d.Ho[0] = 1; d.Wo[0] = rows;
        d.in_pix_per_img = rows; d.out_pix_per_img = rows;
        if (int e = bd_conv2d_fwd(&d, (const bf16_raw*)dy + r0 * Cout, w_dgrad, nullptr, nullptr, gcol, 0, stream)) return e;
        // stage 2
        p.p0 = (int)r0; p.rows = rows;
        bd_note_kernel("deform_bwd_kernel");
        hipLaunchKernelGGL(deform_bwd_kernel, dim3(cdiv(rows, p.PB)), dim3(256), 0, (hipStream_t)stream, p);
        BD_CHECK_LAUNCH("bd_deform_conv_bwd_data");
    }
    const long long n8 = M * Cin / 8;
    hipLaunchKernelGGL(deform_dx_finish_kernel, dim3(grid_for(n8)), dim3(256), 0, (hipStream_t)stream, (const float*)dx_ws,
                       (const bf16_raw*)add, (bf16_raw*)d_x, n8);
    BD_CHECK_LAUNCH("bd_deform_conv_bwd_data(finish)");
    return BD_OK;
}
