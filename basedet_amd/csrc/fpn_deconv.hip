// FPN learned top-down upsampling (MODEL.FPN.UPSAMPLE = "deconv"; fpn_backbone.py:92-103,131-138) on CDNA4 MFMA (gfx950):
// M.ConvTranspose2d(C, C, kernel_size=4, stride=2, padding=1, bias=False) from a dense NHWC bf16 level x [N][H][W][C] (coarse) to
// y [N][2H][2W][C] (fine), its data gradient and its weight gradient.
//
// With oy = 2 iy - 1 + ky every output row parity reads two of the four kernel rows:
//   oy = 2m     <- (iy = m, ky = 1), (iy = m - 1, ky = 3)
//   oy = 2m + 1 <- (iy = m + 1, ky = 0), (iy = m, ky = 2)
// (columns alike), i.e. output class (py, px) is a 2 x 2-tap convolution of x with source offset (py - a, px - b) for tap (a, b),
// ky = 1 - py + 2a, kx = 1 - px + 2b.  The forward runs the four classes as four implicit GEMMs of K = 4 C: no multiply-by-zero taps.
// The data gradient is the plain 4 x 4 / stride-2 / pad-1 convolution of dy (K = 16 C), the weight gradient
//   dW[ci][ky][kx][co] = sum_{n, iy, ix} x[n, iy, ix, ci] dy[n, 2 iy - 1 + ky, 2 ix - 1 + kx, co]
// a pixel-split GEMM per tap with fp32 slabs and the fixed-order reduce of conv_wgrad.hip (bitwise reproducible).
//
// Weight layouts.  The fp32 master lives in the parameter arena as the OHWI weight of the fine -> coarse Conv2d(k4, s2, p1) that the
// reference's (C_coarse, C_fine, 4, 4) array is the OIHW weight of: w[ci_coarse][ky][kx][co_fine].  bd_fpn_deconv_pack writes
//   w_fwd   bf16 [4 classes][C_fine][4 taps][C_coarse]   (forward: A rows = fine channels, K = tap-major coarse channels)
//   w_dgrad bf16 [C_coarse][16 taps][C_fine]             (data gradient: the master in bf16, same index)
//
// Data kernels: one workgroup = 256 threads = 4 waves (2 channel halves x 2 pixel halves), tile 128 output channels x 128 output pixels
// of one class, K step 64 channels of one tap; A = packed weights, B = the gathered source pixels, both staged global -> registers
// -> LDS with range-checked buffer loads (an out-of-image tap reads zeros through an offset past the buffer), two LDS buffers, one barrier
// per K step; fragments are plain 16-byte LDS reads (160-byte padded rows: conflict-free).  Epilogue: y = bf16(add + acc), in place
// when add == y (one read and one write of each element by the same lane).
#include "common.h"
#include "wgrad_reduce.h"

void bd_wgrad_reduce_launch(const float* slab, int splits, long long n, int row_len, const float* row_scale, float* dw, int accumulate,
                            hipStream_t stream);

namespace {

constexpr int DC_TILE = 128;
constexpr int DC_BK = 64;
constexpr int DC_ROWS_PER_PASS = 32;       // 256 threads x 16 bytes = 32 rows of 64 channels
constexpr int DC_PASSES = DC_TILE / DC_ROWS_PER_PASS;
constexpr int DC_STRIDE = 160;             // 128 data bytes + 32 pad per LDS row
constexpr int DC_TILE_BYTES = DC_TILE * DC_STRIDE;
constexpr unsigned DC_NONE = 0x80000000u;  // >= num_records of every buffer: the load returns zeros

struct DcParams {
    const bf16_raw* src;
    const bf16_raw* w;
    const bf16_raw* add;
    bf16_raw* dst;
    int Hc, Wc, C;
    int M;                 // output pixels per class: N * Hc * Wc
    int co_tiles;
    unsigned src_bytes, w_bytes;
};

// MODE 0: forward (4 classes x 4 taps over x); MODE 1: data gradient (one class, 16 taps over dy)
template <int MODE>
__global__ __launch_bounds__(256) void fpn_deconv_kernel(const DcParams p) {
    constexpr int NCLS = MODE == 0 ? 4 : 1;
    constexpr int TAPS = MODE == 0 ? 4 : 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave >> 1, wp = wave & 1;

    // consecutive tile ids: the channel tiles, then the classes of one pixel tile (they share source rows in L2).  The data gradient
    // (one class) keeps consecutive ids on one XCD as conv_igemm.hip's forward does (bijective remap): 203.5 -> 189.4 us at batch 16,
    // 50x84 -> 100x168 (profiles/fpn_deconv_ab.txt)
    int bid = blockIdx.x;
    if (MODE == 1) {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int co_tile = bid % p.co_tiles;
    bid /= p.co_tiles;
    const int cls = bid % NCLS;
    const int m_tile = bid / NCLS;
    const int py = cls >> 1, px = cls & 1;
    const int m0 = m_tile * DC_TILE, co0 = co_tile * DC_TILE;
    const int C = p.C;
    const int HWc = p.Hc * p.Wc;
    const int Hs = MODE == 0 ? p.Hc : 2 * p.Hc, Ws = MODE == 0 ? p.Wc : 2 * p.Wc;   // source grid

    const int chunk = tid & 7, row0 = tid >> 3;
    int r_y[DC_PASSES], r_x[DC_PASSES], r_base[DC_PASSES];
    unsigned a_voff[DC_PASSES], b_voff[DC_PASSES];
#pragma unroll
    for (int i = 0; i < DC_PASSES; ++i) {
        const int row = row0 + i * DC_ROWS_PER_PASS;
        const int m = m0 + row;
        r_base[i] = -1; r_y[i] = 0; r_x[i] = 0;
        if (m < p.M) {
            const int n = m / HWc, rem = m - n * HWc;
            const int iy = rem / p.Wc, ix = rem - iy * p.Wc;
            r_base[i] = n * Hs * Ws;
            if (MODE == 0) { r_y[i] = iy + py; r_x[i] = ix + px; }          // source = (iy + py - a, ix + px - b)
            else           { r_y[i] = 2 * iy - 1; r_x[i] = 2 * ix - 1; }     // source = (2 iy - 1 + ky, 2 ix - 1 + kx)
        }
        const int co = co0 + row;
        a_voff[i] = co < C ? (unsigned)((((cls * C + co) * TAPS) * C + chunk * 8) * 2) : DC_NONE;
        b_voff[i] = DC_NONE;
    }
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(p.src), 0, p.src_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_raw*>(p.w), 0, p.w_bytes, 0x00020000);

    const int kblocks = C / DC_BK;
    const int nsteps = TAPS * kblocks;
    int cur_tap = -1, cur_kb = kblocks;
    u32x4_t ra[DC_PASSES], rb[DC_PASSES];

    auto stage_load = [&]() {
        if (cur_kb == kblocks) {             // next tap (workgroup-uniform): every staged row's source pixel moves
            cur_kb = 0;
            ++cur_tap;
            int oy, ox;
            if (MODE == 0) { oy = -(cur_tap >> 1); ox = -(cur_tap & 1); }
            else           { oy = cur_tap >> 2; ox = cur_tap & 3; }
#pragma unroll
            for (int i = 0; i < DC_PASSES; ++i) {
                const int sy = r_y[i] + oy, sx = r_x[i] + ox;
                const bool ok = r_base[i] >= 0 && sy >= 0 && sx >= 0 && sy < Hs && sx < Ws;
                b_voff[i] = ok ? (unsigned)(((r_base[i] + sy * Ws + sx) * C + chunk * 8) * 2) : DC_NONE;
            }
        }
        int so_a = (cur_tap * C + cur_kb * DC_BK) * 2, so_b = cur_kb * DC_BK * 2;
        asm volatile("" : "+s"(so_a), "+s"(so_b));
#pragma unroll
        for (int i = 0; i < DC_PASSES; ++i) {
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, a_voff[i], so_a, 0);
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, b_voff[i], so_b, 0);
        }
        ++cur_kb;
    };
    auto stage_write = [&](int buf) {
        unsigned char* At = smem + buf * 2 * DC_TILE_BYTES;
        unsigned char* Bt = At + DC_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < DC_PASSES; ++i) {
            const int row = row0 + i * DC_ROWS_PER_PASS;
            *reinterpret_cast<u32x4_t*>(At + row * DC_STRIDE + chunk * 16) = ra[i];
            *reinterpret_cast<u32x4_t*>(Bt + row * DC_STRIDE + chunk * 16) = rb[i];
        }
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int frag_row = lane & 15, frag_chunk = lane >> 4;

    auto compute = [&](int buf) {
        const unsigned char* At = smem + buf * 2 * DC_TILE_BYTES;
        const unsigned char* Bt = At + DC_TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < DC_BK / 32; ++kk) {
            bf16x8_t a[4], b[4];
            const int ch = kk * 4 + frag_chunk;
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(At + (wc * 64 + i * 16 + frag_row) * DC_STRIDE + ch * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(Bt + (wp * 64 + j * 16 + frag_row) * DC_STRIDE + ch * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
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

    // ---- epilogue: lane holds output channels co0 + wc*64 + 16 i + 4 (lane >> 4) + r of pixel m0 + wp*64 + 16 j + (lane & 15) ----
    const int Wd = MODE == 0 ? 2 * p.Wc : p.Wc, Hd = MODE == 0 ? 2 * p.Hc : p.Hc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + wp * 64 + j * 16 + (lane & 15);
        if (m >= p.M) continue;
        const int n = m / HWc, rem = m - n * HWc;
        const int iy = rem / p.Wc, ix = rem - iy * p.Wc;
        const long long dpix = MODE == 0 ? ((long long)n * Hd + 2 * iy + py) * Wd + 2 * ix + px : (long long)m;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co0 + wc * 64 + i * 16 + 4 * (lane >> 4);
            if (co >= C) continue;
            const long long idx = dpix * C + co;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (p.add) {
                const u32x2_t a = *reinterpret_cast<const u32x2_t*>(p.add + idx);
                v[0] += bf_lo(a[0]); v[1] += bf_hi(a[0]); v[2] += bf_lo(a[1]); v[3] += bf_hi(a[1]);
            }
            *reinterpret_cast<u32x2_t*>(p.dst + idx) = (u32x2_t){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        }
    }
}

// ---- weight gradient: D[co_fine][ci_coarse] per tap, reduction over coarse pixels --------------------------------------------------------
// Tiles staged [pixel][channel] as they lie in HBM (16-byte loads, 288-byte rows) and read with gfx950's transposing LDS read
// ds_read_b64_tr_b16; the k -> pixel permutation (same for both operands) of conv_wgrad.hip keeps the reads conflict-free.
// A = dy gathered at (2 iy - 1 + ky, 2 ix - 1 + kx) (rows = fine channels), B = x at (iy, ix) (columns = coarse channels): every lane
// ends up with 4 consecutive fine channels of one coarse channel = one 16-byte store into the [ci][tap][co] slab of its split.
constexpr int WG_TILE = 128;
constexpr int WG_BKP = 64;                 // pixels per K step
constexpr int WG_PITCH = 288;
constexpr int WG_PASSES = WG_BKP / 16;
constexpr int WG_TILE_BYTES = WG_BKP * WG_PITCH;

struct DwParams {
    const bf16_raw* x;
    const bf16_raw* dy;
    float* slab;            // [splits][C][16][C]
    int Hc, Wc, C, M;
    int c_tiles, splits, steps_per_split, total_steps;
};

__global__ __launch_bounds__(256) void fpn_deconv_wgrad_kernel(const DwParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;     // co half (MFMA rows), ci half (MFMA columns)
    const int tiles_per_split = 16 * p.c_tiles * p.c_tiles;
    int bid = blockIdx.x;
    const int split = bid / tiles_per_split;
    bid -= split * tiles_per_split;
    const int tap = bid / (p.c_tiles * p.c_tiles);
    bid -= tap * (p.c_tiles * p.c_tiles);
    const int ci_tile = bid / p.c_tiles, co_tile = bid - ci_tile * p.c_tiles;
    const int ci0 = ci_tile * WG_TILE, co0 = co_tile * WG_TILE;
    const int ky = tap >> 2, kx = tap & 3;
    const int C = p.C, HWc = p.Hc * p.Wc, Hf = 2 * p.Hc, Wf = 2 * p.Wc;

    const int step_begin = split * p.steps_per_split;
    const int step_end = min(step_begin + p.steps_per_split, p.total_steps);
    const int chunk = tid & 15, row0 = tid >> 4;
    const bool ci_ok = ci0 + chunk * 8 < C, co_ok = co0 + chunk * 8 < C;

    u32x4_t rx[WG_PASSES], rg[WG_PASSES];
    auto stage_load = [&](int step) {
#pragma unroll
        for (int i = 0; i < WG_PASSES; ++i) {
            const int m = step * WG_BKP + row0 + i * 16;
            u32x4_t vx = {0u, 0u, 0u, 0u}, vg = {0u, 0u, 0u, 0u};
            if (m < p.M) {
                const int n = m / HWc, rem = m - n * HWc;
                const int iy = rem / p.Wc, ix = rem - iy * p.Wc;
                if (ci_ok) vx = *reinterpret_cast<const u32x4_t*>(p.x + (long long)m * C + ci0 + chunk * 8);
                const int fy = 2 * iy - 1 + ky, fx = 2 * ix - 1 + kx;
                if (co_ok && fy >= 0 && fx >= 0 && fy < Hf && fx < Wf)
                    vg = *reinterpret_cast<const u32x4_t*>(p.dy + (((long long)n * Hf + fy) * Wf + fx) * C + co0 + chunk * 8);
            }
            rx[i] = vx; rg[i] = vg;
        }
    };
    auto stage_write = [&](int buf) {
        unsigned char* Gt = smem + buf * 2 * WG_TILE_BYTES;
        unsigned char* Xt = Gt + WG_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < WG_PASSES; ++i) {
            const int row = row0 + i * 16;
            *reinterpret_cast<u32x4_t*>(Gt + row * WG_PITCH + chunk * 16) = rg[i];
            *reinterpret_cast<u32x4_t*>(Xt + row * WG_PITCH + chunk * 16) = rx[i];
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
        const unsigned char* a0 = tile + (kk * 32 + prow_base + tr_q) * WG_PITCH + (cbase + 4 * tr_p) * 2;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a0));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(a0 + 8 * WG_PITCH));
        s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8_t, v);
    };
    auto compute = [&](int buf) {
        const unsigned char* Gt = smem + buf * 2 * WG_TILE_BYTES;
        const unsigned char* Xt = Gt + WG_TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < WG_BKP / 32; ++kk) {
            bf16x8_t a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = load_frag(Gt, kk, wa * 64 + i * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = load_frag(Xt, kk, wb * 64 + j * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
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

    // D[row = co][col = ci]: lane holds co = 4 (lane >> 4) + r (4 consecutive), ci = lane & 15
    float* slab = p.slab + (long long)split * 16 * C * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + wb * 64 + j * 16 + idx;
        if (ci >= C) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co0 + wa * 64 + i * 16 + g4 * 4;
            if (co >= C) continue;
            *reinterpret_cast<f32x4_t*>(slab + ((long long)ci * 16 + tap) * C + co) = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void fpn_deconv_pack_kernel(const float* __restrict__ w, int C, bf16_raw* __restrict__ w_fwd,
                                                              bf16_raw* __restrict__ w_dgrad) {
    const long long n = 16ll * C * C;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        // w_fwd[cls][co][t][ci] = w[ci][ky][kx][co], ky = 1 - py + 2a, kx = 1 - px + 2b (cls = 2 py + px, t = 2a + b)
        const int ci = (int)(e % C);
        const int t = (int)((e / C) & 3);
        const int co = (int)((e / (4ll * C)) % C);
        const int cls = (int)(e / (4ll * C * C));
        const int ky = 1 - (cls >> 1) + 2 * (t >> 1), kx = 1 - (cls & 1) + 2 * (t & 1);
        w_fwd[e] = f2bf(w[(((long long)ci * 4 + ky) * 4 + kx) * C + co]);
        w_dgrad[e] = f2bf(w[e]);
    }
}

struct DwPlan { int c_tiles, splits, steps_per_split, total_steps; };

DwPlan dw_plan(int N, int Hc, int Wc, int C) {
    DwPlan pl;
    const long long M = (long long)N * Hc * Wc;
    pl.c_tiles = cdiv(C, WG_TILE);
    pl.total_steps = (int)cdiv64(M, WG_BKP);
    const int tiles = 16 * pl.c_tiles * pl.c_tiles;
    int splits = 1024 / tiles;
    if (splits < 1) splits = 1;
    const int max_splits = pl.total_steps / 4 > 0 ? pl.total_steps / 4 : 1;
    if (splits > max_splits) splits = max_splits;
    pl.steps_per_split = cdiv(pl.total_steps, splits);
    pl.splits = cdiv(pl.total_steps, pl.steps_per_split);
    return pl;
}

int check_shape(const char* who, int N, int Hc, int Wc, int Hf, int Wf, int C) {
    BD_REQUIRE(N > 0 && Hc > 0 && Wc > 0, "%s: empty level (N=%d, H=%d, W=%d)", who, N, Hc, Wc);
    BD_REQUIRE(C > 0 && C % 64 == 0, "%s: C=%d must be a positive multiple of 64", who, C);
    BD_REQUIRE(Hf == 2 * Hc && Wf == 2 * Wc, "%s: the fine level must be exactly 2H x 2W of the coarse one (coarse %dx%d, fine %dx%d)", who,
               Hc, Wc, Hf, Wf);
    BD_REQUIRE((long long)N * Hf * Wf * C * 2 < 0x7fffffffll, "%s: tensors of 2 GB or more are not supported (32-bit buffer offsets)", who);
    return BD_OK;
}

}  // namespace

extern "C" int bd_fpn_deconv_pack(const float* w, int C, void* w_fwd, void* w_dgrad, bd_stream_t stream) {
    BD_REQUIRE(w && w_fwd && w_dgrad, "fpn_deconv_pack: null pointer");
    BD_REQUIRE(C > 0 && C % 64 == 0, "fpn_deconv_pack: C=%d must be a positive multiple of 64", C);
    const long long n = 16ll * C * C;
    const int grid = (int)(cdiv64(n, 256) < 2048 ? cdiv64(n, 256) : 2048);
    hipLaunchKernelGGL(fpn_deconv_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, C, (bf16_raw*)w_fwd, (bf16_raw*)w_dgrad);
    BD_CHECK_LAUNCH("bd_fpn_deconv_pack");
    return BD_OK;
}

template <int MODE>
static int deconv_launch(const char* who, const void* src, const void* w, const void* add, void* dst, int N, int Hc, int Wc, int Hf, int Wf,
                         int C, bd_stream_t stream) {
    if (int e = check_shape(who, N, Hc, Wc, Hf, Wf, C)) return e;
    BD_REQUIRE(src && w && dst, "%s: null pointer", who);
    DcParams p{};
    p.src = (const bf16_raw*)src; p.w = (const bf16_raw*)w; p.add = (const bf16_raw*)add; p.dst = (bf16_raw*)dst;
    p.Hc = Hc; p.Wc = Wc; p.C = C;
    p.M = N * Hc * Wc;
    p.co_tiles = cdiv(C, DC_TILE);
    const long long src_pix = MODE == 0 ? (long long)N * Hc * Wc : (long long)N * Hf * Wf;
    p.src_bytes = (unsigned)(src_pix * C * 2);
    p.w_bytes = (unsigned)(16ll * C * C * 2);
    const size_t lds = 4 * DC_TILE_BYTES;
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fpn_deconv_kernel<MODE>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = cdiv(p.M, DC_TILE) * (MODE == 0 ? 4 : 1) * p.co_tiles;
    bd_note_kernel(MODE == 0 ? "fpn_deconv_kernel<fwd>" : "fpn_deconv_kernel<dgrad>");
    hipLaunchKernelGGL(fpn_deconv_kernel<MODE>, dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
    BD_CHECK_LAUNCH(who);
    return BD_OK;
}

extern "C" int bd_fpn_deconv_fwd(const void* x, const void* w_fwd, const void* add, void* y, int N, int Hc, int Wc, int Hf, int Wf, int C,
                                 bd_stream_t stream) {
    return deconv_launch<0>("fpn_deconv_fwd", x, w_fwd, add, y, N, Hc, Wc, Hf, Wf, C, stream);
}

extern "C" int bd_fpn_deconv_dgrad(const void* dy, const void* w_dgrad, const void* add, void* dx, int N, int Hc, int Wc, int Hf, int Wf,
                                   int C, bd_stream_t stream) {
    return deconv_launch<1>("fpn_deconv_dgrad", dy, w_dgrad, add, dx, N, Hc, Wc, Hf, Wf, C, stream);
}

extern "C" size_t bd_fpn_deconv_wgrad_workspace_bytes(int N, int Hc, int Wc, int C) {
    if (N <= 0 || Hc <= 0 || Wc <= 0 || C <= 0 || C % 64 != 0) return 0;
    const DwPlan pl = dw_plan(N, Hc, Wc, C);
    return (size_t)pl.splits * 16 * C * C * sizeof(float);
}

extern "C" int bd_fpn_deconv_wgrad(const void* x, const void* dy, float* dw, int accumulate, void* ws, size_t ws_bytes, int N, int Hc, int Wc,
                                   int Hf, int Wf, int C, bd_stream_t stream) {
    if (int e = check_shape("fpn_deconv_wgrad", N, Hc, Wc, Hf, Wf, C)) return e;
    BD_REQUIRE(x && dy && dw && ws, "fpn_deconv_wgrad: null pointer");
    const size_t need = bd_fpn_deconv_wgrad_workspace_bytes(N, Hc, Wc, C);
    BD_REQUIRE(ws_bytes >= need, "fpn_deconv_wgrad: workspace %zu < required %zu bytes", ws_bytes, need);
    const DwPlan pl = dw_plan(N, Hc, Wc, C);
    DwParams p{};
    p.x = (const bf16_raw*)x; p.dy = (const bf16_raw*)dy; p.slab = (float*)ws;
    p.Hc = Hc; p.Wc = Wc; p.C = C; p.M = N * Hc * Wc;
    p.c_tiles = pl.c_tiles; p.splits = pl.splits; p.steps_per_split = pl.steps_per_split; p.total_steps = pl.total_steps;
    const size_t lds = 4 * WG_TILE_BYTES;
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fpn_deconv_wgrad_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = pl.splits * 16 * pl.c_tiles * pl.c_tiles;
    bd_note_kernel("fpn_deconv_wgrad_kernel");
    hipLaunchKernelGGL(fpn_deconv_wgrad_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
    BD_CHECK_LAUNCH("bd_fpn_deconv_wgrad");
    bd_wgrad_reduce_launch((const float*)ws, pl.splits, 16ll * C * C, 16 * C, nullptr, dw, accumulate, (hipStream_t)stream);
    BD_CHECK_LAUNCH("bd_fpn_deconv_wgrad(reduce)");
    return BD_OK;
}
