// The output convolutions of CenterNet's head (layers/head/center_head.py:91-131: three SingleHead.out_conv, 1x1, C -> K / 2 / 2) in ONE
// launch per direction.
//
// feat [M][3C] bf16 is the ReLU output of the three feat_convs run as one 3C-row 3x3 convolution: channels [0,C) the cls tower, [C,2C)
// the wh tower, [2C,3C) the reg tower.  Forward writes logits [M][cls_ld] (cls_ld = round_up(K, 8), pad slots +0) and wr [M][8] (slots
// 0-1 wh, 2-3 reg, 4-7 +0): exactly what bd_centernet_focal_fwd_bwd, bd_centernet_l1_fwd_bwd (ld 8, off 0 / 2) and bd_centernet_decode
// read.  On the generic kernels this is three launches (two of them padding 2 channels to 8) forward and three data gradients, three
// weight gradients and a ReLU-gate pass backward.
//
// Both kernels are memory-bound (146 MB forward, 246 MB backward at the recipe's 262 144 pixels, against 2.8 / 5.6 GFLOP),
// so everything that is a GEMM runs on v_mfma_f32_16x16x32_bf16 -- the matrix pipe keeps the VALU free for the packing and the gate, and
// at K = 365 the vector pipe alone would cost as much as the memory traffic -- and the design spends its effort on reading each byte once
// with 16-byte accesses.  Only the 2-row wh / reg data gradients (two FMAs per element) run on the VALU.
//
// Forward: a wave owns 16 pixels.  Lane (p = lane % 16, q = lane / 16) loads the 16 bytes feat[p][tower][32 k + 8 q ..] straight from
// memory, one group ahead: the B operand (K index = channel, column = pixel).  The weights are rounded to bf16 once per workgroup into LDS
// (rows = output channels); the A operand of output tile t is one ds_read_b128.  D puts 4 consecutive output channels of its pixel in
// every lane: an 8-byte store.  wh and reg are one 16-row tile each (rows 0-1 / 2-3 hold weights), contracted with their own tower.
//
// Backward: a workgroup of 4 waves walks tiles of 32 pixels.  The tile's feat, d_logits and d_wr rows are contiguous in memory; they are
// read once (16-byte chunks, one tile ahead in registers) and staged into LDS twice: as they are, [pixel][channel], and transposed,
// [channel][pixel].  Pad slots (d_logits >= K, d_wr 4-7) and rows >= M are zeroed on the way: what they hold is never used.
//   * d_feat, cls tower: D[channel][pixel] = sum_o w[o][channel] g[pixel][o]; A = the transposed weights (LDS, rows permuted as in
//     conv1x1_thin.hip so that a lane ends up with 8 consecutive channels of its pixel), B = the natural d_logits tile.
//   * d_feat, wh / reg towers: g0 w[0][c] + g1 w[1][c] in fp32 on the VALU.
//     All three: gated by the bits of feat (a ReLU output), one rounding to bf16, 16-byte stores.
//   * dW / db: D[o][c] = sum_pixel g[pixel][o] feat[pixel][c]: A and B from the transposed tiles (K index = pixel); db is the same
//     product with a column of ones.  The (Kt + 2) x (Ct + 1) output tiles are dealt round-robin to the 4 waves and stay in registers for
//     the whole launch; the per-workgroup partials go to a slab and a second kernel adds them in workgroup order: no atomics, the same
//     bits on every run.
#include "common.h"

namespace {

constexpr int HW_WAVES = 4;
constexpr int TS = 40;                  // row stride (elements) of the transposed tiles: 32 pixels + 8 pad
constexpr int LDS_MAX = 160 * 1024 - 256;
constexpr int MAX_C = 128;

__host__ __device__ inline int rup(int a, int b) { return (a + b - 1) / b * b; }

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
struct HeadFwdParams {
    const bf16_raw* feat;
    const float *w_cls, *b_cls, *w_wh, *b_wh, *w_reg, *b_reg;
    bf16_raw *logits, *wr;
    long long M;
    int C, K, cls_ld, Cp, ksteps, Kt, groups;
};

__global__ __launch_bounds__(HW_WAVES * 64) void center_head_fwd_kernel(const HeadFwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int px = lane & 15, q = lane >> 4;
    const int C = p.C, K = p.K, sw = p.Cp + 8, R = p.Kt * 16 + 32;
    bf16_raw* w_s = reinterpret_cast<bf16_raw*>(lds_raw);                    // [R][sw]: rows < Kt*16 cls; Kt*16 + {0,1} wh; Kt*16 + 16 + {2,3} reg
    float* bias_s = reinterpret_cast<float*>(lds_raw + (size_t)R * sw * 2);   // [R]
    for (int i = tid; i < R * sw; i += HW_WAVES * 64) {
        const int r = i / sw, c = i - r * sw, r2 = r - p.Kt * 16;
        float v = 0.f;
        if (c < C) {
            if (r < K) v = p.w_cls[(long long)r * C + c];
            else if (r2 == 0 || r2 == 1) v = p.w_wh[r2 * C + c];
            else if (r2 == 18 || r2 == 19) v = p.w_reg[(r2 - 18) * C + c];
        }
        w_s[i] = f2bf(v);
    }
    for (int r = tid; r < R; r += HW_WAVES * 64) {
        const int r2 = r - p.Kt * 16;
        float v = 0.f;
        if (r < K) v = p.b_cls ? p.b_cls[r] : 0.f;
        else if (r2 == 0 || r2 == 1) v = p.b_wh ? p.b_wh[r2] : 0.f;
        else if (r2 == 18 || r2 == 19) v = p.b_reg ? p.b_reg[r2 - 18] : 0.f;
        bias_s[r] = v;
    }
    __syncthreads();

    const int nw = gridDim.x * HW_WAVES;
    int grp = blockIdx.x * HW_WAVES + wave;
    u32x4_t cur[3][4], nxt[3][4];
    auto load = [&](u32x4_t (&v)[3][4], int g) {
        const long long row = (long long)g * 16 + px;
        const bool ok = g < p.groups && row < p.M;
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[t][k] = (u32x4_t){0u, 0u, 0u, 0u};
                const int c = 32 * k + 8 * q;
                if (k < p.ksteps && ok && c < C) v[t][k] = *reinterpret_cast<const u32x4_t*>(p.feat + row * 3 * C + t * C + c);
            }
    };
    auto tile = [&](int t, const u32x4_t (&x)[4]) {          // 16 rows of w_s starting at row 16 t, against one tower
        const float* b = bias_s + 16 * t + 4 * q;
        f32x4_t acc = {b[0], b[1], b[2], b[3]};
        const bf16_raw* a = w_s + (16 * t + px) * sw + 8 * q;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < p.ksteps)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(a + 32 * k), __builtin_bit_cast(bf16x8_t, x[k]), acc, 0, 0, 0);
        return acc;
    };
    load(cur, grp);
    for (; grp < p.groups; grp += nw) {
        load(nxt, grp + nw);
        const long long row = (long long)grp * 16 + px;
        const bool ok = row < p.M;
        for (int t = 0; t < p.Kt; ++t) {
            const f32x4_t acc = tile(t, cur[0]);
            const int o0 = 16 * t + 4 * q;
            if (ok && o0 < p.cls_ld) {                       // (cls_ld % 8 == 0: a lane's 4 slots are inside the row or all outside)
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = o0 + i < K ? acc[i] : 0.f;
                *reinterpret_cast<u32x2_t*>(p.logits + row * p.cls_ld + o0) = (u32x2_t){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
            }
        }
        const f32x4_t awh = tile(p.Kt, cur[1]), areg = tile(p.Kt + 1, cur[2]);
        if (ok && q < 2) {
            u32x2_t o = {0u, 0u};
            if (q == 0) o = (u32x2_t){pack_bf2(awh[0], awh[1]), pack_bf2(areg[2], areg[3])};
            *reinterpret_cast<u32x2_t*>(p.wr + row * 8 + 4 * q) = o;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) cur[t][k] = nxt[t][k];
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
struct HeadBwdParams {
    const bf16_raw *feat, *dlog, *dwr;
    const float *w_cls, *w_wh, *w_reg;
    bf16_raw* dfeat;
    float* slab;
    long long M;
    int C, K, cls_ld, Cp, Kp, Kt, Ct, iters, nx, ng;
    int sg, sx;                                    // row strides (elements) of the natural tiles: Kp + 8, 3 Cp + 8
    int o_wT, o_gs, o_xs, o_gT, o_dT, o_xT;        // LDS offsets in bf16 elements (multiples of 8)
    int o_wwr, o_dwr;                              // LDS offsets in floats (multiples of 4)
    int lds_bytes;
};

// fills the LDS layout of a shape; returns false where it does not fit
bool bwd_layout(int C, int K, HeadBwdParams* p) {
    p->C = C; p->K = K; p->cls_ld = rup(K, 8); p->Cp = rup(C, 32); p->Kp = rup(p->cls_ld, 32); p->Kt = (K + 15) / 16; p->Ct = C / 16;
    p->sg = p->Kp + 8; p->sx = 3 * p->Cp + 8;
    p->nx = 32 * (3 * C / 8); p->ng = 32 * (p->cls_ld / 8);
    long long o = 0;
    p->o_wT = (int)o; o += (long long)p->Cp * p->sg;
    p->o_gs = (int)o; o += 32ll * p->sg;
    p->o_xs = (int)o; o += 32ll * p->sx;
    p->o_gT = (int)o; o += (long long)p->Kt * 16 * TS;
    p->o_dT = (int)o; o += 16 * TS;
    p->o_xT = (int)o; o += 3ll * p->Ct * 16 * TS;
    long long f = o / 2;                           // (every size above is a multiple of 8 elements)
    p->o_wwr = (int)f; f += 4 * p->Cp;
    p->o_dwr = (int)f; f += 32 * 4;
    p->lds_bytes = (int)(f * 4);
    return f * 4 <= LDS_MAX;
}

// one 16-byte chunk of the tile a thread stages: where it comes from and where it goes
// (two words: they live in registers for the whole launch)
struct Chunk {
    int where;          // LDS byte offset of the natural copy / 16 | LDS element offset of the transposed copy << 14
    int info;           // kind (0 feat, 1 d_logits, 2 d_wr, 3 none) | pixel << 2 | valid elements << 7 | chunk index inside its tensor's tile << 11
};

template <int MAXT, int MAXCH>
__global__ __launch_bounds__(HW_WAVES * 64) void center_head_bwd_kernel(const HeadBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16_raw* lds = reinterpret_cast<bf16_raw*>(lds_raw);
    float* ldsf = reinterpret_cast<float*>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int px = lane & 15, q = lane >> 4;
    const int C = p.C, K = p.K, Cp = p.Cp, sg = p.sg, sx = p.sx, Kt = p.Kt, Ct = p.Ct;

    for (int i = tid; i < p.lds_bytes / 16; i += HW_WAVES * 64) reinterpret_cast<u32x4_t*>(lds_raw)[i] = (u32x4_t){0u, 0u, 0u, 0u};
    __syncthreads();
    for (int i = tid; i < K * C; i += HW_WAVES * 64) {                      // wT[c][o] = bf16(w_cls[o][c])
        const int o = i / C, c = i - o * C;
        lds[p.o_wT + c * sg + o] = f2bf(p.w_cls[i]);
    }
    for (int i = tid; i < 4 * C; i += HW_WAVES * 64) {                      // wwr[0..1] = w_wh, [2..3] = w_reg, rounded to bf16
        const int r = i / C, c = i - r * C;
        const float v = r < 2 ? p.w_wh[r * C + c] : p.w_reg[(r - 2) * C + c];
        ldsf[p.o_wwr + r * Cp + c] = bf2f(f2bf(v));
    }

    Chunk ch[MAXCH];
#pragma unroll
    for (int j = 0; j < MAXCH; ++j) {
        const int idx = tid + HW_WAVES * 64 * j;
        Chunk c{0, 3};
        if (idx < p.nx) {
            const int per = 3 * C / 8, pp = idx / per, e0 = (idx - pp * per) * 8, tw = e0 / C, cc = e0 - tw * C;
            c.where = (p.o_xs + pp * sx + tw * Cp + cc) / 8 | (p.o_xT + (tw * Ct * 16 + cc) * TS + pp) << 14;
            c.info = 0 | pp << 2 | 8 << 7 | idx << 11;
        } else if (idx < p.nx + p.ng) {
            const int i2 = idx - p.nx, per = p.cls_ld / 8, pp = i2 / per, e0 = (i2 - pp * per) * 8;
            c.where = (p.o_gs + pp * sg + e0) / 8 | (p.o_gT + e0 * TS + pp) << 14;
            c.info = 1 | pp << 2 | (K - e0 < 8 ? K - e0 : 8) << 7 | i2 << 11;
        } else if (idx < p.nx + p.ng + 32) {
            const int pp = idx - p.nx - p.ng;
            c.where = (p.o_dwr + pp * 4) / 4 | (p.o_dT + pp) << 14;
            c.info = 2 | pp << 2 | 4 << 7 | pp << 11;
        }
        ch[j] = c;
    }

    u32x4_t reg[MAXCH];
    auto load = [&](int it) {
        const long long row0 = (long long)it * 32;
#pragma unroll
        for (int j = 0; j < MAXCH; ++j) {
            const int kind = ch[j].info & 3, pp = (ch[j].info >> 2) & 31, nv = (ch[j].info >> 7) & 15;
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (kind != 3 && it < p.iters && row0 + pp < p.M) {
                const bf16_raw* src = kind == 0 ? p.feat + row0 * 3 * C : kind == 1 ? p.dlog + row0 * p.cls_ld : p.dwr + row0 * 8;
                v = *reinterpret_cast<const u32x4_t*>(src + (ch[j].info >> 11) * 8);
#pragma unroll
                for (int w = 0; w < 4; ++w)                                  // pad slots may hold anything: they are zeroed, never used
                    v[w] &= (2 * w < nv ? 0xffffu : 0u) | (2 * w + 1 < nv ? 0xffff0000u : 0u);
            }
            reg[j] = v;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < MAXCH; ++j) {
            const int kind = ch[j].info & 3;
            if (kind == 3) continue;
            const u32x4_t v = reg[j];
            unsigned char* nat = lds_raw + (ch[j].where & 0x3fff) * 16;
            if (kind == 2) *reinterpret_cast<f32x4_t*>(nat) = (f32x4_t){bf_lo(v[0]), bf_hi(v[0]), bf_lo(v[1]), bf_hi(v[1])};
            else *reinterpret_cast<u32x4_t*>(nat) = v;
            bf16_raw* t = lds + (ch[j].where >> 14);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (kind == 2 && w >= 2) break;
                t[(2 * w) * TS] = (bf16_raw)(v[w] & 0xffffu);
                t[(2 * w + 1) * TS] = (bf16_raw)(v[w] >> 16);
            }
        }
    };

    f32x4_t acc[MAXT];
#pragma unroll
    for (int i = 0; i < MAXT; ++i) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int ncb = Cp / 32, nunits = 6 * ncb, ksg = p.Kp / 32;
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)(px == 0 ? 1.f : 0.f);

    const int ot0 = wave / (Ct + 1), ct0 = wave - ot0 * (Ct + 1);
    const int G = gridDim.x;
    int it = blockIdx.x;
    load(it);
    __syncthreads();                                                         // the weights are in place
    for (; it < p.iters; it += G) {
        stage();
        __syncthreads();
        load(it + G);
        const long long row0 = (long long)it * 32;
        // ---- data gradient ----
        for (int u = wave; u < nunits; u += HW_WAVES) {
            const int cb = u % ncb, tw = (u / ncb) % 3, pg = u / (3 * ncb);
            const int pp = pg * 16 + px, cl = cb * 32 + 8 * q;
            u32x4_t out;
            if (tw == 0) {
                f32x4_t r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0;
                const bf16_raw* b = lds + p.o_gs + pp * sg + 8 * q;
                const bf16_raw* a0 = lds + p.o_wT + (cb * 32 + 8 * (px >> 2) + (px & 3)) * sg + 8 * q;
                const bf16_raw* a1 = a0 + 4 * sg;
                for (int s = 0; s < ksg; ++s) {
                    const bf16x8_t bv = *reinterpret_cast<const bf16x8_t*>(b + 32 * s);
                    r0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(a0 + 32 * s), bv, r0, 0, 0, 0);
                    r1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(a1 + 32 * s), bv, r1, 0, 0, 0);
                }
                out = (u32x4_t){pack_bf2(r0[0], r0[1]), pack_bf2(r0[2], r0[3]), pack_bf2(r1[0], r1[1]), pack_bf2(r1[2], r1[3])};
            } else {
                const float* gw = ldsf + p.o_dwr + pp * 4 + 2 * (tw - 1);
                const float g0 = gw[0], g1 = gw[1];
                const float* w0 = ldsf + p.o_wwr + (2 * (tw - 1)) * Cp + cl;
                const float* w1 = w0 + Cp;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaf(g0, w0[e], g1 * w1[e]);
                out = (u32x4_t){pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
            }
            const u32x4_t xv = *reinterpret_cast<const u32x4_t*>(lds + p.o_xs + pp * sx + tw * Cp + cl);
#pragma unroll
            for (int k = 0; k < 4; ++k) {                                    // gate: feat is a ReLU output, a channel passes where its bits are non-zero
                const unsigned w = xv[k];
                out[k] &= ((w & 0x7fffu) ? 0xffffu : 0u) | ((w & 0x7fff0000u) ? 0xffff0000u : 0u);
            }
            if (row0 + pp < p.M && cl < C) *reinterpret_cast<u32x4_t*>(p.dfeat + (row0 + pp) * 3 * C + tw * C + cl) = out;
        }
        // ---- weight / bias gradient ----
        int ot = ot0, ct = ct0;
        asm volatile("" : "+s"(ot), "+s"(ct));                               // (walked, not divided; opaque so that no per-tile address is kept across iterations)
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            if (ot < Kt + 2) {
                const int tw = ot < Kt ? 0 : ot - Kt + 1;
                const bf16_raw* a = ot < Kt ? lds + p.o_gT + (ot * 16 + px) * TS + 8 * q : lds + p.o_dT + px * TS + 8 * q;
                bf16x8_t bv = ones;
                if (ct < Ct) bv = *reinterpret_cast<const bf16x8_t*>(lds + p.o_xT + (tw * Ct * 16 + ct * 16 + px) * TS + 8 * q);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(a), bv, acc[i], 0, 0, 0);
            }
            ct += HW_WAVES;                                                  // tile wave + 4 (i + 1): Ct + 1 >= 2 columns, at most two wraps
            if (ct > Ct) { ct -= Ct + 1; ++ot; }
            if (ct > Ct) { ct -= Ct + 1; ++ot; }
        }
        __syncthreads();
    }
    const int SC = (Ct + 1) * 16;
    float* slab = p.slab + (long long)blockIdx.x * (Kt + 2) * 16 * SC;
    int ot = ot0, ct = ct0;
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        if (ot < Kt + 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[(ot * 16 + 4 * q + r) * SC + ct * 16 + px] = acc[i][r];
        }
        ct += HW_WAVES;
        if (ct > Ct) { ct -= Ct + 1; ++ot; }
        if (ct > Ct) { ct -= Ct + 1; ++ot; }
    }
}

struct HeadReduceParams {
    const float* slab;
    float *dw_cls, *db_cls, *dw_wh, *db_wh, *dw_reg, *db_reg;
    int grid, C, K, Kt, Ct, accumulate;
};

// sums the workgroups' partials: eight lanes per element take every eighth workgroup each (in index order), then the eight partial sums
// are added in lane order -- a fixed tree for a given grid
__global__ __launch_bounds__(256) void center_head_reduce_kernel(const HeadReduceParams p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int e = t >> 3, part = t & 7;
    const int SC = (p.Ct + 1) * 16, SR = (p.Kt + 2) * 16;
    float* dst = nullptr;
    if (e < SR * SC) {
        const int r = e / SC, c = e - r * SC, r2 = r - p.Kt * 16;
        float *dw = nullptr, *db = nullptr;
        int o = 0;
        if (r < p.K) { dw = p.dw_cls; db = p.db_cls; o = r; }
        else if (r2 == 0 || r2 == 1) { dw = p.dw_wh; db = p.db_wh; o = r2; }
        else if (r2 == 18 || r2 == 19) { dw = p.dw_reg; db = p.db_reg; o = r2 - 18; }
        if (c < p.C) dst = dw ? dw + (long long)o * p.C + c : nullptr;
        else if (c == p.C) dst = db ? db + o : nullptr;
    }
    float s = 0.f;
    if (dst)
        for (int b = part; b < p.grid; b += 8) s += p.slab[(long long)b * SR * SC + e];
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) s += __shfl_xor(s, m, 64);
    if (dst && part == 0) *dst = p.accumulate ? *dst + s : s;
}

int bwd_grid(long long M, int lds_bytes) {
    const long long iters = (M + 31) / 32;
    int per_cu = (160 * 1024) / (lds_bytes > 0 ? lds_bytes : 1);
    per_cu = per_cu < 1 ? 1 : per_cu > 2 ? 2 : per_cu;
    const long long g = (long long)bd_num_cus() * per_cu;
    return (int)(iters < g ? iters : g);
}

// the checks both directions share; returns BD_OK or BD_EINVAL with the message set
int check_shape(const char* who, long long M, int C, int K, int cls_ld) {
    BD_REQUIRE(M > 0 && C > 0 && K > 0, "%s: M = %lld, C = %d, K = %d must be positive", who, M, C, K);
    BD_REQUIRE(C % 16 == 0 && C <= MAX_C, "%s: C = %d (supported: multiples of 16 up to %d)", who, C, MAX_C);
    BD_REQUIRE(cls_ld == rup(K, 8), "%s: cls_ld = %d, expected round_up(K = %d, 8) = %d", who, cls_ld, K, rup(K, 8));
    BD_REQUIRE(M * 3 * C * 2 < (1ll << 31) && M * cls_ld * 2 < (1ll << 31), "%s: M = %lld: a tensor reaches 2 GB", who, M);
    return BD_OK;
}

bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

}  // namespace

extern "C" int bd_center_head_out_fwd(const void* feat, const float* w_cls, const float* b_cls, const float* w_wh, const float* b_wh,
                                      const float* w_reg, const float* b_reg, int64_t M, int C, int K, int cls_ld, void* logits, void* wr,
                                      bd_stream_t stream) {
    BD_REQUIRE(feat && w_cls && w_wh && w_reg && logits && wr, "center_head_out_fwd: null pointer");
    const int rc = check_shape("center_head_out_fwd", M, C, K, cls_ld);
    if (rc != BD_OK) return rc;
    BD_REQUIRE(aligned16(feat) && aligned16(logits) && aligned16(wr), "center_head_out_fwd: feat, logits and wr must be 16-byte aligned");
    HeadFwdParams p{};
    p.feat = (const bf16_raw*)feat; p.w_cls = w_cls; p.b_cls = b_cls; p.w_wh = w_wh; p.b_wh = b_wh; p.w_reg = w_reg; p.b_reg = b_reg;
    p.logits = (bf16_raw*)logits; p.wr = (bf16_raw*)wr; p.M = M; p.C = C; p.K = K; p.cls_ld = cls_ld;
    p.Cp = rup(C, 32); p.ksteps = p.Cp / 32; p.Kt = (K + 15) / 16; p.groups = (int)((M + 15) / 16);
    const int R = p.Kt * 16 + 32;
    const long long lds = (long long)R * (p.Cp + 8) * 2 + R * 4;
    BD_REQUIRE(lds <= LDS_MAX, "center_head_out_fwd: C = %d, K = %d: the weights (%lld bytes as bf16) do not fit the LDS (%d)", C, K, lds, LDS_MAX);
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&center_head_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    int per_cu = (int)((160 * 1024) / lds);
    per_cu = per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu;
    int grid = bd_num_cus() * per_cu;
    if (grid > (p.groups + HW_WAVES - 1) / HW_WAVES) grid = (p.groups + HW_WAVES - 1) / HW_WAVES;
    hipLaunchKernelGGL(center_head_fwd_kernel, dim3(grid), dim3(HW_WAVES * 64), (size_t)lds, (hipStream_t)stream, p);
    BD_CHECK_LAUNCH("bd_center_head_out_fwd");
    return BD_OK;
}

extern "C" size_t bd_center_head_out_bwd_workspace_bytes(int64_t M, int C, int K) {
    HeadBwdParams p{};
    if (M <= 0 || C <= 0 || K <= 0 || C % 16 != 0 || C > MAX_C || !bwd_layout(C, K, &p)) return 0;
    return (size_t)bwd_grid(M, p.lds_bytes) * (p.Kt + 2) * 16 * (p.Ct + 1) * 16 * 4 + 256;
}

extern "C" int bd_center_head_out_bwd(const void* feat, const void* d_logits, const void* d_wr, const float* w_cls, const float* w_wh,
                                      const float* w_reg, int64_t M, int C, int K, int cls_ld, void* d_feat, float* dw_cls, float* db_cls,
                                      float* dw_wh, float* db_wh, float* dw_reg, float* db_reg, int accumulate, void* ws, size_t ws_bytes,
                                      bd_stream_t stream) {
    BD_REQUIRE(feat && d_logits && d_wr && w_cls && w_wh && w_reg && d_feat && dw_cls && dw_wh && dw_reg && ws, "center_head_out_bwd: null pointer");
    const int rc = check_shape("center_head_out_bwd", M, C, K, cls_ld);
    if (rc != BD_OK) return rc;
    BD_REQUIRE(aligned16(feat) && aligned16(d_logits) && aligned16(d_wr) && aligned16(d_feat) && aligned16(ws),
               "center_head_out_bwd: feat, d_logits, d_wr, d_feat and ws must be 16-byte aligned");
    HeadBwdParams p{};
    BD_REQUIRE(bwd_layout(C, K, &p), "center_head_out_bwd: C = %d, K = %d: the tiles (%d bytes) do not fit the LDS (%d)", C, K, p.lds_bytes, LDS_MAX);
    const int ntiles = (p.Kt + 2) * (p.Ct + 1), nchunks = p.nx + p.ng + 32;
    BD_REQUIRE(ntiles <= HW_WAVES * 32 && nchunks <= HW_WAVES * 64 * 12,
               "center_head_out_bwd: C = %d, K = %d: %d gradient tiles / %d staging chunks per workgroup (supported: %d / %d)", C, K, ntiles,
               nchunks, HW_WAVES * 32, HW_WAVES * 64 * 12);
    const size_t need = bd_center_head_out_bwd_workspace_bytes(M, C, K);
    if (ws_bytes < need) {
        bd_set_error("center_head_out_bwd: workspace %zu < %zu bytes", ws_bytes, need);
        return BD_EWORKSPACE;
    }
    p.feat = (const bf16_raw*)feat; p.dlog = (const bf16_raw*)d_logits; p.dwr = (const bf16_raw*)d_wr;
    p.w_cls = w_cls; p.w_wh = w_wh; p.w_reg = w_reg; p.dfeat = (bf16_raw*)d_feat; p.slab = (float*)ws; p.M = M;
    p.iters = (int)((M + 31) / 32);
    const int grid = bwd_grid(M, p.lds_bytes);
    hipStream_t st = (hipStream_t)stream;
    BD_ONCE_PER_DEVICE(
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&center_head_bwd_kernel<10, 6>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&center_head_bwd_kernel<32, 12>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    if (ntiles <= HW_WAVES * 10 && nchunks <= HW_WAVES * 64 * 6)
        hipLaunchKernelGGL((center_head_bwd_kernel<10, 6>), dim3(grid), dim3(HW_WAVES * 64), (size_t)p.lds_bytes, st, p);
    else
        hipLaunchKernelGGL((center_head_bwd_kernel<32, 12>), dim3(grid), dim3(HW_WAVES * 64), (size_t)p.lds_bytes, st, p);
    HeadReduceParams r{};
    r.slab = (const float*)ws; r.dw_cls = dw_cls; r.db_cls = db_cls; r.dw_wh = dw_wh; r.db_wh = db_wh; r.dw_reg = dw_reg; r.db_reg = db_reg;
    r.grid = grid; r.C = C; r.K = K; r.Kt = p.Kt; r.Ct = p.Ct; r.accumulate = accumulate;
    const int elems = (p.Kt + 2) * 16 * (p.Ct + 1) * 16;
    hipLaunchKernelGGL(center_head_reduce_kernel, dim3((elems * 8 + 255) / 256), dim3(256), 0, st, r);
    BD_CHECK_LAUNCH("bd_center_head_out_bwd");
    return BD_OK;
}
