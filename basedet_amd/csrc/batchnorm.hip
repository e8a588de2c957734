// BatchNorm2d in training mode for the FPN's lateral / output convolutions (MODEL.FPN.NORM = "BN" / "SyncBN"; fpn_backbone.py:49-76) and for
// the backbone's (MODEL.BACKBONE.NORM; its epilogue, norm + shortcut + ReLU in one pass, is bd_bn_apply_act_fwd):
// NHWC bf16 activations, fp32 statistics.  One call serves ONE pyramid level of a pixel-major tensor that may hold several: row r of the
// level (r < N * n) is pixel row (r / n) * pix_per_img + off + r % n of the buffer, C channels each, C % 8 == 0.
//   fwd: stats (read y) -> apply (read y, write z)              bwd: reduce (read g, y) -> apply (read g, y, write g_y)
// All four passes are HBM-bound; every lane moves 16-byte chunks of 8 channels.
// Reductions are two-stage over fixed 128-row slots with a fixed combination order and no floating-point atomics: the same bits on every
// run.  The variance never goes through a raw sum of squares: a thread accumulates its (at most 16) rows SHIFTED by the first of them
// (differences of bf16 values are exact in fp32), and every combination after that is Chan's pairwise update of (count, mean, M2) -- a
// channel with |mean| = 100 std keeps its variance to a few ulp.
#include "common.h"

namespace {

constexpr int BN_SLOT = 128;     // rows per stage-1 slot
constexpr int BN_PXL = 8;        // pixel lanes of a stage-1 block (x 32 chunk lanes = 256 threads)
constexpr int BN_FL = 128;       // slot lanes of a stage-2 block (x 8 channels = 1024 threads)

struct BnGeo { long long ppi, off; };            // a tensor's row addressing: row (img, p) = img * ppi + off + p
// (BnWelford / bn_combine, Chan et al.'s statistics of the union of two disjoint sets: common.h -- GroupNorm shares them)

__device__ __forceinline__ void unpack8(const u32x4_t v, float* o) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[2 * k] = bf_lo(v[k]); o[2 * k + 1] = bf_hi(v[k]); }
}

__device__ __forceinline__ long long bn_row_addr(long long r, long long n, BnGeo g) {
    const long long img = r / n;
    return img * g.ppi + g.off + (r - img * n);
}

// stage 1 of the statistics.  grid = (slots, ceil(C / 256)); block = 32 chunk lanes x 8 pixel lanes.
// part[(slot * C + c) * 2] = (mean, M2) of the slot's rows (their count follows from the slot index)
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const bf16_raw* __restrict__ y, BnGeo gy, long long n, long long M, int C,
                                                               float* __restrict__ part) {
    __shared__ float red[BN_PXL][32][8][3];
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cl) * 8;
    const long long r0 = (long long)blockIdx.x * BN_SLOT;
    long long r1 = r0 + BN_SLOT;
    if (r1 > M) r1 = M;
    float cnt = 0.f, K[8], s[8], ss[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { K[k] = 0.f; s[k] = 0.f; ss[k] = 0.f; }
    if (c0 < C) {
        for (long long r = r0 + pl; r < r1; r += BN_PXL) {
            float v[8];
            unpack8(*reinterpret_cast<const u32x4_t*>(y + bn_row_addr(r, n, gy) * C + c0), v);
            if (cnt == 0.f) {
#pragma unroll
                for (int k = 0; k < 8; ++k) K[k] = v[k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float d = v[k] - K[k]; s[k] += d; ss[k] = __fmaf_rn(d, d, ss[k]); }
            cnt += 1.f;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
        red[pl][cl][k][0] = cnt;
        red[pl][cl][k][1] = K[k] + s[k] * inv;
        red[pl][cl][k][2] = fmaxf(ss[k] - s[k] * s[k] * inv, 0.f);
    }
    __syncthreads();
    if (pl == 0 && c0 < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            BnWelford a = {red[0][cl][k][0], red[0][cl][k][1], red[0][cl][k][2]};
            for (int q = 1; q < BN_PXL; ++q) a = bn_combine(a, BnWelford{red[q][cl][k][0], red[q][cl][k][1], red[q][cl][k][2]});
            float* o = part + ((long long)blockIdx.x * C + c0 + k) * 2;
            o[0] = a.mean; o[1] = a.m2;
        }
    }
}

// mean, inv_std, sums = [M, sum y, sum y^2] and the running statistics of one channel from its (count, mean, M2)
__device__ __forceinline__ void bn_write_stats(int c, int C, float M, float mu, float m2, float eps, float momentum, float* mean, float* inv_std,
                                               float* sums, float* running_mean, float* running_var) {
    const float var = m2 / M;
    if (mean) mean[c] = mu;
    if (inv_std) inv_std[c] = 1.f / sqrtf(var + eps);
    if (sums) { sums[c] = M; sums[C + c] = mu * M; sums[2 * C + c] = __fmaf_rn(mu * M, mu, m2); }
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (m2 / fmaxf(M - 1.f, 1.f));
}

// stage 2: a block owns 8 channels; 128 lanes walk the slots (lane q: q, q + 128, ... in order), then a fixed binary tree over the lanes
__global__ __launch_bounds__(8 * BN_FL) void bn_stats_final_kernel(const float* __restrict__ part, int slots, long long M, int C, float eps,
                                                                   float momentum, float* __restrict__ mean, float* __restrict__ inv_std,
                                                                   float* __restrict__ sums, float* __restrict__ running_mean,
                                                                   float* __restrict__ running_var) {
    __shared__ float red[BN_FL][8][3];
    const int cl = threadIdx.x & 7, sl = threadIdx.x >> 3;
    const int c = blockIdx.x * 8 + cl;
    BnWelford a = {0.f, 0.f, 0.f};
    if (c < C)
        for (int s = sl; s < slots; s += BN_FL) {
            long long left = M - (long long)s * BN_SLOT;
            const float* o = part + ((long long)s * C + c) * 2;
            a = bn_combine(a, BnWelford{(float)(left < BN_SLOT ? left : BN_SLOT), o[0], o[1]});
        }
    red[sl][cl][0] = a.n; red[sl][cl][1] = a.mean; red[sl][cl][2] = a.m2;
    __syncthreads();
    for (int w = BN_FL / 2; w > 0; w >>= 1) {
        if (sl < w) {
            a = bn_combine(BnWelford{red[sl][cl][0], red[sl][cl][1], red[sl][cl][2]},
                           BnWelford{red[sl + w][cl][0], red[sl + w][cl][1], red[sl + w][cl][2]});
            red[sl][cl][0] = a.n; red[sl][cl][1] = a.mean; red[sl][cl][2] = a.m2;
        }
        __syncthreads();
    }
    if (sl == 0 && c < C) bn_write_stats(c, C, (float)M, red[0][cl][1], red[0][cl][2], eps, momentum, mean, inv_std, sums, running_mean, running_var);
}

// z = [relu](gamma * (y - mean) * inv_std + beta [+ residual]): the epilogue of every normalised convolution in ONE pass (read y and the
// residual, write z).  The FPN's norms (MODEL.FPN.NORM) take neither residual nor ReLU; the backbone's (MODEL.BACKBONE.NORM) are conv -> BN
// -> ReLU, and conv -> BN -> + identity -> ReLU in a block's last stage (models/cls/resnet.py:42-52, 94-113).
// block = 32 chunk lanes x 8 row lanes (blockIdx.y: the 256-channel tile), rows grid-strided: a thread keeps ONE chunk of 8 channels, so
// everything that depends only on the channel is formed once per thread.  The arithmetic is fp64 on the fp32 statistics: the pass is
// HBM-bound (three fp64 operations per element), and where gamma * xhat cancels against beta -- or y against a mean of 100 std -- an fp32
// evaluation is off by more than the bf16 ulp of the small result.  One rounding to fp32, one to bf16; the residual joins in fp64 BEFORE
// that single rounding, so a shortcut that cancels gamma * xhat + beta keeps the bits of the small difference.
template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bn_apply_act_fwd_kernel(const bf16_raw* __restrict__ y, BnGeo gy, const float* __restrict__ mean,
                                                               const float* __restrict__ inv_std, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const bf16_raw* __restrict__ res, BnGeo gr,
                                                               bf16_raw* __restrict__ z, BnGeo gz, long long n, long long M, int C) {
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cl) * 8;
    if (c0 >= C) return;
    double A[8];
    float mu[8], bt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { A[k] = (double)gamma[c0 + k] * (double)inv_std[c0 + k]; mu[k] = mean[c0 + k]; bt[k] = beta[c0 + k]; }
    for (long long r = (long long)blockIdx.x * BN_PXL + pl; r < M; r += (long long)gridDim.x * BN_PXL) {
        float v[8], a[8], o[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(y + bn_row_addr(r, n, gy) * C + c0), v);
        if (RES) unpack8(*reinterpret_cast<const u32x4_t*>(res + bn_row_addr(r, n, gr) * C + c0), a);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double t = ((double)v[k] - (double)mu[k]) * A[k] + (double)bt[k];
            if (RES) t += (double)a[k];
            const float f = (float)t;
            o[k] = RELU ? (f > 0.f ? f : 0.f) : f;
        }
        u32x4_t w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = pack_bf2(o[2 * k], o[2 * k + 1]);
        *reinterpret_cast<u32x4_t*>(z + bn_row_addr(r, n, gz) * C + c0) = w;
    }
}

// stage 1 of the backward sums: part[(slot * C + c) * 2] = (sum g * xhat, sum g) over the slot's rows
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const bf16_raw* __restrict__ g, BnGeo gg, const bf16_raw* __restrict__ y, BnGeo gy,
                                                             const float* __restrict__ mean, const float* __restrict__ inv_std, long long n,
                                                             long long M, int C, float* __restrict__ part) {
    __shared__ float red[BN_PXL][32][8][2];
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cl) * 8;
    const long long r0 = (long long)blockIdx.x * BN_SLOT;
    long long r1 = r0 + BN_SLOT;
    if (r1 > M) r1 = M;
    float dg[8], db[8], mu[8], rs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { dg[k] = 0.f; db[k] = 0.f; mu[k] = 0.f; rs[k] = 0.f; }
    if (c0 < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { mu[k] = mean[c0 + k]; rs[k] = inv_std[c0 + k]; }
        for (long long r = r0 + pl; r < r1; r += BN_PXL) {
            float vg[8], vy[8];
            unpack8(*reinterpret_cast<const u32x4_t*>(g + bn_row_addr(r, n, gg) * C + c0), vg);
            unpack8(*reinterpret_cast<const u32x4_t*>(y + bn_row_addr(r, n, gy) * C + c0), vy);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                dg[k] = __fmaf_rn(vg[k], (vy[k] - mu[k]) * rs[k], dg[k]);
                db[k] += vg[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[pl][cl][k][0] = dg[k]; red[pl][cl][k][1] = db[k]; }
    __syncthreads();
    if (pl == 0 && c0 < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float a = red[0][cl][k][0], b = red[0][cl][k][1];
            for (int q = 1; q < BN_PXL; ++q) { a += red[q][cl][k][0]; b += red[q][cl][k][1]; }
            float* o = part + ((long long)blockIdx.x * C + c0 + k) * 2;
            o[0] = a; o[1] = b;
        }
    }
}

// stage 2: as bn_stats_final_kernel, with plain sums
__global__ __launch_bounds__(8 * BN_FL) void bn_bwd_final_kernel(const float* __restrict__ part, int slots, int C, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta) {
    __shared__ float red[BN_FL][8][2];
    const int cl = threadIdx.x & 7, sl = threadIdx.x >> 3;
    const int c = blockIdx.x * 8 + cl;
    float a = 0.f, b = 0.f;
    if (c < C)
        for (int s = sl; s < slots; s += BN_FL) { a += part[((long long)s * C + c) * 2]; b += part[((long long)s * C + c) * 2 + 1]; }
    red[sl][cl][0] = a; red[sl][cl][1] = b;
    __syncthreads();
    for (int w = BN_FL / 2; w > 0; w >>= 1) {
        if (sl < w) { red[sl][cl][0] += red[sl + w][cl][0]; red[sl][cl][1] += red[sl + w][cl][1]; }
        __syncthreads();
    }
    if (sl == 0 && c < C) { dgamma[c] = red[0][cl][0]; dbeta[c] = red[0][cl][1]; }
}

// g_y = gamma * inv_std * (g - dbeta / M - xhat * dgamma / M), M = count[c] (the first vector of sums).  Layout and fp64 as in
// bn_apply_act_fwd_kernel (the three terms cancel wherever the gradient is mostly its own mean); the divisions are per thread, not per element:
// g_y = A * (g - B - (y - mean) * E) with A = gamma * inv_std, B = dbeta / M, E = inv_std * dgamma / M
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const bf16_raw* __restrict__ g, BnGeo gg, const bf16_raw* __restrict__ y, BnGeo gy,
                                                           const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                           const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                           const float* __restrict__ dbeta, const float* __restrict__ count,
                                                           bf16_raw* __restrict__ out, BnGeo go, long long n, long long M, int C) {
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cl) * 8;
    if (c0 >= C) return;
    double A[8], B[8], E[8];
    float mu[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double rs = (double)inv_std[c0 + k], m = (double)count[c0 + k];
        A[k] = (double)gamma[c0 + k] * rs;
        B[k] = (double)dbeta[c0 + k] / m;
        E[k] = rs * ((double)dgamma[c0 + k] / m);
        mu[k] = mean[c0 + k];
    }
    for (long long r = (long long)blockIdx.x * BN_PXL + pl; r < M; r += (long long)gridDim.x * BN_PXL) {
        float vg[8], vy[8], o[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(g + bn_row_addr(r, n, gg) * C + c0), vg);
        unpack8(*reinterpret_cast<const u32x4_t*>(y + bn_row_addr(r, n, gy) * C + c0), vy);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (float)(A[k] * ((double)vg[k] - B[k] - ((double)vy[k] - (double)mu[k]) * E[k]));
        u32x4_t w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = pack_bf2(o[2 * k], o[2 * k + 1]);
        *reinterpret_cast<u32x4_t*>(out + bn_row_addr(r, n, go) * C + c0) = w;
    }
}

// ---- conv -> BatchNorm -> SiLU (YOLOX: every convolution of the head, the PAFPN and CSPDarknet) --------------------------------------
// SiLU's derivative is a function of the activation input u = gamma * xhat + beta alone, and u follows from the pre-norm y the norm's
// backward reads anyway: the gate folds into the reduce and the apply pass (five tensor passes instead of the ReLU chain's seven, no gated
// gradient tensor, the forward output z is not kept).  ONE device function forms u for the three kernels, exactly as
// bn_apply_act_fwd_kernel does: fp64 on the fp32 statistics, one rounding to fp32.
__device__ __forceinline__ double bn_silu_u64(float y, float mu, double A, float bt) { return ((double)y - (double)mu) * A + (double)bt; }
__device__ __forceinline__ float bn_silu_u(float y, float mu, double A, float bt) { return (float)bn_silu_u64(y, mu, A, bt); }

// s = sigma(u), sm = sigma(-u), both from e = exp(-|u|) <= 1: nothing overflows at |u| ~ 100, and 1 - sigma(u) is never a subtraction
__device__ __forceinline__ void bn_sigmoid_pair(float u, float& s, float& sm) {
    const float e = expf(-fabsf(u));
    const float r = 1.f / (1.f + e);
    const float big = r, small = e * r;          // sigma(|u|), sigma(-|u|)
    s = u >= 0.f ? big : small;
    sm = u >= 0.f ? small : big;
}

__device__ __forceinline__ float bn_silu(float u) {
    float s, sm;
    bn_sigmoid_pair(u, s, sm);
    return u * s;
}

// d silu / du = sigma(u) (1 + u sigma(-u)); exactly 1 where sigma(u) and 1 + u sigma(-u) round to 1 (u > ~ 21), exactly 0 where exp(u) underflows
__device__ __forceinline__ float bn_silu_grad(float u) {
    float s, sm;
    bn_sigmoid_pair(u, s, sm);
    return s * (1.f + u * sm);
}

// The same derivative in fp64 on the UNROUNDED u, for the backward apply: there g_u meets -B - (y - mean) E, and where the three cancel an
// fp32 gate (relative error ~ 1e-7 of g_u) is off by several bf16 steps of the small result (measured: 21 steps at 129 x 264, 3 at
// 1030 x 24) -- the reason bn_bwd_apply_kernel is fp64 throughout.  Exactly 1 where exp(-u) and u exp(-u) vanish against 1 (u > ~ 40).
__device__ __forceinline__ double bn_silu_grad64(double u) {
    const double e = exp(-fabs(u));
    const double r = 1.0 / (1.0 + e);
    const double big = r, small = e * r;
    const double s = u >= 0.0 ? big : small, sm = u >= 0.0 ? small : big;
    return s * (1.0 + u * sm);
}

// z = silu(u): bn_apply_act_fwd_kernel's layout; SiLU in fp32, one rounding to bf16
__global__ __launch_bounds__(256) void bn_silu_fwd_kernel(const bf16_raw* __restrict__ y, BnGeo gy, const float* __restrict__ mean,
                                                          const float* __restrict__ inv_std, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, bf16_raw* __restrict__ z, BnGeo gz, long long n,
                                                          long long M, int C) {
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cl) * 8;
    if (c0 >= C) return;
    double A[8];
    float mu[8], bt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { A[k] = (double)gamma[c0 + k] * (double)inv_std[c0 + k]; mu[k] = mean[c0 + k]; bt[k] = beta[c0 + k]; }
    for (long long r = (long long)blockIdx.x * BN_PXL + pl; r < M; r += (long long)gridDim.x * BN_PXL) {
        float v[8], o[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(y + bn_row_addr(r, n, gy) * C + c0), v);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = bn_silu(bn_silu_u(v[k], mu[k], A[k], bt[k]));
        u32x4_t w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = pack_bf2(o[2 * k], o[2 * k + 1]);
        *reinterpret_cast<u32x4_t*>(z + bn_row_addr(r, n, gz) * C + c0) = w;
    }
}

// stage 1 of the SiLU backward sums: bn_bwd_partial_kernel on g_u = g * silu'(u); part[(slot * C + c) * 2] = (sum g_u * xhat, sum g_u).
// Stage 2 is bn_bwd_final_kernel.
__global__ __launch_bounds__(256) void bn_silu_bwd_partial_kernel(const bf16_raw* __restrict__ g, BnGeo gg, const bf16_raw* __restrict__ y,
                                                                  BnGeo gy, const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta, long long n,
                                                                  long long M, int C, float* __restrict__ part) {
    __shared__ float red[BN_PXL][32][8][2];
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cl) * 8;
    const long long r0 = (long long)blockIdx.x * BN_SLOT;
    long long r1 = r0 + BN_SLOT;
    if (r1 > M) r1 = M;
    float dg[8], db[8], mu[8], rs[8], bt[8];
    double A[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { dg[k] = 0.f; db[k] = 0.f; mu[k] = 0.f; rs[k] = 0.f; bt[k] = 0.f; A[k] = 0.0; }
    if (c0 < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            mu[k] = mean[c0 + k]; rs[k] = inv_std[c0 + k]; bt[k] = beta[c0 + k];
            A[k] = (double)gamma[c0 + k] * (double)rs[k];
        }
        for (long long r = r0 + pl; r < r1; r += BN_PXL) {
            float vg[8], vy[8];
            unpack8(*reinterpret_cast<const u32x4_t*>(g + bn_row_addr(r, n, gg) * C + c0), vg);
            unpack8(*reinterpret_cast<const u32x4_t*>(y + bn_row_addr(r, n, gy) * C + c0), vy);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float gu = vg[k] * bn_silu_grad(bn_silu_u(vy[k], mu[k], A[k], bt[k]));
                dg[k] = __fmaf_rn(gu, (vy[k] - mu[k]) * rs[k], dg[k]);
                db[k] += gu;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[pl][cl][k][0] = dg[k]; red[pl][cl][k][1] = db[k]; }
    __syncthreads();
    if (pl == 0 && c0 < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float a = red[0][cl][k][0], b = red[0][cl][k][1];
            for (int q = 1; q < BN_PXL; ++q) { a += red[q][cl][k][0]; b += red[q][cl][k][1]; }
            float* o = part + ((long long)blockIdx.x * C + c0 + k) * 2;
            o[0] = a; o[1] = b;
        }
    }
}

// g_y = A * (g_u - B - (y - mean) * E): bn_bwd_apply_kernel with g_u = g * silu'(u) recomputed (fp64, see bn_silu_grad64) in place of g
__global__ __launch_bounds__(256) void bn_silu_bwd_apply_kernel(const bf16_raw* __restrict__ g, BnGeo gg, const bf16_raw* __restrict__ y, BnGeo gy,
                                                                const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                                const float* __restrict__ count, bf16_raw* __restrict__ out, BnGeo go,
                                                                long long n, long long M, int C) {
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c0 = (blockIdx.y * 32 + cl) * 8;
    if (c0 >= C) return;
    double A[8], B[8], E[8];
    float mu[8], bt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double rs = (double)inv_std[c0 + k], m = (double)count[c0 + k];
        A[k] = (double)gamma[c0 + k] * rs;
        B[k] = (double)dbeta[c0 + k] / m;
        E[k] = rs * ((double)dgamma[c0 + k] / m);
        mu[k] = mean[c0 + k];
        bt[k] = beta[c0 + k];
    }
    for (long long r = (long long)blockIdx.x * BN_PXL + pl; r < M; r += (long long)gridDim.x * BN_PXL) {
        float vg[8], vy[8], o[8];
        unpack8(*reinterpret_cast<const u32x4_t*>(g + bn_row_addr(r, n, gg) * C + c0), vg);
        unpack8(*reinterpret_cast<const u32x4_t*>(y + bn_row_addr(r, n, gy) * C + c0), vy);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double gu = (double)vg[k] * bn_silu_grad64(bn_silu_u64(vy[k], mu[k], A[k], bt[k]));
            o[k] = (float)(A[k] * (gu - B[k] - ((double)vy[k] - (double)mu[k]) * E[k]));
        }
        u32x4_t w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = pack_bf2(o[2 * k], o[2 * k + 1]);
        *reinterpret_cast<u32x4_t*>(out + bn_row_addr(r, n, go) * C + c0) = w;
    }
}

inline bool bn_geo_ok(int64_t ppi, int64_t off, int64_t n) { return off >= 0 && n >= 1 && off + n <= ppi; }
inline int bn_slots(int64_t M) { return (int)cdiv64(M, BN_SLOT); }
// blocks along the rows of an apply launch: four rows per thread until the cap (the grid-stride loop takes the rest)
inline dim3 bn_apply_grid(long long M, int C) { return dim3(grid_for(M, 4 * BN_PXL, 4096), cdiv(C, 256)); }

}  // namespace

extern "C" size_t bd_bn_workspace_bytes(int64_t rows, int C) {
    return (size_t)(rows > 0 ? bn_slots(rows) : 0) * (size_t)(C > 0 ? C : 0) * 2 * sizeof(float);
}

extern "C" int bd_bn_stats_fwd(const void* y, int N, int64_t pix_per_img, int64_t off, int64_t n, int C, float eps, float momentum,
                               float* mean, float* inv_std, float* sums, float* running_mean, float* running_var, void* ws, size_t ws_bytes,
                               bd_stream_t stream) {
    BD_REQUIRE(y && ws && (mean || sums), "bn_stats_fwd: null pointer");
    BD_REQUIRE(N >= 1 && C >= 8 && C % 8 == 0 && bn_geo_ok(pix_per_img, off, n), "bn_stats_fwd: bad shape (N=%d C=%d)", N, C);
    const long long M = (long long)N * n;
    BD_REQUIRE(M < (1ll << 24), "bn_stats_fwd: %lld rows (the fp32 row count is exact below 2^24)", M);
    if (ws_bytes < bd_bn_workspace_bytes(M, C)) { bd_set_error("bn_stats_fwd: workspace too small"); return BD_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const int S = bn_slots(M);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(S, cdiv(C, 256)), dim3(256), 0, st, (const bf16_raw*)y, BnGeo{pix_per_img, off},
                       (long long)n, M, C, (float*)ws);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(cdiv(C, 8)), dim3(8 * BN_FL), 0, st, (const float*)ws, S, M, C, eps, momentum, mean, inv_std,
                       sums, running_mean, running_var);
    BD_CHECK_LAUNCH("bd_bn_stats_fwd");
    return BD_OK;
}

extern "C" int bd_bn_apply_act_fwd(const void* y, int64_t y_pix_per_img, int64_t y_off, const float* mean, const float* inv_std,
                                   const float* gamma, const float* beta, const void* residual, int64_t r_pix_per_img, int64_t r_off, void* z,
                                   int64_t z_pix_per_img, int64_t z_off, int N, int64_t n, int C, int relu, bd_stream_t stream) {
    BD_REQUIRE(y && mean && inv_std && gamma && beta && z, "bn_apply_act_fwd: null pointer");
    BD_REQUIRE(N >= 1 && C >= 8 && C % 8 == 0 && bn_geo_ok(y_pix_per_img, y_off, n) && bn_geo_ok(z_pix_per_img, z_off, n)
               && (!residual || bn_geo_ok(r_pix_per_img, r_off, n)), "bn_apply_act_fwd: bad shape (N=%d C=%d)", N, C);
    BD_REQUIRE(z != y && z != residual, "bn_apply_act_fwd: the backward pass reads the pre-norm tensor and the shortcut: z needs a buffer of its own");
    const long long M = (long long)N * n;
    const BnGeo gy{y_pix_per_img, y_off}, gr{r_pix_per_img, r_off}, gz{z_pix_per_img, z_off};
    hipStream_t st = (hipStream_t)stream;
#define BD_BN_ACT(RES, RELU)                                                                                                             \
    hipLaunchKernelGGL((bn_apply_act_fwd_kernel<RES, RELU>), bn_apply_grid(M, C), dim3(256), 0, st, (const bf16_raw*)y, gy, mean, inv_std, \
                       gamma, beta, (const bf16_raw*)residual, gr, (bf16_raw*)z, gz, (long long)n, M, C)
    if (residual) { if (relu) BD_BN_ACT(true, true); else BD_BN_ACT(true, false); }
    else { if (relu) BD_BN_ACT(false, true); else BD_BN_ACT(false, false); }
#undef BD_BN_ACT
    BD_CHECK_LAUNCH("bd_bn_apply_act_fwd");
    return BD_OK;
}

extern "C" int bd_bn_bwd_reduce(const void* g, int64_t g_pix_per_img, int64_t g_off, const void* y, int64_t y_pix_per_img, int64_t y_off,
                                const float* mean, const float* inv_std, int N, int64_t n, int C, float* dgamma, float* dbeta, void* ws,
                                size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(g && y && mean && inv_std && dgamma && dbeta && ws, "bn_bwd_reduce: null pointer");
    BD_REQUIRE(N >= 1 && C >= 8 && C % 8 == 0 && bn_geo_ok(g_pix_per_img, g_off, n) && bn_geo_ok(y_pix_per_img, y_off, n),
               "bn_bwd_reduce: bad shape (N=%d C=%d)", N, C);
    const long long M = (long long)N * n;
    if (ws_bytes < bd_bn_workspace_bytes(M, C)) { bd_set_error("bn_bwd_reduce: workspace too small"); return BD_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const int S = bn_slots(M);
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(S, cdiv(C, 256)), dim3(256), 0, st, (const bf16_raw*)g, BnGeo{g_pix_per_img, g_off},
                       (const bf16_raw*)y, BnGeo{y_pix_per_img, y_off}, mean, inv_std, (long long)n, M, C, (float*)ws);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(cdiv(C, 8)), dim3(8 * BN_FL), 0, st, (const float*)ws, S, C, dgamma, dbeta);
    BD_CHECK_LAUNCH("bd_bn_bwd_reduce");
    return BD_OK;
}

extern "C" int bd_bn_bwd_apply(const void* g, int64_t g_pix_per_img, int64_t g_off, const void* y, int64_t y_pix_per_img, int64_t y_off,
                               const float* mean, const float* inv_std, const float* gamma, const float* dgamma, const float* dbeta,
                               const float* count, void* gy, int64_t gy_pix_per_img, int64_t gy_off, int N, int64_t n, int C, bd_stream_t stream) {
    BD_REQUIRE(g && y && mean && inv_std && gamma && dgamma && dbeta && count && gy, "bn_bwd_apply: null pointer");
    BD_REQUIRE(N >= 1 && C >= 8 && C % 8 == 0 && bn_geo_ok(g_pix_per_img, g_off, n) && bn_geo_ok(y_pix_per_img, y_off, n)
               && bn_geo_ok(gy_pix_per_img, gy_off, n), "bn_bwd_apply: bad shape (N=%d C=%d)", N, C);
    BD_REQUIRE(gy != g, "bn_bwd_apply: the result needs a buffer of its own (the top-down path still reads g)");
    const long long M = (long long)N * n;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, bn_apply_grid(M, C), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)g,
                       BnGeo{g_pix_per_img, g_off}, (const bf16_raw*)y, BnGeo{y_pix_per_img, y_off}, mean, inv_std, gamma, dgamma, dbeta, count,
                       (bf16_raw*)gy, BnGeo{gy_pix_per_img, gy_off}, (long long)n, M, C);
    BD_CHECK_LAUNCH("bd_bn_bwd_apply");
    return BD_OK;
}

extern "C" int bd_bn_silu_fwd(const void* y, int64_t y_pix_per_img, int64_t y_off, const float* mean, const float* inv_std, const float* gamma,
                              const float* beta, void* z, int64_t z_pix_per_img, int64_t z_off, int N, int64_t n, int C, bd_stream_t stream) {
    BD_REQUIRE(y && mean && inv_std && gamma && beta && z, "bn_silu_fwd: null pointer");
    BD_REQUIRE(N >= 1 && C >= 8 && C % 8 == 0 && bn_geo_ok(y_pix_per_img, y_off, n) && bn_geo_ok(z_pix_per_img, z_off, n),
               "bn_silu_fwd: bad shape (N=%d C=%d)", N, C);
    BD_REQUIRE(z != y, "bn_silu_fwd: the backward pass reads the pre-norm tensor: z needs a buffer of its own");
    const long long M = (long long)N * n;
    hipLaunchKernelGGL(bn_silu_fwd_kernel, bn_apply_grid(M, C), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)y,
                       BnGeo{y_pix_per_img, y_off}, mean, inv_std, gamma, beta, (bf16_raw*)z, BnGeo{z_pix_per_img, z_off}, (long long)n, M, C);
    BD_CHECK_LAUNCH("bd_bn_silu_fwd");
    return BD_OK;
}

extern "C" int bd_bn_silu_bwd_reduce(const void* g, int64_t g_pix_per_img, int64_t g_off, const void* y, int64_t y_pix_per_img, int64_t y_off,
                                     const float* mean, const float* inv_std, const float* gamma, const float* beta, int N, int64_t n, int C,
                                     float* dgamma, float* dbeta, void* ws, size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(g && y && mean && inv_std && gamma && beta && dgamma && dbeta && ws, "bn_silu_bwd_reduce: null pointer");
    BD_REQUIRE(N >= 1 && C >= 8 && C % 8 == 0 && bn_geo_ok(g_pix_per_img, g_off, n) && bn_geo_ok(y_pix_per_img, y_off, n),
               "bn_silu_bwd_reduce: bad shape (N=%d C=%d)", N, C);
    const long long M = (long long)N * n;
    if (ws_bytes < bd_bn_workspace_bytes(M, C)) { bd_set_error("bn_silu_bwd_reduce: workspace too small"); return BD_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const int S = bn_slots(M);
    hipLaunchKernelGGL(bn_silu_bwd_partial_kernel, dim3(S, cdiv(C, 256)), dim3(256), 0, st, (const bf16_raw*)g, BnGeo{g_pix_per_img, g_off},
                       (const bf16_raw*)y, BnGeo{y_pix_per_img, y_off}, mean, inv_std, gamma, beta, (long long)n, M, C, (float*)ws);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(cdiv(C, 8)), dim3(8 * BN_FL), 0, st, (const float*)ws, S, C, dgamma, dbeta);
    BD_CHECK_LAUNCH("bd_bn_silu_bwd_reduce");
    return BD_OK;
}

extern "C" int bd_bn_silu_bwd_apply(const void* g, int64_t g_pix_per_img, int64_t g_off, const void* y, int64_t y_pix_per_img, int64_t y_off,
                                    const float* mean, const float* inv_std, const float* gamma, const float* beta, const float* dgamma,
                                    const float* dbeta, const float* count, void* gy, int64_t gy_pix_per_img, int64_t gy_off, int N, int64_t n,
                                    int C, bd_stream_t stream) {
    BD_REQUIRE(g && y && mean && inv_std && gamma && beta && dgamma && dbeta && count && gy, "bn_silu_bwd_apply: null pointer");
    BD_REQUIRE(N >= 1 && C >= 8 && C % 8 == 0 && bn_geo_ok(g_pix_per_img, g_off, n) && bn_geo_ok(y_pix_per_img, y_off, n)
               && bn_geo_ok(gy_pix_per_img, gy_off, n), "bn_silu_bwd_apply: bad shape (N=%d C=%d)", N, C);
    BD_REQUIRE(gy != g && gy != y, "bn_silu_bwd_apply: the result needs a buffer of its own (a second tower may still read g; y is re-read per step)");
    const long long M = (long long)N * n;
    hipLaunchKernelGGL(bn_silu_bwd_apply_kernel, bn_apply_grid(M, C), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)g,
                       BnGeo{g_pix_per_img, g_off}, (const bf16_raw*)y, BnGeo{y_pix_per_img, y_off}, mean, inv_std, gamma, beta, dgamma, dbeta,
                       count, (bf16_raw*)gy, BnGeo{gy_pix_per_img, gy_off}, (long long)n, M, C);
    BD_CHECK_LAUNCH("bd_bn_silu_bwd_apply");
    return BD_OK;
}
