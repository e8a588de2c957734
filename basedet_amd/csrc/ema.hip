// Moving average of the fp32 master weights (TRAINER.EMA: layers/common/ema.py:71-81), alone and folded into the SGD launch, and the
// buffer exchange ModelEMA.applied() evaluates through.  HBM-bound passes over the parameter arena: 16-byte accesses per lane, a scalar
// tail, a grid-stride loop under grid_for's cap (common.h).
#include "common.h"

namespace {

// ema_elem (common.h): ema.py:80, both products and the sum rounded to fp32, never an FMA
__global__ void ema_kernel(float* __restrict__ e, const float* __restrict__ w, long long n, float m, float one_minus_m) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += (long long)gridDim.x * blockDim.x) {
        const long long o = i * 4;
        if (o + 4 <= n) {
            f32x4_t ev = *reinterpret_cast<f32x4_t*>(e + o);
            const f32x4_t wv = *reinterpret_cast<const f32x4_t*>(w + o);
#pragma unroll
            for (int k = 0; k < 4; ++k) ev[k] = ema_elem(ev[k], wv[k], m, one_minus_m);
            *reinterpret_cast<f32x4_t*>(e + o) = ev;
        } else {
            for (long long k = o; k < n; ++k) e[k] = ema_elem(e[k], w[k], m, one_minus_m);
        }
    }
}

// sgd_kernel (image_ops.hip) with the average updated from the new weight while it is still in registers.  The three SGD lines are that
// kernel's, character for character and under the same contraction mode, so that w and v come out with its bits
// (tests/test_ema_gpu.py compares the two launches).
__global__ void sgd_ema_kernel(float* __restrict__ w, float* __restrict__ v, const float* __restrict__ g, float* __restrict__ e,
                               long long n, float lr, float momentum, float wd, float grad_scale, float m, float one_minus_m) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += (long long)gridDim.x * blockDim.x) {
        const long long o = i * 4;
        if (o + 4 <= n) {
            f32x4_t wv = *reinterpret_cast<f32x4_t*>(w + o);
            f32x4_t vv = *reinterpret_cast<f32x4_t*>(v + o);
            const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + o);
            f32x4_t ev = *reinterpret_cast<f32x4_t*>(e + o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gg = gv[k] * grad_scale + wd * wv[k];
                vv[k] = momentum * vv[k] + gg;
                wv[k] -= lr * vv[k];
                ev[k] = ema_elem(ev[k], wv[k], m, one_minus_m);
            }
            *reinterpret_cast<f32x4_t*>(w + o) = wv;
            *reinterpret_cast<f32x4_t*>(v + o) = vv;
            *reinterpret_cast<f32x4_t*>(e + o) = ev;
        } else {
            for (long long k = o; k < n; ++k) {
                const float gg = g[k] * grad_scale + wd * w[k];
                v[k] = momentum * v[k] + gg;
                w[k] -= lr * v[k];
                e[k] = ema_elem(e[k], w[k], m, one_minus_m);
            }
        }
    }
}

__global__ void swap_kernel(float* __restrict__ a, float* __restrict__ b, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += (long long)gridDim.x * blockDim.x) {
        const long long o = i * 4;
        if (o + 4 <= n) {
            const f32x4_t av = *reinterpret_cast<const f32x4_t*>(a + o);
            const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(b + o);
            *reinterpret_cast<f32x4_t*>(a + o) = bv;
            *reinterpret_cast<f32x4_t*>(b + o) = av;
        } else {
            for (long long k = o; k < n; ++k) {
                const float t = a[k];
                a[k] = b[k];
                b[k] = t;
            }
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool disjoint(const float* a, const float* b, int64_t n) { return a + n <= b || b + n <= a; }

}  // namespace

extern "C" int bd_ema_update(float* e, const float* w, int64_t n, float m, float one_minus_m, bd_stream_t stream) {
    BD_REQUIRE(n >= 0, "ema_update: negative n");
    if (n == 0) return BD_OK;
    BD_REQUIRE(e && w, "ema_update: null pointer");
    BD_REQUIRE(aligned16(e) && aligned16(w), "ema_update: e and w must be 16-byte aligned");
    BD_REQUIRE(disjoint(e, w, n), "ema_update: e and w overlap");
    hipLaunchKernelGGL(ema_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, e, w, (long long)n, m, one_minus_m);
    BD_CHECK_LAUNCH("bd_ema_update");
    return BD_OK;
}

extern "C" int bd_sgd_momentum_ema_step(float* w, float* v, const float* g, float* e, int64_t n, float lr, float momentum, float wd,
                                        float grad_scale, float m, float one_minus_m, bd_stream_t stream) {
    BD_REQUIRE(n >= 0, "sgd_momentum_ema_step: negative n");
    if (n == 0) return BD_OK;
    BD_REQUIRE(w && v && g && e, "sgd_momentum_ema_step: null pointer");
    BD_REQUIRE(aligned16(w) && aligned16(v) && aligned16(g) && aligned16(e), "sgd_momentum_ema_step: w, v, g and e must be 16-byte aligned");
    BD_REQUIRE(disjoint(e, w, n) && disjoint(e, v, n) && disjoint(e, g, n), "sgd_momentum_ema_step: e overlaps w, v or g");
    hipLaunchKernelGGL(sgd_ema_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, w, v, g, e, (long long)n, lr,
                       momentum, wd, grad_scale, m, one_minus_m);
    BD_CHECK_LAUNCH("bd_sgd_momentum_ema_step");
    return BD_OK;
}

extern "C" int bd_swap_f32(float* a, float* b, int64_t n, bd_stream_t stream) {
    BD_REQUIRE(n >= 0, "swap_f32: negative n");
    if (n == 0) return BD_OK;
    BD_REQUIRE(a && b, "swap_f32: null pointer");
    BD_REQUIRE(aligned16(a) && aligned16(b), "swap_f32: a and b must be 16-byte aligned");
    BD_REQUIRE(disjoint(a, b, n), "swap_f32: a and b overlap");
    hipLaunchKernelGGL(swap_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, b, (long long)n);
    BD_CHECK_LAUNCH("bd_swap_f32");
    return BD_OK;
}
