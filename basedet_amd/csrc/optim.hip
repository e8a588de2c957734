// SOLVER.OPTIMIZER_NAME beyond plain SGD (solver/default_solver.py:47-55, 107-115: getattr(megengine.optimizer, name)): Adam, AdamW and
// SGD(nesterov=True) over the flat fp32 parameter arena, each alone and with the TRAINER.EMA update folded in.  HBM-bound passes shaped
// like sgd_ema_kernel (ema.hip): 16-byte accesses per lane, a scalar tail, a grid-stride loop under grid_for's cap (common.h).
//
// Every operation is ONE fp32 rounding: the file is built with -ffp-contract=off (no a * b + c becomes an FMA) and
// -fhip-fp32-correctly-rounded-divide-sqrt (IEEE division and square root), so a numpy float32 restatement of the rules gives the same
// bits (tests/test_optim_gpu.py).  Step-dependent scalars (1 - beta, the bias corrections) arrive as arguments, formed by the host in
// float64 the way one_minus_m travels: there is no step counter on the device.
#include "common.h"

namespace {

struct AdamArgs {
    float lr, beta1, one_minus_beta1, beta2, one_minus_beta2, bc1, bc2, eps, wd, grad_scale, ema_m, one_minus_ema_m;
};

// megengine.optimizer.Adam (DECOUPLED = false: the decay joins the gradient) / AdamW (true: it joins the update)
template <bool DECOUPLED, bool EMA>
__device__ __forceinline__ void adam_elem(float& w, float& m, float& v, float g, float& e, const AdamArgs& a) {
    float gg = g * a.grad_scale;
    if (!DECOUPLED) gg = gg + a.wd * w;
    m = a.beta1 * m + a.one_minus_beta1 * gg;
    v = a.beta2 * v + a.one_minus_beta2 * (gg * gg);
    float d = (m / a.bc1) / (sqrtf(v / a.bc2) + a.eps);
    if (DECOUPLED) d = d + a.wd * w;
    w = w - a.lr * d;
    if (EMA) e = ema_elem(e, w, a.ema_m, a.one_minus_ema_m);
}

template <bool DECOUPLED, bool EMA>
__global__ void adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                            float* __restrict__ e, long long n, AdamArgs a) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += (long long)gridDim.x * blockDim.x) {
        const long long o = i * 4;
        if (o + 4 <= n) {
            f32x4_t wv = *reinterpret_cast<f32x4_t*>(w + o);
            f32x4_t mv = *reinterpret_cast<f32x4_t*>(m + o);
            f32x4_t vv = *reinterpret_cast<f32x4_t*>(v + o);
            const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + o);
            f32x4_t ev = {0.f, 0.f, 0.f, 0.f};
            if (EMA) ev = *reinterpret_cast<f32x4_t*>(e + o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float wk = wv[k], mk = mv[k], vk = vv[k], ek = ev[k];
                adam_elem<DECOUPLED, EMA>(wk, mk, vk, gv[k], ek, a);
                wv[k] = wk; mv[k] = mk; vv[k] = vk; ev[k] = ek;
            }
            *reinterpret_cast<f32x4_t*>(w + o) = wv;
            *reinterpret_cast<f32x4_t*>(m + o) = mv;
            *reinterpret_cast<f32x4_t*>(v + o) = vv;
            if (EMA) *reinterpret_cast<f32x4_t*>(e + o) = ev;
        } else {
            for (long long k = o; k < n; ++k) {
                float wk = w[k], mk = m[k], vk = v[k], ek = EMA ? e[k] : 0.f;
                adam_elem<DECOUPLED, EMA>(wk, mk, vk, g[k], ek, a);
                w[k] = wk; m[k] = mk; v[k] = vk;
                if (EMA) e[k] = ek;
            }
        }
    }
}

// megengine.optimizer.SGD(nesterov=True): the velocity is sgd_kernel's, the weight moves along gg + momentum * v
template <bool EMA>
__device__ __forceinline__ void nesterov_elem(float& w, float& v, float g, float& e, float lr, float momentum, float wd, float grad_scale,
                                              float ema_m, float one_minus_ema_m) {
    const float gg = g * grad_scale + wd * w;
    v = momentum * v + gg;
    w -= lr * (gg + momentum * v);
    if (EMA) e = ema_elem(e, w, ema_m, one_minus_ema_m);
}

template <bool EMA>
__global__ void sgd_nesterov_kernel(float* __restrict__ w, float* __restrict__ v, const float* __restrict__ g, float* __restrict__ e,
                                    long long n, float lr, float momentum, float wd, float grad_scale, float ema_m,
                                    float one_minus_ema_m) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += (long long)gridDim.x * blockDim.x) {
        const long long o = i * 4;
        if (o + 4 <= n) {
            f32x4_t wv = *reinterpret_cast<f32x4_t*>(w + o);
            f32x4_t vv = *reinterpret_cast<f32x4_t*>(v + o);
            const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(g + o);
            f32x4_t ev = {0.f, 0.f, 0.f, 0.f};
            if (EMA) ev = *reinterpret_cast<f32x4_t*>(e + o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float wk = wv[k], vk = vv[k], ek = ev[k];
                nesterov_elem<EMA>(wk, vk, gv[k], ek, lr, momentum, wd, grad_scale, ema_m, one_minus_ema_m);
                wv[k] = wk; vv[k] = vk; ev[k] = ek;
            }
            *reinterpret_cast<f32x4_t*>(w + o) = wv;
            *reinterpret_cast<f32x4_t*>(v + o) = vv;
            if (EMA) *reinterpret_cast<f32x4_t*>(e + o) = ev;
        } else {
            for (long long k = o; k < n; ++k) {
                float wk = w[k], vk = v[k], ek = EMA ? e[k] : 0.f;
                nesterov_elem<EMA>(wk, vk, g[k], ek, lr, momentum, wd, grad_scale, ema_m, one_minus_ema_m);
                w[k] = wk; v[k] = vk;
                if (EMA) e[k] = ek;
            }
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool disjoint(const float* a, const float* b, int64_t n) { return a + n <= b || b + n <= a; }

// the checks both Adam entries share; e == nullptr: the entry without the average
int adam_launch(const char* name, float* w, float* m, float* v, const float* g, float* e, bool ema, int64_t n, int decoupled,
                const AdamArgs& a, bd_stream_t stream) {
    BD_REQUIRE(n >= 0, "%s: negative n", name);
    if (n == 0) return BD_OK;
    BD_REQUIRE(w && m && v && g && (e || !ema), "%s: null pointer", name);
    BD_REQUIRE(aligned16(w) && aligned16(m) && aligned16(v) && aligned16(g) && aligned16(e),
               "%s: every buffer must be 16-byte aligned", name);
    BD_REQUIRE(disjoint(m, v, n) && disjoint(m, w, n) && disjoint(v, w, n), "%s: w, m and v overlap", name);
    if (ema)
        BD_REQUIRE(disjoint(e, w, n) && disjoint(e, m, n) && disjoint(e, v, n) && disjoint(e, g, n), "%s: e overlaps w, m, v or g", name);
    BD_REQUIRE(a.beta1 >= 0.f && a.beta1 < 1.f && a.beta2 >= 0.f && a.beta2 < 1.f, "%s: betas must lie in [0, 1)", name);
    BD_REQUIRE(a.bc1 > 0.f && a.bc2 > 0.f, "%s: bias corrections must be positive", name);
    BD_REQUIRE(a.eps >= 0.f, "%s: negative eps", name);
    const dim3 grid(grid_for((n + 3) / 4)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (ema) {
        if (decoupled) hipLaunchKernelGGL((adam_kernel<true, true>), grid, block, 0, st, w, m, v, g, e, (long long)n, a);
        else hipLaunchKernelGGL((adam_kernel<false, true>), grid, block, 0, st, w, m, v, g, e, (long long)n, a);
    } else {
        if (decoupled) hipLaunchKernelGGL((adam_kernel<true, false>), grid, block, 0, st, w, m, v, g, e, (long long)n, a);
        else hipLaunchKernelGGL((adam_kernel<false, false>), grid, block, 0, st, w, m, v, g, e, (long long)n, a);
    }
    BD_CHECK_LAUNCH(name);
    return BD_OK;
}

int nesterov_launch(const char* name, float* w, float* v, const float* g, float* e, bool ema, int64_t n, float lr, float momentum,
                    float wd, float grad_scale, float ema_m, float one_minus_ema_m, bd_stream_t stream) {
    BD_REQUIRE(n >= 0, "%s: negative n", name);
    if (n == 0) return BD_OK;
    BD_REQUIRE(w && v && g && (e || !ema), "%s: null pointer", name);
    BD_REQUIRE(aligned16(w) && aligned16(v) && aligned16(g) && aligned16(e), "%s: every buffer must be 16-byte aligned", name);
    BD_REQUIRE(disjoint(v, w, n), "%s: w and v overlap", name);
    if (ema) BD_REQUIRE(disjoint(e, w, n) && disjoint(e, v, n) && disjoint(e, g, n), "%s: e overlaps w, v or g", name);
    const dim3 grid(grid_for((n + 3) / 4)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (ema)
        hipLaunchKernelGGL((sgd_nesterov_kernel<true>), grid, block, 0, st, w, v, g, e, (long long)n, lr, momentum, wd, grad_scale, ema_m,
                           one_minus_ema_m);
    else
        hipLaunchKernelGGL((sgd_nesterov_kernel<false>), grid, block, 0, st, w, v, g, e, (long long)n, lr, momentum, wd, grad_scale,
                           ema_m, one_minus_ema_m);
    BD_CHECK_LAUNCH(name);
    return BD_OK;
}

}  // namespace

extern "C" int bd_adam_step(float* w, float* m, float* v, const float* g, int64_t n, float lr, float beta1, float one_minus_beta1,
                            float beta2, float one_minus_beta2, float bc1, float bc2, float eps, float wd, float grad_scale,
                            int decoupled, bd_stream_t stream) {
    const AdamArgs a = {lr, beta1, one_minus_beta1, beta2, one_minus_beta2, bc1, bc2, eps, wd, grad_scale, 0.f, 0.f};
    return adam_launch("bd_adam_step", w, m, v, g, nullptr, false, n, decoupled, a, stream);
}

extern "C" int bd_adam_ema_step(float* w, float* m, float* v, const float* g, float* e, int64_t n, float lr, float beta1,
                                float one_minus_beta1, float beta2, float one_minus_beta2, float bc1, float bc2, float eps, float wd,
                                float grad_scale, int decoupled, float ema_m, float one_minus_ema_m, bd_stream_t stream) {
    const AdamArgs a = {lr, beta1, one_minus_beta1, beta2, one_minus_beta2, bc1, bc2, eps, wd, grad_scale, ema_m, one_minus_ema_m};
    return adam_launch("bd_adam_ema_step", w, m, v, g, e, true, n, decoupled, a, stream);
}

extern "C" int bd_sgd_nesterov_step(float* w, float* v, const float* g, int64_t n, float lr, float momentum, float wd, float grad_scale,
                                    bd_stream_t stream) {
    return nesterov_launch("bd_sgd_nesterov_step", w, v, g, nullptr, false, n, lr, momentum, wd, grad_scale, 0.f, 0.f, stream);
}

extern "C" int bd_sgd_nesterov_ema_step(float* w, float* v, const float* g, float* e, int64_t n, float lr, float momentum, float wd,
                                        float grad_scale, float ema_m, float one_minus_ema_m, bd_stream_t stream) {
    return nesterov_launch("bd_sgd_nesterov_ema_step", w, v, g, e, true, n, lr, momentum, wd, grad_scale, ema_m, one_minus_ema_m, stream);
}
