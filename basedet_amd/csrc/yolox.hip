// YOLOX behind the head's last convolutions (models/det/yolox.py:119-135, 150-408): the SimOTA assignment (get_assignments,
// get_in_boxes_info, dynamic_k_matching), the four losses with their gradients back to the raw head outputs, and the inference decode.
// Inputs in the layout a fused head writes: cls bf16 [N*P][ld] (ld = round_up(K, 8)), box_obj bf16 [N*P][8] (raw reg 0-3, obj logit 4,
// pad 5-7), points fp32 [P][2], gt fp32 [N][Gmax][5] (xyxy + 1-based label).  All arithmetic fp32; every output is a function of the
// inputs alone: float sums run in a fixed order, the only atomics are integer counters.
//
// The gt is xyxy EVERYWHERE (the reference reads the same four numbers as xyxy in get_in_boxes_info / get_l1_target and as
// xc,yc,w,h in tlbr_iou / iou_loss; only the consistent reading is built).
//
//   bd_yolox_assign, three launches for the batch:
//     yx_prep_kernel      per point: the decoded box (relative to its point), sigmoid(obj) pieces, the candidate flag (inside some gt, or
//                         within 2.5 strides of some gt's centre; both tests strict) and, for candidates, S_bg = sum_k BCE(s_k, 0);
//     yx_gt_kernel        one workgroup per (gt, image) over the image's candidates: k = max(1, int(sum of the 10 largest IoUs)), then
//                         the k candidates of smallest cost by radix select (select_dev.h); each taken point gets its counter bumped;
//     yx_resolve_kernel   per point: none -> -1; one -> that gt; several -> the gt of smallest cost over ALL gts of the image; the last
//                         workgroup to finish writes the foreground count.
//   cost(g, p) = (S_bg(p) - bce0(s_c)) + bce1(s_c) + 3 * -log(iou + 1e-8) + 1e5 * [p not inside both g's box and g's centre box],
//   s_k = sqrt(sigmoid(cls_k) sigmoid(obj)).  log s = (log sigmoid(cls) + log sigmoid(obj)) / 2 and 1 - s = (1 - s^2) / (1 + s) with
//   1 - s^2 = qc + qo - qc qo (q = sigmoid(-x)) are formed without cancellation; the argument of log(1 - s) is clamped at 1e-30, so the
//   cost is finite at any logit.  IoUs are evaluated in coordinates relative to the point (IoU is translation invariant; the roundings
//   then scale with the box, not with its position in the image).  Ties: lowest point / gt index.
#pragma clang fp contract(off)
#include <float.h>

#include "select_dev.h"

namespace {

constexpr int YX_TOPQ = 10;              // n_candidate_k (yolox.py:380)
constexpr int YX_GRID_CAP = 4096;        // workgroups of the loss launch (= rows of its partial sums)
constexpr float YX_LOG_FLOOR = 1e-30f;

struct YxLevels { int start[BD_MAX_SEGS + 1]; float stride[BD_MAX_SEGS]; int L; };

__device__ __forceinline__ float yx_stride_of(const YxLevels& lv, int p) {
    int l = 0;
    for (int k = 1; k < lv.L; ++k) if (p >= lv.start[k]) l = k;
    return lv.stride[l];
}

// p = sigmoid(x), q = sigmoid(-x), lp = log p, all from e = exp(-|x|)
__device__ __forceinline__ void yx_sigmoid(float x, float& p, float& q, float& lp) {
    const float e = expf(-fabsf(x));
    const float inv = 1.f / (1.f + e);
    p = x >= 0.f ? inv : e * inv;
    q = x >= 0.f ? e * inv : inv;
    lp = fminf(x, 0.f) - log1pf(e);
}

// BCE(s, 0) = -log(1 - s) of s = sqrt(pc po)
__device__ __forceinline__ float yx_bce0(float pc, float qc, float po, float qo) {
    const float s = sqrtf(pc * po);
    const float u = (qc + qo) - qc * qo;                 // 1 - s^2
    return -logf(fmaxf(u / (1.f + s), YX_LOG_FLOOR));
}

struct YxRaw { float r0, r1, r2, r3, obj; };
__device__ __forceinline__ YxRaw yx_ld_raw(const bf16_raw* box_obj, long long row) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(box_obj + row * 8);
    return YxRaw{bf_lo(v[0]), bf_hi(v[0]), bf_lo(v[1]), bf_hi(v[1]), bf_lo(v[2])};
}

__device__ __forceinline__ int yx_label(float lab) { return (lab > -1e9f && lab < 1e9f ? (int)lab : 0) - 1; }
__device__ __forceinline__ int yx_num_gt(const int* num_gt, int n, int Gmax) {
    const int g = num_gt[n];
    return g < 0 ? 0 : (g > Gmax ? Gmax : g);
}

// get_in_boxes_info (yolox.py:352, 362-365) of one point against one gt
__device__ __forceinline__ void yx_in_tests(float px, float py, float stride, const Box& gb, bool& in_box, bool& in_ctr) {
    in_box = fminf(fminf(px - gb.x1, py - gb.y1), fminf(gb.x2 - px, gb.y2 - py)) > 0.f;
    const float cx = (gb.x1 + gb.x2) / 2.f, cy = (gb.y1 + gb.y2) / 2.f, r = 2.5f * stride;
    const float tlx = cx - r, tly = cy - r, brx = cx + r, bry = cy + r;
    in_ctr = fminf(fminf(px - tlx, py - tly), fminf(brx - px, bry - py)) > 0.f;
}

struct YxIn {
    const float* points; const bf16_raw* cls; const f32x4_t* dec; const f32x4_t* objp; const float* sbg; const int* cand;
    int P, ld, K;
};

// cost and IoU of candidate point p (row = n*P + p) against one gt
__device__ __forceinline__ void yx_pair(const YxIn& in, long long row, int p, const Box& gb, int cls, float& cost, float& iou) {
    const float px = in.points[2ll * p], py = in.points[2ll * p + 1];
    const f32x4_t d = in.dec[row];          // dx, dy, w, h
    const f32x4_t o = in.objp[row];         // sigmoid(obj), sigmoid(-obj), log sigmoid(obj), stride
    bool in_box, in_ctr;
    yx_in_tests(px, py, o[3], gb, in_box, in_ctr);
    // tlbr_iou (yolox.py:279-294): strict tl < br mask, no epsilon
    const float gx1 = gb.x1 - px, gy1 = gb.y1 - py, gx2 = gb.x2 - px, gy2 = gb.y2 - py;
    const float hw = d[2] / 2.f, hh = d[3] / 2.f;
    const float tlx = fmaxf(gx1, d[0] - hw), tly = fmaxf(gy1, d[1] - hh);
    const float brx = fminf(gx2, d[0] + hw), bry = fminf(gy2, d[1] + hh);
    const float area_i = (tlx < brx && tly < bry) ? (brx - tlx) * (bry - tly) : 0.f;
    const float area_g = (gb.x2 - gb.x1) * (gb.y2 - gb.y1), area_p = d[2] * d[3];
    const float v = area_i / ((area_g + area_p) - area_i);
    iou = v > 0.f ? v : 0.f;                // (a NaN from an overflowed box counts as no overlap)
    float cls_cost = in.sbg[row];
    if (cls >= 0 && cls < in.K) {           // a label outside 1..K matches no class column
        float pc, qc, lpc;
        yx_sigmoid(bf2f(in.cls[row * in.ld + cls]), pc, qc, lpc);
        cls_cost = (cls_cost - yx_bce0(pc, qc, o[0], o[1])) + -0.5f * (lpc + o[2]);
    }
    cost = (cls_cost + 3.f * -logf(iou + 1e-8f)) + ((in_box && in_ctr) ? 0.f : 1e5f);
}

__global__ __launch_bounds__(256) void yx_prep_kernel(const float* __restrict__ points, YxLevels lv, const bf16_raw* __restrict__ cls,
                                                      const bf16_raw* __restrict__ box_obj, const float* __restrict__ gt,
                                                      const int* __restrict__ num_gt, int Gmax, int P, int K, int ld,
                                                      f32x4_t* __restrict__ dec, f32x4_t* __restrict__ objp, float* __restrict__ sbg,
                                                      int* __restrict__ cnt, int* __restrict__ gsel, int* __restrict__ cand,
                                                      int* __restrict__ hdr) {
    const int n = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && n == 0 && threadIdx.x == 0) { hdr[0] = 0; hdr[1] = 0; }
    if (p >= P) return;
    const long long row = (long long)n * P + p;
    const float stride = yx_stride_of(lv, p);
    const YxRaw r = yx_ld_raw(box_obj, row);
    dec[row] = (f32x4_t){r.r0 * stride, r.r1 * stride, stride * expf(r.r2), stride * expf(r.r3)};      // yolox.py:163-164, minus the point
    float po, qo, lpo;
    yx_sigmoid(r.obj, po, qo, lpo);
    objp[row] = (f32x4_t){po, qo, lpo, stride};
    const float px = points[2ll * p], py = points[2ll * p + 1];
    const int G = yx_num_gt(num_gt, n, Gmax);
    bool c = false;
    for (int g = 0; g < G && !c; ++g) {
        bool in_box, in_ctr;
        yx_in_tests(px, py, stride, ld_gt(gt + ((long long)n * Gmax + g) * 5), in_box, in_ctr);
        c = in_box || in_ctr;
    }
    float s = 0.f;
    if (c) {
        const bf16_raw* cp = cls + row * ld;
        for (int k0 = 0; k0 < K; k0 += 8) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(cp + k0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (k0 + j < K) {
                    float pc, qc, lpc;
                    yx_sigmoid((j & 1) ? bf_hi(v[j >> 1]) : bf_lo(v[j >> 1]), pc, qc, lpc);
                    s += yx_bce0(pc, qc, po, qo);
                }
            }
        }
    }
    sbg[row] = s; cnt[row] = 0; gsel[row] = -1; cand[row] = c ? 1 : 0;
}

__global__ __launch_bounds__(1024) void yx_gt_kernel(YxIn in, const float* __restrict__ gt, const int* __restrict__ num_gt, int Gmax,
                                                     int* __restrict__ cnt, int* __restrict__ gsel) {
    __shared__ unsigned int hist[256];
    __shared__ int sh[8];
    __shared__ int wcnt[16];
    __shared__ float s_top[16];
    __shared__ int s_n, s_k;
    const int tid = threadIdx.x, g = blockIdx.x, n = blockIdx.y;
    if (g >= yx_num_gt(num_gt, n, Gmax)) return;
    const float* gp = gt + ((long long)n * Gmax + g) * 5;
    const Box gb = ld_gt(gp);
    const int cls = yx_label(gp[4]);
    const int P = in.P;
    const long long row0 = (long long)n * P;

    // ---- dynamic k from the min(10, C) largest IoUs over the image's C candidates (yolox.py:380-382)
    auto key_iou = [&](int i, bool& valid) -> unsigned int {
        valid = in.cand[row0 + i] != 0;
        if (!valid) return 0u;
        float c, u; yx_pair(in, row0 + i, i, gb, cls, c, u); return f32_asc_key(u);
    };
    const SelResult ri = radix_select_largest(P, YX_TOPQ, 4, key_iou, hist, sh);
    if (ri.n_valid == 0) return;                          // no candidate in the image: nothing to take (uniform over the workgroup)
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < P; i += 1024) {
        bool valid; const unsigned int kv = key_iou(i, valid);
        if (valid && (ri.take_all || kv > ri.T)) { const int q = atomicAdd(&s_n, 1); if (q < 16) s_top[q] = f32_from_asc_key(kv); }
    }
    __syncthreads();
    if (tid == 0) {
        int m = s_n < YX_TOPQ ? s_n : YX_TOPQ;
        if (!ri.take_all) for (int j = 0; j < ri.need_eq && m < YX_TOPQ; ++j) s_top[m++] = f32_from_asc_key(ri.T);
        for (int a = 1; a < m; ++a) {                     // insertion sort, descending: the order F.topk returns
            const float v = s_top[a]; int b = a - 1;
            while (b >= 0 && s_top[b] < v) { s_top[b + 1] = s_top[b]; --b; }
            s_top[b + 1] = v;
        }
        float s = 0.f;
        for (int a = 0; a < m; ++a) s += s_top[a];
        const int k = (int)s;                             // 0 <= s <= 10
        s_k = k < 1 ? 1 : k;
    }
    __syncthreads();
    const int dyn_k = s_k;

    // ---- the dyn_k candidates of smallest cost (yolox.py:383-385)
    auto key_cost = [&](int i, bool& valid) -> unsigned int {
        valid = in.cand[row0 + i] != 0;
        if (!valid) return 0u;
        float c, u; yx_pair(in, row0 + i, i, gb, cls, c, u); return ~f32_asc_key(c);
    };
    const SelResult rc = radix_select_largest(P, dyn_k, 4, key_cost, hist, sh);
    int eq_base = 0;
    for (int c0 = 0; c0 < P; c0 += 1024) {
        const int i = c0 + tid;
        bool valid = false; unsigned int kv = 0;
        if (i < P) kv = key_cost(i, valid);
        bool take = valid && (rc.take_all || kv > rc.T);
        if (!rc.take_all) {
            int tot;
            const bool eq = valid && kv == rc.T;
            const int my = eq_base + block_rank_1024(eq, wcnt, tot);
            eq_base += tot;
            take = take || (eq && my < rc.need_eq);
        }
        if (take) { atomicAdd(&cnt[row0 + i], 1); gsel[row0 + i] = g; }
    }
}

__global__ __launch_bounds__(256) void yx_resolve_kernel(YxIn in, const float* __restrict__ gt, const int* __restrict__ num_gt, int Gmax,
                                                         const int* __restrict__ cnt, const int* __restrict__ gsel,
                                                         int* __restrict__ matched, float* __restrict__ iou_t, int* __restrict__ hdr,
                                                         float* __restrict__ stats) {
    __shared__ int s_fg[4];
    const int n = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    bool fg = false;
    if (p < in.P) {
        const long long row = (long long)n * in.P + p;
        const int G = yx_num_gt(num_gt, n, Gmax);
        const int c = cnt[row];
        int m = -1; float u = 0.f;
        if (c > 0) {
            m = gsel[row];
            float cost;
            if (c > 1) {                                  // yolox.py:390-393: argmin of the cost over all gts, first minimum
                float best = INFINITY;
                for (int g = 0; g < G; ++g) {
                    const float* gp = gt + ((long long)n * Gmax + g) * 5;
                    float iou;
                    yx_pair(in, row, p, ld_gt(gp), yx_label(gp[4]), cost, iou);
                    if (cost < best) { best = cost; m = g; }
                }
            }
            if (m >= 0 && m < G) {
                const float* gp = gt + ((long long)n * Gmax + m) * 5;
                yx_pair(in, row, p, ld_gt(gp), yx_label(gp[4]), cost, u);
                fg = true;
            } else { m = -1; }
        }
        matched[row] = m;
        iou_t[row] = u;
    }
    const unsigned long long bal = __ballot(fg);
    if ((threadIdx.x & 63) == 0) s_fg[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int mine = s_fg[0] + s_fg[1] + s_fg[2] + s_fg[3];
        if (mine) atomicAdd(&hdr[0], mine);
        __threadfence();
        const int total = gridDim.x * gridDim.y;
        if (atomicAdd(&hdr[1], 1) == total - 1) {         // the last workgroup: every count is in
            __threadfence();
            stats[0] = (float)atomicAdd(&hdr[0], 0);
        }
    }
}

// ---- losses ------------------------------------------------------------------------------------------------------------------------------
struct YxLossIn {
    const float* points; const bf16_raw* cls; const bf16_raw* box_obj; const float* gt; const int* matched; const float* iou_t;
    const float* stats; bf16_raw* d_cls; bf16_raw* d_box_obj;
    long long rows; int P, K, ld, Gmax, use_l1; float grad_scale;
};

__device__ __forceinline__ float yx_block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// BCEWithLogits(x, t) and its derivative sigmoid(x) - t
__device__ __forceinline__ void yx_bce_logits(float x, float t, float& loss, float& grad) {
    const float e = expf(-fabsf(x));
    const float inv = 1.f / (1.f + e);
    loss = (fmaxf(x, 0.f) - x * t) + log1pf(e);
    grad = (x >= 0.f ? inv : e * inv) - t;
}

__device__ __forceinline__ float yx_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// One thread per 8-slot vector of cls; the thread of a row's first vector also owns the row of box_obj.  Background rows of cls are
// not read: their gradient is +0.  partial[block][4] = the block's sums of (1 - iou^2), obj BCE, cls BCE, |raw - l1 target|.
// Kinks, as torch.autograd takes them in the float64 restatement: min / max at a tie send half the gradient to each side
// (torch.minimum / torch.maximum), clamp(min=0) passes the gradient where its argument is >= 0, |x| has derivative 0 at 0.
__global__ __launch_bounds__(256) void yx_loss_kernel(YxLossIn a, YxLevels lv, float* __restrict__ partial) {
    __shared__ float red[4];
    const float nf = fmaxf(a.stats[0], 1.f);
    const float gs = a.grad_scale / nf;
    const int kv = a.ld / 8;
    const long long nvec = a.rows * kv;
    const long long step = (long long)gridDim.x * 256;
    float acc_iou = 0.f, acc_obj = 0.f, acc_cls = 0.f, acc_l1 = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += step) {
        const long long row = i / kv;
        const int c0 = (int)(i - row * kv) * 8;
        const long long n = row / a.P;
        const int p = (int)(row - n * a.P);
        const int m = a.matched[row];
        const bool fg = m >= 0 && m < a.Gmax;
        const float* gp = a.gt + (n * a.Gmax + (fg ? m : 0)) * 5;
        u32x4_t o = {0u, 0u, 0u, 0u};
        if (fg) {
            const int c = yx_label(gp[4]);
            const float t = a.iou_t[row];
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(a.cls + i * 8);
            float d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = (j & 1) ? bf_hi(v[j >> 1]) : bf_lo(v[j >> 1]);
                float l, g;
                yx_bce_logits(x, c0 + j == c ? t : 0.f, l, g);
                const bool real = c0 + j < a.K;
                acc_cls += real ? l : 0.f;
                d[j] = real ? g * gs : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = pack_bf2(d[2 * j], d[2 * j + 1]);
        }
        *reinterpret_cast<u32x4_t*>(a.d_cls + i * 8) = o;
        if (c0 != 0) continue;
        const YxRaw r = yx_ld_raw(a.box_obj, row);
        float lo, go;
        yx_bce_logits(r.obj, fg ? 1.f : 0.f, lo, go);
        acc_obj += lo;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
        if (fg) {
            const float stride = yx_stride_of(lv, p);
            const float px = a.points[2ll * p], py = a.points[2ll * p + 1];
            const float dx = r.r0 * stride, dy = r.r1 * stride, w = stride * expf(r.r2), h = stride * expf(r.r3);
            const float gx1 = gp[0] - px, gy1 = gp[1] - py, gx2 = gp[2] - px, gy2 = gp[3] - py;
            const float x1 = dx - w / 2.f, y1 = dy - h / 2.f, x2 = dx + w / 2.f, y2 = dy + h / 2.f;
            // box_iou (structures/op_patch.py:36-76)
            const float iw_raw = fminf(x2, gx2) - fmaxf(x1, gx1), ih_raw = fminf(y2, gy2) - fmaxf(y1, gy1);
            const float iw = fmaxf(iw_raw, 0.f), ih = fmaxf(ih_raw, 0.f);
            const float inter = iw * ih;
            const float pw = x2 - x1, ph = y2 - y1;
            const float uni = (pw * ph + (gx2 - gx1) * (gy2 - gy1)) - inter;
            const float q = inter / uni;
            const float iou = fmaxf(q, 0.f);
            acc_iou += 1.f - iou * iou;
            // d(5 (1 - iou^2)) / d iou, then through q = inter / (ap + ag - inter)
            const float dq = q >= 0.f ? -10.f * iou : 0.f;
            const float d_inter = dq * (uni + inter) / (uni * uni), d_ap = dq * -inter / (uni * uni);
            const float d_iw = iw_raw >= 0.f ? d_inter * ih : 0.f, d_ih = ih_raw >= 0.f ? d_inter * iw : 0.f;
            const float sx2 = x2 < gx2 ? 1.f : (x2 == gx2 ? 0.5f : 0.f), sx1 = x1 > gx1 ? 1.f : (x1 == gx1 ? 0.5f : 0.f);
            const float sy2 = y2 < gy2 ? 1.f : (y2 == gy2 ? 0.5f : 0.f), sy1 = y1 > gy1 ? 1.f : (y1 == gy1 ? 0.5f : 0.f);
            const float d_x2 = d_iw * sx2 + d_ap * ph, d_x1 = -(d_iw * sx1) - d_ap * ph;
            const float d_y2 = d_ih * sy2 + d_ap * pw, d_y1 = -(d_ih * sy1) - d_ap * pw;
            // x1 = dx - w/2, x2 = dx + w/2; dx = raw0 stride, w = stride exp(raw2)
            g0 = stride * (d_x1 + d_x2); g1 = stride * (d_y1 + d_y2);
            g2 = w * ((d_x2 - d_x1) / 2.f); g3 = h * ((d_y2 - d_y1) / 2.f);
            if (a.use_l1) {                               // get_l1_target (yolox.py:267-276)
                const float t0 = ((gp[0] + gp[2]) / 2.f - px) / stride, t1 = ((gp[1] + gp[3]) / 2.f - py) / stride;
                const float t2 = logf((gp[2] - gp[0]) / stride + 1e-8f), t3 = logf((gp[3] - gp[1]) / stride + 1e-8f);
                acc_l1 += ((fabsf(r.r0 - t0) + fabsf(r.r1 - t1)) + fabsf(r.r2 - t2)) + fabsf(r.r3 - t3);
                g0 += yx_sign(r.r0 - t0); g1 += yx_sign(r.r1 - t1); g2 += yx_sign(r.r2 - t2); g3 += yx_sign(r.r3 - t3);
            }
            g0 = g0 * gs + 0.f; g1 = g1 * gs + 0.f; g2 = g2 * gs + 0.f; g3 = g3 * gs + 0.f;      // (+ 0.f: never -0)
        }
        *reinterpret_cast<u32x4_t*>(a.d_box_obj + row * 8) = (u32x4_t){pack_bf2(g0, g1), pack_bf2(g2, g3), pack_bf2(go * gs, 0.f), 0u};
    }
    const float s0 = yx_block_sum_256(acc_iou, red), s1 = yx_block_sum_256(acc_obj, red);
    const float s2 = yx_block_sum_256(acc_cls, red), s3 = yx_block_sum_256(acc_l1, red);
    if (threadIdx.x == 0) *reinterpret_cast<f32x4_t*>(partial + 4ll * blockIdx.x) = (f32x4_t){s0, s1, s2, s3};
}

// loss_out[j] = scale_j * (partial[0][j] + ... + partial[n - 1][j], a fixed order) / nf
__global__ __launch_bounds__(256) void yx_loss_finalize_kernel(const float* __restrict__ partial, int n, const float* __restrict__ stats,
                                                               int use_l1, float* __restrict__ loss_out) {
    __shared__ float red[4];
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < n; b += 256) acc += *reinterpret_cast<const f32x4_t*>(partial + 4ll * b);
    const float s0 = yx_block_sum_256(acc[0], red), s1 = yx_block_sum_256(acc[1], red);
    const float s2 = yx_block_sum_256(acc[2], red), s3 = yx_block_sum_256(acc[3], red);
    if (threadIdx.x == 0) {
        const float nf = fmaxf(stats[0], 1.f);
        loss_out[0] = 5.f * s0 / nf; loss_out[1] = s1 / nf; loss_out[2] = s2 / nf; loss_out[3] = use_l1 ? s3 / nf : 0.f;
    }
}

// ---- inference decode --------------------------------------------------------------------------------------------------------------------
struct YxCandLevels { int row_off[BD_MAX_SEGS]; float stride[BD_MAX_SEGS]; int L; };

// bd_det_candidates mode 1 with YOLOX's decode (yolox.py:120-135): topk_* [B][L][k], outputs [B][L*k]
__global__ __launch_bounds__(256) void yx_candidates_kernel(const int* __restrict__ topk_idx, const float* __restrict__ topk_score,
                                                            const int* __restrict__ topk_cnt, YxCandLevels lv, int k, int K, int P,
                                                            const float* __restrict__ points, const bf16_raw* __restrict__ box_obj,
                                                            float* __restrict__ boxes, float* __restrict__ scores,
                                                            int* __restrict__ labels) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= lv.L * k) return;
    const int l = c / k, rnk = c - l * k;
    const long long n = blockIdx.y, C = (long long)lv.L * k;
    topk_idx += n * C; topk_score += n * C; topk_cnt += n * lv.L;
    boxes += n * C * 4; scores += n * C; labels += n * C;
    f32x4_t b = {0.f, 0.f, 0.f, 0.f};
    float sc = -INFINITY;
    int lab = 0;
    if (rnk < topk_cnt[l]) {
        const int idx = topk_idx[c];
        const long long row = (long long)lv.row_off[l] + idx / K;
        if (idx >= 0 && row < P) {
            sc = topk_score[c];
            lab = idx % K;
            const YxRaw r = yx_ld_raw(box_obj, n * P + row);
            const float s = lv.stride[l];
            const float xc = r.r0 * s + points[row * 2], yc = r.r1 * s + points[row * 2 + 1];
            const float w = s * expf(r.r2), h = s * expf(r.r3);
            b = (f32x4_t){xc - w / 2.f, yc - h / 2.f, xc + w / 2.f, yc + h / 2.f};       // BoxConverter "xcycwh2xyxy"
        }
    }
    *reinterpret_cast<f32x4_t*>(boxes + c * 4ll) = b;
    scores[c] = sc;
    labels[c] = lab;
}

bool yx_levels(const int32_t* lvl_start, const int32_t* strides, int L, int P, YxLevels* lv) {
    lv->L = L;
    for (int l = 0; l < L; ++l) {
        if (strides[l] <= 0 || lvl_start[l] < 0 || lvl_start[l + 1] < lvl_start[l]) return false;
        lv->start[l] = lvl_start[l]; lv->stride[l] = (float)strides[l];
    }
    lv->start[L] = lvl_start[L];
    return lvl_start[0] == 0 && lvl_start[L] == P;
}

}  // namespace

extern "C" size_t bd_yolox_assign_workspace_bytes(int N, int P) {
    if (N <= 0 || P <= 0) return 256;
    return 256 + (size_t)N * P * 48;
}

extern "C" int bd_yolox_assign(const float* points, int P, const int32_t* lvl_start, const int32_t* strides, int L, const void* cls, int K,
                               int ld, const void* box_obj, const float* gt_boxes, const int32_t* num_gt, int N, int Gmax,
                               int32_t* matched, float* iou_t, float* stats, void* ws, size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(points && lvl_start && strides && cls && box_obj && gt_boxes && num_gt && matched && iou_t && stats && ws,
               "yolox_assign: null pointer");
    BD_REQUIRE(L >= 1 && L <= BD_MAX_SEGS, "yolox_assign: L=%d out of range (1..%d)", L, BD_MAX_SEGS);
    BD_REQUIRE(P > 0 && N > 0 && N <= 65535 && Gmax > 0 && K > 0 && (long long)N * P < (1ll << 31) && (long long)N * Gmax * 5 < (1ll << 31),
               "yolox_assign: bad sizes");
    BD_REQUIRE(ld % 8 == 0 && ld >= K && ld - K < 8, "yolox_assign: ld=%d must be K=%d rounded up to a multiple of 8", ld, K);
    BD_REQUIRE(ws_bytes >= bd_yolox_assign_workspace_bytes(N, P), "yolox_assign: workspace %zu < %zu bytes", ws_bytes,
               bd_yolox_assign_workspace_bytes(N, P));
    BD_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)cls & 15) == 0 && ((uintptr_t)box_obj & 15) == 0,
               "yolox_assign: cls, box_obj and the workspace must be 16-byte aligned");
    YxLevels lv{};
    BD_REQUIRE(yx_levels(lvl_start, strides, L, P, &lv), "yolox_assign: lvl_start must rise from 0 to P with positive strides");
    const long long rows = (long long)N * P;
    unsigned char* wb = (unsigned char*)ws;
    int* hdr = (int*)wb;
    f32x4_t* dec = (f32x4_t*)(wb + 256);
    f32x4_t* objp = (f32x4_t*)(wb + 256 + rows * 16);
    float* sbg = (float*)(wb + 256 + rows * 32);
    int* cnt = (int*)(wb + 256 + rows * 36);
    int* gsel = (int*)(wb + 256 + rows * 40);
    int* cand = (int*)(wb + 256 + rows * 44);
    const YxIn in{points, (const bf16_raw*)cls, dec, objp, sbg, cand, P, ld, K};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(yx_prep_kernel, dim3(cdiv(P, 256), N), dim3(256), 0, st, points, lv, (const bf16_raw*)cls, (const bf16_raw*)box_obj,
                       gt_boxes, num_gt, Gmax, P, K, ld, dec, objp, sbg, cnt, gsel, cand, hdr);
    hipLaunchKernelGGL(yx_gt_kernel, dim3(Gmax, N), dim3(1024), 0, st, in, gt_boxes, num_gt, Gmax, cnt, gsel);
    hipLaunchKernelGGL(yx_resolve_kernel, dim3(cdiv(P, 256), N), dim3(256), 0, st, in, gt_boxes, num_gt, Gmax, (const int*)cnt,
                       (const int*)gsel, matched, iou_t, hdr, stats);
    BD_CHECK_LAUNCH("bd_yolox_assign");
    return BD_OK;
}

extern "C" size_t bd_yolox_loss_workspace_bytes(void) { return (size_t)YX_GRID_CAP * 4 * sizeof(float); }

extern "C" int bd_yolox_loss_fwd_bwd(const float* points, int P, const int32_t* lvl_start, const int32_t* strides, int L, const void* cls,
                                     int K, int ld, const void* box_obj, const float* gt_boxes, int N, int Gmax, const int32_t* matched,
                                     const float* iou_t, const float* stats, int use_l1, float grad_scale, float* loss_out, void* d_cls,
                                     void* d_box_obj, void* ws, size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(points && lvl_start && strides && cls && box_obj && gt_boxes && matched && iou_t && stats && loss_out && d_cls && d_box_obj && ws,
               "yolox_loss: null pointer");
    BD_REQUIRE(L >= 1 && L <= BD_MAX_SEGS, "yolox_loss: L=%d out of range (1..%d)", L, BD_MAX_SEGS);
    BD_REQUIRE(P > 0 && N > 0 && Gmax > 0 && K > 0 && (long long)N * P < (1ll << 31) && (long long)N * Gmax * 5 < (1ll << 31),
               "yolox_loss: bad sizes");
    BD_REQUIRE(ld % 8 == 0 && ld >= K && ld - K < 8, "yolox_loss: ld=%d must be K=%d rounded up to a multiple of 8", ld, K);
    BD_REQUIRE(ws_bytes >= bd_yolox_loss_workspace_bytes(), "yolox_loss: workspace %zu < %zu bytes", ws_bytes, bd_yolox_loss_workspace_bytes());
    BD_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)cls & 15) == 0 && ((uintptr_t)box_obj & 15) == 0 && ((uintptr_t)d_cls & 15) == 0 &&
               ((uintptr_t)d_box_obj & 15) == 0, "yolox_loss: cls, box_obj, their gradients and the workspace must be 16-byte aligned");
    YxLevels lv{};
    BD_REQUIRE(yx_levels(lvl_start, strides, L, P, &lv), "yolox_loss: lvl_start must rise from 0 to P with positive strides");
    const long long rows = (long long)N * P;
    const YxLossIn a{points, (const bf16_raw*)cls, (const bf16_raw*)box_obj, gt_boxes, matched, iou_t, stats, (bf16_raw*)d_cls,
                     (bf16_raw*)d_box_obj, rows, P, K, ld, Gmax, use_l1 ? 1 : 0, grad_scale};
    const int grid = grid_for(rows * (ld / 8), 256, YX_GRID_CAP);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(yx_loss_kernel, dim3(grid), dim3(256), 0, st, a, lv, (float*)ws);
    hipLaunchKernelGGL(yx_loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, grid, stats, use_l1 ? 1 : 0, loss_out);
    BD_CHECK_LAUNCH("bd_yolox_loss_fwd_bwd");
    return BD_OK;
}

extern "C" int bd_yolox_candidates(const int32_t* topk_idx, const float* topk_score, const int32_t* topk_cnt, int B, int L, int k,
                                   const int32_t* lvl_start, const int32_t* strides, int K, const float* points, int P, const void* box_obj,
                                   float* boxes, float* scores, int32_t* labels, bd_stream_t stream) {
    BD_REQUIRE(topk_idx && topk_score && topk_cnt && lvl_start && strides && points && box_obj && boxes && scores && labels,
               "yolox_candidates: null pointer");
    BD_REQUIRE(L >= 1 && L <= BD_MAX_SEGS, "yolox_candidates: L=%d out of range (1..%d)", L, BD_MAX_SEGS);
    BD_REQUIRE(B > 0 && B <= 65535 && k > 0 && K > 0 && P > 0 && (long long)B * P < (1ll << 31), "yolox_candidates: bad sizes");
    BD_REQUIRE(((uintptr_t)box_obj & 15) == 0 && ((uintptr_t)boxes & 15) == 0, "yolox_candidates: box_obj and boxes must be 16-byte aligned");
    YxLevels lv{};
    BD_REQUIRE(yx_levels(lvl_start, strides, L, P, &lv), "yolox_candidates: lvl_start must rise from 0 to P with positive strides");
    YxCandLevels cl{};
    cl.L = L;
    for (int l = 0; l < L; ++l) { cl.row_off[l] = lv.start[l]; cl.stride[l] = lv.stride[l]; }
    hipLaunchKernelGGL(yx_candidates_kernel, dim3(cdiv(L * k, 256), B), dim3(256), 0, (hipStream_t)stream, topk_idx, topk_score, topk_cnt, cl,
                       k, K, P, points, (const bf16_raw*)box_obj, boxes, scores, labels);
    BD_CHECK_LAUNCH("bd_yolox_candidates");
    return BD_OK;
}
