// CenterNet after the network's last convolution (models/det/centernet.py): ground-truth maps (get_ground_truth:74-127 + CenterNetGT:378-452),
// the heat-map focal loss (modified_focal_loss:218-242), the gathered L1 losses (reg_l1_loss + gather_feature:189-215) and the decoder
// (CenterNetDecoder.decode / pseudo_nms / topk_score:245-352).  Predictions are pixel-major bf16 [N*H*W][ld]; side data is fp32 / int32.
// Every output is a function of the inputs alone: the only atomics are integer ones (a max on the bits of non-negative floats, LDS
// histogram and slot counters whose results are sorted afterwards), every float sum runs in a fixed order.
//
// Compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt: the Gaussian radius below is the float32 evaluation of the
// reference's expressions, one rounding per operation -- a radius one ulp off at an integer changes a whole disc of the map.
//
// gaussian2D's cut `gauss < eps * gauss.max()` (centernet.py:431) is not coded: with sigma = (2r + 1) / 6 the smallest value of a
// window, its corner, is exp(-36 r^2 / (2r + 1)^2) > exp(-9) = 1.2e-4, far above eps = 2.2e-16; the cut never fires.
#pragma clang fp contract(off)
#include <utility>
#include <vector>

#include "select_dev.h"

namespace {

constexpr int CN_T_MAX = 1024;          // slots per image (HEAD.TENSOR_DIM; the reference's config uses 128)
constexpr int CN_K_MAX = 2048;          // decode: detections per image
constexpr int CN_SPLIT = 8;             // workgroups per image of the target and L1 launches
constexpr int CN_GRID_CAP = 4096;       // = bd_loss_grid_cap()

// ---- targets -------------------------------------------------------------------------------------------------------------------------
struct CnRadiusConst { float omm, opm, m2mo, mom1, fa3; };       // fp32(1 - mo), fp32(1 + mo), fp32(-2 mo), fp32(mo - 1), fp32(4 * (4 mo))

// CenterNetGT.get_gaussian_radius (centernet.py:394-423, the "bug version"), clipped at 0 and truncated (generate_score_map:383-384)
__device__ __forceinline__ int cn_radius(float w, float h, const CnRadiusConst& c) {
    const float hw = h + w;
    const float b1 = hw;
    const float c1 = w * h * c.omm / c.opm;
    const float sq1 = sqrtf(b1 * b1 - 4.f * c1);
    const float r1 = (b1 + sq1) / 2.f;
    const float b2 = 2.f * hw;
    const float c2 = c.omm * w * h;
    const float sq2 = sqrtf(b2 * b2 - 16.f * c2);
    const float r2 = (b2 + sq2) / 2.f;
    const float b3 = c.m2mo * hw;
    const float c3 = c.mom1 * w * h;
    const float sq3 = sqrtf(b3 * b3 - c.fa3 * c3);
    const float r3 = (b3 + sq3) / 2.f;
    float r = fminf(fminf(r1, r2), r3);
    r = fmaxf(r, 0.f);
    return r < 1e9f ? (int)r : 1000000000;      // (a NaN radius draws the centre only: fmaxf drops it)
}

// Workgroup s of CN_SPLIT of image n: compacts the image's boxes into LDS slots (every workgroup of the image does, it is cheap), draws
// the slots s, s + CN_SPLIT, ...; workgroup 0 also writes wh / reg / reg_mask / index and the image's count of distinct drawn
// (class, cell) pairs.  score_map was zeroed before the launch; a drawn value is a positive float, so the integer max of the bit
// patterns is the float max, whatever the order.
__global__ __launch_bounds__(256) void cn_targets_kernel(const float* __restrict__ gt_boxes, const int* __restrict__ num_gt, int G, int K,
                                                         int H, int W, int T, float box_scale, CnRadiusConst rc,
                                                         float* __restrict__ score_map, float* __restrict__ wh, float* __restrict__ reg,
                                                         float* __restrict__ reg_mask, int* __restrict__ index,
                                                         int* __restrict__ counts) {
    __shared__ int s_src[CN_T_MAX];                     // gt row of slot t
    __shared__ int s_cls[CN_T_MAX], s_cx[CN_T_MAX], s_cy[CN_T_MAX], s_r[CN_T_MAX];     // s_cls < 0: the slot draws nothing
    __shared__ int s_wcnt[4], s_red[4];
    const int n = blockIdx.y, split = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* gb = gt_boxes + (long long)n * G * 5;
    int ng = num_gt[n];
    ng = ng < 0 ? 0 : (ng > G ? G : ng);
    // ordered compaction of the boxes with w > 0 and h > 0 (Boxes.filter_by_size, before the scaling): the first T survivors
    int cnt = 0;
    for (int g0 = 0; g0 < ng && cnt < T; g0 += 256) {
        const int g = g0 + tid;
        bool keep = false;
        if (g < ng) keep = (gb[g * 5 + 2] - gb[g * 5 + 0] > 0.f) && (gb[g * 5 + 3] - gb[g * 5 + 1] > 0.f);
        const unsigned long long bal = __ballot(keep);
        __syncthreads();
        if (lane == 0) s_wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
        for (int q = 0; q < 4; ++q) { if (q < wave) before += s_wcnt[q]; tot += s_wcnt[q]; }
        const int slot = cnt + before + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && slot < T) s_src[slot] = g;
        cnt += tot;
    }
    cnt = cnt < T ? cnt : T;
    __syncthreads();
    const long long HW = (long long)H * W;
    for (int t = tid; t < T; t += 256) {
        float ow = 0.f, oh = 0.f, ox = 0.f, oy = 0.f, om = 0.f;
        int oi = 0, cls = -1, cx = 0, cy = 0, r = 0;
        if (t < cnt) {
            const float* b = gb + s_src[t] * 5;
            const float x1 = b[0] * box_scale, y1 = b[1] * box_scale, x2 = b[2] * box_scale, y2 = b[3] * box_scale;
            const float fx = (x1 + x2) / 2.f, fy = (y1 + y2) / 2.f;
            ow = x2 - x1; oh = y2 - y1;
            // centers.astype("int32") truncates; a centre whose cell lies outside the map (the reference would index out of range): no
            // regression target and nothing drawn
            const bool inside = fx > -1.f && fx < (float)W && fy > -1.f && fy < (float)H;
            if (inside) {
                cx = (int)fx; cy = (int)fy;
                ox = fx - (float)cx; oy = fy - (float)cy;
                om = 1.f;
                oi = cy * W + cx;
                const float lab = b[4];
                const int c = (lab > -1e9f && lab < 1e9f ? (int)lab : 0) - 1;
                cls = c >= 0 && c < K ? c : -1;         // class < 0: the slot stays, nothing is drawn (generate_score_map:387)
                r = cn_radius(ow, oh, rc);
            }
        }
        s_cls[t] = cls; s_cx[t] = cx; s_cy[t] = cy; s_r[t] = r;
        if (split == 0) {
            const long long o = (long long)n * T + t;
            wh[o * 2] = ow; wh[o * 2 + 1] = oh;
            reg[o * 2] = ox; reg[o * 2 + 1] = oy;
            reg_mask[o] = om;
            index[o] = oi;
        }
    }
    __syncthreads();
    if (split == 0) {       // distinct drawn (class, cell) pairs: a slot counts unless an earlier slot drew the same pair
        int c = 0;
        for (int t = tid; t < cnt; t += 256) {
            if (s_cls[t] < 0) continue;
            bool first = true;
            for (int u = 0; u < t; ++u)
                if (s_cls[u] == s_cls[t] && s_cx[u] == s_cx[t] && s_cy[u] == s_cy[t]) { first = false; break; }
            c += first ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_red[wave] = c;
        __syncthreads();
        if (tid == 0) counts[n] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    }
    // draw_gaussian (centernet.py:435-452): one wave per slot, the clipped window spread over its lanes
    int* map = reinterpret_cast<int*>(score_map) + (long long)n * HW * K;
    for (int t = split * 4 + wave; t < cnt; t += CN_SPLIT * 4) {
        const int cls = s_cls[t];
        if (cls < 0) continue;
        const int cx = s_cx[t], cy = s_cy[t], r = s_r[t];
        const int left = cx < r ? cx : r, right = W - cx < r + 1 ? W - cx : r + 1;
        const int top = cy < r ? cy : r, bottom = H - cy < r + 1 ? H - cy : r + 1;
        const int ww = left + right, wn = ww * (top + bottom);       // <= W * H
        const float sigma = (float)(2 * r + 1) / 6.f;
        const float den = 2.f * sigma * sigma;
        for (int q = lane; q < wn; q += 64) {
            const int qy = q / ww, qx = q - qy * ww;
            const int dx = qx - left, dy = qy - top;
            const float v = expf(-(float)(dx * dx + dy * dy) / den);      // the centre: expf(-0) = 1 exactly
            atomicMax(map + ((long long)(cy + dy) * W + (cx + dx)) * K + cls, __float_as_int(v));
        }
    }
}

__global__ void cn_count_sum_kernel(const int* __restrict__ counts, int N, float* __restrict__ num_pos) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int s = 0;
        for (int n = 0; n < N; ++n) s += counts[n];
        num_pos[0] = (float)s;
    }
}

// ---- shared by the two losses ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cn_block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// loss[0] += (partial[0] + ... + partial[n - 1], summed in a fixed order) * partial[n]
__global__ __launch_bounds__(256) void cn_finalize_kernel(const float* __restrict__ partial, int n, float* __restrict__ loss) {
    __shared__ float red[4];
    float a = 0.f;
    for (int b = threadIdx.x; b < n; b += 256) a += partial[b];
    const float s = cn_block_sum_256(a, red);
    if (threadIdx.x == 0) loss[0] += s * partial[n];
}

// ---- heat-map focal loss -----------------------------------------------------------------------------------------------------------------
// One logit x against its target gt of the score map.  p = sigmoid(x) and q = 1 - p = sigmoid(-x) are both formed from e = exp(-|x|), so
// neither suffers the cancellation of 1.f - p, and F.clip(pred, 1e-12, 1 - 1e-7) (centernet.py:230) is decided on the accurate side:
// p > fp32(1 - 1e-7) = 1 - 2^-23  <=>  q < 2^-23.  Where the clip is active the gradient is zero, as F.clip's is.
//   gt == 1: l = log(p) q^2,             dl/dx = q^2 (q - 2 p log p)
//   gt <  1: l = log(q) p^2 (1 - gt)^4,  dl/dx = (1 - gt)^4 p^2 (2 q log q - p)
// Hardware exp / log / rcp (1 ulp) as in losses.hip: the gradient is rounded to bf16 and the loss is a sum of 2e7 terms of one sign.
__device__ __forceinline__ void cn_focal_elem(float x, float gt, float& loss, float& grad) {
    const float e = __builtin_amdgcn_exp2f(-fabsf(x) * 1.4426950408889634f);
    const float t1 = 1.f + e;
    const float inv = __builtin_amdgcn_rcpf(t1);
    float p = x >= 0.f ? inv : e * inv;
    float q = x >= 0.f ? e * inv : inv;
    const float l1p = e < 0x1p-10f ? e * (1.f - e * (0.5f - e * 0.33333334f)) : __builtin_amdgcn_logf(t1) * 0.6931471805599453f;
    float lp = fminf(x, 0.f) - l1p;       // log p
    float lq = fminf(-x, 0.f) - l1p;      // log q
    bool open = true;
    if (p < 1e-12f) { p = 1e-12f; q = 1.f; lp = -27.631021f; lq = -1e-12f; open = false; }
    else if (q < 0x1p-23f) { p = 0.99999988f; q = 0x1p-23f; lp = -1.1920930e-07f; lq = -15.942385f; open = false; }
    if (gt == 1.f) {
        const float q2 = q * q;
        loss = lp * q2;
        grad = open ? q2 * (q - 2.f * p * lp) : 0.f;
    } else {
        const float w1 = 1.f - gt, w2 = w1 * w1, w = w2 * w2, p2 = p * p;
        loss = lq * p2 * w;
        grad = open ? w * p2 * (2.f * q * lq - p) : 0.f;
    }
}

// logits / dlogits bf16 [rows][ld], one 8-slot vector per thread and pass; gt fp32 [rows][K].  VEC: K % 4 == 0, the targets of a vector
// are two aligned 16-byte loads.  partial[block] = the sum of l over the block's elements; partial[gridDim.x] = -weight / num_pos.
template <bool VEC>
__global__ __launch_bounds__(256) void cn_focal_kernel(const bf16_raw* __restrict__ logits, const float* __restrict__ gt, long long rows,
                                                       int K, int ld, const float* __restrict__ norm, float weight, float grad_scale,
                                                       float* __restrict__ partial, bf16_raw* __restrict__ dlogits) {
    __shared__ float red[4];
    const float np = norm[0];
    const float inv_np = np == 0.f ? 1.f : 1.f / np;        // loss = -neg when num_pos == 0 (centernet.py:237-240)
    const float gs = -(weight * grad_scale * inv_np);
    const int kv = ld / 8;
    const long long nvec = rows * kv;
    const long long stride = (long long)gridDim.x * 256;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        const long long row = i / kv;
        const int c0 = (int)(i - row * kv) * 8;
        const int nreal = K - c0 < 8 ? K - c0 : 8;
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(logits + i * 8);
        const float* gp = gt + row * K + c0;
        float g[8];
        if (VEC) {
            const f32x4_t g0 = *reinterpret_cast<const f32x4_t*>(gp);
            const f32x4_t g1 = nreal > 4 ? *reinterpret_cast<const f32x4_t*>(gp + 4) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) { g[j] = g0[j]; g[4 + j] = g1[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = j < nreal ? gp[j] : 0.f;
        }
        float d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = (j & 1) ? bf_hi(v[j >> 1]) : bf_lo(v[j >> 1]);
            float l, gr;
            cn_focal_elem(x, g[j], l, gr);
            const bool real = j < nreal;            // pad slots: no loss, gradient +0
            acc += real ? l : 0.f;
            d[j] = real ? gr * gs + 0.f : 0.f;      // (+ 0.f: a zero gradient times the negative scale is -0; the sum is +0)
        }
        u32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf2(d[2 * j], d[2 * j + 1]);
        *reinterpret_cast<u32x4_t*>(dlogits + i * 8) = o;
    }
    const float s = cn_block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s;
        if (blockIdx.x == 0) partial[gridDim.x] = -(weight * inv_np);
    }
}

// ---- gathered L1 loss --------------------------------------------------------------------------------------------------------------------
// Workgroup s of CN_SPLIT of image n owns the pixels [p0, p1) of the image: it writes their dpred rows as zeros, then adds the gradient of
// every slot whose pixel lies in its range -- the slots of one pixel in slot order, by the thread of the first of them.  Workgroup 0 of
// the image also leaves the image's sum of |pred m - tgt m| in partial[n].  Every workgroup forms the batch's denominator itself
// (N * T masks, the same fixed order everywhere): sum(mask broadcast to (N, T, 2)) + 1e-4 = 2 sum(mask) + 1e-4 (centernet.py:210-214).
// A slot whose index lies outside [0, H*W) reads and writes nothing.
__global__ __launch_bounds__(256) void cn_l1_kernel(const bf16_raw* __restrict__ pred, int ld, int off, const int* __restrict__ index,
                                                    const float* __restrict__ mask, const float* __restrict__ target, int N, int HW, int T,
                                                    float weight, float grad_scale, float* __restrict__ partial,
                                                    bf16_raw* __restrict__ dpred) {
    __shared__ int s_idx[CN_T_MAX];
    __shared__ float s_gx[CN_T_MAX], s_gy[CN_T_MAX];
    __shared__ float red[4];
    const int n = blockIdx.y, split = blockIdx.x, tid = threadIdx.x;
    float ms = 0.f;
    for (int i = tid; i < N * T; i += 256) ms += mask[i];
    const float msum = cn_block_sum_256(ms, red);
    const float denom = (msum + msum) + 1e-4f;
    const float gs = weight * grad_scale / denom;
    const int per = (HW + CN_SPLIT - 1) / CN_SPLIT;
    const int p0 = split * per < HW ? split * per : HW, p1 = p0 + per < HW ? p0 + per : HW;
    // zero rows of this range: 16-byte stores (ld % 8 == 0)
    {
        u32x4_t* z = reinterpret_cast<u32x4_t*>(dpred + ((long long)n * HW + p0) * ld);
        const long long nv = (long long)(p1 - p0) * (ld / 8);
        for (long long i = tid; i < nv; i += 256) z[i] = (u32x4_t){0u, 0u, 0u, 0u};
    }
    float lsum = 0.f;
    for (int t = tid; t < T; t += 256) {
        const long long o = (long long)n * T + t;
        const int idx = index[o];
        const float m = mask[o];
        float gx = 0.f, gy = 0.f;
        int keep = -1;
        if (idx >= 0 && idx < HW && m != 0.f) {
            const bf16_raw* pp = pred + ((long long)n * HW + idx) * ld + off;
            const float px = bf2f(pp[0]), py = bf2f(pp[1]);
            const float tx = target[o * 2], ty = target[o * 2 + 1];
            lsum += fabsf(px * m - tx * m) + fabsf(py * m - ty * m);
            const float dx = px - tx, dy = py - ty;
            gx = (dx > 0.f ? 1.f : (dx < 0.f ? -1.f : 0.f)) * m * gs;        // sign(0) = 0
            gy = (dy > 0.f ? 1.f : (dy < 0.f ? -1.f : 0.f)) * m * gs;
            keep = idx;
        }
        s_idx[t] = keep; s_gx[t] = gx; s_gy[t] = gy;
    }
    const float ls = cn_block_sum_256(lsum, red);       // (its barriers also publish the slots)
    if (split == 0 && tid == 0) {
        partial[n] = ls;
        if (n == 0) partial[N] = weight / denom;
    }
    for (int t = tid; t < T; t += 256) {
        const int idx = s_idx[t];
        if (idx < p0 || idx >= p1) continue;
        bool first = true;
        for (int u = 0; u < t; ++u)
            if (s_idx[u] == idx) { first = false; break; }
        if (!first) continue;
        float ax = 0.f, ay = 0.f;
        for (int u = t; u < T; ++u)
            if (s_idx[u] == idx) { ax += s_gx[u]; ay += s_gy[u]; }
        *reinterpret_cast<unsigned int*>(dpred + ((long long)n * HW + idx) * ld + off) = pack_bf2(ax, ay);
    }
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }      // as det_scores_kernel (postprocess.hip)

// pseudo_nms (centernet.py:314-325) on the fp32 scores: a 16 x 16 pixel tile of 8 classes per workgroup, the scores of the tile and its
// one-pixel halo in LDS (out-of-map neighbours hold -1: they do not compete).  peaks [B][K][H*W]: the score where it equals the maximum
// of its 3 x 3 window, else 0 (fmap * keep).
__global__ __launch_bounds__(256) void cn_peak_kernel(const bf16_raw* __restrict__ logits, int ld, int K, int H, int W,
                                                      float* __restrict__ peaks) {
    __shared__ float s[18 * 18][9];
    const int tiles_x = (W + 15) / 16;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int cg = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const long long HW = (long long)H * W;
    const bf16_raw* lg = logits + (long long)b * HW * ld + cg * 8;
    for (int q = tid; q < 18 * 18; q += 256) {
        const int qy = q / 18, qx = q - qy * 18;
        const int y = ty * 16 - 1 + qy, x = tx * 16 - 1 + qx;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(lg + ((long long)y * W + x) * ld);
#pragma unroll
            for (int j = 0; j < 4; ++j) { s[q][2 * j] = cn_sigmoid(bf_lo(v[j])); s[q][2 * j + 1] = cn_sigmoid(bf_hi(v[j])); }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) s[q][j] = -1.f;
        }
    }
    __syncthreads();
    const int py = tid >> 4, px = tid & 15;
    const int y = ty * 16 + py, x = tx * 16 + px;
    if (y >= H || x >= W) return;
    const int c = (py + 1) * 18 + px + 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (cg * 8 + j >= K) break;
        const float v = s[c][j];
        float m = v;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) m = fmaxf(m, s[c + dy * 18 + dx][j]);
        peaks[((long long)b * K + cg * 8 + j) * HW + (long long)y * W + x] = v == m ? v : 0.f;
    }
}

// exclusive prefix of v over the 1024 threads in thread order, and the total.  wsum: 16 ints of LDS.
__device__ __forceinline__ int cn_excl_scan_1024(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int c = wsum[w];
        if (w < wave) before += c;
        tot += c;
    }
    total = tot;
    return before + inc - v;
}

// topk_score + the gathers of decode (centernet.py:258-291, 328-352), one workgroup per image: radix select of the k largest peak scores
// over item i = class * H*W + pixel (zeros do not enter the histogram: they are the bulk of the map, and they fill the list in index
// order when fewer than k peaks are positive), ties at the k-th score taken in index order, then an LDS sort of (score, ~index):
// score descending, class ascending, pixel ascending.
__global__ __launch_bounds__(1024) void cn_topk_kernel(const float* __restrict__ peaks, int K, int H, int W, int k,
                                                       const bf16_raw* __restrict__ wh, int wh_ld, int wh_off,
                                                       const bf16_raw* __restrict__ reg, int reg_ld, int reg_off,
                                                       float* __restrict__ boxes, float* __restrict__ scores, int* __restrict__ classes) {
    __shared__ unsigned long long keys[CN_K_MAX];
    __shared__ unsigned int hist[256];
    __shared__ int sh[8], wsum[16], s_slots;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int HW = H * W, n = K * HW;
    const float* pk = peaks + (long long)b * n;
    if (tid == 0) s_slots = 0;
    const SelResult r = radix_select_largest(n, k, 4, [&](int i, bool& valid) {
        const float v = pk[i];
        valid = v > 0.f;
        return __float_as_uint(v);
    }, hist, sh);
    const int need_eq = r.take_all ? k - r.n_valid : r.need_eq;
    // every thread owns a contiguous run of items: the items above the threshold go to slots in any order, the ties are counted, ranked
    // by one scan over the threads and taken in index order
    const int per = (n + 1023) / 1024;
    const int i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    int neq = 0;
    for (int i = i0; i < i1; ++i) {
        const float v = pk[i];
        const unsigned int u = __float_as_uint(v);
        const bool pos = v > 0.f;
        const bool gt = r.take_all ? pos : (pos && u > r.T);
        const bool eq = r.take_all ? !pos : (pos && u == r.T);
        if (gt) {
            const int slot = atomicAdd(&s_slots, 1);
            if (slot < CN_K_MAX) keys[slot] = ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (unsigned int)i);
        }
        neq += eq ? 1 : 0;
    }
    int total;
    int rank = cn_excl_scan_1024(neq, wsum, total);      // (its barriers order the slot counter)
    const int base = k - need_eq;                        // = the number of items above the threshold
    if (rank < need_eq && neq > 0) {
        for (int i = i0; i < i1 && rank < need_eq; ++i) {
            const float v = pk[i];
            const bool pos = v > 0.f;
            const bool eq = r.take_all ? !pos : (pos && __float_as_uint(v) == r.T);
            if (eq) {
                const unsigned int u = pos ? __float_as_uint(v) : 0u;
                keys[base + rank] = ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (unsigned int)i);
                ++rank;
            }
        }
    }
    int P = 2;
    while (P < k) P <<= 1;
    for (int i = k + tid; i < P; i += 1024) keys[i] = 0ull;     // (a selected key ends in ~index >= 2^31: never 0)
    __syncthreads();
    bitonic_sort_1024<true>(keys, P);
    for (int j = tid; j < k; j += 1024) {
        const unsigned long long ck = keys[j];
        const int i = (int)(0xffffffffu - (unsigned int)(ck & 0xffffffffull));
        const int c = i / HW, p = i - c * HW;
        const int y = p / W, x = p - y * W;
        const long long row = (long long)b * HW + p;
        const float w = bf2f(wh[row * wh_ld + wh_off]), h = bf2f(wh[row * wh_ld + wh_off + 1]);
        const float rx = reg ? bf2f(reg[row * reg_ld + reg_off]) : 0.5f, ry = reg ? bf2f(reg[row * reg_ld + reg_off + 1]) : 0.5f;
        const float xs = (float)x + rx, ys = (float)y + ry;
        const float hw_ = w / 2.f, hh = h / 2.f;
        const long long o = (long long)b * k + j;
        *reinterpret_cast<f32x4_t*>(boxes + o * 4) = (f32x4_t){xs - hw_, ys - hh, xs + hw_, ys + hh};
        scores[o] = __uint_as_float((unsigned int)(ck >> 32));
        classes[o] = c;
    }
}

// ---- boxes to image coordinates ----------------------------------------------------------------------------------------------------------
// CenterNet.post_process's transform_boxes (centernet.py:163-186, 293-311) for a whole batch: one thread per box, one 16-byte load and
// store.  affine [B][6] = the image's 2 x 3 map (a b c / d e f) from output-map to image coordinates, solved on the host in float64 and
// rounded once.  The order is fixed: x' = fma(a, x, fma(b, y, c)), y' = fma(d, x, fma(e, y, f)) -- two roundings in the chain (a third is the rounding of the
// coefficients), written as explicit fmaf calls (the file is compiled with contraction off, so nothing else fuses).  scores and classes pass through into the
// caller's dense per-image tensors in the same launch.
__global__ __launch_bounds__(256) void cn_boxes_to_image_kernel(const float* __restrict__ boxes, const float* __restrict__ affine,
                                                                const float* __restrict__ scores, const int* __restrict__ classes, int k,
                                                                long long total, float* __restrict__ boxes_out,
                                                                float* __restrict__ scores_out, int* __restrict__ labels_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float* m = affine + (i / k) * 6;
    const float a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5];
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(boxes + i * 4);
    f32x4_t o;
    o[0] = fmaf(a, v[0], fmaf(b, v[1], c));
    o[1] = fmaf(d, v[0], fmaf(e, v[1], f));
    o[2] = fmaf(a, v[2], fmaf(b, v[3], c));
    o[3] = fmaf(d, v[2], fmaf(e, v[3], f));
    *reinterpret_cast<f32x4_t*>(boxes_out + i * 4) = o;
    scores_out[i] = scores[i];
    labels_out[i] = classes[i];
}

}  // namespace

// Scratch of the loss partials: one grow-only buffer per (device, stream), as losses.hip keeps for its launches.
static float* cn_partials(hipStream_t stream, size_t floats) {
    struct Buf { float* p = nullptr; size_t n = 0; };
    static std::mutex mu;
    static std::vector<std::pair<std::pair<int, hipStream_t>, Buf>> bufs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    Buf* b = nullptr;
    for (auto& e : bufs)
        if (e.first.first == dev && e.first.second == stream) b = &e.second;
    if (!b) {
        bufs.push_back({{dev, stream}, Buf{}});
        b = &bufs.back().second;
    }
    if (b->n < floats) {
        if (b->p) (void)hipFree(b->p);
        b->p = nullptr; b->n = 0;
        const size_t n = floats < 8192 ? 8192 : floats;
        if (hipMalloc((void**)&b->p, n * sizeof(float)) != hipSuccess) return nullptr;
        b->n = n;
    }
    return b->p;
}

extern "C" size_t bd_centernet_targets_workspace_bytes(int N) {
    return ((size_t)(N > 0 ? N : 1) * sizeof(int) + 255) / 256 * 256;
}

extern "C" int bd_centernet_targets(const float* gt_boxes, const int32_t* num_gt, int N, int Gmax, int K, int H, int W, int T,
                                    float box_scale, double min_overlap, float* score_map, float* wh, float* reg, float* reg_mask,
                                    int32_t* index, float* num_pos, void* ws, size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(gt_boxes && num_gt && score_map && wh && reg && reg_mask && index && num_pos && ws, "centernet_targets: null pointer");
    BD_REQUIRE(N > 0 && N <= 65535 && Gmax > 0 && K > 0 && H > 0 && W > 0, "centernet_targets: bad sizes");
    BD_REQUIRE(T > 0 && T <= CN_T_MAX, "centernet_targets: T=%d out of range (1..%d)", T, CN_T_MAX);
    BD_REQUIRE((long long)H * W < (1ll << 31) && (long long)Gmax * 5 < (1ll << 31), "centernet_targets: map or box list too large");
    BD_REQUIRE(box_scale > 0.f && min_overlap > 0.0 && min_overlap < 1.0, "centernet_targets: box_scale > 0 and 0 < min_overlap < 1");
    BD_REQUIRE(ws_bytes >= bd_centernet_targets_workspace_bytes(N), "centernet_targets: workspace of %zu bytes, %zu needed", ws_bytes,
               bd_centernet_targets_workspace_bytes(N));
    // Python forms (1 - min_overlap), 4 * a3 ... in float64 before the tensor operation rounds them to float32: once
    const CnRadiusConst rc = {(float)(1.0 - min_overlap), (float)(1.0 + min_overlap), (float)(-2.0 * min_overlap),
                              (float)(min_overlap - 1.0), (float)(4.0 * (4.0 * min_overlap))};
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(score_map, 0, (size_t)N * H * W * K * sizeof(float), st) != hipSuccess) {
        bd_set_error("centernet_targets: hipMemsetAsync failed");
        return BD_EINVAL;
    }
    hipLaunchKernelGGL(cn_targets_kernel, dim3(CN_SPLIT, N), dim3(256), 0, st, gt_boxes, num_gt, Gmax, K, H, W, T, box_scale, rc,
                       score_map, wh, reg, reg_mask, index, (int*)ws);
    hipLaunchKernelGGL(cn_count_sum_kernel, dim3(1), dim3(64), 0, st, (const int*)ws, N, num_pos);
    BD_CHECK_LAUNCH("bd_centernet_targets");
    return BD_OK;
}

extern "C" int bd_centernet_focal_fwd_bwd(const void* logits, const float* score_map, int64_t rows, int K, int ld, const float* norm,
                                          float weight, float grad_scale, float* loss_sum, void* dlogits, bd_stream_t stream) {
    BD_REQUIRE(logits && score_map && norm && loss_sum && dlogits, "centernet_focal: null pointer");
    BD_REQUIRE(K > 0 && ld % 8 == 0 && ld >= K && ld - K < 8, "centernet_focal: the row stride ld=%d must be K=%d rounded up to a multiple of 8", ld, K);
    BD_REQUIRE(rows >= 0, "centernet_focal: rows < 0");
    if (rows == 0) return BD_OK;
    long long g = cdiv64(rows * (ld / 8), 256);
    const int grid = (int)(g < CN_GRID_CAP ? g : CN_GRID_CAP);
    float* part = cn_partials((hipStream_t)stream, (size_t)grid + 1);
    BD_REQUIRE(part != nullptr, "centernet_focal: cannot allocate the partial-sum scratch");
    auto kernel = K % 4 == 0 ? cn_focal_kernel<true> : cn_focal_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)logits, score_map, (long long)rows, K, ld,
                       norm, weight, grad_scale, part, (bf16_raw*)dlogits);
    hipLaunchKernelGGL(cn_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)part, grid, loss_sum);
    BD_CHECK_LAUNCH("bd_centernet_focal_fwd_bwd");
    return BD_OK;
}

extern "C" int bd_centernet_l1_fwd_bwd(const void* pred, int ld, int off, const int32_t* index, const float* reg_mask, const float* target,
                                       int N, int H, int W, int T, float weight, float grad_scale, float* loss_sum, void* dpred,
                                       bd_stream_t stream) {
    BD_REQUIRE(pred && index && reg_mask && target && loss_sum && dpred, "centernet_l1: null pointer");
    BD_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "centernet_l1: bad sizes");
    BD_REQUIRE(T > 0 && T <= CN_T_MAX && (long long)N * T < (1ll << 31), "centernet_l1: T=%d out of range (1..%d)", T, CN_T_MAX);
    BD_REQUIRE(ld > 0 && ld % 8 == 0 && off >= 0 && off % 2 == 0 && off + 2 <= ld,
               "centernet_l1: ld=%d must be a multiple of 8 and the even column off=%d must leave two channels", ld, off);
    float* part = cn_partials((hipStream_t)stream, (size_t)N + 1);
    BD_REQUIRE(part != nullptr, "centernet_l1: cannot allocate the partial-sum scratch");
    hipLaunchKernelGGL(cn_l1_kernel, dim3(CN_SPLIT, N), dim3(256), 0, (hipStream_t)stream, (const bf16_raw*)pred, ld, off, index, reg_mask,
                       target, N, H * W, T, weight, grad_scale, part, (bf16_raw*)dpred);
    hipLaunchKernelGGL(cn_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)part, N, loss_sum);
    BD_CHECK_LAUNCH("bd_centernet_l1_fwd_bwd");
    return BD_OK;
}

extern "C" size_t bd_centernet_decode_workspace_bytes(int B, int K, int H, int W) {
    if (B <= 0 || K <= 0 || H <= 0 || W <= 0) return 256;
    return ((size_t)B * K * H * W * sizeof(float) + 255) / 256 * 256;
}

extern "C" int bd_centernet_decode(const void* logits, int ld, const void* wh, int wh_ld, int wh_off, const void* reg, int reg_ld,
                                   int reg_off, int B, int K, int H, int W, int k, float* boxes, float* scores, int32_t* classes, void* ws,
                                   size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(logits && wh && boxes && scores && classes && ws, "centernet_decode: null pointer");
    BD_REQUIRE(B > 0 && B <= 65535 && K > 0 && H > 0 && W > 0, "centernet_decode: bad sizes");
    BD_REQUIRE(ld % 8 == 0 && ld >= K && ld - K < 8, "centernet_decode: the row stride ld=%d must be K=%d rounded up to a multiple of 8", ld, K);
    BD_REQUIRE((long long)K * H * W < (1ll << 31) && ld / 8 <= 65535, "centernet_decode: K * H * W must stay below 2^31");
    BD_REQUIRE(k > 0 && k <= CN_K_MAX && k <= H * W, "centernet_decode: k=%d out of range (1..min(%d, H*W))", k, CN_K_MAX);
    BD_REQUIRE(wh_ld > 0 && wh_off >= 0 && wh_off + 2 <= wh_ld, "centernet_decode: bad wh layout");
    BD_REQUIRE(!reg || (reg_ld > 0 && reg_off >= 0 && reg_off + 2 <= reg_ld), "centernet_decode: bad reg layout");
    BD_REQUIRE(ws_bytes >= bd_centernet_decode_workspace_bytes(B, K, H, W), "centernet_decode: workspace of %zu bytes, %zu needed", ws_bytes,
               bd_centernet_decode_workspace_bytes(B, K, H, W));
    hipStream_t st = (hipStream_t)stream;
    const int tiles = cdiv(W, 16) * cdiv(H, 16);
    hipLaunchKernelGGL(cn_peak_kernel, dim3(tiles, ld / 8, B), dim3(256), 0, st, (const bf16_raw*)logits, ld, K, H, W, (float*)ws);
    hipLaunchKernelGGL(cn_topk_kernel, dim3(B), dim3(1024), 0, st, (const float*)ws, K, H, W, k, (const bf16_raw*)wh, wh_ld, wh_off,
                       (const bf16_raw*)reg, reg_ld, reg_off, boxes, scores, classes);
    BD_CHECK_LAUNCH("bd_centernet_decode");
    return BD_OK;
}

extern "C" int bd_centernet_boxes_to_image(const float* boxes, const float* affine, const float* scores, const int32_t* classes, int B, int k,
                                           float* boxes_out, float* scores_out, int32_t* labels_out, bd_stream_t stream) {
    BD_REQUIRE(B > 0 && k > 0, "centernet_boxes_to_image: B=%d and k=%d must be positive", B, k);
    BD_REQUIRE(boxes && affine && scores && classes && boxes_out && scores_out && labels_out, "centernet_boxes_to_image: null pointer");
    BD_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)boxes_out & 15) == 0, "centernet_boxes_to_image: boxes and boxes_out must be 16-byte aligned");
    const long long total = (long long)B * k;
    BD_REQUIRE(total < (1ll << 31) * 256, "centernet_boxes_to_image: B * k too large");
    hipLaunchKernelGGL(cn_boxes_to_image_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, boxes, affine, scores,
                       classes, k, total, boxes_out, scores_out, labels_out);
    BD_CHECK_LAUNCH("bd_centernet_boxes_to_image");
    return BD_OK;
}
