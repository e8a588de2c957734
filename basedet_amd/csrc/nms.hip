// Greedy NMS (layers/common/post_processing.py:17-47, py_cpu_nms :101-134), the one copy every keep list of the project comes from:
// bd_batched_nms (one problem), bd_nms_batched (B problems: every detector's inference) and, through nms.h, the RPN proposal chain of
// rcnn_ops.hip (one problem per image, or one per (image, level) + merge).  Three steps:
//   prepare  one workgroup per problem: the shift step (largest coordinate + 1), boxes shifted apart by class, the greedy order
//            (score descending, then index ascending: an LDS bitonic sort of score key << 32 | index);
//   mask     one wave per 64 x 64 tile of the sorted list's upper triangle: bit b of mask[i][w] = sorted box i suppresses sorted box 64w+b;
//   scan     one wave per problem walks the sorted list 64 boxes at a time.
// The mask and scan kernels are written once over a problem VIEW (where problem b's sorted list, boxes, mask rows and keep list are); the
// per-level view keeps its capacity and row stride at compile time.  Every keep decision is exact fp32 work, bit-identical to
// oracle/box_ops.py: compiled with -ffp-contract=off like boxops.hip.
#pragma clang fp contract(off)
#include "nms.h"
#include "select_dev.h"

namespace {

constexpr int NMSL_WORDS = NMSL_CAP / 64;

// B independent problems of capacity C
struct JointView {
    static constexpr int MAX_WORDS = NMS_MAX / 64;
    int C, nwords, max_output, keep_ld;
    __device__ long long boxes0(int b) const { return (long long)b * C; }          // the box array that the order's values index
    __device__ long long order0(int b) const { return (long long)b * C; }
    __device__ long long mask0(int b) const { return (long long)b * C * nwords; }
    __device__ int words() const { return nwords; }
    __device__ long long keep0(int b) const { return (long long)b * keep_ld; }
    __device__ int keep_cap(int nv) const { return max_output > 0 ? max_output : nv; }
};

// The RPN's batched NMS level by level.  rpn.py:163-172 runs ONE batched_nms over an image's candidates with the pyramid level as the
// class id: boxes of different levels are shifted apart before the greedy pass (post_processing.py:44-45), so that pass decomposes into L
// independent ones -- 16 x 5 problems of <= 2 048 boxes instead of 16 of ~8 900 (a 157-chunk serial scan per image) -- and the joint keep
// list (score descending, candidate index ascending, first post_k) is the MERGE of the per-level lists (nmsl_merge_kernel).  The boxes keep
// the joint form's shift (level x (max coordinate + 1), in fp32): the IoUs, and with them every keep decision, are the same bits.
// Problem b = (image n, level l): candidates cand_off[l] .. cand_off[l + 1] of image n's C.  A level keeps at most post_k boxes (no more
// of them can reach the joint list's first post_k).
struct LevelView {
    static constexpr int MAX_WORDS = NMSL_WORDS;
    RpnLevels lv;
    int C, post_k;
    __device__ long long boxes0(int b) const { return (long long)(b / lv.L) * C; }
    __device__ long long order0(int b) const { const int n = b / lv.L; return (long long)n * C + lv.cand_off[b - n * lv.L]; }
    __device__ long long mask0(int b) const { return (long long)b * NMSL_CAP * NMSL_WORDS; }
    __device__ int words() const { return NMSL_WORDS; }
    __device__ long long keep0(int b) const { return (long long)b * post_k; }
    __device__ int keep_cap(int) const { return post_k; }
};

// One workgroup prepares the problem of items i0 .. i0 + cnt of a box array of C items (boxes, scores, sboxes and order point at that
// array): step = largest coordinate of the WHOLE array + 1, sboxes = boxes + shift(item, step), order[i0 ..] = the items sorted by score
// descending, then index ascending, *nvalid = how many of them take part.  ABSENT: an item with score == -inf is left out of the maximum
// and of nvalid (it sorts behind every other item, so the first nvalid of the order are the items that take part); otherwise every item
// is present, as in oracle.box_ops.batched_nms (boxes.max(), a stable argsort).  keys: npow2 >= cnt words of LDS, npow2 a power of two.
template <bool ABSENT, class ShiftFn>
__device__ __forceinline__ void nms_prepare(const float* __restrict__ boxes, const float* __restrict__ scores, int C, int i0, int cnt,
                                            int npow2, ShiftFn shift, float* __restrict__ sboxes, int* __restrict__ order,
                                            int* __restrict__ nvalid, unsigned long long* keys) {
    __shared__ float red[16];
    __shared__ int cnt_sh;
    const int tid = threadIdx.x;
    if (tid == 0) cnt_sh = 0;
    float mx = -INFINITY;
    for (int i = tid; i < C; i += 1024) {
        if (!ABSENT || scores[i] > -INFINITY) {
            const Box b = ld_box(boxes + i * 4ll);
            mx = fmaxf(mx, fmaxf(fmaxf(b.x1, b.y1), fmaxf(b.x2, b.y2)));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int q = 1; q < 16; ++q) mx = fmaxf(mx, red[q]);
    const float step = mx + 1.f;                                   // post_processing.py:44-45
    int nv = 0;
    for (int i = tid; i < npow2; i += 1024) {
        unsigned long long key = ~0ull;
        if (i < cnt) {
            const int c = i0 + i;
            const float sc = scores[c];
            key = ((unsigned long long)float_desc_key(sc) << 32) | (unsigned int)c;
            nv += !ABSENT || sc > -INFINITY;
            const float off = shift(c, step);
            const Box b = ld_box(boxes + c * 4ll);
            f32x4_t o = {b.x1 + off, b.y1 + off, b.x2 + off, b.y2 + off};
            *reinterpret_cast<f32x4_t*>(sboxes + c * 4ll) = o;
        }
        keys[i] = key;
    }
    if (nv) atomicAdd(&cnt_sh, nv);
    __syncthreads();
    bitonic_sort_1024<false>(keys, npow2);
    for (int i = tid; i < cnt; i += 1024) order[i0 + i] = (int)(keys[i] & 0xffffffffu);
    if (tid == 0) *nvalid = cnt_sh;
}

// grid (B): problem b is the whole array b, shifted by its class ids (none: no shift); npow2 * 8 bytes of dynamic LDS
template <bool ABSENT>
__global__ __launch_bounds__(1024) void nms_prepare_joint_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                 const int* __restrict__ idxs, int C, int npow2,
                                                                 float* __restrict__ sboxes, int* __restrict__ order,
                                                                 int* __restrict__ nvalid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const long long b0 = (long long)blockIdx.x * C;
    if (idxs) idxs += b0;
    nms_prepare<ABSENT>(boxes + b0 * 4, scores + b0, C, 0, C, npow2,
                        [&](int i, float step) { return idxs ? (float)idxs[i] * step : 0.f; }, sboxes + b0 * 4, order + b0,
                        nvalid + blockIdx.x, reinterpret_cast<unsigned long long*>(smem));
}

// grid (L, N): one level's candidates of image n, shifted by the level with the step of the JOINT problem (all of the image's candidates)
__global__ __launch_bounds__(1024) void nms_prepare_level_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                 RpnLevels lv, int C, float* __restrict__ sboxes,
                                                                 int* __restrict__ order, int* __restrict__ nvalid) {
    __shared__ unsigned long long keys[NMSL_CAP];
    const int l = blockIdx.x, n = blockIdx.y;
    const long long b0 = (long long)n * C;
    const int c0 = lv.cand_off[l];
    nms_prepare<true>(boxes + b0 * 4, scores + b0, C, c0, lv.cand_off[l + 1] - c0, NMSL_CAP,
                      [&](int, float step) { return (float)l * step; }, sboxes + b0 * 4, order + b0, nvalid + n * lv.L + l, keys);
}

// grid (row tiles, words, problems), one wave: 64 sorted rows x 64 sorted columns.  Only the upper triangle (w >= i/64) inside the valid
// range is written -- the scan never reads anything else.
template <class View>
__global__ __launch_bounds__(64) void nms_mask_kernel(View v, const float* __restrict__ sboxes, const int* __restrict__ order,
                                                      const int* __restrict__ nvalid, float thr, unsigned long long* __restrict__ mask) {
    __shared__ float rows[64 * 4];
    const int rt = blockIdx.x, w = blockIdx.y, b = blockIdx.z;
    const int nv = nvalid[b];
    if (w < rt || rt * 64 >= nv || w * 64 >= nv) return;
    sboxes += v.boxes0(b) * 4; order += v.order0(b); mask += v.mask0(b);
    const int lane = threadIdx.x;
    const int j = w * 64 + lane;
    Box cb{0.f, 0.f, 0.f, 0.f};
    if (j < nv) cb = ld_box(sboxes + order[j] * 4ll);
    const int ri = rt * 64 + lane;
    f32x4_t rb = {0.f, 0.f, 0.f, 0.f};
    if (ri < nv) rb = *reinterpret_cast<const f32x4_t*>(sboxes + order[ri] * 4ll);
    *reinterpret_cast<f32x4_t*>(rows + lane * 4) = rb;
    __syncthreads();
    const float ca = box_area(cb);
    const int rmax = min(64, nv - rt * 64);
    unsigned long long mine = 0ull;
    for (int q = 0; q < rmax; ++q) {
        const int i = rt * 64 + q;
        const Box a = Box{rows[q * 4], rows[q * 4 + 1], rows[q * 4 + 2], rows[q * 4 + 3]};
        bool sup = false;
        if (j < nv && j > i) {
            const float inter = box_inter(a, cb);
            const float uni = (box_area(a) + ca) - inter;
            sup = (inter / uni) > thr;     // keep iff iou <= thr (py_cpu_nms, post_processing.py:130)
        }
        const unsigned long long bal = __ballot(sup);
        if (lane == q) mine = bal;
    }
    if (lane < rmax) mask[(long long)(rt * 64 + lane) * v.words() + w] = mine;
}

// grid (problems), one wave: the diagonal 64x64 block of a chunk is resolved in registers, then the rows of the survivors are OR-ed into
// the LDS `removed` bitmap with independent (pipelined) loads -- in one trip where the view's problems have at most 64 words.
template <class View>
__global__ __launch_bounds__(64) void nms_scan_kernel(View v, const unsigned long long* __restrict__ mask, const int* __restrict__ order,
                                                      const int* __restrict__ nvalid, int* __restrict__ keep, int* __restrict__ num_keep) {
    constexpr bool ONE_TRIP = View::MAX_WORDS <= 64;
    __shared__ unsigned long long removed[View::MAX_WORDS];
    const int b = blockIdx.x, lane = threadIdx.x;
    mask += v.mask0(b); order += v.order0(b); keep += v.keep0(b);
    const int words = v.words();
    const int nv = nvalid[b];
    const int nw = (nv + 63) >> 6;
    for (int w = lane; w < nw; w += 64) { removed[w] = 0ull; if (ONE_TRIP) break; }
    __syncthreads();
    int cnt = 0;
    const int cap = v.keep_cap(nv);
    for (int c = 0; c < nw && cnt < cap; ++c) {
        const int i0 = c * 64;
        const int i = i0 + lane;
        const unsigned long long diag = i < nv ? mask[(long long)i * words + c] : 0ull;
        const int nin = min(64, nv - i0);
        unsigned long long alive = ~removed[c];
        if (nin < 64) alive &= (1ull << nin) - 1ull;
        unsigned long long kept = 0ull;
        const unsigned int dlo = (unsigned int)diag, dhi = (unsigned int)(diag >> 32);
        for (int q = 0; q < nin; ++q) {
            if ((alive >> q) & 1ull) {                                   // wave-uniform
                kept |= 1ull << q;
                const unsigned long long row = ((unsigned long long)(unsigned int)__shfl((int)dhi, q, 64) << 32) |
                                               (unsigned int)__shfl((int)dlo, q, 64);
                alive &= ~row;
            }
        }
        // honour the cap: keep only the first (cap - cnt) survivors of this chunk
        int nk = __popcll(kept);
        if (cnt + nk > cap) {
            int drop = cnt + nk - cap;
            while (drop > 0) { kept &= ~(1ull << (63 - __builtin_clzll(kept))); --drop; }
            nk = cap - cnt;
        }
        if ((kept >> lane) & 1ull) keep[cnt + __popcll(kept & ((1ull << lane) - 1ull))] = order[i];
        cnt += nk;
        if (cnt >= cap) break;
        for (int w = c + 1 + lane; w < nw; w += 64) {
            unsigned long long acc = 0ull;
            unsigned long long kk = kept;
            while (kk) {
                const int q = __ffsll((long long)kk) - 1;
                kk &= kk - 1ull;
                acc |= mask[(long long)(i0 + q) * words + w];
            }
            removed[w] |= acc;
            if (ONE_TRIP) break;
        }
        __syncthreads();
    }
    if (lane == 0) num_keep[b] = cnt;
}

// grid (N): joint rank of every kept box = its rank inside its level + the kept boxes of the other levels that precede it in
// (score descending, candidate index ascending) order -- levels are laid out in candidate-index order, so a box of a LOWER level precedes
// on a score tie, one of a higher level does not.  Binary searches over the per-level lists (sorted by construction).
__global__ __launch_bounds__(1024) void nmsl_merge_kernel(const float* __restrict__ scores, const int* __restrict__ keep_l,
                                                          const int* __restrict__ num_l, RpnLevels lv, int C, int post_k,
                                                          int* __restrict__ keep, int* __restrict__ num_keep) {
    const int n = blockIdx.x, tid = threadIdx.x;
    scores += (long long)n * C; keep_l += (long long)n * lv.L * post_k; num_l += n * lv.L; keep += (long long)n * post_k;
    int tot = 0;
    for (int l = 0; l < lv.L; ++l) tot += num_l[l];
    for (int l = 0; l < lv.L; ++l) {
        const int nl = num_l[l];
        for (int r = tid; r < nl; r += 1024) {
            const int c = keep_l[l * post_k + r];
            const unsigned int key = float_desc_key(scores[c]);
            int rank = r;
            for (int o = 0; o < lv.L; ++o) {
                if (o == l) continue;
                const int* lst = keep_l + o * post_k;
                int lo = 0, hi = num_l[o];               // first index whose key is > key (o < l: ties precede) or >= key (o > l)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const unsigned int km = float_desc_key(scores[lst[mid]]);
                    const bool before = o < l ? km <= key : km < key;
                    if (before) lo = mid + 1; else hi = mid;
                }
                rank += lo;
            }
            if (rank < post_k) keep[rank] = c;
        }
    }
    if (tid == 0) num_keep[n] = tot < post_k ? tot : post_k;
}

inline int next_pow2_i(int n) { int p = 1; while (p < n) p <<= 1; return p; }
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

struct JointWs { size_t sboxes, order, nvalid, mask, total; };
inline JointWs joint_ws(int B, int C) {
    JointWs l;
    size_t o = 0;
    l.sboxes = o; o += align256((size_t)B * C * 16);
    l.order = o; o += align256((size_t)B * C * 4);
    l.nvalid = o; o += align256((size_t)B * 4);
    l.mask = o; o += align256((size_t)B * C * cdiv(C, 64) * 8);
    l.total = o;
    return l;
}
// bd_batched_nms's one problem inside the size bd_nms_workspace_bytes has always returned (sections 16-byte aligned, 64 bytes of slack
// that now hold nvalid): a caller's buffer of that size stays large enough
inline JointWs single_ws(int n) {
    JointWs l;
    l.sboxes = 0;
    l.order = (size_t)n * 16;
    l.mask = l.order + ((size_t)n * 4 + 15) / 16 * 16;
    l.nvalid = l.mask + (size_t)n * cdiv(n, 64) * 8;
    l.total = (size_t)n * 16 + (size_t)n * 4 + (size_t)n * cdiv(n, 64) * 8 + 64;
    return l;
}

void joint_run(const float* boxes, const float* scores, const int32_t* idxs, int B, int C, bool absent, float thr, int max_output,
               int keep_ld, int32_t* keep, int32_t* num_keep, unsigned char* ws, const JointWs& l, hipStream_t st) {
    float* sboxes = (float*)(ws + l.sboxes);
    int* order = (int*)(ws + l.order);
    int* nvalid = (int*)(ws + l.nvalid);
    unsigned long long* mask = (unsigned long long*)(ws + l.mask);
    const int npow2 = next_pow2_i(C), words = cdiv(C, 64);
    BD_ONCE_PER_DEVICE(
        (void)hipFuncSetAttribute((const void*)nms_prepare_joint_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, NMS_MAX * 8);
        (void)hipFuncSetAttribute((const void*)nms_prepare_joint_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, NMS_MAX * 8));
    if (absent)
        hipLaunchKernelGGL(nms_prepare_joint_kernel<true>, dim3(B), dim3(1024), (size_t)npow2 * 8, st, boxes, scores, idxs, C, npow2, sboxes,
                           order, nvalid);
    else
        hipLaunchKernelGGL(nms_prepare_joint_kernel<false>, dim3(B), dim3(1024), (size_t)npow2 * 8, st, boxes, scores, idxs, C, npow2, sboxes,
                           order, nvalid);
    const JointView v{C, words, max_output, keep_ld};
    hipLaunchKernelGGL(nms_mask_kernel<JointView>, dim3(words, words, B), dim3(64), 0, st, v, sboxes, order, nvalid, thr, mask);
    hipLaunchKernelGGL(nms_scan_kernel<JointView>, dim3(B), dim3(64), 0, st, v, mask, order, nvalid, keep, num_keep);
}

struct LevelWs { size_t sboxes, order, nvalid, mask, keep_l, num_l, total; };
inline LevelWs level_ws(int N, int L, int C, int post_k) {
    LevelWs l;
    size_t o = 0;
    l.sboxes = o; o += align256((size_t)N * C * 16);
    l.order = o; o += align256((size_t)N * C * 4);
    l.nvalid = o; o += align256((size_t)N * L * 4);
    l.mask = o; o += align256((size_t)N * L * NMSL_CAP * NMSL_WORDS * 8);
    l.keep_l = o; o += align256((size_t)N * L * post_k * 4);
    l.num_l = o; o += align256((size_t)N * L * 4);
    l.total = o;
    return l;
}

}  // namespace

size_t bd_nms_joint_ws_bytes(int B, int C) { return joint_ws(B, C).total; }
size_t bd_nms_levels_ws_bytes(int N, int L, int C, int post_k) { return level_ws(N, L, C, post_k).total; }

int bd_nms_joint_run(const float* boxes, const float* scores, const int32_t* idxs, int B, int C, float thr, int max_output, int keep_ld,
                     int32_t* keep, int32_t* num_keep, unsigned char* ws, hipStream_t st) {
    joint_run(boxes, scores, idxs, B, C, true, thr, max_output, keep_ld, keep, num_keep, ws, joint_ws(B, C), st);
    return BD_OK;
}

int bd_nms_levels_run(const float* boxes, const float* scores, const RpnLevels& lv, int N, int C, float thr, int post_k, int32_t* keep,
                      int32_t* num_keep, unsigned char* ws, hipStream_t st) {
    const LevelWs l = level_ws(N, lv.L, C, post_k);
    float* sboxes = (float*)(ws + l.sboxes);
    int* order = (int*)(ws + l.order);
    int* nvalid = (int*)(ws + l.nvalid);
    unsigned long long* mask = (unsigned long long*)(ws + l.mask);
    int* keep_l = (int*)(ws + l.keep_l);
    int* num_l = (int*)(ws + l.num_l);
    const LevelView v{lv, C, post_k};
    hipLaunchKernelGGL(nms_prepare_level_kernel, dim3(lv.L, N), dim3(1024), 0, st, boxes, scores, lv, C, sboxes, order, nvalid);
    hipLaunchKernelGGL(nms_mask_kernel<LevelView>, dim3(NMSL_WORDS, NMSL_WORDS, N * lv.L), dim3(64), 0, st, v, sboxes, order, nvalid, thr, mask);
    hipLaunchKernelGGL(nms_scan_kernel<LevelView>, dim3(N * lv.L), dim3(64), 0, st, v, mask, order, nvalid, keep_l, num_l);
    hipLaunchKernelGGL(nmsl_merge_kernel, dim3(N), dim3(1024), 0, st, scores, keep_l, num_l, lv, C, post_k, keep, num_keep);
    return BD_OK;
}

extern "C" size_t bd_nms_workspace_bytes(int n) {
    if (n <= 0) return 16;
    return single_ws(n).total;
}

// one problem in which every item is present (a score of -inf sorts last and is kept unless suppressed), as the reference's batched_nms
extern "C" int bd_batched_nms(const float* boxes, const float* scores, const int32_t* idxs, int n, float iou_thresh,
                              int max_output, int32_t* keep, int32_t* num_keep, void* ws, size_t ws_bytes,
                              bd_stream_t stream) {
    BD_REQUIRE(num_keep, "batched_nms: null num_keep");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { (void)hipMemsetAsync(num_keep, 0, sizeof(int32_t), st); return BD_OK; }
    BD_REQUIRE(boxes && scores && keep && ws, "batched_nms: null pointer");
    BD_REQUIRE(n > 0 && n <= NMS_MAX, "batched_nms: n=%d out of range (1..%d)", n, NMS_MAX);
    if (ws_bytes < bd_nms_workspace_bytes(n)) {
        bd_set_error("batched_nms: workspace %zu < %zu bytes", ws_bytes, bd_nms_workspace_bytes(n));
        return BD_EWORKSPACE;
    }
    joint_run(boxes, scores, idxs, 1, n, false, iou_thresh, max_output, 0, keep, num_keep, (unsigned char*)ws, single_ws(n), st);
    BD_CHECK_LAUNCH("bd_batched_nms");
    return BD_OK;
}

extern "C" size_t bd_nms_batched_workspace_bytes(int B, int C) {
    if (B <= 0 || C <= 0) return 256;
    return joint_ws(B, C).total;
}

// B problems of capacity C; an item with score == -inf is absent
extern "C" int bd_nms_batched(const float* boxes, const float* scores, const int32_t* idxs, int B, int C, float iou_thresh,
                              int max_output, int keep_ld, int32_t* keep, int32_t* num_keep, void* ws, size_t ws_bytes,
                              bd_stream_t stream) {
    BD_REQUIRE(boxes && scores && keep && num_keep && ws, "nms_batched: null pointer");
    BD_REQUIRE(B > 0 && C > 0 && C <= NMS_MAX, "nms_batched: C=%d out of range (1..%d)", C, NMS_MAX);
    BD_REQUIRE(keep_ld >= (max_output > 0 ? (max_output < C ? max_output : C) : C), "nms_batched: keep_ld too small");
    if (ws_bytes < bd_nms_batched_workspace_bytes(B, C)) {
        bd_set_error("nms_batched: workspace %zu < %zu bytes", ws_bytes, bd_nms_batched_workspace_bytes(B, C));
        return BD_EWORKSPACE;
    }
    bd_nms_joint_run(boxes, scores, idxs, B, C, iou_thresh, max_output, keep_ld, keep, num_keep, (unsigned char*)ws, (hipStream_t)stream);
    BD_CHECK_LAUNCH("bd_nms_batched");
    return BD_OK;
}
