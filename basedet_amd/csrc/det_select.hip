// Fused score + per-level top-k of the one-stage detectors at inference (retinanet.py:183-192, fcos.py:194-204) for a whole batch:
// bd_det_select = bd_det_scores -> bd_segment_topk(min_score), bit for bit, without the fp32 score tensor.  The scores are recomputed in
// registers from the bf16 logits in every pass (same expressions and the same -ffp-contract=off as det_scores_kernel in postprocess.hip).
//
// Selection: the k largest of the composite keys  ck = (score key - key(min_score)) << 24 | (2^24 - 1 - item)  of one (image, level).
// All composite keys of a segment differ, so "score descending, then item index ascending" is their plain descending order and the
// result is a function of the inputs alone:
//   1. histogram passes over 13-bit digits of ck from the top (LDS histogram per workgroup, integer adds into the segment's global
//      histogram), each followed by a scan that finds the digit holding the k-th largest key.  A segment is RESOLVED as soon as that
//      digit's bin holds <= SORT_N - k keys (or fewer than k items pass the threshold at all): everything at or above the bin's lower
//      bound is < SORT_N keys.  The first pass resolves the usual case (13 bits below the threshold's exponent separate the scores
//      of distinct bf16 logits); later passes exit at once for resolved segments and only run into heavy ties.
//   2. compaction: every key >= the segment's bound goes to a slot handed out by an atomic counter (order arbitrary);
//   3. one workgroup per segment sorts its < SORT_N keys in LDS (bitonic, 64-bit) and writes the first k.
// Workspace per (image, level): 32 B of state + NBINS * 4 B of histogram + SORT_N * 8 B of keys = 96 KiB + 32 B, whatever rows and K.
#pragma clang fp contract(off)
#include "select_dev.h"

namespace {

constexpr int DS_DIGIT = 13;
constexpr int DS_NBINS = 1 << DS_DIGIT;
constexpr int DS_SORT_N = 8192;
constexpr int DS_CHUNK = 65536;         // items of one segment per workgroup (a multiple of the 8-item vector)
constexpr int DS_K_MAX = 2048;
constexpr int DS_IDX_BITS = 24;

struct SegState {
    unsigned long long prefix;          // digits of the k-th largest key fixed so far
    unsigned long long collect_min;     // resolved: keys >= this are collected
    int remaining;                      // how many of the keys that share `prefix` are still to be selected
    int resolved;
    int n_valid;                        // items above min_score
    int n_slots;                        // compaction counter
};
static_assert(sizeof(SegState) == 32, "SegState layout");

struct SelSegs { int item0[BD_MAX_SEGS]; int count[BD_MAX_SEGS]; int chunk0[BD_MAX_SEGS + 1]; int nseg; };

struct SelWs { SegState* st; unsigned int* hist; unsigned long long* cand; size_t total; };

inline SelWs sel_layout(void* ws, int B, int L) {
    SelWs w;
    const size_t n = (size_t)B * L;
    char* p = (char*)ws;
    size_t o = 0;
    w.st = (SegState*)(p + o); o += (n * sizeof(SegState) + 255) / 256 * 256;
    w.hist = (unsigned int*)(p + o); o += n * DS_NBINS * sizeof(unsigned int);
    w.cand = (unsigned long long*)(p + o); o += n * DS_SORT_N * sizeof(unsigned long long);
    w.total = o;
    return w;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// f(i, ck) for every item i in [i0, i1) of the segment whose score passes the threshold.  lg / ctr: this image's logits / centerness rows;
// item i is element item0 + i of the image's [rows][ld] logits.  i0 is a multiple of 8: 16-byte loads wherever the segment starts on one.
// ld > K (ld = round_up(K, 8): a vector never leaves its row): the slots >= K of a row are padding -- a pad logit of 0 would score 0.5 --
// and are skipped; the index handed to f and kept in ck is the compact one, (row in the segment) * K + class, which grows with i: the
// order of the keys, ties included, is that of the compact [rows][K] tensor.
template <class F>
__device__ __forceinline__ void for_each_valid(const bf16_raw* __restrict__ lg, const bf16_raw* __restrict__ ctr, int ctr_ld, int ctr_off,
                                               int K, int ld, long long item0, int i0, int i1, float min_score, unsigned int key_lo,
                                               unsigned int kk_max, F f) {
    const bool vec = (reinterpret_cast<unsigned long long>(lg + item0) & 15ull) == 0ull;
    for (int i = i0 + (int)threadIdx.x * 8; i < i1; i += 256 * 8) {
        const int n = i1 - i < 8 ? i1 - i : 8;
        const bf16_raw* p = lg + item0 + i;
        bf16_raw v[8];
        if (vec && n == 8) {
            const u32x4_t q = *reinterpret_cast<const u32x4_t*>(p);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[2 * j] = (bf16_raw)(q[j] & 0xffffu); v[2 * j + 1] = (bf16_raw)(q[j] >> 16); }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < n ? p[j] : (bf16_raw)0;
        }
        long long row = (item0 + i) / ld;
        int c = (int)(item0 + i - row * ld);
        const int ci = ld == K ? i : i - (i / ld) * (ld - K);       // compact index of slot j = 0 (the segment starts on a row)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < n && c < K) {
                float s = sigmoid_f(bf2f(v[j]));
                if (ctr) s = sqrtf(s * sigmoid_f(bf2f(ctr[row * ctr_ld + ctr_off])));
                if (s > min_score) {
                    unsigned int kk = f32_asc_key(s) - key_lo;          // >= 1: the key is strictly increasing in the score
                    kk = kk < kk_max ? kk : kk_max;                      // (a sigmoid score is <= 1: never taken, keeps ck below 2^T)
                    f(ci + j, ((unsigned long long)kk << DS_IDX_BITS) | (unsigned long long)((1u << DS_IDX_BITS) - 1u - (unsigned int)(ci + j)));
                }
            }
            if (++c == ld) { c = 0; ++row; }
        }
    }
}

// COMPACT = false: histogram of digit `pass` over the keys that share the segment's prefix.  COMPACT = true: keys >= collect_min -> slots.
template <bool COMPACT>
__global__ __launch_bounds__(256) void det_select_pass_kernel(const bf16_raw* __restrict__ logits, const bf16_raw* __restrict__ ctr,
                                                              int ctr_ld, int ctr_off, long long rows, int K, int ld, SelSegs segs,
                                                              float min_score, unsigned int key_lo, unsigned int kk_max, int T, int pass,
                                                              SegState* __restrict__ st, unsigned int* __restrict__ hist,
                                                              unsigned long long* __restrict__ cand) {
    __shared__ unsigned int h[COMPACT ? 1 : DS_NBINS];
    int seg = 0;
    for (int q = 1; q < segs.nseg; ++q) if ((int)blockIdx.x >= segs.chunk0[q]) seg = q;
    const int b = blockIdx.y;
    const long long sid = (long long)b * segs.nseg + seg;
    SegState* s = st + sid;
    const int i0 = ((int)blockIdx.x - segs.chunk0[seg]) * DS_CHUNK;
    const int i1 = i0 + DS_CHUNK < segs.count[seg] ? i0 + DS_CHUNK : segs.count[seg];
    const bf16_raw* lg = logits + (long long)b * rows * ld;
    const bf16_raw* ct = ctr ? ctr + (long long)b * rows * ctr_ld : nullptr;
    if (COMPACT) {
        const unsigned long long lo = s->collect_min;
        unsigned long long* out = cand + sid * DS_SORT_N;
        for_each_valid(lg, ct, ctr_ld, ctr_off, K, ld, segs.item0[seg], i0, i1, min_score, key_lo, kk_max, [&](int, unsigned long long ck) {
            if (ck >= lo) {
                const int slot = atomicAdd(&s->n_slots, 1);
                if (slot < DS_SORT_N) out[slot] = ck;       // (the scan bounds the count below SORT_N)
            }
        });
    } else {
        if (s->resolved) return;                            // uniform over the workgroup
        const int hi = T - DS_DIGIT * pass;                 // key bits above this digit
        const int w = hi < DS_DIGIT ? hi : DS_DIGIT;
        const int shift = hi - w;
        const unsigned long long prefix = s->prefix;
        for (int q = threadIdx.x; q < DS_NBINS; q += 256) h[q] = 0u;
        __syncthreads();
        for_each_valid(lg, ct, ctr_ld, ctr_off, K, ld, segs.item0[seg], i0, i1, min_score, key_lo, kk_max, [&](int, unsigned long long ck) {
            if ((ck >> hi) == prefix) atomicAdd(&h[(unsigned int)(ck >> shift) & ((1u << w) - 1u)], 1u);
        });
        __syncthreads();
        unsigned int* g = hist + sid * DS_NBINS;
        for (int q = threadIdx.x; q < DS_NBINS; q += 256) {
            const unsigned int c = h[q];
            if (c) atomicAdd(&g[q], c);
        }
    }
}

// One workgroup per segment: the bin of digit `pass` that holds the remaining-th largest key; clears the histogram for the next pass.
__global__ __launch_bounds__(1024) void det_select_scan_kernel(SegState* __restrict__ st, unsigned int* __restrict__ hist, int k, int T,
                                                               int pass) {
    __shared__ unsigned int wsum[16];
    SegState* s = st + blockIdx.x;
    if (s->resolved) return;
    unsigned int* g = hist + (long long)blockIdx.x * DS_NBINS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = T - DS_DIGIT * pass;
    const int w = hi < DS_DIGIT ? hi : DS_DIGIT;
    const int shift = hi - w;
    const unsigned int remaining = pass == 0 ? (unsigned int)k : (unsigned int)s->remaining;
    const unsigned long long prefix = s->prefix;
    constexpr int PER = DS_NBINS / 1024;
    unsigned int c[PER], sum = 0;                           // thread t owns bins NBINS-1-PER*t .. (descending key order)
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int bin = DS_NBINS - 1 - (PER * tid + j);
        c[j] = g[bin];
        g[bin] = 0u;
        sum += c[j];
    }
    unsigned int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();                                        // (also: every thread has read the state before one of them writes it)
    unsigned int total = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const unsigned int t = wsum[q];
        if (q < wave) inc += t;
        total += t;
    }
    if (pass == 0 && total <= (unsigned int)k) {            // fewer than k items pass the threshold: all of them
        if (tid == 0) { s->n_valid = (int)total; s->collect_min = 0ull; s->resolved = 1; }
        return;
    }
    if (inc >= remaining && inc - sum < remaining) {        // exactly one thread
        unsigned int before = inc - sum;
        int j = 0;
        while (before + c[j] < remaining) { before += c[j]; ++j; }
        const unsigned long long d = (unsigned long long)(DS_NBINS - 1 - (PER * tid + j));
        const unsigned long long np = (prefix << w) | d;
        if (pass == 0) s->n_valid = (int)total;
        if (c[j] <= (unsigned int)(DS_SORT_N - k) || shift == 0) {   // (k - remaining') + c[j] <= k - 1 + SORT_N - k keys to sort
            s->collect_min = np << shift;
            s->resolved = 1;
        } else {
            s->prefix = np;
            s->remaining = (int)(remaining - before);
        }
    }
}

__global__ __launch_bounds__(1024) void det_select_sort_kernel(const SegState* __restrict__ st, const unsigned long long* __restrict__ cand,
                                                               int k, unsigned int key_lo, int* __restrict__ out_idx,
                                                               float* __restrict__ out_score, int* __restrict__ out_cnt) {
    __shared__ unsigned long long keys[DS_SORT_N];
    const int tid = threadIdx.x;
    const long long sid = blockIdx.x;
    int n = st[sid].n_slots;
    n = n < DS_SORT_N ? n : DS_SORT_N;
    const int m = n < k ? n : k;
    int P = 2;
    while (P < n) P <<= 1;
    const unsigned long long* src = cand + sid * DS_SORT_N;
    for (int i = tid; i < P; i += 1024) keys[i] = i < n ? src[i] : 0ull;       // (a valid key is >= 2^24)
    __syncthreads();
    bitonic_sort_1024<true>(keys, P);
    for (int i = tid; i < k; i += 1024) {
        int idx = -1;
        float sc = 0.f;
        if (i < m) {
            const unsigned long long ck = keys[i];
            idx = (int)((1u << DS_IDX_BITS) - 1u - (unsigned int)(ck & ((1ull << DS_IDX_BITS) - 1ull)));
            sc = f32_from_asc_key((unsigned int)(ck >> DS_IDX_BITS) + key_lo);
        }
        out_idx[sid * k + i] = idx;
        out_score[sid * k + i] = sc;
    }
    if (tid == 0) out_cnt[sid] = m;
}

inline unsigned int host_asc_key(float f) {
    unsigned int u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace

extern "C" size_t bd_det_select_workspace_bytes(int B, int L, int64_t rows, int K, int k) {
    (void)rows; (void)K; (void)k;
    if (B <= 0 || L <= 0) return 256;
    return sel_layout(nullptr, B, L).total;
}

// logits [B][rows][ld], ld = K or round_up(K, 8) (the slots >= K of a row are padding and never selected); the indices are the compact
// row * K + class whatever ld is.  SelSegs.item0 / count / chunk0 walk the PADDED items (rows * ld < 2^31).
extern "C" int bd_det_select(const void* logits, int ld, const void* ctr, int ctr_ld, int ctr_off, int B, int64_t rows, int K, int L,
                             const int32_t* seg_start_host, const int32_t* seg_rows_host, int k, float min_score, int32_t* out_idx,
                             float* out_score, int32_t* out_cnt, void* ws, size_t ws_bytes, bd_stream_t stream) {
    BD_REQUIRE(logits && seg_start_host && seg_rows_host && out_idx && out_score && out_cnt && ws, "det_select: null pointer");
    BD_REQUIRE(K > 0 && (ld == K || (ld % 8 == 0 && ld > K && ld - K < 8)), "det_select: ld=%d must be K=%d or K rounded up to a multiple of 8", ld, K);
    BD_REQUIRE(B > 0 && L > 0 && L <= BD_MAX_SEGS && rows >= 0 && rows * ld < (1ll << 31), "det_select: bad sizes");
    BD_REQUIRE(k > 0 && k <= DS_K_MAX, "det_select: k=%d out of range (1..%d)", k, DS_K_MAX);
    BD_REQUIRE(!ctr || (ctr_ld > 0 && ctr_off >= 0 && ctr_off < ctr_ld), "det_select: bad centerness layout");
    BD_REQUIRE(min_score == min_score, "det_select: min_score is NaN");
    SelSegs segs{};
    segs.nseg = L;
    for (int s = 0; s < L; ++s) {
        BD_REQUIRE(seg_start_host[s] >= 0 && seg_rows_host[s] >= 0 && (long long)seg_start_host[s] + seg_rows_host[s] <= rows,
                   "det_select: segment %d leaves the %lld rows", s, (long long)rows);
        BD_REQUIRE((long long)seg_rows_host[s] * K < (1ll << DS_IDX_BITS), "det_select: segment of %lld items is too long",
                   (long long)seg_rows_host[s] * K);
        const long long c = (long long)seg_rows_host[s] * ld;
        segs.item0[s] = (int)((long long)seg_start_host[s] * ld);
        segs.count[s] = (int)c;
        segs.chunk0[s + 1] = segs.chunk0[s] + (int)cdiv64(c, DS_CHUNK);
    }
    const SelWs w = sel_layout(ws, B, L);
    BD_REQUIRE(ws_bytes >= w.total, "det_select: workspace of %zu bytes, %zu needed", ws_bytes, w.total);
    // key range of the scores that can pass: (min_score, 1] -- a sigmoid, and the square root of a product of two, never exceeds 1
    const unsigned int key_lo = host_asc_key(min_score), key_one = host_asc_key(1.f);
    const unsigned int kk_max = key_one > key_lo ? key_one - key_lo : 1u;
    int nbits = 1;
    while (nbits < 32 && (kk_max >> nbits)) ++nbits;
    const int T = nbits + DS_IDX_BITS;
    const int npass = cdiv(T, DS_DIGIT);
    hipStream_t st = (hipStream_t)stream;
    const size_t head = (size_t)((char*)w.cand - (char*)ws);         // state + histograms start at zero
    if (hipMemsetAsync(ws, 0, head, st) != hipSuccess) {
        bd_set_error("det_select: hipMemsetAsync failed");
        return BD_EINVAL;
    }
    const int nchunk = segs.chunk0[L];
    const bf16_raw* lg = (const bf16_raw*)logits;
    const bf16_raw* ct = (const bf16_raw*)ctr;
    for (int p = 0; p < npass; ++p) {
        if (nchunk > 0)
            hipLaunchKernelGGL(det_select_pass_kernel<false>, dim3(nchunk, B), dim3(256), 0, st, lg, ct, ctr_ld, ctr_off, (long long)rows, K, ld,
                               segs, min_score, key_lo, kk_max, T, p, w.st, w.hist, w.cand);
        hipLaunchKernelGGL(det_select_scan_kernel, dim3(B * L), dim3(1024), 0, st, w.st, w.hist, k, T, p);
    }
    if (nchunk > 0)
        hipLaunchKernelGGL(det_select_pass_kernel<true>, dim3(nchunk, B), dim3(256), 0, st, lg, ct, ctr_ld, ctr_off, (long long)rows, K, ld, segs,
                           min_score, key_lo, kk_max, T, 0, w.st, w.hist, w.cand);
    hipLaunchKernelGGL(det_select_sort_kernel, dim3(B * L), dim3(1024), 0, st, w.st, w.cand, k, key_lo, out_idx, out_score, out_cnt);
    BD_CHECK_LAUNCH("bd_det_select");
    return BD_OK;
}
