// Gradient-skip scan (bd_conv_desc.gskip): which patches of a gradient operand g hold a nonzero bit, for the data and weight gradients
// that then compute only those (conv3x3_pp.hip, conv_wgrad3x3_ring.hip).
//
// The box tower's gradients of a detection head are nonzero only around the foreground anchors (a few per cent of the pyramid): the
// regression loss writes an exact +0 for every other anchor, and each 3x3 layer widens the nonzero region by one pixel.  Skipping the
// all-zero patches is exact -- they add exact zeros -- so the results keep their bits.
//
//   gskip_scan_kernel     one workgroup per PH x PW patch of g (g's own geometry: the conv's output levels): mask[patch] = GS_ANY if any
//                         element of any channel has a nonzero bit pattern (-0 counts), plus which border rows / columns / corners do.
//                         Every mask word is written exactly once: the scratch needs no clearing between calls.
//   gskip_compact_kernel  ONE workgroup (a fixed order, no inter-workgroup communication): output patch q of the data gradient is live if
//                         g is nonzero anywhere in its (PH + 2) x (PW + 2) footprint inside the same image and level -- its own patch, the
//                         facing border row / column of its four neighbours and the facing corner of its four diagonal neighbours.
//                         live[q] = 0 / 1, list = the live patches in ascending order, count = their number.
#include "common.h"

namespace {

enum { GS_ANY = 1, GS_TOP = 2, GS_BOT = 4, GS_LEFT = 8, GS_RIGHT = 16, GS_TL = 32, GS_TR = 64, GS_BL = 128, GS_BR = 256 };

struct GsSeg { int patch_start, H, W, pw, off; };

struct GsParams {
    const bf16_raw* g;
    int* mask;
    int C, ppi, ph, pw_px, nseg, patches_per_img, total;
    GsSeg seg[BD_MAX_SEGS];
};

__device__ __forceinline__ int gs_level(const GsParams& p, int rem) {
    int s = 0;
#pragma unroll
    for (int k = 1; k < BD_MAX_SEGS; ++k)
        if (k < p.nseg && rem >= p.seg[k].patch_start) s = k;
    return s;
}

__global__ __launch_bounds__(256) void gskip_scan_kernel(const GsParams p) {
    __shared__ int sbits;
    const int tid = threadIdx.x;
    const int pid = blockIdx.x;
    const int n = pid / p.patches_per_img, rem = pid - n * p.patches_per_img;
    const int s = gs_level(p, rem);
    const int H = p.seg[s].H, W = p.seg[s].W, pwn = p.seg[s].pw;
    const int local = rem - p.seg[s].patch_start, by = local / pwn, bx = local - by * pwn;
    const int y0 = by * p.ph, x0 = bx * p.pw_px;
    const int cpp = p.C >> 3;                               // 16-byte chunks per pixel
    const int items = p.ph * p.pw_px * cpp;
    const long long img = (long long)n * p.ppi + p.seg[s].off;
    if (tid == 0) sbits = 0;
    __syncthreads();
    int bits = 0;
    constexpr int U = 8;                                    // (256 x 8 chunks = one 4 x 16 patch of 256 channels in one pass)
    for (int b = 0; b < items; b += 256 * U) {
        u32x4_t v[U];
        int pix[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {                        // all loads of the pass first, then the tests
            const int i = b + k * 256 + tid;
            v[k] = (u32x4_t){0u, 0u, 0u, 0u};
            pix[k] = -1;
            if (i < items) {
                const int px = i / cpp, ch = i - px * cpp;
                const int py = px / p.pw_px, pxx = px - py * p.pw_px;
                const int y = y0 + py, x = x0 + pxx;
                if (y < H && x < W) {
                    v[k] = *reinterpret_cast<const u32x4_t*>(p.g + (img + (long long)y * W + x) * p.C + ch * 8);
                    pix[k] = px;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (pix[k] >= 0 && (v[k][0] | v[k][1] | v[k][2] | v[k][3])) {
                const int py = pix[k] / p.pw_px, pxx = pix[k] - py * p.pw_px;
                const bool t = py == 0, bo = py == p.ph - 1, l = pxx == 0, r = pxx == p.pw_px - 1;
                bits |= GS_ANY | (t ? GS_TOP : 0) | (bo ? GS_BOT : 0) | (l ? GS_LEFT : 0) | (r ? GS_RIGHT : 0) | (t && l ? GS_TL : 0) |
                        (t && r ? GS_TR : 0) | (bo && l ? GS_BL : 0) | (bo && r ? GS_BR : 0);
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bits |= __shfl_xor(bits, m, 64);
    if ((tid & 63) == 0 && bits) atomicOr(&sbits, bits);
    __syncthreads();
    if (tid == 0) p.mask[pid] = sbits;
}

// (each thread takes KP consecutive patches, their 9 x KP mask reads in flight together: one memory round trip per 8 192 patches -- the
// one-patch-per-thread form spent ~6 round trips, 18 - 36 us, on the head's 6 144 patches)
// FRESH: the masks were written by other workgroups of the SAME launch (gskip_fill_kernel's last workgroup): device-scope loads
template <bool FRESH>
__device__ __forceinline__ int gs_mask(const int* m, int i) {
    if (FRESH) return __hip_atomic_load(m + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return m[i];
}

template <bool FRESH>
__device__ __forceinline__ void gs_compact_body(const GsParams& p, int* live, int* list, int* count, int* wsum) {
    constexpr int KP = 8;
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    int base = 0;
    for (int c0 = 0; c0 < p.total; c0 += 1024 * KP) {
        int lv[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const int q = c0 + tid * KP + j;
            lv[j] = 0;
            if (q < p.total) {
                const int n = q / p.patches_per_img, rem = q - n * p.patches_per_img;
                const int s = gs_level(p, rem);
                const int pwn = p.seg[s].pw, rows = (p.seg[s].H + p.ph - 1) / p.ph;
                const int local = rem - p.seg[s].patch_start, by = local / pwn, bx = local - by * pwn;
                const int* m = p.mask + (long long)n * p.patches_per_img + p.seg[s].patch_start;
                const bool up = by > 0, dn = by + 1 < rows, lf = bx > 0, rt = bx + 1 < pwn;
                int v = gs_mask<FRESH>(m, by * pwn + bx) & GS_ANY;
                if (up) v |= gs_mask<FRESH>(m, (by - 1) * pwn + bx) & GS_BOT;
                if (dn) v |= gs_mask<FRESH>(m, (by + 1) * pwn + bx) & GS_TOP;
                if (lf) v |= gs_mask<FRESH>(m, by * pwn + bx - 1) & GS_RIGHT;
                if (rt) v |= gs_mask<FRESH>(m, by * pwn + bx + 1) & GS_LEFT;
                if (up && lf) v |= gs_mask<FRESH>(m, (by - 1) * pwn + bx - 1) & GS_BR;
                if (up && rt) v |= gs_mask<FRESH>(m, (by - 1) * pwn + bx + 1) & GS_BL;
                if (dn && lf) v |= gs_mask<FRESH>(m, (by + 1) * pwn + bx - 1) & GS_TR;
                if (dn && rt) v |= gs_mask<FRESH>(m, (by + 1) * pwn + bx + 1) & GS_TL;
                lv[j] = v != 0;
            }
        }
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < KP; ++j) cnt += lv[j];
        int inc = cnt;                               // inclusive prefix over the wave's lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o, 64);
            if (ln >= o) inc += y;
        }
        if (ln == 63) wsum[wv] = inc;
        __syncthreads();
        int off = base + inc - cnt, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            off += w < wv ? wsum[w] : 0;
            tot += wsum[w];
        }
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const int q = c0 + tid * KP + j;
            if (q < p.total) live[q] = lv[j];
            if (lv[j]) list[off++] = q;
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

__global__ __launch_bounds__(1024) void gskip_compact_kernel(const GsParams p, int* live, int* list, int* count) {
    __shared__ int wsum[16];
    gs_compact_body<false>(p, live, list, count, wsum);
}

// ---- liveness maps (bd_conv_desc.gskip_gmap / gskip_dxmap) ----
// A map belongs to one gradient tensor T and holds what both of T's consumers need, so that nobody scans T again:
//   hdr[8]      [0] = which of the two lists is current (bit 0), [1] = finished-workgroup counter of gskip_fill_kernel, [2], [3] = the lists' counts
//   m4[P4]      the GS_* word of every 4 x 16 patch of T (what gskip_scan_kernel writes)
//   m8[P8]      nonzero iff the 8 x 8 patch of T holds a nonzero bit (the sparse ring walk's gflags)
//   live[P4]    0 / 1 per output patch of the data gradient that reads T: g nonzero in its footprint (gskip_compact_kernel's live[])
//   list[2][P4] that data gradient's live patches, ascending: the current list and the previous call's
// gskip_fill_kernel: ONE launch behind the data gradient that wrote T = dx.  Its workgroups walk the 8 x 16 blocks of T, one block = two 4 x 16 patches one
// above the other = two 8 x 8 patches side by side: the patches the launch computed (its own live[]; NULL: all) are tested for nonzero
// bits, every other patch holds +0 and gets zero flags; each word is written exactly once.  The last workgroup to finish (device-scope
// counter) runs the compaction -- one workgroup, ascending order, as gskip_compact_kernel -- into the list that is not current and flips.
enum { GM_HDR = 8 };

struct GmSeg { int H, W, off, s4, s8, ss; };

struct GmParams {
    const bf16_raw* t;
    const int* live_in;      // the producing launch's live[] over T's 4 x 16 patches (NULL: test every patch)
    int* map;
    int C, ppi, nseg, pi4, pi8, pis, tot4, tot8;
    GmSeg seg[BD_MAX_SEGS];
};

__global__ __launch_bounds__(1024) void gskip_fill_kernel(const GmParams p, const GsParams cp, int total) {
    __shared__ int sbits, slast;
    __shared__ int wsum[16];
    const int tid = threadIdx.x;
    int* m4 = p.map + GM_HDR;
    int* m8 = m4 + p.tot4;
    const int cpp = p.C >> 3;
    const int items = 4 * 16 * cpp;
    // a few workgroups walk all blocks: the release fence below writes the L2 back, and one per block (3 100 of them on the head's pyramid)
    // cost 130 us -- one per workgroup costs a few
    for (int pid = blockIdx.x; pid < total; pid += gridDim.x) {
        const int n = pid / p.pis, rem = pid - n * p.pis;
        int s = 0;
#pragma unroll
        for (int k = 1; k < BD_MAX_SEGS; ++k)
            if (k < p.nseg && rem >= p.seg[k].ss) s = k;
        const int H = p.seg[s].H, W = p.seg[s].W;
        const int sc = (W + 15) >> 4, r4 = (H + 3) >> 2, c8 = (W + 7) >> 3;
        const int local = rem - p.seg[s].ss, sy = local / sc, sx = local - sy * sc;
        int q4[2], q8[2];
        bool ok4[2], ok8[2], lv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ok4[h] = 2 * sy + h < r4;
            q4[h] = n * p.pi4 + p.seg[s].s4 + (2 * sy + h) * sc + sx;
            ok8[h] = 2 * sx + h < c8;
            q8[h] = n * p.pi8 + p.seg[s].s8 + sy * c8 + 2 * sx + h;
            lv[h] = ok4[h] && (p.live_in == nullptr || p.live_in[q4[h]] != 0);
        }
        int b = 0;                                           // [0, 9): GS_* of the upper patch, [9, 18): of the lower, 18 / 19: the 8 x 8 patches
        if (lv[0] || lv[1]) {                                // (uniform: every thread read the same two flags)
            if (tid == 0) sbits = 0;
            __syncthreads();
            const long long img = (long long)n * p.ppi + p.seg[s].off;
            int bits = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!lv[h]) continue;
                for (int i = tid; i < items; i += 1024) {
                    const int px = i / cpp, ch = i - px * cpp;
                    const int py = px >> 4, pxx = px & 15;
                    const int y = 8 * sy + 4 * h + py, x = 16 * sx + pxx;
                    if (y < H && x < W) {
                        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(p.t + (img + (long long)y * W + x) * p.C + ch * 8);
                        if (v[0] | v[1] | v[2] | v[3]) {
                            const bool t = py == 0, bo = py == 3, l = pxx == 0, r = pxx == 15;
                            const int w = GS_ANY | (t ? GS_TOP : 0) | (bo ? GS_BOT : 0) | (l ? GS_LEFT : 0) | (r ? GS_RIGHT : 0) |
                                          (t && l ? GS_TL : 0) | (t && r ? GS_TR : 0) | (bo && l ? GS_BL : 0) | (bo && r ? GS_BR : 0);
                            bits |= (w << (9 * h)) | (1 << (18 + (pxx >> 3)));
                        }
                    }
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) bits |= __shfl_xor(bits, m, 64);
            if ((tid & 63) == 0 && bits) atomicOr(&sbits, bits);
            __syncthreads();
            b = sbits;
            __syncthreads();                                 // (sbits is cleared again by the next live block)
        }
        if (tid == 0) {
            if (ok4[0]) m4[q4[0]] = b & 511;
            if (ok4[1]) m4[q4[1]] = (b >> 9) & 511;
            if (ok8[0]) m8[q8[0]] = (b >> 18) & 1;
            if (ok8[1]) m8[q8[1]] = (b >> 19) & 1;
        }
    }
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // this workgroup's flags are visible device-wide before it counts as finished
        slast = atomicAdd(p.map + 1, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!slast) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int nxt = (p.map[0] & 1) ^ 1;
    int* live = m8 + p.tot8;
    gs_compact_body<true>(cp, live, live + p.tot4 * (1 + nxt), p.map + 2 + nxt, wsum);
    if (tid == 0) { p.map[0] = nxt; p.map[1] = 0; }
}

// ---- forward liveness (bd_conv_desc.fwd_map; the sparse FORWARD instance of conv3x3_pp.hip) ----
// A tower of n 3x3 layers whose last output is read only at the foreground pixels F of each image and level (a pixel with an anchor whose
// label is > 0) needs the output of the layer k steps above that one only inside F dilated k times (each 3x3 layer reaches one pixel further;
// the dilation stops at the borders of the image and level).  bd_fwd_live_maps builds, from the labels alone, one map per depth k = 1 .. depths:
//   hdr[8]      [0] = which of the two lists is current (bit 0), [2], [3] = the lists' counts; [1] of the depth-1 map = finished-workgroup counter
//   live[P4]    0 / 1 per 4 x 16 patch: the patch holds a pixel of F dilated k times
//   list[2][P4] the live patches, ascending: the current list and the previous call's
// fwd_live_kernel: one workgroup per (image, level) keeps the level's pixel bitmap (one byte per pixel, two buffers) in LDS, dilates it
// pixel by pixel and writes the level's patch flags of every depth; the last workgroup to finish (device-scope counter, nobody waits)
// compacts every depth's flags into the list that is not current and flips.
enum { FL_HDR = 8, FL_MAX_DEPTH = 8 };

struct FlSeg { int H, W, off, s4, pw; };

struct FlParams {
    const int* labels;
    int* map[FL_MAX_DEPTH];
    int A, ppi, nseg, depths, pi4, tot4;
    FlSeg seg[BD_MAX_SEGS];
};

__global__ __launch_bounds__(1024) void fwd_live_kernel(const FlParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fl_bm[];      // [2][H * W]
    __shared__ int slast;
    __shared__ int wsum[16];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / p.nseg, s = blockIdx.x - n * p.nseg;
    const int H = p.seg[s].H, W = p.seg[s].W, HW = H * W, pwn = p.seg[s].pw;
    const int npatch = ((H + 3) >> 2) * pwn;
    unsigned char* cur = fl_bm;
    unsigned char* nxt = fl_bm + HW;
    for (int i = tid; i < HW; i += 1024) cur[i] = 0;
    __syncthreads();
    const int* lab = p.labels + ((long long)n * p.ppi + p.seg[s].off) * p.A;
    for (int i = tid; i < HW * p.A; i += 1024)
        if (lab[i] > 0) cur[i / p.A] = 1;                    // (several anchors of a pixel may store the same 1)
    __syncthreads();
    for (int k = 0; k < p.depths; ++k) {
        for (int i = tid; i < HW; i += 1024) {
            const int y = i / W, x = i - y * W;
            const int y0 = y > 0 ? y - 1 : 0, y1 = y + 1 < H ? y + 1 : H - 1, x0 = x > 0 ? x - 1 : 0, x1 = x + 1 < W ? x + 1 : W - 1;
            int v = 0;
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx) v |= cur[yy * W + xx];
            nxt[i] = (unsigned char)v;
        }
        __syncthreads();
        int* live = p.map[k] + FL_HDR + n * p.pi4 + p.seg[s].s4;
        for (int q = tid; q < npatch; q += 1024) {
            const int by = q / pwn, bx = q - by * pwn;
            const int ye = by * 4 + 4 < H ? by * 4 + 4 : H, xe = bx * 16 + 16 < W ? bx * 16 + 16 : W;
            int v = 0;
            for (int y = by * 4; y < ye; ++y)
                for (int x = bx * 16; x < xe; ++x) v |= nxt[y * W + x];
            live[q] = v;
        }
        unsigned char* t = cur; cur = nxt; nxt = t;
        __syncthreads();
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // every thread's flags are visible device-wide before the workgroup counts as finished
    __syncthreads();
    if (tid == 0) slast = atomicAdd(p.map[0] + 1, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!slast) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // compaction, one depth after the other: each thread takes KP consecutive patches (ascending order: prefix sums over lanes, then waves)
    constexpr int KP = 8;
    const int wv = tid >> 6, ln = tid & 63;
    for (int k = 0; k < p.depths; ++k) {
        int* hdr = p.map[k];
        const int* live = hdr + FL_HDR;
        const int to = (hdr[0] & 1) ^ 1;
        int* list = hdr + FL_HDR + p.tot4 * (1 + to);
        int base = 0;
        for (int c0 = 0; c0 < p.tot4; c0 += 1024 * KP) {
            int lv[KP];
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                const int q = c0 + tid * KP + j;
                lv[j] = q < p.tot4 ? (__hip_atomic_load(live + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) : 0;
                cnt += lv[j];
            }
            int inc = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(inc, o, 64);
                if (ln >= o) inc += y;
            }
            if (ln == 63) wsum[wv] = inc;
            __syncthreads();
            int off = base + inc - cnt, tot = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                off += w < wv ? wsum[w] : 0;
                tot += wsum[w];
            }
#pragma unroll
            for (int j = 0; j < KP; ++j)
                if (lv[j]) list[off++] = c0 + tid * KP + j;
            base += tot;
            __syncthreads();
        }
        if (tid == 0) { hdr[2 + to] = base; hdr[0] = to; }
    }
    if (tid == 0) p.map[0][1] = 0;
}

// side 0: the geometry of g (the conv's output levels), side 1: of dx (its input levels)
GsParams gs_params(const bd_conv_desc* d, int ph, int pw, int side = 0) {
    GsParams p{};
    p.C = side ? d->Cin : d->Cout; p.ppi = side ? d->in_pix_per_img : d->out_pix_per_img; p.ph = ph; p.pw_px = pw; p.nseg = d->nseg;
    int ps = 0;
    for (int s = 0; s < d->nseg; ++s) {
        GsSeg& sg = p.seg[s];
        const int H = side ? d->Hi[s] : d->Ho[s], W = side ? d->Wi[s] : d->Wo[s];
        sg.patch_start = ps; sg.H = H; sg.W = W; sg.pw = cdiv(W, pw); sg.off = side ? d->in_off[s] : d->out_off[s];
        ps += cdiv(H, ph) * sg.pw;
    }
    p.patches_per_img = ps;
    p.total = ps * d->N;
    return p;
}

}  // namespace

// patches of g (the conv's output levels) in ph x pw tiles, all images
int bd_gskip_patches(const bd_conv_desc* d, int ph, int pw) {
    return gs_params(d, ph, pw).total;
}

// mask[patch] (bd_gskip_patches ints): nonzero iff g has a nonzero bit in that patch (GS_* bits: see above)
void bd_gskip_scan(const bd_conv_desc* d, const void* g, int ph, int pw, int* mask, hipStream_t stream) {
    GsParams p = gs_params(d, ph, pw);
    p.g = (const bf16_raw*)g; p.mask = mask;
    if (p.total > 0) hipLaunchKernelGGL(gskip_scan_kernel, dim3(p.total), dim3(256), 0, stream, p);
}

// data-gradient liveness from bd_gskip_scan's masks: live[q], list[0 .. *count) ascending
void bd_gskip_compact(const bd_conv_desc* d, int ph, int pw, const int* mask, int* live, int* list, int* count, hipStream_t stream) {
    GsParams p = gs_params(d, ph, pw);
    p.mask = const_cast<int*>(mask);
    hipLaunchKernelGGL(gskip_compact_kernel, dim3(1), dim3(1024), 0, stream, p, live, list, count);
}

// ---- liveness maps: layout (see gskip_fill_kernel) ----
void bd_gskip_map_layout(const bd_conv_desc* d, int side, BdGskipMap* out) {
    const int p4 = gs_params(d, 4, 16, side).total, p8 = gs_params(d, 8, 8, side).total;
    out->p4 = p4; out->p8 = p8;
    out->m4 = GM_HDR; out->m8 = GM_HDR + p4; out->live = out->m8 + p8; out->list = out->live + p4;
    out->ints = (size_t)GM_HDR + (size_t)4 * p4 + p8;
}

extern "C" size_t bd_conv2d_gskip_map_bytes(const bd_conv_desc* d, int of_dx) {
    if (!d || d->nseg < 1 || d->nseg > BD_MAX_SEGS || !(d->R == 3 && d->S == 3 && d->stride == 1 && d->pad == 1)) return 0;
    BdGskipMap m;
    bd_gskip_map_layout(d, of_dx ? 1 : 0, &m);
    return m.ints * sizeof(int);
}

// the map of the tensor a sparse data gradient just wrote (side 1 of d), from the patches it computed (live_in over dx's 4 x 16 patches)
void bd_gskip_fill(const bd_conv_desc* d, int side, const void* t, const int* live_in, int* map, hipStream_t stream) {
    const GsParams g4 = gs_params(d, 4, 16, side), g8 = gs_params(d, 8, 8, side), gs = gs_params(d, 8, 16, side);
    GmParams p{};
    p.t = (const bf16_raw*)t; p.live_in = live_in; p.map = map;
    p.C = g4.C; p.ppi = g4.ppi; p.nseg = g4.nseg;
    p.pi4 = g4.patches_per_img; p.pi8 = g8.patches_per_img; p.pis = gs.patches_per_img; p.tot4 = g4.total; p.tot8 = g8.total;
    for (int s = 0; s < g4.nseg; ++s)
        p.seg[s] = GmSeg{g4.seg[s].H, g4.seg[s].W, g4.seg[s].off, g4.seg[s].patch_start, g8.seg[s].patch_start, gs.seg[s].patch_start};
    GsParams cp = g4;
    cp.mask = map + GM_HDR;
    const int grid = gs.total < 128 ? gs.total : 128;
    if (grid > 0) hipLaunchKernelGGL(gskip_fill_kernel, dim3(grid), dim3(1024), 0, stream, p, cp, gs.total);
}

// A map of a tensor nobody left a map for (the first gradient of a chain; the reference of the map tests): the full scans in both
// geometries and the one-workgroup compaction, into list 0.  side as above.
extern "C" int bd_gskip_map_scan(const bd_conv_desc* d, int of_dx, const void* t, void* map, size_t map_bytes, bd_stream_t stream) {
    BD_REQUIRE(d && t && map, "gskip_map_scan: null pointer");
    const size_t need = bd_conv2d_gskip_map_bytes(d, of_dx);
    BD_REQUIRE(need > 0, "gskip_map_scan: liveness maps belong to 3x3 / stride 1 / pad 1 descriptors");
    BD_REQUIRE(map_bytes >= need, "gskip_map_scan: map %zu < required %zu bytes", map_bytes, need);
    const int side = of_dx ? 1 : 0;
    BdGskipMap m;
    bd_gskip_map_layout(d, side, &m);
    int* mp = (int*)map;
    if (hipMemsetAsync(mp, 0, GM_HDR * sizeof(int), (hipStream_t)stream) != hipSuccess) { bd_set_error("gskip_map_scan: memset failed"); return BD_ELAUNCH; }
    GsParams p4 = gs_params(d, 4, 16, side), p8 = gs_params(d, 8, 8, side);
    p4.g = p8.g = (const bf16_raw*)t;
    p4.mask = mp + m.m4; p8.mask = mp + m.m8;
    if (p4.total > 0) {
        hipLaunchKernelGGL(gskip_scan_kernel, dim3(p4.total), dim3(256), 0, (hipStream_t)stream, p4);
        hipLaunchKernelGGL(gskip_scan_kernel, dim3(p8.total), dim3(256), 0, (hipStream_t)stream, p8);
    }
    hipLaunchKernelGGL(gskip_compact_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, p4, mp + m.live, mp + m.list, mp + 2);
    BD_CHECK_LAUNCH("bd_gskip_map_scan");
    return BD_OK;
}

// ---- forward liveness: layout and launch (see fwd_live_kernel) ----
void bd_fwd_map_layout(const bd_conv_desc* d, BdFwdMap* out) {
    const int p4 = gs_params(d, 4, 16, 0).total;
    out->p4 = p4; out->live = FL_HDR; out->list = FL_HDR + p4;
    out->ints = (size_t)FL_HDR + (size_t)3 * p4;
}

extern "C" size_t bd_fwd_live_map_bytes(const bd_conv_desc* d) {
    if (!d || d->nseg < 1 || d->nseg > BD_MAX_SEGS || !(d->R == 3 && d->S == 3 && d->stride == 1 && d->pad == 1)) return 0;
    BdFwdMap m;
    bd_fwd_map_layout(d, &m);
    return m.ints * sizeof(int);
}

extern "C" int bd_fwd_live_maps(const bd_conv_desc* d, const int32_t* labels, int A, int depths, void* const* maps, size_t map_bytes,
                                int reset, bd_stream_t stream) {
    BD_REQUIRE(d && labels && maps, "fwd_live_maps: null pointer");
    const size_t need = bd_fwd_live_map_bytes(d);
    BD_REQUIRE(need > 0, "fwd_live_maps: forward liveness maps belong to 3x3 / stride 1 / pad 1 descriptors");
    BD_REQUIRE(A >= 1 && depths >= 1 && depths <= FL_MAX_DEPTH, "fwd_live_maps: A=%d depths=%d (1 .. %d)", A, depths, (int)FL_MAX_DEPTH);
    BD_REQUIRE(map_bytes >= need, "fwd_live_maps: map %zu < required %zu bytes", map_bytes, need);
    const GsParams g4 = gs_params(d, 4, 16, 0);
    FlParams p{};
    p.labels = labels; p.A = A; p.ppi = g4.ppi; p.nseg = g4.nseg; p.depths = depths; p.pi4 = g4.patches_per_img; p.tot4 = g4.total;
    size_t lds = 0;
    for (int s = 0; s < g4.nseg; ++s) {
        BD_REQUIRE(d->Hi[s] == d->Ho[s] && d->Wi[s] == d->Wo[s], "fwd_live_maps: level %d changes size", s);
        p.seg[s] = FlSeg{g4.seg[s].H, g4.seg[s].W, g4.seg[s].off, g4.seg[s].patch_start, g4.seg[s].pw};
        const size_t b = (size_t)2 * g4.seg[s].H * g4.seg[s].W;
        BD_REQUIRE((long long)g4.seg[s].H * g4.seg[s].W * A < 0x7fffffffll, "fwd_live_maps: level %d too large", s);
        lds = b > lds ? b : lds;
    }
    BD_REQUIRE(lds <= 160 * 1024 - 256, "fwd_live_maps: a level of %zu pixels does not fit the LDS bitmap", lds / 2);
    for (int k = 0; k < depths; ++k) {
        BD_REQUIRE(maps[k], "fwd_live_maps: null map %d", k);
        p.map[k] = (int*)maps[k];
        // reset: the maps hold no usable state (new or re-bound memory) -- list 0 current and both lists empty before the launch
        if (reset && hipMemsetAsync(maps[k], 0, FL_HDR * sizeof(int), (hipStream_t)stream) != hipSuccess) {
            bd_set_error("fwd_live_maps: memset failed");
            return BD_ELAUNCH;
        }
    }
    if (d->N < 1 || g4.total < 1) return BD_OK;
    BD_ONCE_PER_DEVICE((void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_live_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 160 * 1024 - 256));
    hipLaunchKernelGGL(fwd_live_kernel, dim3(d->N * g4.nseg), dim3(1024), lds, (hipStream_t)stream, p);
    BD_CHECK_LAUNCH("bd_fwd_live_maps");
    return BD_OK;
}
