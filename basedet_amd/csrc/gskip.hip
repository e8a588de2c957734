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
__global__ __launch_bounds__(1024) void gskip_compact_kernel(const GsParams p, int* live, int* list, int* count) {
    constexpr int KP = 8;
    __shared__ int wsum[16];
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
                int v = m[by * pwn + bx] & GS_ANY;
                if (up) v |= m[(by - 1) * pwn + bx] & GS_BOT;
                if (dn) v |= m[(by + 1) * pwn + bx] & GS_TOP;
                if (lf) v |= m[by * pwn + bx - 1] & GS_RIGHT;
                if (rt) v |= m[by * pwn + bx + 1] & GS_LEFT;
                if (up && lf) v |= m[(by - 1) * pwn + bx - 1] & GS_BR;
                if (up && rt) v |= m[(by - 1) * pwn + bx + 1] & GS_BL;
                if (dn && lf) v |= m[(by + 1) * pwn + bx - 1] & GS_TR;
                if (dn && rt) v |= m[(by + 1) * pwn + bx + 1] & GS_TL;
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

GsParams gs_params(const bd_conv_desc* d, int ph, int pw) {
    GsParams p{};
    p.C = d->Cout; p.ppi = d->out_pix_per_img; p.ph = ph; p.pw_px = pw; p.nseg = d->nseg;
    int ps = 0;
    for (int s = 0; s < d->nseg; ++s) {
        GsSeg& sg = p.seg[s];
        sg.patch_start = ps; sg.H = d->Ho[s]; sg.W = d->Wo[s]; sg.pw = cdiv(d->Wo[s], pw); sg.off = d->out_off[s];
        ps += cdiv(d->Ho[s], ph) * sg.pw;
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
