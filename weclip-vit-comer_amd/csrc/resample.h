// Resampling arithmetic shared by every kernel file that resizes something, defined once:
//   ATen bilinear      : half-pixel source index, four-tap lerp, first-maximum arg-max over classes
//   Pillow 8-bit       : precompute_coeffs + normalize_coeffs_8bpc tables, the two-pass tap gather
//   confusion histogram: the "zero LDS cells, count in LDS or global, flush once per workgroup" skeleton
// Everything is __forceinline__ arithmetic: with -ffp-contract=off every includer computes the same bits, which is what the
// equalities of tests/test_eval_finish_gpu.py, test_trainlog_gpu.py and test_seg_augment_gpu.py rely on.
#pragma once
#include "common.h"

// ---- ATen bilinear -----------------------------------------------------------------------------------------------
// taps and weight of source coordinate s >= 0 on an axis of `in` samples: the second tap is clamped to the last sample
__device__ __forceinline__ void wc_bil_taps(float s, int in, int& i0, int& i1, float& l1) {
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - i0;
}

// ATen's area_pixel_compute_source_index with align_corners=False (= OpenCV's INTER_LINEAR for float data): `scale` is in / out for
// size= calls and 1 / scale_factor for scale_factor= calls
__device__ __forceinline__ void wc_bil_src(int d, int in, float scale, int& i0, int& i1, float& l1) {
    wc_bil_taps(fmaxf(scale * (d + 0.5f) - 0.5f, 0.f), in, i0, i1, l1);
}

// align_corners=True: scale = (in - 1) / (out - 1)
__device__ __forceinline__ void wc_bil_src_aligned(int d, int in, float scale, int& i0, int& i1, float& l1) {
    wc_bil_taps(scale * d, in, i0, i1, l1);
}

// a, b = taps (y0, x0), (y0, x1); c, d = taps (y1, x0), (y1, x1)
__device__ __forceinline__ float wc_lerp4(float a, float b, float c, float d, float ly, float lx) {
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * a + lx * b) + ly * (hx * c + lx * d);
}

__device__ __forceinline__ float wc_bilerp(const float* __restrict__ S, int Ws, int y0, int y1, int x0, int x1, float ly, float lx) {
    return wc_lerp4(S[(long)y0 * Ws + x0], S[(long)y0 * Ws + x1], S[(long)y1 * Ws + x0], S[(long)y1 * Ws + x1], ly, lx);
}

// argmax_c bilinear(seg (C, Hs, Ws))[c] at one destination pixel; the first maximum wins, like torch.argmax on the CPU
__device__ __forceinline__ int wc_resize_argmax_at(const float* __restrict__ seg, int C, int Hs, int Ws, int y0, int y1, int x0, int x1,
                                                   float ly, float lx) {
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
        const float v = wc_bilerp(seg + (long)c * Hs * Ws, Ws, y0, y1, x0, x1, ly, lx);
        if (v > best) { best = v; arg = c; }
    }
    return arg;
}

// X pass of the separable bilinear backward (csrc/losses.hip, seg_bwd_x2_kernel): grad (rows, w) from the row passes' tmpA (rows, W)
// + tmpB (rows, W; the first of every h rows is not read), every output's window summed in ascending x.  W <= 8192 (LDS).
int wc_bilinear_bwd_x(const float* tmpA, const float* tmpB, float* grad, long rows, int h, int w, int W, void* stream);

// ---- Pillow ImagingResample, 8 bits per channel ------------------------------------------------------------------
#define PIL_PREC 22                      // Pillow: PRECISION_BITS = 32 - 8 - 2
#define PIL_ENT(KMAX) ((KMAX) + 3)       // ints per table entry: first tap, tap count, KMAX fixed-point weights, pad
#define AUG_KMAX 9                       // triangle tables of both training augmentations: 2 * ceil(support) + 1 with support <= 4,
#define AUG_ENT PIL_ENT(AUG_KMAX)        // i.e. down-scaling by at most 4; 12 ints (48 B) per entry

__device__ __forceinline__ int pil_clip8(int v) {
    v >>= PIL_PREC;                      // arithmetic shift: a negative sum clips to 0
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct PilTriangle {                     // Image.BILINEAR
    static constexpr double SUPPORT = 1.0;
    static __device__ __forceinline__ double weight(double x) {
        x = x < 0.0 ? -x : x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
};

struct PilBicubic {                      // Image.BICUBIC (a = -0.5)
    static constexpr double SUPPORT = 2.0;
    static __device__ __forceinline__ double weight(double x) {
        const double a = -0.5;
        x = x < 0.0 ? -x : x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
};

// precompute_coeffs(inSize, in0 = 0, in1 = inSize, outSize, FILTER) + normalize_coeffs_8bpc for output coordinate r, in double
// precision and Pillow's operation order.  Writes e[0 .. PIL_ENT(KMAX)) with the tap count capped at KMAX and returns the
// uncapped count: what becomes of a window that does not fit (poison, or "the host refused the shape") is the caller's policy.
// KMAX = 2 * ceil(SUPPORT * max down-scaling) + 1.
template <class FILTER, int KMAX>
__device__ __forceinline__ int pil_coeffs(int r, int in_size, int out_size, int* __restrict__ e) {
    const double scale = (double)((float)in_size - 0.f) / out_size;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = FILTER::SUPPORT * fscale;
    const double center = 0.0 + (r + 0.5) * scale;
    const double ss = 1.0 / fscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin, nt = n > KMAX ? KMAX : n;
    // The results do not depend on SHORT; it only keeps the code the two table widths had before they shared this routine, because
    // the coefficient launch is latency-bound and sits in front of every batch (the augmentation chain measured 0.6 us slower with
    // one branchy form for both).  A short table (triangle, 9 taps) is fully unrolled and evaluates all KMAX weights branch-free, so
    // the second loop reuses the first loop's weights from registers; a long one (bicubic, 33 taps) stays rolled, sums only its
    // window and skips the filter beyond it.
    constexpr bool SHORT = KMAX <= 16;
    constexpr int UNROLL = SHORT ? KMAX : 1;
    const auto weight = [&](int x) {
        if (!SHORT && x >= nt) return 0.0;
        const double w = FILTER::weight(((double)(x + xmin) - center + 0.5) * ss);
        return x < nt ? w : 0.0;
    };
    double ww = 0.0;
#pragma unroll UNROLL
    for (int x = 0; x < (SHORT ? KMAX : nt); ++x) ww += weight(x);
    e[0] = xmin;
    e[1] = nt;
#pragma unroll UNROLL
    for (int x = 0; x < KMAX; ++x) {
        double v = weight(x);
        if (ww != 0.0) v = v / ww;
        e[2 + x] = (int)((v < 0.0 ? -0.5 : 0.5) + v * (double)(1 << PIL_PREC));   // round half away from zero
    }
    e[2 + KMAX] = 0;
    return n;
}

// The two passes at one output pixel of a 3-channel uint8 HWC image (row pitch Ws pixels) from its row entry ey and its column entry
// ex: the horizontal pass of each source row is rounded to uint8, the vertical pass runs over those values.
// Returns 0: canvas padding (either axis outside the rescaled image, whatever the other axis' entry says), -1: poisoned entry,
// 1: c0..c2 hold the uint8-valued result.
__device__ __forceinline__ int pil_gather_rgb8(const int* __restrict__ ey, const int* __restrict__ ex, const unsigned char* __restrict__ src,
                                               int Ws, int& c0, int& c1, int& c2) {
    const int ymin = ey[0], ny = ey[1], xmin = ex[0], nx = ex[1];
    if (ny == 0 || nx == 0) return 0;
    if (ny < 0 || nx < 0) return -1;
    const unsigned char* S = src + ((long)ymin * Ws + xmin) * 3;
    int a0 = 1 << (PIL_PREC - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < ny; ++j) {
        const unsigned char* row = S + (long)j * Ws * 3;
        int h0 = 1 << (PIL_PREC - 1), h1 = h0, h2 = h0;                    // horizontal pass of source row ymin + j
        for (int i = 0; i < nx; ++i) {
            const int kx = ex[2 + i];
            h0 += kx * row[3 * i];
            h1 += kx * row[3 * i + 1];
            h2 += kx * row[3 * i + 2];
        }
        const int ky = ey[2 + j];                                          // vertical pass over the uint8-rounded rows
        a0 += ky * pil_clip8(h0);
        a1 += ky * pil_clip8(h1);
        a2 += ky * pil_clip8(h2);
    }
    c0 = pil_clip8(a0);
    c1 = pil_clip8(a1);
    c2 = pil_clip8(a2);
    return 1;
}

// ---- confusion histogram: 32-bit LDS cells per workgroup, 64-bit global cells -------------------------------------
__device__ __forceinline__ void wc_hist_zero(unsigned int* sh, int n) {
    for (int i = threadIdx.x; i < n; i += 256) sh[i] = 0;
    __syncthreads();
}

// one count: LDS cell when sh != NULL, else straight global atomic
__device__ __forceinline__ void wc_hist_count(unsigned int* sh, unsigned long long* hist, int cell) {
    if (sh) atomicAdd(&sh[cell], 1u);
    else atomicAdd(&hist[cell], 1ull);
}

// non-zero LDS cells -> one global atomic each; the counting must be behind a barrier (wc_hist_flush adds it)
__device__ __forceinline__ void wc_hist_flush_cells(const unsigned int* sh, unsigned long long* hist, int n) {
    for (int i = threadIdx.x; i < n; i += 256)
        if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}
__device__ __forceinline__ void wc_hist_flush(const unsigned int* sh, unsigned long long* hist, int n) {
    __syncthreads();
    wc_hist_flush_cells(sh, hist, n);
}

// about per_thread items per thread of 256, at most 1024 workgroups: long-lived workgroups make an LDS histogram worth its flush
// (a workgroup then counts n / 1024 items: 32-bit cells hold 2^42 of them)
static inline unsigned wc_hist_blocks(long items, int per_thread) {
    const long per_block = 256L * per_thread;
    long blocks = (items + per_block - 1) / per_block;
    if (blocks > 1024) blocks = 1024;
    return (unsigned)blocks;
}
