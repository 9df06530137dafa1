// The dense energy loss as a term of the training step: everything around the all-pairs filter of csrc/energy.hip, from the
// low-resolution head output (N, K, h, w) to a low-resolution gradient, without a full-resolution (N, K, H, W) tensor and
// without a host read.  The composition is the reference's get_energy_loss (utils/losses.py:35-50)
// on F.interpolate(seg, (H, W), bilinear, align_corners=False) followed by DenseEnergyLoss.forward (:102-111) at
// scale_factor = 2^-e, e in {0, 1, 2}.  For these factors ATen's source coordinates are exact:
//   nearest  : scaled pixel d reads full-resolution pixel d << e;
//   bilinear : scaled pixel d reads the two pixels around (d + 0.5) 2^e - 0.5, i.e. (d << e) + 2^(e-1) - 1 and the next one,
//              each with weight 1/2 (e = 0: pixel d with weight 1);
//   Hs = H >> e, Ws = W >> e.
//
//   energy_term_fwd_kernel<DOWN> : one thread per scaled pixel: the de-normalised image, the ROI from the device box rows, the
//                                  unlabelled mask (nearest sources), and P_s = the down-sample of soft-max_k of the up-sampled
//                                  logits: 1 (e = 0) or 2 x 2 (DOWN) full-resolution pixels, each interpolated from 2 x 2
//                                  low-resolution ones (resample.h).  Three sweeps over the classes, EP_G classes' loads at a
//                                  time: maximum, sum of exponentials, probabilities (soft-max as torch forms it).
//   energy_term_bwd_kernel       : the transposes, in the separable shape of ce_loss_fused_kernel (csrc/losses.hip).  Thread
//                                  (x, ys): the full-resolution pixels of column x whose upper source row is ys.  A pixel is
//                                  tapped by at most one scaled pixel (Y, X), with weight wd in {1, 1/4}:
//                                  g_k = wd * (coef * A_k) * ROI, p = soft-max recomputed, g_z(k) = p_k (g_k - sum_j p_j g_j);
//                                  g_z goes to row ys with weight 1 - ly (tmpA) and to row ys + 1 with ly (tmpB).  Classes in
//                                  register chunks of EP_CH per workgroup; the pixel's maximum, sum and sum_j p_j g_j come
//                                  from one online sweep over all classes from memory.
//   X pass                       : seg_bwd_x2_kernel of csrc/losses.hip (wc_bilinear_bwd_x): every low-resolution column sums
//                                  its window of tmpA + tmpB in ascending x.
// No atomics; every sum has a fixed order: two calls give the same bits.
#include "common.h"
#include "resample.h"

#define EP_MAX_K 128
#define EP_MAX_HW (640 * 640)     // the filter's limit on the scaled size (csrc/energy.hip)
#define EP_CH 32                  // classes per register chunk of the backward pixel pass
#define EP_G 4                    // classes whose loads are issued together

// offsets of the 2 x 2 low-resolution taps of one full-resolution pixel inside a class plane, and its two weights
struct EpTap {
    int o00, o01, o10, o11;
    float ly, lx;
};

__device__ __forceinline__ EpTap ep_tap(int fy, int fx, int h, int w, float sy, float sx) {
    int y0, y1, x0, x1;
    EpTap t;
    wc_bil_src(fy, h, sy, y0, y1, t.ly);
    wc_bil_src(fx, w, sx, x0, x1, t.lx);
    t.o00 = y0 * w + x0, t.o01 = y0 * w + x1, t.o10 = y1 * w + x0, t.o11 = y1 * w + x1;
    return t;
}

__device__ __forceinline__ float ep_logit(const float* __restrict__ Sc, const EpTap& t) {
    return wc_lerp4(Sc[t.o00], Sc[t.o01], Sc[t.o10], Sc[t.o11], t.ly, t.lx);
}

struct EpNorm {
    float mean[3], std[3];
};

template <bool DOWN>
__global__ __launch_bounds__(256) void energy_term_fwd_kernel(const float* __restrict__ img, const float* __restrict__ seg,
                                                               const long* __restrict__ label, const int* __restrict__ box,
                                                               float* __restrict__ images_s, float* __restrict__ P_s,
                                                               float* __restrict__ rois_s, uint8_t* __restrict__ unl, EpNorm nm,
                                                               int K, int h, int w, int H, int W, int Hs, int Ws, int e, float sy,
                                                               float sx) {
    constexpr int NT = DOWN ? 4 : 1;
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (X >= Ws || Y >= Hs) return;                        // (no barrier below)
    const int Yn = Y << e, Xn = X << e;                    // nearest source
    const long HW = (long)H * W, HWs = (long)Hs * Ws, so = (long)Y * Ws + X;
    const long fo = (long)Yn * W + Xn;
    const float c0 = img[(long)n * 3 * HW + fo], c1 = img[((long)n * 3 + 1) * HW + fo], c2 = img[((long)n * 3 + 2) * HW + fo];
    const long lab = label[(long)n * HW + fo];
    // img * std + mean as two separately rounded operations (torch's two eager ops)
    images_s[(long)n * 3 * HWs + so] = __fadd_rn(__fmul_rn(c0, nm.std[0]), nm.mean[0]);
    images_s[((long)n * 3 + 1) * HWs + so] = __fadd_rn(__fmul_rn(c1, nm.std[1]), nm.mean[1]);
    images_s[((long)n * 3 + 2) * HWs + so] = __fadd_rn(__fmul_rn(c2, nm.std[2]), nm.mean[2]);
    unl[(long)n * HWs + so] = (lab & 255) == 255 ? 1 : 0;
    bool in = true;
    if (box) {
        const int4 b = *reinterpret_cast<const int4*>(box + 4 * n);     // (y0, y1, x0, x1)
        in = Yn >= b.x && Yn < b.y && Xn >= b.z && Xn < b.w;
    }
    rois_s[(long)n * HWs + so] = in ? 1.f : 0.f;

    const int off = DOWN ? (1 << (e - 1)) - 1 : 0;
    EpTap tap[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tap[t] = ep_tap(Yn + off + (t >> 1), Xn + off + (t & 1), h, w, sy, sx);
    const float* S = seg + (long)n * K * h * w;
    const int hw = h * w;
    float mx[NT], sum[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) mx[t] = -INFINITY, sum[t] = 0.f;
    for (int k0 = 0; k0 < K; k0 += EP_G)                   // (a class past K re-reads class K - 1: the maximum is unchanged)
#pragma unroll
        for (int u = 0; u < EP_G; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) mx[t] = fmaxf(mx[t], ep_logit(S + (long)min(k0 + u, K - 1) * hw, tap[t]));
    for (int k0 = 0; k0 < K; k0 += EP_G)
#pragma unroll
        for (int u = 0; u < EP_G; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float ex = __expf(ep_logit(S + (long)min(k0 + u, K - 1) * hw, tap[t]) - mx[t]);
                sum[t] += k0 + u < K ? ex : 0.f;
            }
    float* Pn = P_s + (long)n * K * HWs + so;
    for (int k0 = 0; k0 < K; k0 += EP_G)
#pragma unroll
        for (int u = 0; u < EP_G; ++u) {
            float p[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) p[t] = __expf(ep_logit(S + (long)min(k0 + u, K - 1) * hw, tap[t]) - mx[t]) / sum[t];
            float out = p[0];
            if constexpr (DOWN) out = wc_lerp4(p[0], p[1], p[2], p[3], 0.5f, 0.5f);
            if (k0 + u < K) Pn[(long)(k0 + u) * HWs] = out;
        }
}

// the scaled pixel that taps full-resolution coordinate f on an axis of `ns` scaled pixels: -1 when none does
__device__ __forceinline__ int ep_tapped_by(int f, int e, int ns) {
    if (e == 0) return f;
    const int r = f - ((1 << (e - 1)) - 1);
    return (r >= 0 && (r & ((1 << e) - 1)) < 2 && (r >> e) < ns) ? r >> e : -1;
}

__global__ __launch_bounds__(256) void energy_term_bwd_kernel(const float* __restrict__ A, const float* __restrict__ roi,
                                                               const float* __restrict__ seg, float* __restrict__ tmpA,
                                                               float* __restrict__ tmpB, float coef, int K, int nchunk, int h, int w,
                                                               int H, int W, int Hs, int Ws, int e, float sy, float sx) {
    constexpr int CH = EP_CH;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), ys = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z / nchunk, ck = blockIdx.z - n * nchunk, c0 = ck * CH;
    if (x >= W || ys >= h) return;                         // (no barrier below)
    int x0, x1;
    float lx;
    wc_bil_src(x, w, sx, x0, x1, lx);
    const int y1s = ys + (ys < h - 1 ? 1 : 0);
    const float* S = seg + (long)n * K * h * w;
    const long r0 = (long)ys * w, r1 = (long)y1s * w, hw = (long)h * w, HWs = (long)Hs * Ws;
    float av[CH], dv[CH], accT[CH], accB[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        accT[c] = accB[c] = 0.f;
        const float* Sc = S + (long)min(c0 + c, K - 1) * hw;          // clamped class: no branch around the loads
        const float a = (1.f - lx) * Sc[r0 + x0] + lx * Sc[r0 + x1];
        const float bb = (1.f - lx) * Sc[r1 + x0] + lx * Sc[r1 + x1];
        av[c] = a;
        dv[c] = bb - a;
    }
    const int Xt = ep_tapped_by(x, e, Ws), X = max(Xt, 0);           // an untapped column weighs 0 and reads column 0
    const float wd1 = e ? 0.5f : 1.f, gx = Xt >= 0 ? wd1 : 0.f;
    const float iy = 1.0f / sy;
    int y_lo = ys == 0 ? 0 : (int)floorf((ys + 0.5f) * iy - 0.5f) - 1;
    int y_hi = ys == h - 1 ? H - 1 : (int)ceilf((ys + 1.5f) * iy - 0.5f) + 1;
    if (y_lo < 0) y_lo = 0;
    if (y_hi > H - 1) y_hi = H - 1;
    for (int y = y_lo; y <= y_hi; ++y) {
        int y0, y1;
        float ly;
        wc_bil_src(y, h, sy, y0, y1, ly);
        const int Y = ep_tapped_by(y, e, Hs);
        if (y0 != ys || Y < 0) continue;                   // wave-uniform
        const float gw = gx * wd1;
        const long po = ((long)n * Hs + Y) * Ws + X;
        const float* An = A + ((long)n * K * Hs + Y) * Ws + X;
        const float r = roi[po];
        // one online sweep over all K classes: maximum, sum of exponentials, sum_j exp_j g_j
        float mx = -INFINITY, sum = 0.f, dot = 0.f;
        for (int cb = 0; cb < K; cb += EP_G) {
            float zz[EP_G], gg[EP_G];
#pragma unroll
            for (int u = 0; u < EP_G; ++u) {
                const int k = min(cb + u, K - 1);
                const float* Sc = S + (long)k * hw;
                const float a = (1.f - lx) * Sc[r0 + x0] + lx * Sc[r0 + x1];
                const float bb = (1.f - lx) * Sc[r1 + x0] + lx * Sc[r1 + x1];
                zz[u] = cb + u < K ? fmaf(ly, bb - a, a) : -INFINITY;
                gg[u] = gw * ((coef * An[(long)k * HWs]) * r);
            }
            float m8 = mx;
#pragma unroll
            for (int u = 0; u < EP_G; ++u) m8 = fmaxf(m8, zz[u]);
            float s8 = 0.f, d8 = 0.f;
#pragma unroll
            for (int u = 0; u < EP_G; ++u) {
                const float ex = __expf(zz[u] - m8);       // class past K: exp(-inf) = 0
                s8 += ex;
                d8 = fmaf(ex, gg[u], d8);
            }
            const float f = __expf(mx - m8);
            sum = sum * f + s8;
            dot = dot * f + d8;
            mx = m8;
        }
        const float sbar = dot / sum, inv = 1.0f / sum;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float z = c0 + c < K ? fmaf(ly, dv[c], av[c]) : -INFINITY;       // the sweep's bits: z <= mx
            const float g = gw * ((coef * An[(long)min(c0 + c, K - 1) * HWs]) * r);
            const float gz = (__expf(z - mx) * inv) * (g - sbar);
            accT[c] += gz;
            accB[c] = fmaf(ly, gz, accB[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (c0 + c < K) {
            const long o = (((long)n * K + c0 + c) * h) * W + x;
            if (y1s == ys) tmpA[o + (long)ys * W] = accT[c];                   // last row: both weights land on it
            else {
                tmpA[o + (long)ys * W] = accT[c] - accB[c];
                tmpB[o + (long)y1s * W] = accB[c];
            }
        }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

struct EpPlan {
    int Hs, Ws, nchunk;
};

int ep_plan(EpPlan& p, int N, int K, int h, int w, int H, int W, int e, const char* who) {
    WC_CHECK_ARG(K >= 1 && K <= EP_MAX_K, "%s: bad argument: K = %d outside [1, %d]", who, K, EP_MAX_K);
    WC_CHECK_ARG(e >= 0 && e <= 2, "%s: bad argument: e = %d outside [0, 2] (scale_factor = 2^-e)", who, e);
    WC_CHECK_ARG(h >= 1 && w >= 1 && (long)h * w <= (1L << 24) && H >= 1 && W >= 1 && W <= 8192,
                 "%s: bad argument: h x w = %d x %d, H x W = %d x %d (W <= 8192)", who, h, w, H, W);
    p.Hs = H >> e, p.Ws = W >> e;
    WC_CHECK_ARG(p.Hs >= 1 && p.Ws >= 1 && (long)p.Hs * p.Ws <= EP_MAX_HW,
                 "%s: bad argument: scaled size %d x %d outside [1, 640*640] pixels", who, p.Hs, p.Ws);
    WC_CHECK_ARG(h <= 4 * 65535 && p.Hs <= 4 * 65535, "%s: bad argument: more than %d rows", who, 4 * 65535);   // a grid dimension
    p.nchunk = (K + EP_CH - 1) / EP_CH;
    WC_CHECK_ARG(N >= 1 && (long)N * p.nchunk <= 65535, "%s: bad argument: N = %d outside [1, %d]", who, N, 65535 / p.nchunk);
    return WC_OK;
}

}  // namespace

extern "C" int wc_energy_prep_fwd(const float* img, const float* seg, const int64_t* label, const int* img_box, const float* mean,
                                  const float* std, float* images_s, float* P_s, float* rois_s, void* unlabel_u8, int N, int K, int h,
                                  int w, int H, int W, int e, void* stream) {
    WC_CHECK_ARG(img && seg && label && mean && std && images_s && P_s && rois_s && unlabel_u8,
                 "wc_energy_prep_fwd: bad argument: null pointer");
    EpPlan p;
    if (int rc = ep_plan(p, N, K, h, w, H, W, e, "wc_energy_prep_fwd")) return rc;
    WC_CHECK_ARG((uintptr_t)img_box % 16 == 0 && (uintptr_t)label % 8 == 0, "wc_energy_prep_fwd: bad argument: misaligned pointer");
    EpNorm nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.std[c] = std[c];
    const dim3 grid(wc_cdiv(p.Ws, 64), wc_cdiv(p.Hs, 4), N);
    const float sy = (float)h / H, sx = (float)w / W;
    const auto k = e ? energy_term_fwd_kernel<true> : energy_term_fwd_kernel<false>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, (hipStream_t)stream, img, seg, (const long*)label, img_box, images_s, P_s, rois_s,
                       (uint8_t*)unlabel_u8, nm, K, h, w, H, W, p.Hs, p.Ws, e, sy, sx);
    WC_LAUNCH_CHECK("energy_term_fwd_kernel");
    return WC_OK;
}

extern "C" int wc_energy_prep_workspace_floats(int N, int K, int h, int W, long* n_floats) {
    WC_CHECK_ARG(n_floats, "wc_energy_prep_workspace_floats: bad argument: null pointer");
    WC_CHECK_ARG(N >= 1 && K >= 1 && K <= EP_MAX_K && h >= 1 && W >= 1, "wc_energy_prep_workspace_floats: bad argument: N, K, h, W = %d, %d, %d, %d",
                 N, K, h, W);
    *n_floats = 2L * N * K * h * W;
    return WC_OK;
}

extern "C" int wc_energy_prep_bwd(const float* A, const float* rois_s, const float* seg, float* grad_seg, void* ws, float coef, int N,
                                  int K, int h, int w, int H, int W, int e, void* stream) {
    WC_CHECK_ARG(A && rois_s && seg && grad_seg && ws, "wc_energy_prep_bwd: bad argument: null pointer");
    EpPlan p;
    if (int rc = ep_plan(p, N, K, h, w, H, W, e, "wc_energy_prep_bwd")) return rc;
    WC_CHECK_ARG(coef == coef && coef - coef == 0.f, "wc_energy_prep_bwd: bad argument: coef must be finite");
    hipStream_t st = (hipStream_t)stream;
    float* tmpA = (float*)ws;
    float* tmpB = tmpA + (long)N * K * h * W;
    const float sy = (float)h / H, sx = (float)w / W;
    hipLaunchKernelGGL(energy_term_bwd_kernel, dim3(wc_cdiv(W, 64), wc_cdiv(h, 4), N * p.nchunk), dim3(256), 0, st, A, rois_s, seg, tmpA,
                       tmpB, coef, K, p.nchunk, h, w, H, W, p.Hs, p.Ws, e, sy, sx);
    WC_LAUNCH_CHECK("energy_term_bwd_kernel");
    return wc_bilinear_bwd_x(tmpA, tmpB, grad_seg, (long)N * K * h, h, w, W, stream);
}
