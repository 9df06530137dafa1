// CAM seeds -> threshold sweep, seed label maps and their scores, on the maps the dumpers leave on the device.
//
// Input of every kernel: the bucket buffer of clip/generate_cams.py, (P, HW) fp16, the pairs (image, class) of an image
// consecutive; first (B+1) int32 = first pair of every image; keys (P) int32 = 0-based foreground class id of every pair (the
// dumpers' first-seen order, not sorted, distinct within an image); gt (B, HW) uint8.
//   per pixel     v = max_k cam[k], c = 1 + the class id attaining it, smallest class id on a tie: the arg-max over the class
//                 axis of the dense `cls_label * cam` of utils/camutils.py:11-14 (the maps are scale_cam_image's, >= 0).  fp16
//                 widens to f32 exactly and every comparison is f32.
//   sweep_kernel  `_fast_hist(gt, where(v > t_j, c, 0), nc)` (utils/camutils.py:13-15 `cam_value <= bkg_score`,
//                 utils/evaluate.py:9-16) for T ascending thresholds at once: with j* = #{j : t_j < v} the pixel is foreground
//                 exactly for j < j*, so it costs ONE increment bins[gt][c][j*] += 1, int64 (nc, nc, T+1).
//   labels_kernel the two slot maps of the per-image body of utils/camutils.py:55-79 (`cam_to_fg_bg_label`) at the image's own
//                 size: slot = 1 + rank of c among the image's ids ascending (:56) where v > thre, else 0.
//   merge_kernel  :77-79 on two slot maps + `pseudo_scores` (utils/evaluate.py:38-45: 255 is dropped) + the coverage counters +
//                 the VOC colour image.
// Integer atomics only: no count depends on order or placement.  Nothing here allocates or reads device memory on the host.
#include "common.h"
#include "resample.h"
#include "voc_colour.h"
#include <limits.h>
#include <math.h>

#define CS_MAXT 64
#define CS_LDS_BYTES (64 * 1024)      // the budget of wc_eval_finish
struct CsThr {
    float t[CS_MAXT];
    float inv;                        // (T - 1) / (t[T-1] - t[0]), 0 for T = 1: the slope of cs_jstar's guess
};

__device__ __forceinline__ float cs_half(unsigned int bits) { return __half2float(__ushort_as_half((unsigned short)bits)); }

// 8 fp16 values from element e of cam.  A pair starts at an odd element when HW is odd, so nothing but 2-byte alignment of
// cam + e is assumed: one 16-byte load when the address allows it, otherwise aligned 32-bit words, shifted by one element when
// the address is 2 mod 4 (that form reads one element BEFORE e and one AFTER e + 7: the caller keeps both inside the buffer).
__device__ __forceinline__ void cs_load8(const unsigned short* __restrict__ cam, long e, float* v) {
    const uintptr_t a = (uintptr_t)(cam + e);
    unsigned int d[4];
    if ((a & 15) == 0) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(a);
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else {
        const unsigned int* w = reinterpret_cast<const unsigned int*>(a & ~(uintptr_t)3);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = w[k];
        if (a & 2) {
            const unsigned int d4 = w[4];
            d[0] = (d[0] >> 16) | (d[1] << 16);
            d[1] = (d[1] >> 16) | (d[2] << 16);
            d[2] = (d[2] >> 16) | (d[3] << 16);
            d[3] = (d[3] >> 16) | (d4 << 16);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = cs_half(d[k] & 0xffffu);
        v[2 * k + 1] = cs_half(d[k] >> 16);
    }
}

// 8 bytes from gt + o (any alignment): aligned words, shifted; reads up to 3 bytes before o and 3 after o + 7
__device__ __forceinline__ void cs_load8_u8(const unsigned char* __restrict__ gt, long o, unsigned int* g) {
    const uintptr_t a = (uintptr_t)(gt + o);
    const unsigned int sh = 8u * (unsigned int)(a & 3);
    const unsigned int* w = reinterpret_cast<const unsigned int*>(a & ~(uintptr_t)3);
    unsigned int lo = w[0], hi = w[1];
    if (sh) {
        const unsigned int top = w[2];
        lo = (lo >> sh) | (hi << (32u - sh));
        hi = (hi >> sh) | (top << (32u - sh));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g[k] = (lo >> (8 * k)) & 255u;
        g[4 + k] = (hi >> (8 * k)) & 255u;
    }
}

// The per-pixel maximum over the K maps of one image for the 8 pixels [i0, i0 + n) of it: best = v, slot = the pair (0..K-1)
// and key = the class id that attain it (smallest class id on a tie).  wide: the 16 pixels from i0 lie inside the image, so the
// shifted loads above stay inside the pair; the last groups of an image are read element by element.
__device__ __forceinline__ void cs_group_max(const unsigned short* __restrict__ cam, const int* __restrict__ keys, int p0, int K,
                                             long HW, long i0, int n, bool wide, float* best, int* slot, int* key) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        best[q] = -INFINITY;
        slot[q] = 0;
        key[q] = INT_MAX;
    }
    for (int k = 0; k < K; ++k) {
        const int kk = keys[p0 + k];
        const long e = (long)(p0 + k) * HW + i0;
        float v[8];
        if (wide) {
            cs_load8(cam, e, v);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = q < n ? cs_half(cam[e + q]) : -INFINITY;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (v[q] > best[q] || (v[q] == best[q] && kk < key[q])) {
                best[q] = v[q];
                slot[q] = k;
                key[q] = kk;
            }
    }
}

__device__ __forceinline__ void cs_group_gt(const unsigned char* __restrict__ gt, long o, int n, bool wide, unsigned int* g) {
    if (wide) {
        cs_load8_u8(gt, o, g);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) g[q] = q < n ? gt[o + q] : 255u;
    }
}

// j* = #{j : st[j] < v} for ascending thresholds st[0..T) in LDS: a guess from the straight line through the first and the last
// threshold (exact up to rounding when they are evenly spaced, as a sweep's are), then stepped up or down until
// st[j-1] < v <= st[j] holds -- which is the count, whatever the spacing and however bad the guess.  A loop over all T thresholds
// costs 2 VALU operations per threshold and pixel and was what the kernel spent its time on beyond T = 4.
__device__ __forceinline__ int cs_jstar(const float* st, int T, float t0, float inv, float v) {
    int j = (int)fminf(fmaxf(fmaf(v - t0, inv, 1.f), 0.f), (float)T);          // NaN -> 0
    while (j < T && st[j] < v) ++j;
    while (j > 0 && !(st[j - 1] < v)) --j;
    return j;
}

// The image's pair range, checked against the buffer: a bad table raises the flag and the workgroup does nothing.
__device__ __forceinline__ bool cs_image(const int* __restrict__ first, int b, int P, int Kmax, int* __restrict__ flag, int& p0,
                                         int& K) {
    p0 = first[b];
    K = first[b + 1] - p0;
    if (p0 < 0 || K < 1 || K > Kmax || p0 + K > P) {
        if (threadIdx.x == 0) *flag = 1;
        return false;
    }
    return true;
}

// Workgroup (x, b): image b, 8-pixel groups x * 256 + thread, grid-stride.  LDS: the thresholds (cs_jstar reads them by a lane's own
// index), then 32-bit cells over (gt, the image's slot, j*), nc * K * (T+1) of them, flushed with one 64-bit global atomic per non-zero cell; otherwise one global atomic per pixel.
// A class id outside [0, nc - 1) raises the flag and is not counted.
template <bool LDS>
__global__ __launch_bounds__(256) void cam_seed_sweep_kernel(const unsigned short* __restrict__ cam, const int* __restrict__ first,
                                                              const int* __restrict__ keys, const unsigned char* __restrict__ gt,
                                                              unsigned long long* __restrict__ bins, int* __restrict__ flag,
                                                              CsThr thr, int P, long HW, int nc, int T, int Kmax) {
    extern __shared__ unsigned int sh[];
    const int b = blockIdx.y, T1 = T + 1;
    int p0, K;
    if (!cs_image(first, b, P, Kmax, flag, p0, K)) return;
    float* st = reinterpret_cast<float*>(sh);                      // the thresholds, then the cells
    unsigned int* cells = sh + CS_MAXT;
    if (threadIdx.x == 0)
        for (int j = 0; j < T; ++j) st[j] = thr.t[j];
    if (LDS) wc_hist_zero(cells, nc * K * T1);
    else __syncthreads();
    const float t0 = thr.t[0], inv = thr.inv;
    const long groups = (HW + 7) >> 3;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long i0 = g * 8;
        const int n = HW - i0 < 8 ? (int)(HW - i0) : 8;
        const bool wide = i0 + 16 <= HW;
        float best[8];
        int slot[8], key[8];
        unsigned int gv[8];
        cs_group_max(cam, keys, p0, K, HW, i0, n, wide, best, slot, key);
        cs_group_gt(gt, (long)b * HW + i0, n, wide, gv);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q >= n || gv[q] >= (unsigned int)nc) continue;
            const int js = cs_jstar(st, T, t0, inv, best[q]);
            if (LDS) {
                atomicAdd(&cells[((int)gv[q] * K + slot[q]) * T1 + js], 1u);
            } else if ((unsigned int)key[q] >= (unsigned int)(nc - 1)) {
                *flag = 1;
            } else {
                atomicAdd(&bins[((long)gv[q] * nc + 1 + key[q]) * T1 + js], 1ull);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        const int per = K * T1;
        for (int i = threadIdx.x; i < nc * per; i += 256) {
            const unsigned int c = cells[i];
            if (!c) continue;
            const int g = i / per, r = i - g * per, s = r / T1, j = r - s * T1;
            const int kk = keys[p0 + s];
            if ((unsigned int)kk >= (unsigned int)(nc - 1)) *flag = 1;
            else atomicAdd(&bins[((long)g * nc + 1 + kk) * T1 + j], (unsigned long long)c);
        }
    }
}

// lab_low / lab_high (B, HW) int64: 1 + rank of the winning class among the image's ids where v > low / high, else 0.
__global__ __launch_bounds__(256) void cam_seed_labels_kernel(const unsigned short* __restrict__ cam, const int* __restrict__ first,
                                                               const int* __restrict__ keys, long* __restrict__ lab_low,
                                                               long* __restrict__ lab_high, int* __restrict__ flag, int P, long HW,
                                                               float low, float high) {
    __shared__ int rank1[256];                                     // 1 + rank of pair k's class id; K <= 255
    const int b = blockIdx.y;
    int p0, K;
    if (!cs_image(first, b, P, 255, flag, p0, K)) return;
    for (int k = threadIdx.x; k < K; k += 256) {
        const int kk = keys[p0 + k];
        int r = 1;
        for (int m = 0; m < K; ++m) r += keys[p0 + m] < kk ? 1 : 0;
        rank1[k] = r;
    }
    __syncthreads();
    const long groups = (HW + 7) >> 3;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long i0 = g * 8;
        const int n = HW - i0 < 8 ? (int)(HW - i0) : 8;
        float best[8];
        int slot[8], key[8];
        cs_group_max(cam, keys, p0, K, HW, i0, n, i0 + 16 <= HW, best, slot, key);
        const long o = (long)b * HW + i0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q >= n) continue;
            const long s = rank1[slot[q]];
            lab_low[o + q] = best[q] > low ? s : 0;
            lab_high[o + q] = best[q] > high ? s : 0;
        }
    }
}

// The merge of utils/camutils.py:77-79 for every image of the bucket, 4 pixels per thread: label = slot_class[b][high], 255
// where high == 0, 0 where high == 0 and low == 0.  A slot outside [0, S) gives 255 and raises the flag.  With gt: the
// pseudo_scores histogram (pixels labelled 255 are dropped) and cover[0] = labelled pixels with gt < nc, cover[1] = pixels with
// gt < nc.
__global__ __launch_bounds__(256) void cam_seed_merge_kernel(const long* __restrict__ low, const long* __restrict__ high,
                                                              const int* __restrict__ slot_class, const unsigned char* __restrict__ gt,
                                                              unsigned char* __restrict__ label, unsigned char* __restrict__ rgb,
                                                              unsigned long long* __restrict__ hist, unsigned long long* __restrict__ cover,
                                                              int* __restrict__ flag, long HW, int S, int nc, int use_lds) {
    extern __shared__ unsigned int sh[];
    __shared__ unsigned int cov[2];
    const int b = blockIdx.y, cells = nc * nc;
    if (threadIdx.x < 2) cov[threadIdx.x] = 0;
    if (use_lds) wc_hist_zero(sh, cells);
    else __syncthreads();
    const int* table = slot_class + (long)b * S;
    unsigned int n_lab = 0, n_valid = 0;
    const long groups = (HW + 3) >> 2;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long i0 = g * 4, o = (long)b * HW + i0;
        const int n = HW - i0 < 4 ? (int)(HW - i0) : 4;
        unsigned int lab[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int cell = -1;
            if (q < n) {
                const long h = high[o + q], l = low[o + q];
                unsigned int v;
                if (h < 0 || h >= S || l < 0 || l >= S) {
                    *flag = 1;
                    v = 255u;
                } else if (h == 0) {
                    v = l == 0 ? 0u : 255u;
                } else {
                    v = (unsigned int)table[h] & 255u;
                }
                lab[q] = v;
                const unsigned int t = gt ? gt[o + q] : 255u;
                if (gt && t < (unsigned int)nc) {
                    ++n_valid;
                    if (v < (unsigned int)nc) {
                        ++n_lab;
                        cell = (int)t * nc + (int)v;
                    } else if (v != 255u) {
                        *flag = 1;
                    }
                }
            }
            if (cell >= 0) wc_hist_count(use_lds ? sh : nullptr, hist, cell);
        }
        ef_store(lab, n, o, label, rgb);
    }
    if (gt) {
        if (n_lab) atomicAdd(&cov[0], n_lab);
        if (n_valid) atomicAdd(&cov[1], n_valid);
    }
    __syncthreads();
    if (use_lds) wc_hist_flush_cells(sh, hist, cells);
    if (gt && threadIdx.x < 2 && cov[threadIdx.x]) atomicAdd(&cover[threadIdx.x], (unsigned long long)cov[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// the sweep's LDS: CS_MAXT floats of thresholds, then the cells
static size_t cs_sweep_lds(int nc, int Kmax, int T) { return ((size_t)nc * Kmax * (T + 1) + CS_MAXT) * sizeof(unsigned int); }
static bool cs_lds_fits(int nc, int Kmax, int T) { return cs_sweep_lds(nc, Kmax, T) <= CS_LDS_BYTES; }

// 4 groups per thread (a group is K 16-byte loads): long-lived workgroups make the LDS cells worth their flush
static dim3 cs_grid(long HW, int per_group, int B) { return dim3(wc_hist_blocks((HW + per_group - 1) / per_group, 4), (unsigned)B); }

#define CS_CHECK_COMMON(name)                                                                                                  \
    WC_CHECK_ARG(B >= 1 && B <= 65535 && P >= B && HW >= 1 && HW <= (1L << 28), name ": bad argument (1 <= B <= 65535, P >= B, " \
                                                                                     "1 <= HW <= 2^28)")

extern "C" int wc_cam_seed_sweep_path(int nc, int Kmax, int T, int* use_lds) {
    WC_CHECK_ARG(use_lds && nc >= 2 && nc <= 256 && Kmax >= 1 && Kmax <= nc - 1 && T >= 1 && T <= CS_MAXT,
                 "wc_cam_seed_sweep_path: bad argument (2 <= nc <= 256, 1 <= Kmax <= nc - 1, 1 <= T <= 64)");
    *use_lds = cs_lds_fits(nc, Kmax, T) ? 1 : 0;
    return WC_OK;
}

extern "C" int wc_cam_seed_sweep(const void* cam_f16, const int* first, const int* keys, const void* gt_u8, const float* thresholds,
                                 long* bins, int* flag, int B, int P, long HW, int nc, int T, int Kmax, int force_global,
                                 void* stream) {
    WC_CHECK_ARG(cam_f16 && first && keys && gt_u8 && thresholds && bins && flag, "wc_cam_seed_sweep: null pointer");
    CS_CHECK_COMMON("wc_cam_seed_sweep");
    WC_CHECK_ARG(T >= 1 && T <= CS_MAXT, "wc_cam_seed_sweep: T = %d thresholds (1 <= T <= 64)", T);
    WC_CHECK_ARG(nc >= 2 && nc <= 256, "wc_cam_seed_sweep: nc = %d classes (2 <= nc <= 256)", nc);
    WC_CHECK_ARG(Kmax >= 1 && Kmax <= nc - 1, "wc_cam_seed_sweep: Kmax = %d maps per image (1 <= Kmax <= nc - 1)", Kmax);
    WC_CHECK_ARG(((uintptr_t)cam_f16 & 15) == 0 && ((uintptr_t)gt_u8 & 3) == 0,
                 "wc_cam_seed_sweep: cam must be 16-byte and gt 4-byte aligned");
    CsThr thr;
    for (int j = 0; j < CS_MAXT; ++j) thr.t[j] = 0.f;
    for (int j = 0; j < T; ++j) {
        WC_CHECK_ARG(isfinite(thresholds[j]) && (j == 0 || thresholds[j] > thresholds[j - 1]),
                     "wc_cam_seed_sweep: thresholds must be finite and strictly ascending (entry %d)", j);
        thr.t[j] = thresholds[j];
    }
    thr.inv = T > 1 ? (float)(T - 1) / (thr.t[T - 1] - thr.t[0]) : 0.f;
    const dim3 grid = cs_grid(HW, 8, B);
    if (!force_global && cs_lds_fits(nc, Kmax, T)) {
        hipLaunchKernelGGL(cam_seed_sweep_kernel<true>, grid, dim3(256), cs_sweep_lds(nc, Kmax, T), (hipStream_t)stream, (const unsigned short*)cam_f16, first,
                           keys, (const unsigned char*)gt_u8, (unsigned long long*)bins, flag, thr, P, HW, nc, T, Kmax);
    } else {
        hipLaunchKernelGGL(cam_seed_sweep_kernel<false>, grid, dim3(256), CS_MAXT * sizeof(float), (hipStream_t)stream, (const unsigned short*)cam_f16, first,
                           keys, (const unsigned char*)gt_u8, (unsigned long long*)bins, flag, thr, P, HW, nc, T, Kmax);
    }
    WC_LAUNCH_CHECK("cam_seed_sweep_kernel");
    return WC_OK;
}

extern "C" int wc_cam_seed_labels(const void* cam_f16, const int* first, const int* keys, long* lab_low, long* lab_high, int* flag,
                                  int B, int P, long HW, float low_thre, float high_thre, void* stream) {
    WC_CHECK_ARG(cam_f16 && first && keys && lab_low && lab_high && flag, "wc_cam_seed_labels: null pointer");
    CS_CHECK_COMMON("wc_cam_seed_labels");
    WC_CHECK_ARG(isfinite(low_thre) && isfinite(high_thre) && low_thre <= high_thre,
                 "wc_cam_seed_labels: thresholds must be finite with low_thre <= high_thre");
    WC_CHECK_ARG(((uintptr_t)cam_f16 & 15) == 0, "wc_cam_seed_labels: cam must be 16-byte aligned");
    hipLaunchKernelGGL(cam_seed_labels_kernel, cs_grid(HW, 8, B), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)cam_f16,
                       first, keys, lab_low, lab_high, flag, P, HW, low_thre, high_thre);
    WC_LAUNCH_CHECK("cam_seed_labels_kernel");
    return WC_OK;
}

extern "C" int wc_cam_seed_merge(const long* lab_low, const long* lab_high, const int* slot_class, const void* gt_u8, void* label_u8,
                                 void* cmap_rgb, long* hist, long* cover, int* flag, int B, long HW, int S, int nc, void* stream) {
    WC_CHECK_ARG(lab_low && lab_high && slot_class && label_u8 && flag, "wc_cam_seed_merge: null pointer");
    WC_CHECK_ARG(B >= 1 && B <= 65535 && HW >= 1 && HW <= (1L << 28) && S >= 2 && S <= 256 && nc >= 2 && nc <= 256,
                 "wc_cam_seed_merge: bad argument (1 <= B <= 65535, 1 <= HW <= 2^28, 2 <= S <= 256, 2 <= nc <= 256)");
    WC_CHECK_ARG(!gt_u8 || (hist && cover), "wc_cam_seed_merge: gt needs hist and cover");
    const size_t lds = (size_t)nc * nc * sizeof(unsigned int);
    const int use_lds = gt_u8 && lds <= CS_LDS_BYTES - 64;
    hipLaunchKernelGGL(cam_seed_merge_kernel, cs_grid(HW, 4, B), dim3(256), use_lds ? lds : 0, (hipStream_t)stream, lab_low, lab_high,
                       slot_class, (const unsigned char*)gt_u8, (unsigned char*)label_u8, (unsigned char*)cmap_rgb,
                       (unsigned long long*)hist, (unsigned long long*)cover, flag, HW, S, nc, use_lds);
    WC_LAUNCH_CHECK("cam_seed_merge_kernel");
    return WC_OK;
}
