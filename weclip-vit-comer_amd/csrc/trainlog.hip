// Step metrics and validation histograms of the training driver (train.py, validate.py), on the device (fp32 / int64).
//
// Neither kernel is hot: both exist so that the loop around the train step has no host round trip
// (reference scripts/dist_clip_voc.py:71-102 `validate`, :274-277 `pseudo_seg_mAcc`):
//   val_pair_hist_kernel     : per validated image, seg_hist[gt, argmax_c bilinear(seg)[c]] += 1 and cam_hist[gt, cam] += 1
//                              in ONE launch; the (Hl, Wl) prediction map is never written                       (:86-100)
//   label_match_count_kernel : #pixels with argmax_c bilinear(seg)[c] == pseudo label, and the pixel count       (:274-277)
// Bilinear index arithmetic = ATen's area_pixel_compute_source_index with align_corners=False and a size-derived scale,
// restated from evalops.hip (ev_src / ev_bilerp, resize_argmax_kernel) operation for operation: with -ffp-contract=off the
// interpolated values, and so the arg-max, are the bits resize_argmax_kernel computes (tests/test_trainlog_gpu.py pins it).
#include "common.h"

__device__ __forceinline__ void tl_src(int d, int in, float scale, int& i0, int& i1, float& l1) {
    const float s = fmaxf(scale * (d + 0.5f) - 0.5f, 0.f);
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - i0;
}

__device__ __forceinline__ float tl_bilerp(const float* __restrict__ S, int Ws, int y0, int y1, int x0, int x1, float ly,
                                           float lx) {
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * S[(long)y0 * Ws + x0] + lx * S[(long)y0 * Ws + x1]) +
           ly * (hx * S[(long)y1 * Ws + x0] + lx * S[(long)y1 * Ws + x1]);
}

// argmax_c bilinear(seg (C, Hs, Ws))[c, y, x] on the (Hd, Wd) grid; the first maximum wins, as in resize_argmax_kernel
__device__ __forceinline__ int tl_resize_argmax(const float* __restrict__ seg, int C, int Hs, int Ws, int y, int x, float sy,
                                                float sx) {
    int y0, y1, x0, x1;
    float ly, lx;
    tl_src(y, Hs, sy, y0, y1, ly);
    tl_src(x, Ws, sx, x0, x1, lx);
    float best = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
        const float v = tl_bilerp(seg + (long)c * Hs * Ws, Ws, y0, y1, x0, x1, ly, lx);
        if (v > best) { best = v; arg = c; }
    }
    return arg;
}

// Over the label pixels with 0 <= gt < nc: seg_hist[gt * nc + p] += 1, p = the arg-max above, and (cam != NULL)
// cam_hist[gt * nc + cam] += 1.  A p or cam value outside [0, nc) is skipped and raises flag[0] (confusion_hist_kernel's
// contract), each histogram on its own.  Integer atomics: the result does not depend on their order.  use_lds: per-workgroup
// LDS histograms ([seg | cam], 32-bit cells) flushed once, else straight global atomics.
__global__ __launch_bounds__(256) void val_pair_hist_kernel(const float* __restrict__ seg, const long* __restrict__ cam,
                                                             const long* __restrict__ gt, unsigned long long* __restrict__ seg_hist,
                                                             unsigned long long* __restrict__ cam_hist, int* __restrict__ flag,
                                                             int C, int Hs, int Ws, int Hl, int Wl, float sy, float sx, int nc,
                                                             int use_lds) {
    extern __shared__ unsigned int sh[];
    const int cells = nc * nc;
    const int lds_cells = cam ? 2 * cells : cells;
    if (use_lds) {
        for (int i = threadIdx.x; i < lds_cells; i += 256) sh[i] = 0;
        __syncthreads();
    }
    const long n = (long)Hl * Wl;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long t = gt[i];
        if (t < 0 || t >= nc) continue;
        const int y = (int)(i / Wl), x = (int)(i - (long)y * Wl);
        const int p = tl_resize_argmax(seg, C, Hs, Ws, y, x, sy, sx);
        if (p >= nc) {
            *flag = 1;
        } else if (use_lds) {
            atomicAdd(&sh[t * nc + p], 1u);
        } else {
            atomicAdd(&seg_hist[t * nc + p], 1ull);
        }
        if (cam) {
            const long c = cam[i];
            if (c < 0 || c >= nc) {
                *flag = 1;
            } else if (use_lds) {
                atomicAdd(&sh[cells + t * nc + c], 1u);
            } else {
                atomicAdd(&cam_hist[t * nc + c], 1ull);
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < lds_cells; i += 256)
            if (sh[i]) atomicAdd(i < cells ? &seg_hist[i] : &cam_hist[i - cells], (unsigned long long)sh[i]);
    }
}

// counts[0] += #pixels of (B, H, W) with argmax_c bilinear(seg[b])[c] == label[b]; counts[1] = B*H*W.  The entry zeroes
// counts ahead of the launch.  One global atomic per workgroup.
__global__ __launch_bounds__(256) void label_match_count_kernel(const float* __restrict__ seg, const long* __restrict__ label,
                                                                 unsigned long long* __restrict__ counts, int B, int C, int Hs,
                                                                 int Ws, int H, int W, float sy, float sx) {
    __shared__ unsigned int block_hits;
    if (threadIdx.x == 0) block_hits = 0;
    __syncthreads();
    const long plane = (long)H * W, n = plane * B;
    unsigned int hits = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int b = (int)(i / plane);
        const long r = i - (long)b * plane;
        const int y = (int)(r / W), x = (int)(r - (long)y * W);
        const int p = tl_resize_argmax(seg + (long)b * C * Hs * Ws, C, Hs, Ws, y, x, sy, sx);
        hits += (label[i] == (long)p) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(&block_hits, hits);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (block_hits) atomicAdd(&counts[0], (unsigned long long)block_hits);
        if (blockIdx.x == 0) counts[1] = (unsigned long long)n;
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" int wc_val_pair_hist(const float* seg, const long* cam, const long* gt, long* seg_hist, long* cam_hist, int* flag,
                                int C, int Hs, int Ws, int Hl, int Wl, int nc, void* stream) {
    WC_CHECK_ARG(seg && gt && seg_hist && flag && (cam_hist || !cam) && C > 0 && Hs > 0 && Ws > 0 && Hl > 0 && Wl > 0 &&
                     nc > 0 && nc <= 4096,
                 "wc_val_pair_hist: bad argument");
    const long n = (long)Hl * Wl;
    const size_t lds = (size_t)nc * nc * sizeof(unsigned int) * (cam ? 2 : 1);
    const int use_lds = lds <= 64 * 1024;
    long blocks = (n + 256 * 16 - 1) / (256 * 16);         // ~16 pixels per thread, so the LDS histograms are worth their flush
    if (blocks > 1024) blocks = 1024;                      // (a workgroup then counts n / 1024 pixels: 32-bit cells hold 2^42 pixels)
    hipLaunchKernelGGL(val_pair_hist_kernel, dim3((unsigned)blocks), dim3(256), use_lds ? lds : 0, (hipStream_t)stream, seg, cam,
                       gt, (unsigned long long*)seg_hist, (unsigned long long*)cam_hist, flag, C, Hs, Ws, Hl, Wl,
                       (float)Hs / Hl, (float)Ws / Wl, nc, use_lds);
    WC_LAUNCH_CHECK("val_pair_hist_kernel");
    return WC_OK;
}

extern "C" int wc_label_match_count(const float* seg, const long* label, long* counts, int B, int C, int Hs, int Ws, int H,
                                    int W, void* stream) {
    WC_CHECK_ARG(seg && label && counts && B > 0 && C > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0,
                 "wc_label_match_count: bad argument");
    if (hipMemsetAsync(counts, 0, 2 * sizeof(long), (hipStream_t)stream) != hipSuccess) {
        wc_set_error("wc_label_match_count: hipMemsetAsync failed");
        return WC_ERR_HIP;
    }
    const long n = (long)B * H * W;
    long blocks = (n + 256 * 4 - 1) / (256 * 4);
    if (blocks > 1024) blocks = 1024;                      // one global atomic per workgroup
    hipLaunchKernelGGL(label_match_count_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, seg, label,
                       (unsigned long long*)counts, B, C, Hs, Ws, H, W, (float)Hs / H, (float)Ws / W);
    WC_LAUNCH_CHECK("label_match_count_kernel");
    return WC_OK;
}
