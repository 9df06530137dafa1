// Step metrics and validation histograms of the training driver (train.py, validate.py), on the device (fp32 / int64).
//
// Neither kernel is hot: both exist so that the loop around the train step has no host round trip
// (reference scripts/dist_clip_voc.py:71-102 `validate`, :274-277 `pseudo_seg_mAcc`):
//   val_pair_hist_kernel     : per validated image, seg_hist[gt, argmax_c bilinear(seg)[c]] += 1 and cam_hist[gt, cam] += 1
//                              in ONE launch; the (Hl, Wl) prediction map is never written                       (:86-100)
//   label_match_count_kernel : #pixels with argmax_c bilinear(seg)[c] == pseudo label, and the pixel count       (:274-277)
// Bilinear arithmetic and the arg-max are resize_argmax_kernel's (resample.h), with a size-derived scale.
#include "common.h"
#include "resample.h"

// argmax_c bilinear(seg (C, Hs, Ws))[c, y, x] on the (Hd, Wd) grid
__device__ __forceinline__ int tl_resize_argmax(const float* __restrict__ seg, int C, int Hs, int Ws, int y, int x, float sy,
                                                float sx) {
    int y0, y1, x0, x1;
    float ly, lx;
    wc_bil_src(y, Hs, sy, y0, y1, ly);
    wc_bil_src(x, Ws, sx, x0, x1, lx);
    return wc_resize_argmax_at(seg, C, Hs, Ws, y0, y1, x0, x1, ly, lx);
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
    unsigned int* const sh_seg = use_lds ? sh : nullptr;
    unsigned int* const sh_cam = use_lds ? sh + cells : nullptr;
    if (use_lds) wc_hist_zero(sh, cam ? 2 * cells : cells);
    const long n = (long)Hl * Wl;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long t = gt[i];
        if (t < 0 || t >= nc) continue;
        const int y = (int)(i / Wl), x = (int)(i - (long)y * Wl);
        const int p = tl_resize_argmax(seg, C, Hs, Ws, y, x, sy, sx);
        if (p >= nc) *flag = 1;
        else wc_hist_count(sh_seg, seg_hist, (int)t * nc + p);
        if (cam) {
            const long c = cam[i];
            if (c < 0 || c >= nc) *flag = 1;
            else wc_hist_count(sh_cam, cam_hist, (int)t * nc + (int)c);
        }
    }
    if (use_lds) {
        wc_hist_flush(sh_seg, seg_hist, cells);
        if (cam) wc_hist_flush_cells(sh_cam, cam_hist, cells);
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
    hipLaunchKernelGGL(val_pair_hist_kernel, dim3(wc_hist_blocks(n, 16)), dim3(256), use_lds ? lds : 0, (hipStream_t)stream, seg, cam,
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
    hipLaunchKernelGGL(label_match_count_kernel, dim3(wc_hist_blocks(n, 4)), dim3(256), 0, (hipStream_t)stream, seg, label,
                       (unsigned long long*)counts, B, C, Hs, Ws, H, W, (float)Hs / H, (float)Ws / W);
    WC_LAUNCH_CHECK("label_match_count_kernel");
    return WC_OK;
}
