// The per-image tail of the evaluation entry point (msc_flip_eval.py), on the device (fp32 / int64 / uint8).
//
// Neither kernel is hot next to the four encoder forwards an image costs: both exist so that the loop around the model has no
// host round trip per image beyond the device-to-host copy of the bytes that must reach the disk
// (reference test_msc_flip_voc.py:92-107 `validate`, :158-161 `crf_proc`; utils/imutils.py:136-154 `colormap`):
//   eval_finish_kernel  : per image, ONE launch over the (Hl, Wl) label grid: both arg-maxes (scale-1 and multi-scale logits share
//                         a grid, so a pixel's source indices and weights are computed once), the uint8 prediction maps, the
//                         colour image and the three histograms (gt, seg1 pred), (gt, msc pred), (gt, CAM label)     (:92-107)
//   label_finish_kernel : the same outputs for a ready int64 arg-max map (the CRF leg)                               (:158-161)
// Bilinear arithmetic (so each arg-max is resize_argmax_kernel's) and the histogram skeleton: resample.h.  Flag contract =
// confusion_hist_kernel's.
// The colour of label v is the PASCAL VOC bit-interleaved map, ef_colour of voc_colour.h (shared with panels.hip); the 4-label
// store ef_store lives there too (shared with camseed.hip).
#include "common.h"
#include "resample.h"
#include "voc_colour.h"

// One thread per group of 4 adjacent x of one label row (grid-stride over the Hl * ceil(Wl / 4) groups).  lds_mask bit k: histogram
// k (0 seg1, 1 msc, 2 cam) is counted in LDS, at cell offset (number of lower set bits) * nc * nc; a histogram that is absent
// (NULL pointer) has its bit clear.  Integer atomics throughout: the counts do not depend on the order or on the placement.
__global__ __launch_bounds__(256) void eval_finish_kernel(const float* __restrict__ seg1, const float* __restrict__ msc,
                                                           const long* __restrict__ cam, const long* __restrict__ gt,
                                                           unsigned char* __restrict__ pred1_u8, unsigned char* __restrict__ predm_u8,
                                                           unsigned char* __restrict__ cmap_rgb, unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ msc_hist,
                                                           unsigned long long* __restrict__ cam_hist, int* __restrict__ flag, int C,
                                                           int Hs, int Ws, int Hl, int Wl, float sy, float sx, int nc, int lds_mask) {
    extern __shared__ unsigned int sh[];
    const int cells = nc * nc;
    unsigned long long* const dst[3] = {hist, msc_hist, cam_hist};
    unsigned int* lds[3];
    int lds_cells = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lds[k] = (lds_mask >> k) & 1 ? sh + lds_cells : nullptr;
        if ((lds_mask >> k) & 1) lds_cells += cells;
    }
    if (lds_cells) wc_hist_zero(sh, lds_cells);
    const int G = (Wl + 3) >> 2;
    const long groups = (long)Hl * G, plane = (long)Hs * Ws;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const int y = (int)(g / G), xb = (int)(g - (long)y * G) * 4;
        const int n = Wl - xb < 4 ? Wl - xb : 4;
        int y0, y1, x0[4], x1[4];
        float ly, lx[4];
        wc_bil_src(y, Hs, sy, y0, y1, ly);
#pragma unroll
        for (int k = 0; k < 4; ++k) wc_bil_src(xb + (k < n ? k : 0), Ws, sx, x0[k], x1[k], lx[k]);
        float best1[4], bestm[4];
        unsigned int arg1[4] = {0, 0, 0, 0}, argm[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) best1[k] = bestm[k] = -INFINITY;
        for (int c = 0; c < C; ++c) {
            const float* S1 = seg1 + c * plane;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = wc_bilerp(S1, Ws, y0, y1, x0[k], x1[k], ly, lx[k]);
                if (v > best1[k]) { best1[k] = v; arg1[k] = c; }
            }
            if (msc) {
                const float* Sm = msc + c * plane;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = wc_bilerp(Sm, Ws, y0, y1, x0[k], x1[k], ly, lx[k]);
                    if (v > bestm[k]) { bestm[k] = v; argm[k] = c; }
                }
            }
        }
        const long i = (long)y * Wl + xb;
        ef_store(arg1, n, i, pred1_u8, msc ? nullptr : cmap_rgb);
        if (msc) ef_store(argm, n, i, predm_u8, cmap_rgb);
        if (!gt) continue;
        for (int k = 0; k < n; ++k) {
            const long t = gt[i + k];
            if (t < 0 || t >= nc) continue;
            if (hist) {
                if ((int)arg1[k] >= nc) *flag = 1;
                else wc_hist_count(lds[0], hist, (int)t * nc + (int)arg1[k]);
            }
            if (msc && msc_hist) {
                if ((int)argm[k] >= nc) *flag = 1;
                else wc_hist_count(lds[1], msc_hist, (int)t * nc + (int)argm[k]);
            }
            if (cam && cam_hist) {
                const long cv = cam[i + k];
                if (cv < 0 || cv >= nc) *flag = 1;
                else wc_hist_count(lds[2], cam_hist, (int)t * nc + (int)cv);
            }
        }
    }
    if (lds_cells) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (lds[k]) wc_hist_flush_cells(lds[k], dst[k], cells);
    }
}

// pred (H, W) int64 -> out_u8, cmap_rgb and hist[gt, pred].  A pred outside [0, 255] is written as 255 and raises flag[0]; a pred
// outside [0, nc) at a pixel with 0 <= gt < nc is skipped in the histogram and raises flag[0].
__global__ __launch_bounds__(256) void label_finish_kernel(const long* __restrict__ pred, const long* __restrict__ gt,
                                                            unsigned char* __restrict__ out_u8, unsigned char* __restrict__ cmap_rgb,
                                                            unsigned long long* __restrict__ hist, int* __restrict__ flag, int H, int W,
                                                            int nc, int use_lds) {
    extern __shared__ unsigned int sh[];
    const int cells = nc * nc;
    if (use_lds) wc_hist_zero(sh, cells);
    const int G = (W + 3) >> 2;
    const long groups = (long)H * G;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const int y = (int)(g / G), xb = (int)(g - (long)y * G) * 4;
        const int n = W - xb < 4 ? W - xb : 4;
        const long i = (long)y * W + xb;
        unsigned int lab[4] = {0, 0, 0, 0};
        for (int k = 0; k < n; ++k) {
            const long p = pred[i + k];
            if (p < 0 || p > 255) { *flag = 1; lab[k] = 255u; }
            else lab[k] = (unsigned int)p;
            if (!gt) continue;
            const long t = gt[i + k];
            if (t < 0 || t >= nc) continue;
            if (p < 0 || p >= nc) *flag = 1;
            else wc_hist_count(use_lds ? sh : nullptr, hist, (int)t * nc + (int)p);
        }
        ef_store(lab, n, i, out_u8, cmap_rgb);
    }
    if (use_lds) wc_hist_flush(sh, hist, cells);
}

// ---------------------------------------------------------------------------------------------
// groups_per_thread: 1 for eval_finish_kernel (a group costs 8 * C dependent-latency loads per logit tensor: the launch wants every
// CU busy), 4 for label_finish_kernel (a group is 4 loads: fewer, longer-lived workgroups make the LDS histogram worth its flush)
static unsigned ef_blocks(int H, int W, int groups_per_thread) { return wc_hist_blocks((long)H * ((W + 3) / 4), groups_per_thread); }

extern "C" int wc_eval_finish(const float* seg1, const float* msc, const long* cam, const long* gt, void* pred1_u8, void* predm_u8,
                              void* cmap_rgb, long* hist, long* msc_hist, long* cam_hist, int* flag, int C, int Hs, int Ws, int Hl,
                              int Wl, int nc, void* stream) {
    WC_CHECK_ARG(seg1 && flag && C > 0 && Hs > 0 && Ws > 0 && Hl > 0 && Wl > 0 && nc > 0 && nc <= 4096, "wc_eval_finish: bad argument");
    WC_CHECK_ARG(C <= 256, "wc_eval_finish: C = %d classes do not fit the uint8 maps (C <= 256)", C);
    WC_CHECK_ARG(msc || !(predm_u8 || msc_hist), "wc_eval_finish: predm_u8 / msc_hist need msc");
    WC_CHECK_ARG(!cam || cam_hist || !gt, "wc_eval_finish: cam with gt needs cam_hist");
    // what is counted at all, and of that what fits the 64 KiB of LDS a workgroup gets (3 histograms at nc = 81 are 78,732 bytes:
    // the first two go to LDS, the CAM histogram to global atomics)
    const size_t one = (size_t)nc * nc * sizeof(unsigned int);
    const bool present[3] = {gt && hist, gt && msc && msc_hist, gt && cam && cam_hist};
    int lds_mask = 0;
    size_t lds = 0;
    for (int k = 0; k < 3; ++k)
        if (present[k] && lds + one <= 64 * 1024) {
            lds_mask |= 1 << k;
            lds += one;
        }
    hipLaunchKernelGGL(eval_finish_kernel, dim3(ef_blocks(Hl, Wl, 1)), dim3(256), lds, (hipStream_t)stream, seg1, msc, cam, gt,
                       (unsigned char*)pred1_u8, (unsigned char*)predm_u8, (unsigned char*)cmap_rgb, (unsigned long long*)hist,
                       (unsigned long long*)msc_hist, (unsigned long long*)cam_hist, flag, C, Hs, Ws, Hl, Wl, (float)Hs / Hl,
                       (float)Ws / Wl, nc, lds_mask);
    WC_LAUNCH_CHECK("eval_finish_kernel");
    return WC_OK;
}

extern "C" int wc_label_finish(const long* pred, const long* gt, void* out_u8, void* cmap_rgb, long* hist, int* flag, int H, int W,
                               int nc, void* stream) {
    WC_CHECK_ARG(pred && flag && H > 0 && W > 0 && nc > 0 && nc <= 4096 && (hist || !gt), "wc_label_finish: bad argument");
    const size_t lds = (size_t)nc * nc * sizeof(unsigned int);
    const int use_lds = gt && lds <= 64 * 1024;
    hipLaunchKernelGGL(label_finish_kernel, dim3(ef_blocks(H, W, 4)), dim3(256), use_lds ? lds : 0, (hipStream_t)stream, pred, gt,
                       (unsigned char*)out_u8, (unsigned char*)cmap_rgb, (unsigned long long*)hist, flag, H, W, nc, use_lds);
    WC_LAUNCH_CHECK("label_finish_kernel");
    return WC_OK;
}
