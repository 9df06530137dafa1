// Step metrics and validation histograms of the training driver (train.py, validate.py), on the device (fp32 / int64).
//
// Neither kernel is hot: both exist so that the loop around the train step has no host round trip
// (reference scripts/dist_clip_voc.py:71-102 `validate`, :274-277 `pseudo_seg_mAcc`):
//   val_pair_hist_kernel     : per validated image, seg_hist[gt, argmax_c bilinear(seg)[c]] += 1 and cam_hist[gt, cam] += 1
//                              in ONE launch; the (Hl, Wl) prediction map is never written                       (:86-100)
//   label_match_count_kernel : #pixels with argmax_c bilinear(seg)[c] == pseudo label, and the pixel count       (:274-277)
//   step_pair_hist_kernel    : the batched form of the first one for the supervised train step: hist[label, arg-max] += 1 over
//                              a (B, H, W) ground-truth batch, inside the step's captured graph (train.LoggedSupervisedTrainStep)
// Bilinear arithmetic and the arg-max are resize_argmax_kernel's (resample.h), with a size-derived scale.
#include <stdlib.h>

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

// One count per lane of a wave (cell < 0: nothing to count), pre-aggregated: the first active lane's cell is broadcast, the
// lanes that hold the same cell are balloted and the lowest of them adds their number in ONE atomic; every other lane adds
// its own 1.  On a real mask most lanes of a wave sit on (background, background): 64 serialised atomics on one LDS cell
// become one.  Same counts as wc_hist_count per lane (integer adds).
__device__ __forceinline__ void tl_hist_count_wave(unsigned int* sh, unsigned long long* hist, int cell) {
    const int lead = __builtin_amdgcn_readfirstlane(cell);
    const unsigned long long same = __ballot(cell == lead);
    if (cell == lead) {
        if (lead >= 0 && (int)__lane_id() == __ffsll((unsigned long long)same) - 1) {
            const unsigned int k = (unsigned int)__popcll(same);
            if (sh) atomicAdd(&sh[lead], k);
            else atomicAdd(&hist[lead], (unsigned long long)k);
        }
    } else if (cell >= 0) {
        wc_hist_count(sh, hist, cell);
    }
}

// Over the pixels of label (B, H, W) with 0 <= label < nc: hist[label * nc + p] += 1, p = argmax_c bilinear(seg[b])[c] on the
// (H, W) grid; p >= nc is skipped and raises flag[0] (val_pair_hist_kernel's contract).  hist is added to, never zeroed.
// The kernel is bound by the C x 4 tap loads of the arg-max, not by the label read or the atomics, so one thread takes
// SPH_Q = 4 neighbouring pixels of a row: when they share their two source columns (always, when up-sampling by a multiple
// of 8) the four taps of a class are loaded once for all of them.  Each pixel's value is still wc_lerp4 of the same four
// taps with its own weights, classes in ascending order, first maximum wins: the bits of wc_resize_argmax_at.
// AGG: tl_hist_count_wave instead of one atomic per lane (the entry picks the form; DESIGN.md section 13.2 has both times).
#define SPH_Q 4
template <bool AGG>
__global__ __launch_bounds__(256) void step_pair_hist_kernel(const float* __restrict__ seg, const long* __restrict__ label,
                                                              unsigned long long* __restrict__ hist, int* __restrict__ flag, int B,
                                                              int C, int Hs, int Ws, int H, int W, float sy, float sx, int nc,
                                                              int use_lds) {
    extern __shared__ unsigned int sh[];
    const int cells = nc * nc;
    unsigned int* const shh = use_lds ? sh : nullptr;
    if (use_lds) wc_hist_zero(sh, cells);
    const int Wq = (W + SPH_Q - 1) / SPH_Q;
    const long rowq = (long)H * Wq, n = rowq * B;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int b = (int)(i / rowq);
        const long r = i - (long)b * rowq;
        const int y = (int)(r / Wq), x = (int)(r - (long)y * Wq) * SPH_Q;
        const long* const lab = label + ((long)b * H + y) * W + x;
        long t[SPH_Q];
        bool any = false;
#pragma unroll
        for (int k = 0; k < SPH_Q; ++k) {
            t[k] = x + k < W ? lab[k] : -1;                               // past the row's end: counted nowhere
            if (t[k] < 0 || t[k] >= nc) t[k] = -1;
            any = any || t[k] >= 0;
        }
        int p[SPH_Q] = {0, 0, 0, 0};
        if (any) {
            const float* const S = seg + (long)b * C * Hs * Ws;
            int y0, y1, x0[SPH_Q], x1[SPH_Q];
            float ly, lx[SPH_Q];
            wc_bil_src(y, Hs, sy, y0, y1, ly);
            bool shared = true;
#pragma unroll
            for (int k = 0; k < SPH_Q; ++k) {
                wc_bil_src(min(x + k, W - 1), Ws, sx, x0[k], x1[k], lx[k]);
                shared = shared && x0[k] == x0[0] && x1[k] == x1[0];
            }
            if (shared) {
                float best[SPH_Q];
#pragma unroll
                for (int k = 0; k < SPH_Q; ++k) best[k] = -INFINITY;
                const long o00 = (long)y0 * Ws + x0[0], o01 = (long)y0 * Ws + x1[0], o10 = (long)y1 * Ws + x0[0],
                           o11 = (long)y1 * Ws + x1[0];
                for (int c = 0; c < C; ++c) {
                    const float* const P = S + (long)c * Hs * Ws;
                    const float va = P[o00], vb = P[o01], vc = P[o10], vd = P[o11];
#pragma unroll
                    for (int k = 0; k < SPH_Q; ++k) {
                        const float v = wc_lerp4(va, vb, vc, vd, ly, lx[k]);
                        if (v > best[k]) { best[k] = v; p[k] = c; }
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < SPH_Q; ++k)
                    if (t[k] >= 0) p[k] = wc_resize_argmax_at(S, C, Hs, Ws, y0, y1, x0[k], x1[k], ly, lx[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < SPH_Q; ++k) {
            int cell = -1;
            if (t[k] >= 0) {
                if (p[k] >= nc) *flag = 1;
                else cell = (int)t[k] * nc + p[k];
            }
            if (AGG) tl_hist_count_wave(shh, hist, cell);
            else if (cell >= 0) wc_hist_count(shh, hist, cell);
        }
    }
    if (use_lds) wc_hist_flush(sh, hist, cells);
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

extern "C" int wc_step_pair_hist(const float* seg, const long* label, long* hist, int* flag, int B, int C, int Hs, int Ws, int H,
                                 int W, int nc, void* stream) {
    WC_CHECK_ARG(seg && label && hist && flag && B > 0 && C > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && nc > 0 && nc <= 4096,
                 "wc_step_pair_hist: bad argument");
    // WECLIP_STEP_HIST_AGG=0|1 picks the counting form for the A/B of tools/seg_train_bench.py (read per call, so one process
    // can time both); unset: the form that measured faster
    const char* const env = getenv("WECLIP_STEP_HIST_AGG");
    const int agg = env ? atoi(env) : 1;
    const long n = (long)B * H * ((W + SPH_Q - 1) / SPH_Q);               // one thread per SPH_Q pixels of a row
    const size_t lds = (size_t)nc * nc * sizeof(unsigned int);
    const int use_lds = lds <= 64 * 1024;
    const auto kernel = agg ? step_pair_hist_kernel<true> : step_pair_hist_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(wc_hist_blocks(n, 16 / SPH_Q)), dim3(256), use_lds ? lds : 0, (hipStream_t)stream, seg, label,
                       (unsigned long long*)hist, flag, B, C, Hs, Ws, H, W, (float)Hs / H, (float)Ws / W, nc, use_lds);
    WC_LAUNCH_CHECK("step_pair_hist_kernel");
    return WC_OK;
}
