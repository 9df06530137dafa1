// The per-image tail of the predict entry point (predict.py), on the device (fp32 / int64 / uint8): what evalfinish.hip is to
// the evaluation entry point, for images that have no label map.  The output grid is the image's own (H, W); besides the arg-max
// the kernel keeps what the evaluator throws away, the model's confidence in it
// (reference test_msc_flip_voc.py:92-96 `validate`: resize + arg-max; :146-161 `crf_proc`: the CRF's Q and its arg-max;
//  utils/imutils.py:136-154 `colormap`):
//   predict_finish_kernel<0> : src = logits (C, Hs, Ws) on the model's grid.  Per pixel the bilinear value of every class, the first
//                              maximum, and the soft-max probability of that maximum, 1 / sum_c exp(v_c - v_best)
//   predict_finish_kernel<1> : src = probabilities (C, H, W), the CRF's Q: the first maximum and its value
// and from those the uint8 label map (255 where the confidence is below a threshold), its colour image, the uint8 confidence map,
// the colour image blended over the input image, and per written label the pixel count and the confidence sum.
// Bilinear arithmetic (so the arg-max is resize_argmax_kernel's, bit for bit) and the LDS counting skeleton: resample.h.  Colour of a
// label and the 4-label store: voc_colour.h.  Not hot next to the four encoder forwards an image costs; it exists so that nothing
// but the bytes that must reach the disk leaves the device.
#include "common.h"
#include "resample.h"
#include "voc_colour.h"

// 4 packed colours (r | g << 8 | b << 16) -> RGB bytes at pixels [i, i + n), with ef_store's rule: three 32-bit words where the
// group is full and its first byte 4-aligned, bytes otherwise
__device__ __forceinline__ void pf_store_rgb(const unsigned int* c, int n, long i, unsigned char* __restrict__ rgb) {
    if (n == 4 && ((size_t)(rgb + 3 * i) & 3) == 0) {
        unsigned int* o = reinterpret_cast<unsigned int*>(rgb + 3 * i);
        o[0] = c[0] | (c[1] << 24);
        o[1] = (c[1] >> 8) | (c[2] << 16);
        o[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
        for (int k = 0; k < n; ++k) {
            rgb[3 * (i + k) + 0] = (unsigned char)(c[k] & 255u);
            rgb[3 * (i + k) + 1] = (unsigned char)((c[k] >> 8) & 255u);
            rgb[3 * (i + k) + 2] = (unsigned char)(c[k] >> 16);
        }
    }
}

// the reverse: RGB bytes of pixels [i, i + n) -> 4 packed colours (the unused ones 0)
__device__ __forceinline__ void pf_load_rgb(const unsigned char* __restrict__ rgb, int n, long i, unsigned int* c) {
    if (n == 4 && ((size_t)(rgb + 3 * i) & 3) == 0) {
        const unsigned int* s = reinterpret_cast<const unsigned int*>(rgb + 3 * i);
        const unsigned int w0 = s[0], w1 = s[1], w2 = s[2];
        c[0] = w0 & 0xffffffu;
        c[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
        c[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
        c[3] = w2 >> 8;
    } else {
        for (int k = 0; k < 4; ++k)
            c[k] = k < n ? (unsigned int)rgb[3 * (i + k)] | ((unsigned int)rgb[3 * (i + k) + 1] << 8) |
                               ((unsigned int)rgb[3 * (i + k) + 2] << 16)
                         : 0u;
    }
}

// (alpha256 * colour + (256 - alpha256) * image + 128) >> 8 per channel of a packed colour: at most 256 * 255 + 128 < 2^16
__device__ __forceinline__ unsigned int pf_blend(unsigned int col, unsigned int img, unsigned int a) {
    unsigned int o = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned int cc = (col >> (8 * ch)) & 255u, ii = (img >> (8 * ch)) & 255u;
        o |= ((a * cc + (256u - a) * ii + 128u) >> 8) << (8 * ch);
    }
    return o;
}

// One thread per group of 4 adjacent x of one output row (grid-stride over the H * ceil(W / 4) groups; one group per thread and
// pass).  LDS cells (32-bit, only when stats is given): [0, C) pixels per written label, [C, 2C) sum of
// their conf_u8, [2C] ignored pixels; flushed once per workgroup with 64-bit integer atomics, so the sums do not depend on the order.
// MODE 0, the soft-max in ONE pass over c with a running maximum: a class that raises the maximum rescales the sum by
// exp(old - new), every other class adds exp(v - max): one exponential per class and pixel, and each logit is loaded once.
template <int MODE>
__global__ __launch_bounds__(256) void predict_finish_kernel(const float* __restrict__ src, const unsigned char* __restrict__ image,
                                                              unsigned char* __restrict__ pred_u8, unsigned char* __restrict__ cmap_rgb,
                                                              unsigned char* __restrict__ conf_u8,
                                                              unsigned char* __restrict__ overlay_rgb,
                                                              unsigned long long* __restrict__ stats, int C, int Hs, int Ws, int H,
                                                              int W, float sy, float sx, unsigned int alpha256,
                                                              unsigned int ignore_below) {
    extern __shared__ unsigned int sh[];
    const int cells = 2 * C + 1;
    if (stats) wc_hist_zero(sh, cells);
    const int G = (W + 3) >> 2;
    const long groups = (long)H * G, plane = (long)Hs * Ws;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const int y = (int)(g / G), xb = (int)(g - (long)y * G) * 4;
        const int n = W - xb < 4 ? W - xb : 4;
        int y0, y1, x0[4], x1[4];
        float ly, lx[4];
        wc_bil_src(y, Hs, sy, y0, y1, ly);
#pragma unroll
        for (int k = 0; k < 4; ++k) wc_bil_src(xb + (k < n ? k : 0), Ws, sx, x0[k], x1[k], lx[k]);
        float best[4], sum[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned int arg[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) best[k] = -INFINITY;
        for (int c = 0; c < C; ++c) {
            const float* S = src + c * plane;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = wc_bilerp(S, Ws, y0, y1, x0[k], x1[k], ly, lx[k]);
                const bool up = v > best[k];                                   // the first maximum wins
                if (MODE == 0) {
                    const float e = expf((up ? best[k] : v) - (up ? v : best[k]));
                    sum[k] = up ? sum[k] * e + 1.f : sum[k] + e;
                }
                if (up) { best[k] = v; arg[k] = c; }
            }
        }
        unsigned int lab[4], cu[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float conf = fminf(fmaxf(MODE == 0 ? 1.f / sum[k] : best[k], 0.f), 1.f);
            cu[k] = (unsigned int)(int)(255.f * conf + 0.5f);
            lab[k] = cu[k] < ignore_below ? 255u : arg[k];                     // ignore_below = 0: never
        }
        const long i = (long)y * W + xb;
        ef_store(lab, n, i, pred_u8, cmap_rgb);
        ef_store(cu, n, i, conf_u8, nullptr);
        if (overlay_rgb) {
            unsigned int px[4];
            pf_load_rgb(image, n, i, px);
#pragma unroll
            for (int k = 0; k < 4; ++k) px[k] = pf_blend(ef_colour(lab[k]), px[k], alpha256);
            pf_store_rgb(px, n, i, overlay_rgb);
        }
        if (stats) {
            for (int k = 0; k < n; ++k) {
                if (lab[k] == 255u) {
                    atomicAdd(&sh[2 * C], 1u);
                } else {
                    atomicAdd(&sh[lab[k]], 1u);
                    atomicAdd(&sh[C + lab[k]], cu[k]);
                }
            }
        }
    }
    if (stats) wc_hist_flush(sh, stats, cells);
}

// ---------------------------------------------------------------------------------------------
extern "C" int wc_predict_finish(const float* src, const unsigned char* image, void* pred_u8, void* cmap_rgb, void* conf_u8,
                                 void* overlay_rgb, long* stats, int C, int Hs, int Ws, int H, int W, int mode, int alpha256,
                                 int ignore_below, void* stream) {
    WC_CHECK_ARG(src, "wc_predict_finish: src is NULL");
    WC_CHECK_ARG(C >= 1 && C <= 255, "wc_predict_finish: C = %d outside [1, 255] (label 255 is reserved for ignore)", C);
    WC_CHECK_ARG(Hs > 0 && Ws > 0, "wc_predict_finish: Hs x Ws = %d x %d must be positive", Hs, Ws);
    WC_CHECK_ARG(H > 0 && W > 0, "wc_predict_finish: H x W = %d x %d must be positive", H, W);
    WC_CHECK_ARG(mode == 0 || mode == 1, "wc_predict_finish: mode = %d, must be 0 (logits) or 1 (probabilities)", mode);
    WC_CHECK_ARG(mode == 0 || (Hs == H && Ws == W), "wc_predict_finish: mode 1 needs Hs == H and Ws == W, got %d x %d and %d x %d",
                 Hs, Ws, H, W);
    WC_CHECK_ARG(alpha256 >= 0 && alpha256 <= 256, "wc_predict_finish: alpha256 = %d outside [0, 256]", alpha256);
    WC_CHECK_ARG(ignore_below >= 0 && ignore_below <= 255, "wc_predict_finish: ignore_below = %d outside [0, 255]", ignore_below);
    WC_CHECK_ARG(image || !overlay_rgb, "wc_predict_finish: overlay_rgb needs image");
    // a workgroup's 32-bit conf_sum cell holds 2^32 / 255 pixels, and the workgroup counts 1024 pixels per pass of its grid-stride loop
    const long groups = (long)H * ((W + 3) / 4);
    const unsigned blocks = wc_hist_blocks(groups, 1);
    const long passes = (groups + 256L * blocks - 1) / (256L * blocks);
    WC_CHECK_ARG(passes * 1024 * 255 < (1L << 32), "wc_predict_finish: H x W = %d x %d is too large for the 32-bit LDS sums", H, W);
    const size_t lds = stats ? (size_t)(2 * C + 1) * sizeof(unsigned int) : 0;
    const float sy = (float)Hs / H, sx = (float)Ws / W;
    if (mode == 0)
        hipLaunchKernelGGL(predict_finish_kernel<0>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, src, image,
                           (unsigned char*)pred_u8, (unsigned char*)cmap_rgb, (unsigned char*)conf_u8, (unsigned char*)overlay_rgb,
                           (unsigned long long*)stats, C, Hs, Ws, H, W, sy, sx, (unsigned int)alpha256, (unsigned int)ignore_below);
    else
        hipLaunchKernelGGL(predict_finish_kernel<1>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, src, image,
                           (unsigned char*)pred_u8, (unsigned char*)cmap_rgb, (unsigned char*)conf_u8, (unsigned char*)overlay_rgb,
                           (unsigned long long*)stats, C, Hs, Ws, H, W, sy, sx, (unsigned int)alpha256, (unsigned int)ignore_below);
    WC_LAUNCH_CHECK("predict_finish_kernel");
    return WC_OK;
}
