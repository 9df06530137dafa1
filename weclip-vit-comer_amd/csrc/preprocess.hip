// CLIP's own preprocessing and the output stage of the stand-alone CAM dumpers.
//
// Replaces, per image of the reference's `clip/generate_cams_voc12.py` / `generate_cams_coco14.py`:
//   generate_cams_voc12.py:76-82   _transform_resize(h, w): Resize((h, w), BICUBIC) -> ToTensor -> Normalize(CLIP mean / std)
//   generate_cams_voc12.py:84-93   img_ms_and_flip: (h, w) = scale * original size rounded up to the patch size, [image, flip]
//   pytorch_grad_cam/utils/image.py:51-61  scale_cam_image([cam], (ori_w, ori_h)): min-max, cv2.resize (bilinear), float16
// Kernels:
//   clipprep_coeff_kernel   Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BICUBIC filter, both axes (resample.h):
//                           per output coordinate {first tap, tap count, 22-bit fixed-point weights}
//   clipprep_hpass_kernel   horizontal pass: uint8 HWC (B,H0,W0,3) -> uint8 (B,H0,w,3); integer arithmetic only
//   clipprep_vpass_kernel   vertical pass -> uint8 (B,h,w,3) (optional), then x / 255, - mean, / std in fp32 -> CHW, and the
//                           horizontally flipped copy (optional)
//   cam_scale_resize_kernel per (image, class) pair: min / max of the refined CAM, (v - min) / (1e-7 + max), bilinear resize
//                           to the pair's own (ori_h, ori_w), fp16 (round to nearest even)
// The tap loads of a thread are issued together: indices are clamped into the row, taps beyond the window carry weight 0.
#include "common.h"
#include "resample.h"

#define PREP_KMAX 33                    // 2 * ceil(2 * 8) + 1 taps: down-scaling by at most 8
#define PREP_ENT PIL_ENT(PREP_KMAX)     // 36
#define CAM_MAX_TOKENS 4096 // refined CAM of one pair held in LDS (a 1024 x 1024 input at patch size 16)

typedef unsigned char u8;

// grid (cdiv(max(h, w), 256), 2).  tab[(axis * OM + o) * PREP_ENT ...], OM = max(h, w); axis 0 = vertical (H0 -> h).
__global__ __launch_bounds__(256) void clipprep_coeff_kernel(int* __restrict__ tab, int H0, int W0, int h, int w, int OM) {
    const int o = blockIdx.x * 256 + threadIdx.x, axis = blockIdx.y;
    const int in_size = axis ? W0 : H0, out_size = axis ? w : h;
    if (o >= out_size) return;
    // a window beyond PREP_KMAX taps is clamped to the table; unreachable: the host refuses down-scaling beyond 8
    pil_coeffs<PilBicubic, PREP_KMAX>(o, in_size, out_size, tab + ((long)axis * OM + o) * PREP_ENT);
}

// grid (cdiv(w, 64), cdiv(H0, 4), B): one thread per pixel of the intermediate
template <int KT>
__global__ __launch_bounds__(256) void clipprep_hpass_kernel(const u8* __restrict__ src, const int* __restrict__ tab,
                                                             u8* __restrict__ mid, int H0, int W0, int w, int OM, int ksize) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= w || y >= H0) return;
    const int* e = tab + ((long)OM + x) * PREP_ENT;
    const int xmin = e[0];
    const u8* row = src + ((long)b * H0 + y) * W0 * 3;
    int a0 = 1 << (PIL_PREC - 1), a1 = a0, a2 = a0;
    const int nk = KT ? KT : ksize;
#pragma unroll
    for (int i = 0; i < nk; ++i) {
        const int k = e[2 + i], sx = min(xmin + i, W0 - 1) * 3;            // beyond the window: weight 0, index clamped
        a0 += k * row[sx];
        a1 += k * row[sx + 1];
        a2 += k * row[sx + 2];
    }
    u8* D = mid + (((long)b * H0 + y) * w + x) * 3;
    D[0] = (u8)pil_clip8(a0);
    D[1] = (u8)pil_clip8(a1);
    D[2] = (u8)pil_clip8(a2);
}

// grid (cdiv(w, 64), cdiv(h, 4), B): one thread per output pixel
template <int KT>
__global__ __launch_bounds__(256) void clipprep_vpass_kernel(const u8* __restrict__ mid, const int* __restrict__ tab,
                                                             u8* __restrict__ out_u8, float* __restrict__ dst,
                                                             float* __restrict__ dst_flip, int H0, int h, int w, int OM, int ksize,
                                                             float m0, float m1, float m2, float s0, float s1, float s2) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= w || y >= h) return;
    const int* e = tab + (long)y * PREP_ENT;
    const int ymin = e[0];
    const u8* col = mid + ((long)b * H0 * w + x) * 3;
    int a0 = 1 << (PIL_PREC - 1), a1 = a0, a2 = a0;
    const int nk = KT ? KT : ksize;
#pragma unroll
    for (int j = 0; j < nk; ++j) {
        const int k = e[2 + j];
        const u8* p = col + (long)min(ymin + j, H0 - 1) * w * 3;
        a0 += k * p[0];
        a1 += k * p[1];
        a2 += k * p[2];
    }
    const int c0 = pil_clip8(a0), c1 = pil_clip8(a1), c2 = pil_clip8(a2);
    if (out_u8) {
        u8* U = out_u8 + (((long)b * h + y) * w + x) * 3;
        U[0] = (u8)c0;
        U[1] = (u8)c1;
        U[2] = (u8)c2;
    }
    // ToTensor: float32(x).div(255); Normalize: sub_(mean).div_(std) -- three separately rounded fp32 operations
    float v0 = (float)c0 / 255.f, v1 = (float)c1 / 255.f, v2 = (float)c2 / 255.f;
    v0 = v0 - m0;
    v1 = v1 - m1;
    v2 = v2 - m2;
    v0 = v0 / s0;
    v1 = v1 / s1;
    v2 = v2 / s2;
    const long plane = (long)h * w;
    float* D = dst + (long)b * 3 * plane + (long)y * w + x;
    D[0] = v0;
    D[plane] = v1;
    D[2 * plane] = v2;
    if (dst_flip) {
        float* F = dst_flip + (long)b * 3 * plane + (long)y * w + (w - 1 - x);
        F[0] = v0;
        F[plane] = v1;
        F[2 * plane] = v2;
    }
}

static int prep_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / out_size, fscale = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(2.0 * fscale) * 2 + 1;
}

static int prep_check(const char* who, int B, int H0, int W0, int h, int w) {
    WC_CHECK_ARG(B > 0 && B <= 65535 && H0 > 0 && W0 > 0 && H0 <= 16384 && W0 <= 16384, "%s: bad argument (batch / source size)", who);
    WC_CHECK_ARG(h > 0 && w > 0 && h <= 16384 && w <= 16384, "%s: bad argument (output size)", who);
    WC_CHECK_ARG(prep_ksize(H0, h) <= PREP_KMAX && prep_ksize(W0, w) <= PREP_KMAX, "%s: down-scaling beyond 8x is not supported", who);
    return WC_OK;
}

extern "C" int wc_clip_preprocess_workspace_bytes(int B, int H0, int W0, int h, int w, long* n_bytes) {
    WC_CHECK_ARG(n_bytes, "wc_clip_preprocess_workspace_bytes: bad argument");
    if (int rc = prep_check("wc_clip_preprocess_workspace_bytes", B, H0, W0, h, w)) return rc;
    const long om = h > w ? h : w;
    *n_bytes = 2 * om * PREP_ENT * (long)sizeof(int) + (long)B * H0 * w * 3;
    return WC_OK;
}

extern "C" int wc_clip_preprocess(const void* src_u8, float* dst, float* dst_flip, void* out_u8, void* ws, long ws_bytes, int B, int H0,
                                  int W0, int h, int w, const float* mean3, const float* std3, void* stream) {
    WC_CHECK_ARG(src_u8 && dst && ws && mean3 && std3, "wc_clip_preprocess: bad argument");
    if (int rc = prep_check("wc_clip_preprocess", B, H0, W0, h, w)) return rc;
    WC_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "wc_clip_preprocess: zero std");
    hipStream_t st = (hipStream_t)stream;
    const int OM = h > w ? h : w;
    WC_CHECK_ARG(ws_bytes >= 2 * (long)OM * PREP_ENT * (long)sizeof(int) + (long)B * H0 * w * 3,
                 "wc_clip_preprocess: workspace too small (see wc_clip_preprocess_workspace_bytes)");
    int* tab = (int*)ws;
    u8* mid = (u8*)ws + 2 * (long)OM * PREP_ENT * sizeof(int);
    hipLaunchKernelGGL(clipprep_coeff_kernel, dim3(wc_cdiv(OM, 256), 2), dim3(256), 0, st, tab, H0, W0, h, w, OM);
    WC_LAUNCH_CHECK("clipprep_coeff_kernel");
    const int kx = prep_ksize(W0, w), ky = prep_ksize(H0, h);
    const dim3 gh(wc_cdiv(w, 64), wc_cdiv(H0, 4), B), gv(wc_cdiv(w, 64), wc_cdiv(h, 4), B);
    if (kx == 5)          // enlarging (the dumpers' scales = [1.0] only ever does): five taps, fully unrolled
        hipLaunchKernelGGL(clipprep_hpass_kernel<5>, gh, dim3(256), 0, st, (const u8*)src_u8, (const int*)tab, mid, H0, W0, w, OM, kx);
    else
        hipLaunchKernelGGL(clipprep_hpass_kernel<0>, gh, dim3(256), 0, st, (const u8*)src_u8, (const int*)tab, mid, H0, W0, w, OM, kx);
    WC_LAUNCH_CHECK("clipprep_hpass_kernel");
    if (ky == 5)
        hipLaunchKernelGGL(clipprep_vpass_kernel<5>, gv, dim3(256), 0, st, (const u8*)mid, (const int*)tab, (u8*)out_u8, dst, dst_flip, H0,
                           h, w, OM, ky, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    else
        hipLaunchKernelGGL(clipprep_vpass_kernel<0>, gv, dim3(256), 0, st, (const u8*)mid, (const int*)tab, (u8*)out_u8, dst, dst_flip, H0,
                           h, w, OM, ky, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    WC_LAUNCH_CHECK("clipprep_vpass_kernel");
    return WC_OK;
}

// ---- output stage ------------------------------------------------------------------------------------------------
// grid (cdiv(max_pixels, 256), P).  sizes (P,2) int32 {ori_h, ori_w}; offsets (P) int64: first element of pair p in `out`.
// Bilinear rule: resample.h -- OpenCV's INTER_LINEAR for float images and F.interpolate(mode="bilinear", align_corners=False), in fp32.
__global__ __launch_bounds__(256) void cam_scale_resize_kernel(const float* __restrict__ cam, const int* __restrict__ sizes,
                                                               const long long* __restrict__ offsets, __half* __restrict__ out, long out_elems,
                                                               int gh, int gw) {
    __shared__ float tile[CAM_MAX_TOKENS];
    __shared__ float red[16];
    const int p = blockIdx.y, t = threadIdx.x, n = gh * gw;
    const int oh = sizes[2 * p], ow = sizes[2 * p + 1];
    if ((long)blockIdx.x * 256 >= (long)oh * ow) return;                   // whole block beyond this pair's map
    const float* C = cam + (long)p * n;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = t; i < n; i += 256) {
        const float v = C[i];
        tile[i] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = block_min(lo, red);
    hi = block_max(hi, red);                                               // (ends with every tile[] write visible)
    const float den = 1e-7f + (hi - lo);                                   // img / (1e-7 + np.max(img - np.min(img)))
    const long i = (long)blockIdx.x * 256 + t;
    if (i >= (long)oh * ow) return;
    const int y = (int)(i / ow), x = (int)(i - (long)y * ow);
    const float sy = (float)gh / (float)oh, sx = (float)gw / (float)ow;
    int y0, y1, x0, x1;
    float ly, lx;
    wc_bil_src(y, gh, sy, y0, y1, ly);
    wc_bil_src(x, gw, sx, x0, x1, lx);
    const float a = (tile[y0 * gw + x0] - lo) / den, b = (tile[y0 * gw + x1] - lo) / den;
    const float c = (tile[y1 * gw + x0] - lo) / den, d = (tile[y1 * gw + x1] - lo) / den;
    const long o = offsets[p] + i;                                         // a table that disagrees with `out` never writes outside it
    if (o >= 0 && o < out_elems) out[o] = __float2half_rn(wc_lerp4(a, b, c, d, ly, lx));
}

// normalise = 0: the plain resize of GradCAM.__call__(target_size=...) (cv2.resize of the map as it is)
__global__ __launch_bounds__(256) void cam_resize_kernel(const float* __restrict__ cam, const int* __restrict__ sizes,
                                                         const long long* __restrict__ offsets, float* __restrict__ out, long out_elems,
                                                         int gh, int gw) {
    const int p = blockIdx.y;
    const int oh = sizes[2 * p], ow = sizes[2 * p + 1];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)oh * ow) return;
    const float* C = cam + (long)p * gh * gw;
    const int y = (int)(i / ow), x = (int)(i - (long)y * ow);
    const float sy = (float)gh / (float)oh, sx = (float)gw / (float)ow;
    int y0, y1, x0, x1;
    float ly, lx;
    wc_bil_src(y, gh, sy, y0, y1, ly);
    wc_bil_src(x, gw, sx, x0, x1, lx);
    const float a = C[y0 * gw + x0], b = C[y0 * gw + x1], c = C[y1 * gw + x0], d = C[y1 * gw + x1];
    const long o = offsets[p] + i;
    if (o >= 0 && o < out_elems) out[o] = wc_lerp4(a, b, c, d, ly, lx);
}

static int cam_check(const char* who, const void* cam, const void* sizes, const void* offsets, const void* out, long out_elems, int P,
                     int gh, int gw, int max_pixels) {
    WC_CHECK_ARG(cam && sizes && offsets && out && out_elems > 0, "%s: bad argument", who);
    WC_CHECK_ARG(P > 0 && P <= 65535 && gh > 0 && gw > 0 && (long)gh * gw <= CAM_MAX_TOKENS, "%s: bad argument (pairs / token grid)", who);
    WC_CHECK_ARG(max_pixels > 0 && max_pixels <= (1 << 28), "%s: bad argument (max_pixels)", who);
    return WC_OK;
}

extern "C" int wc_cam_scale_resize_f16(const float* cam, const int* sizes, const int64_t* offsets, void* out_f16, long out_elems, int P, int gh,
                                       int gw, int max_pixels, void* stream) {
    if (int rc = cam_check("wc_cam_scale_resize_f16", cam, sizes, offsets, out_f16, out_elems, P, gh, gw, max_pixels)) return rc;
    hipLaunchKernelGGL(cam_scale_resize_kernel, dim3(wc_cdiv(max_pixels, 256), P), dim3(256), 0, (hipStream_t)stream, cam, sizes,
                       (const long long*)offsets, (__half*)out_f16, out_elems, gh, gw);
    WC_LAUNCH_CHECK("cam_scale_resize_kernel");
    return WC_OK;
}

extern "C" int wc_cam_resize_f32(const float* cam, const int* sizes, const int64_t* offsets, float* out, long out_elems, int P, int gh, int gw,
                                 int max_pixels, void* stream) {
    if (int rc = cam_check("wc_cam_resize_f32", cam, sizes, offsets, out, out_elems, P, gh, gw, max_pixels)) return rc;
    hipLaunchKernelGGL(cam_resize_kernel, dim3(wc_cdiv(max_pixels, 256), P), dim3(256), 0, (hipStream_t)stream, cam, sizes,
                       (const long long*)offsets, out, out_elems, gh, gw);
    WC_LAUNCH_CHECK("cam_resize_kernel");
    return WC_OK;
}
