// Device-side input pipeline of the training step: uint8 HWC image -> random rescale ->
// horizontal flip -> zero pad + random crop -> mean/std normalise -> float32 CHW.
//
// Replaces the host-side numpy / PIL chain of the reference loader, per image:
//   datasets/transforms.py:26-49  random_scaling (PIL Image.BILINEAR resize to (int(s*w), int(s*h)), uint8 result)
//   datasets/transforms.py:70-84  random_fliplr
//   datasets/transforms.py:119-176 random_crop (pad to >= crop with mean_rgb = [0,0,0] at a random offset, crop window)
//   datasets/transforms.py:8-15   normalize_img ((x - mean) / std per channel), then HWC -> CHW (datasets/voc.py:137-143)
// The random draws stay on the host (a few scalars per image, data.DeviceAugment); the kernels apply them.
//
// PIL's BILINEAR (Pillow, ImagingResample 8 bits per channel) is NOT plain half-pixel bilinear: it is a separable
// triangle filter whose support grows with the down-scaling ratio (support = max(in / out, 1), up to
// 2 * ceil(support) + 1 taps), evaluated with coefficients normalised in double precision and rounded to 22-bit fixed
// point, a horizontal pass whose result is rounded to uint8, then a vertical pass over those uint8 values.  resample.h
// follows that arithmetic step by step (same double-precision operation order, same integer rounding), so
// the output equals PIL's on every pixel, up- and down-scaling (tests/golden/augment_ref.npz, made by the reference's
// own transforms with real PIL).
//   aug_coeff_kernel: per image and axis, for the `crop` output coordinates only: first tap, tap count and the
//                     fixed-point coefficients (or "outside the rescaled image": zero padding);
//   augment_normalize_kernel: one thread per output pixel, ny x nx taps (3 x 3 when up-scaling, 5 x 5 at scale 0.5).
#include "common.h"
#include "resample.h"
#include "augment_shape.h"

struct AugParams {      // one per image, 8 ints / floats = 32 B
    float scale;        // s of random_scaling
    int flip;           // 1: np.fliplr
    int rh, rw;         // rescaled size (int(s*h), int(s*w))
    int pad_y, pad_x;   // where the rescaled image sits in the padded canvas (H_pad, W_pad)
    int crop_y, crop_x; // crop window origin in the canvas (H_start, W_start)
};

// grid (cdiv(crop, 256), 2, B); axis 0 = rows, 1 = columns.  RAGGED: per-image source size and offset (augment_shape.h)
template <bool RAGGED>
__global__ __launch_bounds__(256) void aug_coeff_kernel(const AugParams* __restrict__ params, int* __restrict__ tab, int Hs, int Ws,
                                                         int crop, const long long* __restrict__ offsets,
                                                         const int* __restrict__ sizes, long src_bytes) {
    const int o = blockIdx.x * 256 + threadIdx.x, axis = blockIdx.y, b = blockIdx.z;
    if (o >= crop) return;
    const AugParams p = params[b];
    const AugShape sh = aug_shape<RAGGED>(b, Hs, Ws, offsets, sizes, src_bytes);
    const int in_size = axis ? sh.W : sh.H, out_size = axis ? p.rw : p.rh;
    int r = o + (axis ? p.crop_x - p.pad_x : p.crop_y - p.pad_y);          // coordinate in the rescaled image
    int* e = tab + (((long)b * 2 + axis) * crop + o) * AUG_ENT;
    if (RAGGED && !sh.ok) {                                                // image outside the packed buffer: POISONED,
        e[0] = 0;                                                          // nothing of it is read
        e[1] = -1;
        return;
    }
    if (r < 0 || r >= out_size) {
        e[0] = 0;
        e[1] = 0;                                                          // canvas padding
        return;
    }
    if (axis && p.flip) r = out_size - 1 - r;
    // down-scaling beyond 4x: the table cannot hold Pillow's filter -> the pixel is POISONED (NaN), never a silently different
    // filter (checked precondition).  The weights of the capped window stay behind e[1] = -1; they mean nothing and are never read.
    if (pil_coeffs<PilTriangle, AUG_KMAX>(r, in_size, out_size, e) > AUG_KMAX) {
        e[0] = 0;
        e[1] = -1;
    }
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void augment_normalize_kernel(const unsigned char* __restrict__ src, const int* __restrict__ tab,
                                                                 float* __restrict__ dst, int Hs, int Ws, int crop,
                                                                 float m0, float m1, float m2, float s0, float s1, float s2,
                                                                 const long long* __restrict__ offsets,
                                                                 const int* __restrict__ sizes, long src_bytes) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= crop || y >= crop) return;
    if constexpr (RAGGED) {                                                // taps lie in [0, H) x [0, W) of a checked image
        const AugShape sh = aug_shape<true>(b, Hs, Ws, offsets, sizes, src_bytes);
        Ws = sh.W;
        src += sh.off;
    } else {
        src += (long)b * Hs * Ws * 3;
    }
    const int* ey = tab + (((long)b * 2 + 0) * crop + y) * AUG_ENT;       // one entry per wave
    const int* ex = tab + (((long)b * 2 + 1) * crop + x) * AUG_ENT;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;                                    // canvas padding (mean_rgb = [0, 0, 0])
    int c0, c1, c2;
    const int got = pil_gather_rgb8(ey, ex, src, Ws, c0, c1, c2);
    if (got < 0) {                                                         // precondition in/out <= 4 violated (aug_coeff_kernel)
        v0 = v1 = v2 = __builtin_nanf("");
    } else if (got) {
        v0 = (float)c0;
        v1 = (float)c1;
        v2 = (float)c2;
    }
    const long plane = (long)crop * crop;
    float* D = dst + (long)b * 3 * plane + (long)y * crop + x;
    D[0] = (v0 - m0) / s0;
    D[plane] = (v1 - m1) / s1;
    D[2 * plane] = (v2 - m2) / s2;
}

extern "C" int wc_augment_workspace_ints(int B, int crop, long* n_ints) {
    WC_CHECK_ARG(n_ints && B > 0 && crop > 0, "wc_augment_workspace_ints: bad argument");
    *n_ints = (long)B * 2 * crop * AUG_ENT;
    return WC_OK;
}

extern "C" int wc_augment_normalize(const void* src_u8, const void* params, float* dst, int* coeff_ws, int B, int Hs, int Ws,
                                    int crop, const float* mean3, const float* std3, void* stream) {
    WC_CHECK_ARG(src_u8 && params && dst && coeff_ws && mean3 && std3 && B > 0 && B <= 65535 && Hs > 0 && Ws > 0 && crop > 0,
                 "wc_augment_normalize: bad argument");
    WC_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "wc_augment_normalize: zero std");
    hipLaunchKernelGGL(aug_coeff_kernel<false>, dim3(wc_cdiv(crop, 256), 2, B), dim3(256), 0, (hipStream_t)stream,
                       (const AugParams*)params, coeff_ws, Hs, Ws, crop, nullptr, nullptr, 0L);
    WC_LAUNCH_CHECK("aug_coeff_kernel");
    hipLaunchKernelGGL(augment_normalize_kernel<false>, dim3(wc_cdiv(crop, 64), wc_cdiv(crop, 4), B), dim3(256), 0,
                       (hipStream_t)stream, (const unsigned char*)src_u8, (const int*)coeff_ws, dst, Hs, Ws, crop, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2], nullptr, nullptr, 0L);
    WC_LAUNCH_CHECK("augment_normalize_kernel");
    return WC_OK;
}

extern "C" int wc_augment_normalize_ragged(const void* src_u8, long src_bytes, const int64_t* offsets, const int* sizes,
                                           const void* params, float* dst, int* coeff_ws, int B, int crop, const float* mean3,
                                           const float* std3, void* stream) {
    WC_CHECK_ARG(src_u8 && src_bytes >= 3 && offsets && sizes && params && dst && coeff_ws && mean3 && std3 && B > 0 && B <= 65535 &&
                     crop > 0,
                 "wc_augment_normalize_ragged: bad argument");
    WC_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "wc_augment_normalize_ragged: zero std");
    hipLaunchKernelGGL(aug_coeff_kernel<true>, dim3(wc_cdiv(crop, 256), 2, B), dim3(256), 0, (hipStream_t)stream,
                       (const AugParams*)params, coeff_ws, 0, 0, crop, (const long long*)offsets, sizes, src_bytes);
    WC_LAUNCH_CHECK("aug_coeff_kernel<ragged>");
    hipLaunchKernelGGL(augment_normalize_kernel<true>, dim3(wc_cdiv(crop, 64), wc_cdiv(crop, 4), B), dim3(256), 0,
                       (hipStream_t)stream, (const unsigned char*)src_u8, (const int*)coeff_ws, dst, 0, 0, crop, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2], (const long long*)offsets, sizes, src_bytes);
    WC_LAUNCH_CHECK("augment_normalize_kernel<ragged>");
    return WC_OK;
}

// aug=False path (datasets/voc.py:137-143, :247-249 without augmentation): normalize_img on the uint8 image itself.  numpy
// evaluates (uint8 - float) / float in DOUBLE there and rounds once on the store into the float32 array; float32 arithmetic
// differs from that in the last place for about half of the 768 (value, channel) pairs, hence double mean / std here.
// grid cdiv(H * W, 256): one thread per pixel.
__global__ __launch_bounds__(256) void normalize_u8_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ lab,
                                                            float* __restrict__ dst, long long* __restrict__ dst_lab, long n,
                                                            double m0, double m1, double m2, double s0, double s1, double s2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dst[i] = (float)(((double)src[3 * i] - m0) / s0);
    dst[n + i] = (float)(((double)src[3 * i + 1] - m1) / s1);
    dst[2 * n + i] = (float)(((double)src[3 * i + 2] - m2) / s2);
    if (lab) dst_lab[i] = lab[i];
}

extern "C" int wc_normalize_u8(const void* src_u8, const void* lab_u8, float* dst, int64_t* dst_label, int H, int W,
                               const double* mean3, const double* std3, void* stream) {
    WC_CHECK_ARG(src_u8 && dst && mean3 && std3 && H > 0 && W > 0 && H <= AUG_MAX_SIDE && W <= AUG_MAX_SIDE,
                 "wc_normalize_u8: bad argument");
    WC_CHECK_ARG((lab_u8 == nullptr) == (dst_label == nullptr), "wc_normalize_u8: lab_u8 and dst_label go together");
    WC_CHECK_ARG(std3[0] != 0.0 && std3[1] != 0.0 && std3[2] != 0.0, "wc_normalize_u8: zero std");
    const long n = (long)H * W;
    hipLaunchKernelGGL(normalize_u8_kernel, dim3(wc_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src_u8,
                       (const unsigned char*)lab_u8, dst, (long long*)dst_label, n, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                       std3[2]);
    WC_LAUNCH_CHECK("normalize_u8_kernel");
    return WC_OK;
}
