// Label-aware device-side input pipeline of the fully supervised variant: uint8 HWC image + uint8 label map
// -> (optional random rescale) -> horizontal flip -> photometric distortion -> pad + label-aware random crop -> normalise
// -> float32 CHW image, int64 label, img_box.
//
// Replaces the host chain of the reference's `VOC12SegDataset.__transforms` (datasets/voc.py:216-251), per image:
//   datasets/transforms.py:35-51   _img_rescaling(image, label): PIL BILINEAR for the image, PIL NEAREST for the label
//   datasets/transforms.py:75-88   random_fliplr(image, label)
//   datasets/transforms.py:178-264 PhotoMetricDistortion (brightness, contrast before or after, saturation, hue; uint8)
//   datasets/transforms.py:119-176 random_crop(image, label): image padded with mean_rgb = [0,0,0], label with ignore_index,
//                                  crop box from get_random_cropbox (:137-156): up to 10 candidates, the first whose most
//                                  frequent non-ignored class covers < 0.75 of the non-ignored pixels, else the last
//   datasets/transforms.py:8-15    normalize_img, then HWC -> CHW (voc.py:247-249)
// All random draws (the candidates included) are made on the host (data.DeviceSegAugment); nothing returns to the host:
//   segaug_index_kernel  per image and axis, for every canvas coordinate: the source label row / column behind it
//                        (pad -> flip -> Pillow NEAREST), or -1 in the padding
//   segaug_hist_kernel   per (image, candidate, 32-row slab): class histogram of the label as the crop would see it
//   segaug_select_kernel per image: integer acceptance rule over the candidates -> chosen box, index, img_box
//   segaug_coeff_kernel  Pillow BILINEAR tables of the chosen window (resample.h, the tables of augment.hip's aug_coeff_kernel)
//   segaug_gather_kernel one thread per output pixel: image taps -> photometric chain on the uint8 triple -> normalise;
//                        label through the index tables
#include "common.h"
#include "resample.h"
#include "augment_shape.h"

#define SEG_MAX_CAND 16
#define SEG_SLAB 32         // rows of the crop window per histogram block
#define SEG_RUN 16          // consecutive pixels of a row per thread

struct SegAugParams {   // one per image, 16 x 32 bit = 64 B
    float scale;        // s of random_scaling (1 without rescale; informational, the kernels use rh / rw)
    int flip;           // 1: np.fliplr of image and label
    int rh, rw;         // rescaled size (int(s*h), int(s*w)); (Hs, Ws) without rescale
    int pad_y, pad_x;   // H_pad, W_pad of random_crop
    int photo;          // bit 0 brightness, 1 contrast, 2 saturation, 3 hue gates; bit 4: `mode` (1: contrast before saturation)
    float beta;         // brightness offset
    float alpha_c;      // contrast factor
    float alpha_s;      // saturation factor
    int hue;            // hue offset in [-18, 18)
    int reserved[5];
};

typedef unsigned char u8;

__device__ __forceinline__ int seg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- OpenCV's 8-bit BGR <-> HSV (H in [0,180)), restated in tests/photo_ref.py ------------------------------------
// round-half-even of num / den (num, den > 0): saturate_cast<int>(double) of the division tables, without floating point
__device__ __forceinline__ int seg_rdiv(int num, int den) {
    const int q = num / den, r2 = 2 * (num - q * den);
    return q + ((r2 > den || (r2 == den && (q & 1))) ? 1 : 0);
}

__device__ __forceinline__ void seg_bgr2hsv(int b, int g, int r, int& h, int& s, int& v) {
    v = max(b, max(g, r));
    const int vmin = min(b, min(g, r)), diff = v - vmin;
    const int sdiv = v ? seg_rdiv(255 << 12, v) : 0, hdiv = diff ? seg_rdiv(180 << 12, 6 * diff) : 0;
    s = (diff * sdiv + (1 << 11)) >> 12;
    int hh = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    hh = (hh * hdiv + (1 << 11)) >> 12;                 // arithmetic shift: hh may be negative
    hh += hh < 0 ? 180 : 0;
    h = seg_clampi(hh, 0, 255);
    s = s & 255;
}

__device__ __forceinline__ int seg_sat8(float f) {
    const int i = (int)rintf(f);                        // cvRound: half to even
    return seg_clampi(i, 0, 255);
}

__device__ __forceinline__ void seg_hsv2bgr(int H, int S, int V, int& b, int& g, int& r) {
    float h = (float)H;
    const float s = (float)S * (1.f / 255.f), v = (float)V * (1.f / 255.f);
    float fb = v, fg = v, fr = v;
    if (s != 0.f) {
        h *= 6.f / 180.f;
        h = fmodf(h, 6.f);
        int sector = (int)floorf(h);
        h -= (float)sector;
        if ((unsigned)sector >= 6u) {
            sector = 0;
            h = 0.f;
        }
        const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * h), t3 = v * (1.f - s * (1.f - h));
        // sector_data {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}: indices of (b, g, r) into tab
        fb = sector == 0 ? t1 : sector == 1 ? t1 : sector == 2 ? t3 : sector == 3 ? t0 : sector == 4 ? t0 : t2;
        fg = sector == 0 ? t3 : sector == 1 ? t0 : sector == 2 ? t0 : sector == 3 ? t2 : sector == 4 ? t1 : t1;
        fr = sector == 0 ? t0 : sector == 1 ? t2 : sector == 2 ? t1 : sector == 3 ? t1 : sector == 4 ? t3 : t0;
    }
    b = seg_sat8(fb * 255.f);
    g = seg_sat8(fg * 255.f);
    r = seg_sat8(fr * 255.f);
}

// PhotoMetricDistortion.convert (transforms.py:191-195): clip(float32(x) * alpha + beta, 0, 255) truncated to uint8
__device__ __forceinline__ int seg_convert(int x, float alpha, float beta) {
    float f = (float)x * alpha;
    f = f + beta;
    f = fminf(fmaxf(f, 0.f), 255.f);
    return (int)f;
}

// transforms.py:235-264 on one uint8 triple; channel 0 is treated as blue (the reference hands its RGB image to bgr2hsv)
__device__ __forceinline__ void seg_photometric(const SegAugParams& p, int& c0, int& c1, int& c2) {
    if (p.photo & 1) {
        c0 = seg_convert(c0, 1.f, p.beta);
        c1 = seg_convert(c1, 1.f, p.beta);
        c2 = seg_convert(c2, 1.f, p.beta);
    }
    const bool contrast = (p.photo & 2) != 0, first = (p.photo & 16) != 0;
    if (contrast && first) {
        c0 = seg_convert(c0, p.alpha_c, 0.f);
        c1 = seg_convert(c1, p.alpha_c, 0.f);
        c2 = seg_convert(c2, p.alpha_c, 0.f);
    }
    if (p.photo & 4) {
        int h, s, v;
        seg_bgr2hsv(c0, c1, c2, h, s, v);
        s = seg_convert(s, p.alpha_s, 0.f);
        seg_hsv2bgr(h, s, v, c0, c1, c2);
    }
    if (p.photo & 8) {
        int h, s, v;
        seg_bgr2hsv(c0, c1, c2, h, s, v);
        h = (h + p.hue) % 180;
        h += h < 0 ? 180 : 0;
        seg_hsv2bgr(h, s, v, c0, c1, c2);
    }
    if (contrast && !first) {
        c0 = seg_convert(c0, p.alpha_c, 0.f);
        c1 = seg_convert(c1, p.alpha_c, 0.f);
        c2 = seg_convert(c2, p.alpha_c, 0.f);
    }
}

// n triples, forward (BGR -> HSV) or inverse: the conversions alone, for the exhaustive comparison with tests/photo_ref.py
__global__ __launch_bounds__(256) void seg_hsv8_kernel(const u8* __restrict__ src, u8* __restrict__ dst, long n, int inverse) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int a = src[3 * i], b = src[3 * i + 1], c = src[3 * i + 2];
    int x, y, z;
    if (inverse) seg_hsv2bgr(a, b, c, x, y, z);
    else seg_bgr2hsv(a, b, c, x, y, z);
    dst[3 * i] = (u8)x;
    dst[3 * i + 1] = (u8)y;
    dst[3 * i + 2] = (u8)z;
}

// ---- geometry ----------------------------------------------------------------------------------------------------
// grid (cdiv(CM, 256), 2, B).  idx[(b * 2 + axis) * CM + u]: source row / column of the label behind canvas coordinate u.
// RAGGED: per-image source size and offset (augment_shape.h); an image outside the packed buffer is all padding here.
template <bool RAGGED>
__global__ __launch_bounds__(256) void segaug_index_kernel(const SegAugParams* __restrict__ params, int* __restrict__ idx, int Hs,
                                                            int Ws, int crop, int CM, const long long* __restrict__ offsets,
                                                            const int* __restrict__ sizes, long src_bytes) {
    const int u = blockIdx.x * 256 + threadIdx.x, axis = blockIdx.y, b = blockIdx.z;
    if (u >= CM) return;
    const SegAugParams p = params[b];
    const AugShape sh = aug_shape<RAGGED>(b, Hs, Ws, offsets, sizes, src_bytes);
    const int in_size = axis ? sh.W : sh.H, out_size = axis ? p.rw : p.rh;
    int r = u - (axis ? p.pad_x : p.pad_y);
    int v = -1;
    if (r >= 0 && r < out_size && out_size <= CM && sh.ok) {
        if (axis && p.flip) r = out_size - 1 - r;
        if (out_size == in_size) {
            v = r;
        } else {
            // Pillow ImagingScaleAffine with the NEAREST filter (Image.resize -> ImagingTransform): the source coordinate is
            // accumulated in double precision, xo = a/2, xo += a per output pixel, a = in / out
            const double a = (double)(float)in_size / out_size;
            double xo = a * 0.5;
            for (int i = 0; i < r; ++i) xo += a;
            v = seg_clampi((int)xo, 0, in_size - 1);
        }
    }
    idx[((long)b * 2 + axis) * CM + u] = v;
}

__device__ __forceinline__ void seg_candidate(const SegAugParams& p, const int* __restrict__ cand, int b, int c, int NC, int crop,
                                              int CM, int& cy, int& cx) {
    // a valid candidate lies in [0, canvas - crop]; anything else is clamped into the canvas, never read out of bounds
    const int ch = min(max(crop, p.rh), CM), cw = min(max(crop, p.rw), CM);
    cy = seg_clampi(cand[((long)b * NC + c) * 2], 0, ch - crop);
    cx = seg_clampi(cand[((long)b * NC + c) * 2 + 1], 0, cw - crop);
}

// grid (cdiv(crop, SEG_SLAB), NC, B).  Label maps are piecewise constant, so a wave's 64 lanes would all hit one bin: every
// thread folds SEG_RUN consecutive pixels into runs first (one LDS atomic per run), into its wave's private 256 bins.
template <bool RAGGED>
__global__ __launch_bounds__(256) void segaug_hist_kernel(const u8* __restrict__ lab, const SegAugParams* __restrict__ params,
                                                           const int* __restrict__ cand, const int* __restrict__ idx,
                                                           int* __restrict__ hist, int Hs, int Ws, int crop, int CM, int NC,
                                                           int ignore, const long long* __restrict__ offsets,
                                                           const int* __restrict__ sizes, long src_bytes) {
    __shared__ int h[4][256];
    const int t = threadIdx.x, w = t >> 6, c = blockIdx.y, b = blockIdx.z;
    h[0][t] = h[1][t] = h[2][t] = h[3][t] = 0;
    __syncthreads();
    const SegAugParams p = params[b];
    int cy, cx;
    seg_candidate(p, cand, b, c, NC, crop, CM, cy, cx);
    const int* ty = idx + ((long)b * 2 + 0) * CM + cy;
    const int* tx = idx + ((long)b * 2 + 1) * CM + cx;
    if constexpr (RAGGED) {                                                // indices lie in [0, H) x [0, W) of a checked image
        const AugShape sh = aug_shape<true>(b, Hs, Ws, offsets, sizes, src_bytes);
        Ws = sh.W;
        lab += sh.off / 3;
    } else {
        lab += (long)b * Hs * Ws;
    }
    const u8* L = lab;
    const int nseg = (crop + SEG_RUN - 1) / SEG_RUN, y0 = blockIdx.x * SEG_SLAB;
    for (int i = t; i < SEG_SLAB * nseg; i += 256) {
        const int y = y0 + i / nseg, xs = (i % nseg) * SEG_RUN;
        if (y >= crop) break;
        const int iy = ty[y];
        const u8* row = L + (long)max(iy, 0) * Ws;
        int ix[SEG_RUN], v[SEG_RUN];
#pragma unroll
        for (int k = 0; k < SEG_RUN; ++k) ix[k] = tx[min(xs + k, crop - 1)];
#pragma unroll
        for (int k = 0; k < SEG_RUN; ++k) v[k] = row[max(ix[k], 0)];
        int val = -1, cnt = 0;
#pragma unroll
        for (int k = 0; k < SEG_RUN; ++k) {
            const int vk = (iy < 0 || ix[k] < 0) ? ignore : v[k];
            if (xs + k < crop) {
                if (vk == val) {
                    ++cnt;
                } else {
                    if (cnt) atomicAdd(&h[w][val], cnt);
                    val = vk;
                    cnt = 1;
                }
            }
        }
        if (cnt) atomicAdd(&h[w][val], cnt);
    }
    __syncthreads();
    const int s = h[0][t] + h[1][t] + h[2][t] + h[3][t];
    if (s) atomicAdd(&hist[((long)b * NC + c) * 256 + t], s);
}

__device__ __forceinline__ int seg_wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int seg_wave_imax(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// grid B, 256 threads (one per class bin).  sel[b] = {crop_y, crop_x, chosen candidate, accepted}; img_box[b] as transforms.py:162-166.
__global__ __launch_bounds__(256) void segaug_select_kernel(const SegAugParams* __restrict__ params, const int* __restrict__ cand,
                                                             const int* __restrict__ hist, int* __restrict__ sel,
                                                             int* __restrict__ img_box, int crop, int CM, int NC, int ignore) {
    __shared__ int red[2][SEG_MAX_CAND][4];
    const int t = threadIdx.x, b = blockIdx.x;
    for (int c = 0; c < NC; ++c) {
        int v = hist[((long)b * NC + c) * 256 + t];
        if (t == ignore) v = 0;
        const int s = seg_wave_isum(v), m = seg_wave_imax(v);
        if ((t & 63) == 0) {
            red[0][c][t >> 6] = s;
            red[1][c][t >> 6] = m;
        }
    }
    __syncthreads();
    if (t) return;
    int chosen = NC - 1, accepted = 0;
    for (int c = 0; c < NC; ++c) {
        const int n_valid = red[0][c][0] + red[0][c][1] + red[0][c][2] + red[0][c][3];
        const int mx = max(max(red[1][c][0], red[1][c][1]), max(red[1][c][2], red[1][c][3]));
        // np.max(cnt) / np.sum(cnt) < 0.75 on a non-empty cnt, in integers (crop <= 4096: 4 * max < 2^27)
        if (n_valid > 0 && 4 * mx < 3 * n_valid) {
            chosen = c;
            accepted = 1;
            break;
        }
    }
    const SegAugParams p = params[b];
    int cy, cx;
    seg_candidate(p, cand, b, chosen, NC, crop, CM, cy, cx);
    sel[b * 4 + 0] = cy;
    sel[b * 4 + 1] = cx;
    sel[b * 4 + 2] = chosen;
    sel[b * 4 + 3] = accepted;
    img_box[b * 4 + 0] = max(p.pad_y - cy, 0);
    img_box[b * 4 + 1] = min(cy + crop, p.pad_y + p.rh);
    img_box[b * 4 + 2] = max(p.pad_x - cx, 0);
    img_box[b * 4 + 3] = min(cx + crop, p.pad_x + p.rw);
}

// grid (cdiv(crop, 256), 2, B): augment.hip's aug_coeff_kernel with the crop origin read from sel
template <bool RAGGED>
__global__ __launch_bounds__(256) void segaug_coeff_kernel(const SegAugParams* __restrict__ params, const int* __restrict__ sel,
                                                            int* __restrict__ tab, int Hs, int Ws, int crop, int CM,
                                                            const long long* __restrict__ offsets, const int* __restrict__ sizes,
                                                            long src_bytes) {
    const int o = blockIdx.x * 256 + threadIdx.x, axis = blockIdx.y, b = blockIdx.z;
    if (o >= crop) return;
    const SegAugParams p = params[b];
    const AugShape sh = aug_shape<RAGGED>(b, Hs, Ws, offsets, sizes, src_bytes);
    const int in_size = axis ? sh.W : sh.H, out_size = axis ? p.rw : p.rh;
    int r = o + sel[b * 4 + axis] - (axis ? p.pad_x : p.pad_y);           // coordinate in the rescaled image
    int* e = tab + (((long)b * 2 + axis) * crop + o) * AUG_ENT;
    if (p.rh < 1 || p.rw < 1 || p.rh > CM || p.rw > CM || !sh.ok) {        // record outside the checked preconditions: poison
        e[0] = 0;
        e[1] = -1;
        return;
    }
    if (r < 0 || r >= out_size) {
        e[0] = 0;
        e[1] = 0;                                                          // canvas padding
        return;
    }
    if (axis && p.flip) r = out_size - 1 - r;
    // down-scaling beyond 4x: POISONED (NaN), as augment.hip; the weights left behind e[1] = -1 mean nothing and are never read
    if (pil_coeffs<PilTriangle, AUG_KMAX>(r, in_size, out_size, e) > AUG_KMAX) {
        e[0] = 0;
        e[1] = -1;
    }
}

// grid (cdiv(crop, 64), cdiv(crop, 4), B): one thread per output pixel
template <bool RAGGED>
__global__ __launch_bounds__(256) void segaug_gather_kernel(const u8* __restrict__ src, const u8* __restrict__ lab,
                                                             const SegAugParams* __restrict__ params, const int* __restrict__ sel,
                                                             const int* __restrict__ idx, const int* __restrict__ tab,
                                                             float* __restrict__ dst, long long* __restrict__ dst_lab, int Hs, int Ws,
                                                             int crop, int CM, int ignore, float m0, float m1, float m2, float s0,
                                                             float s1, float s2, const long long* __restrict__ offsets,
                                                             const int* __restrict__ sizes, long src_bytes) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= crop || y >= crop) return;
    if constexpr (RAGGED) {
        const AugShape sh = aug_shape<true>(b, Hs, Ws, offsets, sizes, src_bytes);
        Ws = sh.W;
        src += sh.off;
        lab += sh.off / 3;
    } else {
        src += (long)b * Hs * Ws * 3;
        lab += (long)b * Hs * Ws;
    }
    const SegAugParams p = params[b];
    const int cy = sel[b * 4], cx = sel[b * 4 + 1];                        // clamped into the canvas by segaug_select_kernel
    // label: pad -> flip -> NEAREST through the index tables
    const int iy = idx[((long)b * 2 + 0) * CM + cy + y], ix = idx[((long)b * 2 + 1) * CM + cx + x];
    const int lv = lab[(long)max(iy, 0) * Ws + max(ix, 0)];
    const long plane = (long)crop * crop;
    dst_lab[(long)b * plane + (long)y * crop + x] = (iy < 0 || ix < 0) ? ignore : lv;

    const int* ey = tab + (((long)b * 2 + 0) * crop + y) * AUG_ENT;
    const int* ex = tab + (((long)b * 2 + 1) * crop + x) * AUG_ENT;
    // canvas padding (mean_rgb = [0, 0, 0]) is not distorted: the reference pads after PhotoMetricDistortion
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    int c0, c1, c2;
    const int got = pil_gather_rgb8(ey, ex, src, Ws, c0, c1, c2);
    if (got < 0) {
        v0 = v1 = v2 = __builtin_nanf("");
    } else if (got) {
        if (p.photo & 15) seg_photometric(p, c0, c1, c2);
        v0 = (float)c0;
        v1 = (float)c1;
        v2 = (float)c2;
    }
    float* D = dst + (long)b * 3 * plane + (long)y * crop + x;
    D[0] = (v0 - m0) / s0;
    D[plane] = (v1 - m1) / s1;
    D[2 * plane] = (v2 - m2) / s2;
}

static int seg_check_shape(const char* who, int B, int Hs, int Ws, int crop, int canvas_max, int n_cand, int ignore_index) {
    WC_CHECK_ARG(B > 0 && B <= 65535 && Hs > 0 && Ws > 0 && Hs <= 16384 && Ws <= 16384, "%s: bad argument (batch / source size)", who);
    WC_CHECK_ARG(crop > 0 && crop <= 4096, "%s: crop must be in [1, 4096]", who);
    WC_CHECK_ARG(canvas_max >= crop && canvas_max <= 65536, "%s: canvas_max must be in [crop, 65536]", who);
    WC_CHECK_ARG(n_cand >= 1 && n_cand <= SEG_MAX_CAND, "%s: n_cand must be in [1, 16]", who);
    WC_CHECK_ARG(ignore_index >= 0 && ignore_index <= 255, "%s: ignore_index must be in [0, 255]", who);
    return WC_OK;
}

extern "C" int wc_seg_augment_workspace_ints(int B, int crop, int canvas_max, int n_cand, long* n_ints) {
    WC_CHECK_ARG(n_ints, "wc_seg_augment_workspace_ints: bad argument");
    if (int rc = seg_check_shape("wc_seg_augment_workspace_ints", B, 1, 1, crop, canvas_max, n_cand, 0)) return rc;
    *n_ints = (long)B * 2 * canvas_max + (long)B * n_cand * 256 + (long)B * 2 * crop * AUG_ENT;
    return WC_OK;
}

template <bool RAGGED>
static int seg_select_launch(const void* lab_u8, const void* params, const int* cand, int* sel, int* img_box, int* ws, int B, int Hs,
                             int Ws, int crop, int CM, int NC, int ignore, hipStream_t st, const long long* offsets,
                             const int* sizes, long src_bytes) {
    int* idx = ws;
    int* hist = ws + (long)B * 2 * CM;
    hipLaunchKernelGGL(segaug_index_kernel<RAGGED>, dim3(wc_cdiv(CM, 256), 2, B), dim3(256), 0, st, (const SegAugParams*)params, idx,
                       Hs, Ws, crop, CM, offsets, sizes, src_bytes);
    WC_LAUNCH_CHECK("segaug_index_kernel");
    if (hipMemsetAsync(hist, 0, sizeof(int) * (size_t)B * NC * 256, st) != hipSuccess) {
        wc_set_error("wc_seg_augment: hipMemsetAsync failed");
        return WC_ERR_HIP;
    }
    hipLaunchKernelGGL(segaug_hist_kernel<RAGGED>, dim3(wc_cdiv(crop, SEG_SLAB), NC, B), dim3(256), 0, st, (const u8*)lab_u8,
                       (const SegAugParams*)params, cand, (const int*)idx, hist, Hs, Ws, crop, CM, NC, ignore, offsets, sizes,
                       src_bytes);
    WC_LAUNCH_CHECK("segaug_hist_kernel");
    hipLaunchKernelGGL(segaug_select_kernel, dim3(B), dim3(256), 0, st, (const SegAugParams*)params, cand, (const int*)hist, sel,
                       img_box, crop, CM, NC, ignore);
    WC_LAUNCH_CHECK("segaug_select_kernel");
    return WC_OK;
}

extern "C" int wc_seg_crop_select(const void* lab_u8, const void* params, const int* cand, int* sel, int* img_box, int* ws, int B,
                                  int Hs, int Ws, int crop, int canvas_max, int n_cand, int ignore_index, void* stream) {
    WC_CHECK_ARG(lab_u8 && params && cand && sel && img_box && ws, "wc_seg_crop_select: bad argument");
    if (int rc = seg_check_shape("wc_seg_crop_select", B, Hs, Ws, crop, canvas_max, n_cand, ignore_index)) return rc;
    return seg_select_launch<false>(lab_u8, params, cand, sel, img_box, ws, B, Hs, Ws, crop, canvas_max, n_cand, ignore_index,
                                    (hipStream_t)stream, nullptr, nullptr, 0L);
}

template <bool RAGGED>
static int seg_augment_launch(const void* src_u8, const void* lab_u8, const void* params, const int* cand, float* dst,
                              int64_t* dst_label, int* sel, int* img_box, int* ws, int B, int Hs, int Ws, int crop, int CM, int n_cand,
                              int ignore_index, const float* mean3, const float* std3, hipStream_t st, const long long* offsets,
                              const int* sizes, long src_bytes) {
    if (int rc = seg_select_launch<RAGGED>(lab_u8, params, cand, sel, img_box, ws, B, Hs, Ws, crop, CM, n_cand, ignore_index, st,
                                           offsets, sizes, src_bytes))
        return rc;
    const int* idx = ws;
    int* tab = ws + (long)B * 2 * CM + (long)B * n_cand * 256;
    hipLaunchKernelGGL(segaug_coeff_kernel<RAGGED>, dim3(wc_cdiv(crop, 256), 2, B), dim3(256), 0, st, (const SegAugParams*)params,
                       (const int*)sel, tab, Hs, Ws, crop, CM, offsets, sizes, src_bytes);
    WC_LAUNCH_CHECK("segaug_coeff_kernel");
    hipLaunchKernelGGL(segaug_gather_kernel<RAGGED>, dim3(wc_cdiv(crop, 64), wc_cdiv(crop, 4), B), dim3(256), 0, st, (const u8*)src_u8,
                       (const u8*)lab_u8, (const SegAugParams*)params, (const int*)sel, idx, (const int*)tab, dst,
                       (long long*)dst_label, Hs, Ws, crop, CM, ignore_index, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                       offsets, sizes, src_bytes);
    WC_LAUNCH_CHECK("segaug_gather_kernel");
    return WC_OK;
}

extern "C" int wc_seg_augment(const void* src_u8, const void* lab_u8, const void* params, const int* cand, float* dst,
                              int64_t* dst_label, int* sel, int* img_box, int* ws, int B, int Hs, int Ws, int crop, int canvas_max,
                              int n_cand, int ignore_index, const float* mean3, const float* std3, void* stream) {
    WC_CHECK_ARG(src_u8 && lab_u8 && params && cand && dst && dst_label && sel && img_box && ws && mean3 && std3,
                 "wc_seg_augment: bad argument");
    if (int rc = seg_check_shape("wc_seg_augment", B, Hs, Ws, crop, canvas_max, n_cand, ignore_index)) return rc;
    WC_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "wc_seg_augment: zero std");
    return seg_augment_launch<false>(src_u8, lab_u8, params, cand, dst, dst_label, sel, img_box, ws, B, Hs, Ws, crop, canvas_max,
                                     n_cand, ignore_index, mean3, std3, (hipStream_t)stream, nullptr, nullptr, 0L);
}

extern "C" int wc_seg_augment_ragged(const void* src_u8, const void* lab_u8, long src_bytes, const int64_t* offsets,
                                     const int* sizes, const void* params, const int* cand, float* dst, int64_t* dst_label, int* sel,
                                     int* img_box, int* ws, int B, int crop, int canvas_max, int n_cand, int ignore_index,
                                     const float* mean3, const float* std3, void* stream) {
    WC_CHECK_ARG(src_u8 && lab_u8 && src_bytes >= 3 && offsets && sizes && params && cand && dst && dst_label && sel && img_box && ws &&
                     mean3 && std3,
                 "wc_seg_augment_ragged: bad argument");
    if (int rc = seg_check_shape("wc_seg_augment_ragged", B, 1, 1, crop, canvas_max, n_cand, ignore_index)) return rc;
    WC_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "wc_seg_augment_ragged: zero std");
    return seg_augment_launch<true>(src_u8, lab_u8, params, cand, dst, dst_label, sel, img_box, ws, B, 0, 0, crop, canvas_max, n_cand,
                                    ignore_index, mean3, std3, (hipStream_t)stream, (const long long*)offsets, sizes, src_bytes);
}

extern "C" int wc_hsv8_convert(const void* src_u8, void* dst_u8, long n, int inverse, void* stream) {
    WC_CHECK_ARG(src_u8 && dst_u8 && n > 0 && n <= (1L << 31), "wc_hsv8_convert: bad argument");
    hipLaunchKernelGGL(seg_hsv8_kernel, dim3(wc_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const u8*)src_u8, (u8*)dst_u8, n,
                       inverse);
    WC_LAUNCH_CHECK("seg_hsv8_kernel");
    return WC_OK;
}
