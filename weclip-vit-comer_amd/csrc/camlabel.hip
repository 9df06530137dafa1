// The AFA pseudo-label chain of the reference's utils/camutils.py on the device:
//
//   aff_prep_kernel       : the operand X of the random walk as Xt (B, n, KP) f32, KP = 32 ceil(K / 32), padding columns zero.
//                           with_bkg: the soft-max over {bkg_score} + {cams[c] : cls[b, c] != 0} per token, absent rows zero
//                           (camutils.py:281-288, :309-312); otherwise the CAMs themselves (:268).
//   aff_walk_kernel       : out[b, k, j] = (sum_i X[b, k, i] A[b, i, j]) / (sum_i A[b, i, j] + eps) with A = (aff * [mask != 0])^2
//                           (camutils.py:254-271 and :298-315: mask, square, column sum, quotient and one matmul per image).
//                           Numerator and denominator contract over the same i, so `aff` is read ONCE: a workgroup owns 32
//                           columns j, its four waves take the rows i in interleaved blocks of 32 (16 past K = 32), a row's slice is
//                           128 contiguous bytes.  The products go through the f32-input MFMA (v_mfma_f32_32x32x2_f32: A
//                           operand = Xt, B operand = A, the two halves of a wave hold two consecutive rows i); the column
//                           sums are kept per lane.  Epilogue: the four waves' accumulators and the eight column-sum partials are
//                           added through LDS in a fixed order, then one IEEE division per element.
//   cam_label_kernel      : cam_to_label (camutils.py:8-28): valid_cam = cls * cam, first maximum over the classes, the
//                           thresholds, the box; four pixels per thread with 128-bit loads when H * W is a multiple of four.
//   box_ignore_kernel     : ignore_img_box (camutils.py:30-37) for int64 and f32 labels.
//   bkg_prep_kernel       : refine_cams_with_bkg_v2 up to the PAR call (camutils.py:152-177): bilinear down-sample of the
//                           present classes' CAMs, soft-max with the high and the low background score, one compact stack.
//   bkg_finish_kernel     : the rest (camutils.py:182-198): bilinear up-sample of both halves, arg-max over the image's
//                           channels, valid_key, box, combine.
//   box_gather_* / box_scatter_kernel : the crops of refine_cams_with_cls_label (camutils.py:210-221).
// No atomics anywhere: every sum has a fixed order, two runs on the same input give the same bits.
// Error model of the walk (per element, relative to the value itself since every term is non-negative): the MFMA chain's
// ~1.5e-7 (measured, K <= 1024), as much again for the column sum, a few ulp of the soft-max and the division: <= 2^-20.
#include "resample.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CL_MAX_B 65535            // the image index is a grid dimension
#define CL_MAX_N 4096
#define CL_MAX_K 128
#define CL_MAX_HW (1 << 24)       // pixels per image: every pixel index fits an int with room to spare
#define CL_CB 32                  // columns per walk workgroup

// Python's slice clamping of one bound on an axis of n samples
__device__ __forceinline__ int cl_slice(int v, int n) { return v < 0 ? max(v + n, 0) : min(v, n); }

__device__ __forceinline__ bool cl_in_box(const int* __restrict__ box, int y, int x, int H, int W) {
    return y >= cl_slice(box[0], H) && y < cl_slice(box[1], H) && x >= cl_slice(box[2], W) && x < cl_slice(box[3], W);
}

// ------------------------------------------------------------------------------------------------ random walk
__global__ __launch_bounds__(256) void aff_prep_kernel(const float* __restrict__ cams, const float* __restrict__ cls,
                                                       float* __restrict__ Xt, int C, int n, int KP, float bkg, int with_bkg) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* cb = cams + (long)b * C * n + i;
    float* x = Xt + ((long)b * n + i) * KP;
    if (!with_bkg) {
        for (int c = 0; c < C; ++c) x[c] = cb[(long)c * n];
        for (int c = C; c < KP; ++c) x[c] = 0.f;
        return;
    }
    const float* lb = cls + (long)b * C;
    float m = bkg;
    for (int c = 0; c < C; ++c)
        if (lb[c] != 0.f) m = fmaxf(m, cb[(long)c * n]);
    const float e0 = expf(bkg - m);
    float s = e0;
    for (int c = 0; c < C; ++c)
        if (lb[c] != 0.f) s += expf(cb[(long)c * n] - m);
    x[0] = e0 / s;
    for (int c = 0; c < C; ++c) x[1 + c] = lb[c] != 0.f ? expf(cb[(long)c * n] - m) / s : 0.f;
    for (int c = C + 1; c < KP; ++c) x[c] = 0.f;
}

template <int CT>
__global__ __launch_bounds__(256) void aff_walk_kernel(const float* __restrict__ aff, const float* __restrict__ mask,
                                                       const float* __restrict__ Xt, float* __restrict__ out, int n, int K,
                                                       float eps) {
    constexpr int KP = 32 * CT;
    constexpr int CL_RU = CT == 1 ? 16 : 8;            // row pairs a wave has in flight (registers: CT operands per pair)
    __shared__ float red[4][32 * CL_CB];
    __shared__ float sred[8][CL_CB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.y, j0 = blockIdx.x * CL_CB;
    const int jc = min(j0 + l31, n - 1);
    const float* A = aff + (long)b * n * n + jc;
    const float* M = mask ? mask + jc : nullptr;
    const float* X = Xt + (long)b * n * KP + l31;

    f32x16 acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    float s = 0.f;

    // the next block's loads are in flight while this block's products are formed
    float a[CL_RU], mk[CL_RU], x[CL_RU][CT];
    const auto gload = [&](int i0, float* a_, float* mk_, float (*x_)[CT]) {
#pragma unroll
        for (int u = 0; u < CL_RU; ++u) {
            const int ic = min(i0 + 2 * u + h, n - 1);
            a_[u] = A[(long)ic * n];
            mk_[u] = M ? M[(long)ic * n] : 1.f;
#pragma unroll
            for (int c = 0; c < CT; ++c) x_[u][c] = X[(long)ic * KP + 32 * c];
        }
    };
    constexpr int STEP = 4 * 2 * CL_RU;
    int i0 = wave * 2 * CL_RU;
    gload(i0, a, mk, x);                                    // (row indices are clamped: a wave without rows loads row n - 1, unused)
    for (; i0 < n; i0 += STEP) {
        float an[CL_RU], mkn[CL_RU], xn[CL_RU][CT];
        gload(i0 + STEP, an, mkn, xn);
#pragma unroll
        for (int u = 0; u < CL_RU; ++u) {
            float v = mk[u] == 0.f ? 0.f : a[u];
            v = i0 + 2 * u + h < n ? v * v : 0.f;           // rows past the end contribute nothing
            s += v;
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u][c], v, acc[c], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < CL_RU; ++u) {
            a[u] = an[u], mk[u] = mkn[u];
#pragma unroll
            for (int c = 0; c < CT; ++c) x[u][c] = xn[u][c];
        }
    }

    // epilogue: acc[c][r] = sum over this wave's rows for class 32c + (r & 3) + 8 (r >> 2) + 4h, column j0 + l31
    sred[wave * 2 + h][l31] = s;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        __syncthreads();                                    // the previous tile's sums are read
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][((r & 3) + 8 * (r >> 2) + 4 * h) * CL_CB + l31] = acc[c][r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, row = e >> 5, col = e & 31;
            const int k = 32 * c + row, j = j0 + col;
            const float num = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
            const float den = ((sred[0][col] + sred[1][col]) + (sred[2][col] + sred[3][col])) +
                              ((sred[4][col] + sred[5][col]) + (sred[6][col] + sred[7][col]));
            if (k < K && j < n) out[((long)b * K + k) * n + j] = num / (den + eps);
        }
    }
}

// ------------------------------------------------------------------------------------------------ labels
template <int V>
__global__ __launch_bounds__(256) void cam_label_kernel(const float* __restrict__ cam, const float* __restrict__ cls,
                                                        const int* __restrict__ box, long* __restrict__ label,
                                                        float* __restrict__ valid, int C, int H, int W, float bkg, float hi,
                                                        float lo, int ignore_mid, long ignore) {
    const int HW = H * W, b = blockIdx.y;
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (p0 >= HW) return;
    const float* cb = cam + (long)b * C * HW + p0;
    float* vb = valid ? valid + (long)b * C * HW + p0 : nullptr;
    const float* lb = cls + (long)b * C;
    float best[V];
    int arg[V];
    for (int c = 0; c < C; ++c) {
        float v[V];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(cb + (long)c * HW);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
            v[0] = cb[(long)c * HW];
        }
        const float l = lb[c];
#pragma unroll
        for (int u = 0; u < V; ++u) {
            v[u] = l * v[u];
            if (c == 0 || v[u] > best[u]) best[u] = v[u], arg[u] = c;      // the first maximum wins; a NaN never wins (torch.max would return it)
        }
        if (vb) {
            if constexpr (V == 4) *reinterpret_cast<float4*>(vb + (long)c * HW) = make_float4(v[0], v[1], v[2], v[3]);
            else vb[(long)c * HW] = v[0];
        }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
        const int p = p0 + u;
        long l = arg[u] + 1;
        if (best[u] <= bkg) l = 0;
        if (box) {
            if (ignore_mid) {
                if (best[u] <= hi) l = ignore;
                if (best[u] <= lo) l = 0;
            }
            const int y = p / W;
            if (!cl_in_box(box + 4 * b, y, p - y * W, H, W)) l = ignore;
        }
        label[(long)b * HW + p] = l;
    }
}

template <class T>
__global__ __launch_bounds__(256) void box_ignore_kernel(const T* __restrict__ in, const int* __restrict__ box, T* __restrict__ out,
                                                         int H, int W, T ignore) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W;
    const long e = (long)b * H * W + p;
    out[e] = cl_in_box(box + 4 * b, y, p - y * W, H, W) ? in[e] : ignore;
}

// ------------------------------------------------------------------------------------------------ refine with background
// meta (B, 1 + Kmax) int32: the image's channel count nch in [1, Kmax], then its label values: 0 for the background, 1 + class
__device__ __forceinline__ int cl_nch(const int* __restrict__ m, int Kmax) { return min(max(m[0], 1), Kmax); }

__global__ __launch_bounds__(256) void bkg_prep_kernel(const float* __restrict__ cams, const int* __restrict__ meta,
                                                       float* __restrict__ stack, int C, int H, int W, int h2, int w2, int Kmax,
                                                       float hi, float lo, float sy, float sx) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, hw2 = h2 * w2;
    if (p >= hw2) return;
    const int y = p / w2, x = p - y * w2;
    int y0, y1, x0, x1;
    float ly, lx;
    wc_bil_src(y, H, sy, y0, y1, ly);
    wc_bil_src(x, W, sx, x0, x1, lx);
    const int* m = meta + (long)b * (1 + Kmax);
    const int nch = cl_nch(m, Kmax);
    const float* cb = cams + (long)b * C * H * W;
    const auto at = [&](int k) {
        const int c = min(max(m[1 + k] - 1, 0), C - 1);
        return wc_bilerp(cb + (long)c * H * W, W, y0, y1, x0, x1, ly, lx);
    };
    float mx = -INFINITY;
    for (int k = 1; k < nch; ++k) mx = fmaxf(mx, at(k));
    const float mh = fmaxf(mx, hi), ml = fmaxf(mx, lo);
    const float eh = expf(hi - mh), el = expf(lo - ml);
    float sh = eh, sl = el;
    for (int k = 1; k < nch; ++k) {
        const float v = at(k);
        sh += expf(v - mh);
        sl += expf(v - ml);
    }
    float* oh = stack + (long)b * 2 * Kmax * hw2 + p;
    float* ol = oh + (long)Kmax * hw2;
    oh[0] = eh / sh;
    ol[0] = el / sl;
    for (int k = 1; k < Kmax; ++k) {
        float vh = 0.f, vl = 0.f;
        if (k < nch) {
            const float v = at(k);
            vh = expf(v - mh) / sh;
            vl = expf(v - ml) / sl;
        }
        oh[(long)k * hw2] = vh;
        ol[(long)k * hw2] = vl;
    }
}

__global__ __launch_bounds__(256) void bkg_finish_kernel(const float* __restrict__ stack, const int* __restrict__ meta,
                                                         const int* __restrict__ box, float* __restrict__ out, int H, int W, int h2,
                                                         int w2, int Kmax, float ignore, float sy, float sx) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    float r = ignore;
    if (cl_in_box(box + 4 * b, y, x, H, W)) {
        int y0, y1, x0, x1;
        float ly, lx;
        wc_bil_src(y, h2, sy, y0, y1, ly);
        wc_bil_src(x, w2, sx, x0, x1, lx);
        const int* m = meta + (long)b * (1 + Kmax);
        const int nch = cl_nch(m, Kmax);
        const float* sh = stack + (long)b * 2 * Kmax * h2 * w2;
        const int lh = m[1 + wc_resize_argmax_at(sh, nch, h2, w2, y0, y1, x0, x1, ly, lx)];
        const int ll = m[1 + wc_resize_argmax_at(sh + (long)Kmax * h2 * w2, nch, h2, w2, y0, y1, x0, x1, ly, lx)];
        r = lh == 0 ? ignore : (float)lh;
        if (lh + ll == 0) r = 0.f;
    }
    out[(long)b * H * W + p] = r;
}

// ------------------------------------------------------------------------------------------------ box crops
// meta (G, 3 + Kg) int32 per member: image index, y0, x0 of its box, then the channel of each compact slot (-1: padding).
// A member whose image index, box or channel does not fit the tensors is skipped: nothing outside them is touched.
__device__ __forceinline__ bool cl_member_ok(const int* __restrict__ m, int B, int H, int W, int hb, int wb) {
    return m[0] >= 0 && m[0] < B && m[1] >= 0 && m[2] >= 0 && m[1] <= H - hb && m[2] <= W - wb;
}

__global__ __launch_bounds__(256) void box_gather_cams_kernel(const float* __restrict__ cams, const int* __restrict__ meta,
                                                              float* __restrict__ dst, int B, int C, int H, int W, int hb, int wb,
                                                              int Kg) {
    const int g = blockIdx.z, k = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hb * wb) return;
    const int* m = meta + (long)g * (3 + Kg);
    const int key = m[3 + k], y = p / wb, x = p - y * wb;
    float v = 0.f;
    if (key >= 0 && key < C && cl_member_ok(m, B, H, W, hb, wb)) v = cams[(((long)m[0] * C + key) * H + m[1] + y) * W + m[2] + x];
    dst[((long)g * Kg + k) * hb * wb + p] = v;
}

__global__ __launch_bounds__(256) void box_gather_img_kernel(const float* __restrict__ img, const int* __restrict__ meta,
                                                             float* __restrict__ dst, int B, int H, int W, int hb, int wb, int hs,
                                                             int ws, int Kg, float sy, float sx) {
    const int g = blockIdx.z, ch = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hs * ws) return;
    const int* m = meta + (long)g * (3 + Kg);
    const int y = p / ws, x = p - y * ws;
    float v = 0.f;
    if (cl_member_ok(m, B, H, W, hb, wb)) {
        int y0, y1, x0, x1;
        float ly, lx;
        wc_bil_src(y, hb, sy, y0, y1, ly);
        wc_bil_src(x, wb, sx, x0, x1, lx);
        v = wc_bilerp(img + (((long)m[0] * 3 + ch) * H + m[1]) * W + m[2], W, y0, y1, x0, x1, ly, lx);
    }
    dst[((long)g * 3 + ch) * hs * ws + p] = v;
}

__global__ __launch_bounds__(256) void box_scatter_kernel(const float* __restrict__ src, const int* __restrict__ meta,
                                                          float* __restrict__ out, int B, int C, int H, int W, int hb, int wb,
                                                          int Kg) {
    const int g = blockIdx.z, k = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hb * wb) return;
    const int* m = meta + (long)g * (3 + Kg);
    const int key = m[3 + k], y = p / wb, x = p - y * wb;
    if (key >= 0 && key < C && cl_member_ok(m, B, H, W, hb, wb))
        out[(((long)m[0] * C + key) * H + m[1] + y) * W + m[2] + x] = src[((long)g * Kg + k) * hb * wb + p];
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

int walk_plan(int B, int n, int C, int with_bkg, const char* who) {
    WC_CHECK_ARG(B >= 1 && B <= CL_MAX_B, "%s: bad argument: B = %d outside [1, %d]", who, B, CL_MAX_B);
    WC_CHECK_ARG(n >= 1 && n <= CL_MAX_N, "%s: bad argument: n = %d outside [1, %d]", who, n, CL_MAX_N);
    WC_CHECK_ARG(with_bkg == 0 || with_bkg == 1, "%s: bad argument: with_bkg = %d is not 0 or 1", who, with_bkg);
    WC_CHECK_ARG(C >= 0 && C + with_bkg >= 1 && C + with_bkg <= CL_MAX_K, "%s: bad argument: C + with_bkg = %d outside [1, %d]", who,
                 C + with_bkg, CL_MAX_K);
    return WC_OK;
}

int image_plan(int B, int C, int H, int W, const char* who) {
    WC_CHECK_ARG(B >= 1 && B <= CL_MAX_B, "%s: bad argument: B = %d outside [1, %d]", who, B, CL_MAX_B);
    WC_CHECK_ARG(C >= 1 && C <= CL_MAX_B, "%s: bad argument: C = %d outside [1, %d]", who, C, CL_MAX_B);
    WC_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= CL_MAX_HW, "%s: bad argument: H x W = %d x %d outside [1, 2^24] pixels", who, H, W);
    return WC_OK;
}

}  // namespace

extern "C" int wc_aff_propagate_workspace_floats(int B, int n, int C, int with_bkg, long* n_floats) {
    WC_CHECK_ARG(n_floats, "wc_aff_propagate_workspace_floats: bad argument: null pointer");
    if (int rc = walk_plan(B, n, C, with_bkg, "wc_aff_propagate_workspace_floats")) return rc;
    *n_floats = (long)B * n * (32L * ((C + with_bkg + 31) / 32));
    return WC_OK;
}

extern "C" int wc_aff_propagate(const float* aff, const float* mask, const float* cams, const float* cls, float* out, void* ws, int B,
                                int n, int C, float bkg_score, int with_bkg, void* stream) {
    WC_CHECK_ARG(aff && cams && out && ws, "wc_aff_propagate: bad argument: null pointer");
    if (int rc = walk_plan(B, n, C, with_bkg, "wc_aff_propagate")) return rc;
    WC_CHECK_ARG(!with_bkg || cls, "wc_aff_propagate: bad argument: null pointer (with_bkg needs the class labels)");
    WC_CHECK_ARG(!with_bkg || (bkg_score - bkg_score == 0.f), "wc_aff_propagate: bad argument: bkg_score must be finite");
    const int K = C + with_bkg, CT = (K + 31) / 32, KP = 32 * CT;
    float* Xt = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aff_prep_kernel, dim3(wc_cdiv(n, 256), B), dim3(256), 0, st, cams, cls, Xt, C, n, KP, bkg_score, with_bkg);
    WC_LAUNCH_CHECK("aff_prep_kernel");
    const dim3 grid(wc_cdiv(n, CL_CB), B), block(256);
    const float eps = with_bkg ? 1e-1f : 1e-4f;
    const int idx = wc_prof_begin(st);
    switch (CT) {
        case 1: hipLaunchKernelGGL(aff_walk_kernel<1>, grid, block, 0, st, aff, mask, Xt, out, n, K, eps); break;
        case 2: hipLaunchKernelGGL(aff_walk_kernel<2>, grid, block, 0, st, aff, mask, Xt, out, n, K, eps); break;
        case 3: hipLaunchKernelGGL(aff_walk_kernel<3>, grid, block, 0, st, aff, mask, Xt, out, n, K, eps); break;
        default: hipLaunchKernelGGL(aff_walk_kernel<4>, grid, block, 0, st, aff, mask, Xt, out, n, K, eps); break;
    }
    WC_LAUNCH_CHECK("aff_walk_kernel");
    wc_prof_end2(idx, "aff_walk_kernel", 2.0 * B * (double)n * n * KP, 4.0 * B * (double)n * n, st);
    return WC_OK;
}

extern "C" int wc_cam_to_label(const float* cam, const float* cls, const int* box, long* label, float* valid_cam, int B, int C, int H,
                               int W, float bkg_score, float high_thre, float low_thre, int ignore_mid, long ignore_index,
                               void* stream) {
    WC_CHECK_ARG(cam && cls && label, "wc_cam_to_label: bad argument: null pointer");
    if (int rc = image_plan(B, C, H, W, "wc_cam_to_label")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    const bool aligned = ((uintptr_t)cam | (uintptr_t)valid_cam) % 16 == 0;     // (a view may start anywhere in its storage)
    if (HW % 4 == 0 && aligned)
        hipLaunchKernelGGL(cam_label_kernel<4>, dim3(wc_cdiv(HW / 4, 256), B), dim3(256), 0, st, cam, cls, box, label, valid_cam, C, H,
                           W, bkg_score, high_thre, low_thre, ignore_mid, ignore_index);
    else
        hipLaunchKernelGGL(cam_label_kernel<1>, dim3(wc_cdiv(HW, 256), B), dim3(256), 0, st, cam, cls, box, label, valid_cam, C, H, W,
                           bkg_score, high_thre, low_thre, ignore_mid, ignore_index);
    WC_LAUNCH_CHECK("cam_label_kernel");
    return WC_OK;
}

extern "C" int wc_box_ignore(const void* label, const int* box, void* out, int B, int H, int W, int is_f32, long ignore_index,
                             void* stream) {
    WC_CHECK_ARG(label && box && out, "wc_box_ignore: bad argument: null pointer");
    if (int rc = image_plan(B, 1, H, W, "wc_box_ignore")) return rc;
    const dim3 grid(wc_cdiv((long)H * W, 256), B), block(256);
    if (is_f32)
        hipLaunchKernelGGL(box_ignore_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)label, box, (float*)out, H, W,
                           (float)ignore_index);
    else
        hipLaunchKernelGGL(box_ignore_kernel<long>, grid, block, 0, (hipStream_t)stream, (const long*)label, box, (long*)out, H, W,
                           ignore_index);
    WC_LAUNCH_CHECK("box_ignore_kernel");
    return WC_OK;
}

extern "C" int wc_bkg_refine_prep(const float* cams, const int* meta, float* stack, int B, int C, int H, int W, int h2, int w2,
                                  int Kmax, float high_thre, float low_thre, void* stream) {
    WC_CHECK_ARG(cams && meta && stack, "wc_bkg_refine_prep: bad argument: null pointer");
    if (int rc = image_plan(B, C, H, W, "wc_bkg_refine_prep")) return rc;
    WC_CHECK_ARG(h2 >= 1 && h2 <= H && w2 >= 1 && w2 <= W, "wc_bkg_refine_prep: bad argument: mask size %d x %d outside [1, %d] x [1, %d]",
                 h2, w2, H, W);
    WC_CHECK_ARG(Kmax >= 1 && Kmax <= C + 1, "wc_bkg_refine_prep: bad argument: Kmax = %d outside [1, C + 1]", Kmax);
    hipLaunchKernelGGL(bkg_prep_kernel, dim3(wc_cdiv((long)h2 * w2, 256), B), dim3(256), 0, (hipStream_t)stream, cams, meta, stack, C,
                       H, W, h2, w2, Kmax, high_thre, low_thre, (float)H / h2, (float)W / w2);
    WC_LAUNCH_CHECK("bkg_prep_kernel");
    return WC_OK;
}

extern "C" int wc_bkg_refine_finish(const float* stack, const int* meta, const int* box, float* out, int B, int H, int W, int h2,
                                    int w2, int Kmax, float ignore_index, void* stream) {
    WC_CHECK_ARG(stack && meta && box && out, "wc_bkg_refine_finish: bad argument: null pointer");
    if (int rc = image_plan(B, 1, H, W, "wc_bkg_refine_finish")) return rc;
    WC_CHECK_ARG(h2 >= 1 && h2 <= H && w2 >= 1 && w2 <= W,
                 "wc_bkg_refine_finish: bad argument: mask size %d x %d outside [1, %d] x [1, %d]", h2, w2, H, W);
    WC_CHECK_ARG(Kmax >= 1 && Kmax <= CL_MAX_B, "wc_bkg_refine_finish: bad argument: Kmax = %d outside [1, %d]", Kmax, CL_MAX_B);
    hipLaunchKernelGGL(bkg_finish_kernel, dim3(wc_cdiv((long)H * W, 256), B), dim3(256), 0, (hipStream_t)stream, stack, meta, box, out,
                       H, W, h2, w2, Kmax, ignore_index, (float)h2 / H, (float)w2 / W);
    WC_LAUNCH_CHECK("bkg_finish_kernel");
    return WC_OK;
}

namespace {
int gather_plan(int G, int B, int C, int H, int W, int hb, int wb, int Kg, const char* who) {
    if (int rc = image_plan(B, C, H, W, who)) return rc;
    WC_CHECK_ARG(G >= 1 && G <= CL_MAX_B, "%s: bad argument: G = %d outside [1, %d]", who, G, CL_MAX_B);
    WC_CHECK_ARG(hb >= 2 && hb <= H && wb >= 2 && wb <= W, "%s: bad argument: box size %d x %d outside [2, %d] x [2, %d]", who, hb, wb,
                 H, W);
    WC_CHECK_ARG(Kg >= 1 && Kg <= C, "%s: bad argument: Kg = %d outside [1, C]", who, Kg);
    return WC_OK;
}
}  // namespace

extern "C" int wc_box_gather(const float* cams, const float* images, const int* meta, float* cams_out, float* img_out, int G, int B,
                             int C, int H, int W, int hb, int wb, int Kg, void* stream) {
    WC_CHECK_ARG(cams && images && meta && cams_out && img_out, "wc_box_gather: bad argument: null pointer");
    if (int rc = gather_plan(G, B, C, H, W, hb, wb, Kg, "wc_box_gather")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int hs = hb / 2, ws = wb / 2;
    hipLaunchKernelGGL(box_gather_cams_kernel, dim3(wc_cdiv((long)hb * wb, 256), Kg, G), dim3(256), 0, st, cams, meta, cams_out, B, C, H,
                       W, hb, wb, Kg);
    WC_LAUNCH_CHECK("box_gather_cams_kernel");
    hipLaunchKernelGGL(box_gather_img_kernel, dim3(wc_cdiv((long)hs * ws, 256), 3, G), dim3(256), 0, st, images, meta, img_out, B, H, W,
                       hb, wb, hs, ws, Kg, (float)hb / hs, (float)wb / ws);
    WC_LAUNCH_CHECK("box_gather_img_kernel");
    return WC_OK;
}

extern "C" int wc_box_scatter(const float* src, const int* meta, float* out, int G, int B, int C, int H, int W, int hb, int wb, int Kg,
                              void* stream) {
    WC_CHECK_ARG(src && meta && out, "wc_box_scatter: bad argument: null pointer");
    if (int rc = gather_plan(G, B, C, H, W, hb, wb, Kg, "wc_box_scatter")) return rc;
    hipLaunchKernelGGL(box_scatter_kernel, dim3(wc_cdiv((long)hb * wb, 256), Kg, G), dim3(256), 0, (hipStream_t)stream, src, meta, out,
                       B, C, H, W, hb, wb, Kg);
    WC_LAUNCH_CHECK("box_scatter_kernel");
    return WC_OK;
}
