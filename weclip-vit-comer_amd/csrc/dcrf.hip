// Dense CRF: exact mean-field inference of the fully connected CRF with Potts compatibility (the model of DESIGN.md
// "Dense CRF"), the device form of the reference's utils/dcrf.py (`DenseCRF`, `crf_inference`, `crf_inference_label`,
// a wrapper over the third-party pydensecrf, whose permutohedral lattice only approximates this model).
//
//   unary preps      : U (C,N) = -ln clamp(p, 1e-5, 1) from probabilities, from a label map (gt_prob), or from logits
//                      (bilinear align_corners=False to the label grid + softmax over C, never writing the resized logits).
//   dcrf_feat_kernel : per-pixel raw features (x, y, R, G, B) -> (N, 8) f32 rows (one 32-B row per key in LDS).
//   Gaussian kernel  : k_pos factorises over x and y: a row pass and a column pass of 2R + 1 taps,
//                      R = ceil(pos_xy_std * sqrt(60 ln 2)) (the taps dropped weigh < 2^-30 of a 1-D sum, < 2^-29 of S_pos);
//                      the normaliser S_pos = Sx(x) Sy(y) directly from the same truncated 1-D sums.
//   dcrf_bil_kernel  : the bilateral message, the hot path: the exact all-pairs sum bil_exact_sum of csrc/bilateral_exact.h
//                      (which csrc/energy.hip's energy_filter_kernel runs too) over the operand V(j, l) = n(j) Q(l, j), under
//                      this kernel's three epilogues.  Mode 2 fuses n(i) w, the Gaussian message, -U, the softmax over labels
//                      and the writes of Q and of both next-pass operands.
//                      No atomics: every output is one wave's fixed-order sum, bit-identical from run to run.
// Error model (per message element, relative to the sum of its non-negative terms sum_j n_i k_ij n_j Q_j(l)): that of
//   bil_exact_sum, stated in csrc/bilateral_exact.h: eps = 2^-10 (include/weclip_hip.h).
#include "common.h"
#include "bilateral_exact.h"
#include "resample.h"

#define DCRF_MAX_C 128
#define DCRF_MAX_N (640 * 640)
#define LOG2E 1.4426950408889634f

// ------------------------------------------------------------------------------------------------ unary preps
__device__ __forceinline__ float dcrf_unary(float p) { return -logf(fminf(fmaxf(p, 1e-5f), 1.0f)); }

__global__ __launch_bounds__(256) void dcrf_unary_prob_kernel(const float* __restrict__ P, float* __restrict__ U, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) U[i] = dcrf_unary(P[i]);
}

__global__ __launch_bounds__(256) void dcrf_unary_label_kernel(const int64_t* __restrict__ lab, float* __restrict__ U, int C,
                                                               int N, float u_on, float u_off) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t l = lab[i];
    for (int c = 0; c < C; ++c) U[(long)c * N + i] = (l == c) ? u_on : u_off;
}

// one thread per label-grid pixel: bilinear logits of every class (recomputed in each of the three sweeps, never stored),
// max, sum of exponentials, U = -ln clamp(softmax)
__global__ __launch_bounds__(256) void dcrf_unary_logits_kernel(const float* __restrict__ lg, float* __restrict__ U, int C, int h,
                                                                int w, int H, int W, float sy, float sx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    int y0, y1, x0, x1;
    float ly, lx;
    wc_bil_src(y, h, sy, y0, y1, ly);
    wc_bil_src(x, w, sx, x0, x1, lx);
    const long plane = (long)h * w;
    const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
    const auto logit = [&](int c) {
        return wc_lerp4(lg[c * plane + o00], lg[c * plane + o01], lg[c * plane + o10], lg[c * plane + o11], ly, lx);
    };
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, logit(c));
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += __builtin_amdgcn_exp2f((logit(c) - mx) * LOG2E);
    const float inv = 1.f / sum;
    const long N = (long)H * W;
    for (int c = 0; c < C; ++c) U[c * N + i] = dcrf_unary(__builtin_amdgcn_exp2f((logit(c) - mx) * LOG2E) * inv);
}

// ------------------------------------------------------------------------------------------------ features, init
__global__ __launch_bounds__(256) void dcrf_feat_kernel(const void* __restrict__ img, int is_u8, float* __restrict__ feat, int H,
                                                        int W) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    float r, g, b;
    if (is_u8) {
        const uint8_t* p = (const uint8_t*)img + 3L * i;
        r = p[0], g = p[1], b = p[2];
    } else {
        const float* p = (const float*)img + 3L * i;
        r = p[0], g = p[1], b = p[2];
    }
    const int y = i / W;
    float4* f = reinterpret_cast<float4*>(feat + 8L * i);
    f[0] = make_float4((float)(i - y * W), (float)y, r, g);
    f[1] = make_float4(b, 0.f, 0.f, 0.f);
}

// Q0 = softmax(-U) and the first operands: Vb (N, CP) = n_bil Q, Vp (C, N) = n_pos Q
__global__ __launch_bounds__(256) void dcrf_init_kernel(const float* __restrict__ U, const float* __restrict__ nrm,
                                                        float* __restrict__ Q, float* __restrict__ Vb, float* __restrict__ Vp,
                                                        int C, int CP, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float mn = INFINITY;
    for (int c = 0; c < C; ++c) mn = fminf(mn, U[(long)c * N + i]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += __builtin_amdgcn_exp2f((mn - U[(long)c * N + i]) * LOG2E);
    const float inv = 1.f / sum, np = nrm[i], nb = nrm[N + i];
    for (int c = 0; c < C; ++c) {
        const float q = __builtin_amdgcn_exp2f((mn - U[(long)c * N + i]) * LOG2E) * inv;
        Q[(long)c * N + i] = q;
        Vp[(long)c * N + i] = np * q;
        Vb[(long)i * CP + c] = nb * q;
    }
}

// the single-message entry's operands from a given Q (C, N): Vp = n_pos Q (C, N), Vb (N, CP) = n_bil Q
__global__ __launch_bounds__(256) void dcrf_operands_kernel(const float* __restrict__ Q, const float* __restrict__ nrm,
                                                            float* __restrict__ Vb, float* __restrict__ Vp, int C, int CP, int N) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * N) return;
    const int l = (int)(e / N), i = (int)(e - (long)l * N);
    const float q = Q[e];
    Vp[e] = nrm[i] * q;
    Vb[(long)i * CP + l] = nrm[N + i] * q;
}

__global__ __launch_bounds__(256) void dcrf_ones_col_kernel(float* __restrict__ V, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) V[32L * i] = 1.f;
}

// msg (C, N) = nrm[i] G
__global__ __launch_bounds__(256) void dcrf_scale_kernel(const float* __restrict__ G, const float* __restrict__ nrm,
                                                         float* __restrict__ msg, int C, int N) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < (long)C * N) msg[e] = nrm[e % N] * G[e];
}

// ------------------------------------------------------------------------------------------------ Gaussian kernel
// 1-D pass along a line of `len` elements at stride `st` (1: rows, W: columns): out[p] = sum_{|d| <= R, inside} 2^(-a d^2) in[p + d st].
// Four taps per step, their loads issued together (clamped index, zero weight outside).
__global__ __launch_bounds__(256) void dcrf_gauss_pass_kernel(const float* __restrict__ in, float* __restrict__ out, long total,
                                                              int len, int st, int R, float a) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int pos = st == 1 ? (int)(p % len) : (int)((p / st) % len);
    const int lo = -min(R, pos), hi = min(R, len - 1 - pos);
    const float* base = in + p;
    float acc = 0.f;
    for (int d = lo; d <= hi; d += 4) {
        float v[4], wt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int dd = min(d + u, hi);
            v[u] = base[(long)dd * st];
            wt[u] = d + u <= hi ? __builtin_amdgcn_exp2f(-a * (float)(dd * dd)) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fmaf(wt[u], v[u], acc);
    }
    out[p] = acc;
}

__device__ __forceinline__ float dcrf_gauss_1d_sum(int pos, int len, int R, float a) {
    const int lo = -min(R, pos), hi = min(R, len - 1 - pos);
    float s = 0.f;
    for (int d = lo; d <= hi; ++d) s += __builtin_amdgcn_exp2f(-a * (float)(d * d));
    return s;
}

// S_pos(i) = Sx(x_i) Sy(y_i) (the separable passes applied to a plane of ones) -> S[i], nrm[i] = S^-1/2
__global__ __launch_bounds__(256) void dcrf_gauss_norm_kernel(float* __restrict__ S, float* __restrict__ nrm, int H, int W, int R,
                                                              float a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W;
    const float s = dcrf_gauss_1d_sum(i - y * W, W, R, a) * dcrf_gauss_1d_sum(y, H, R, a);
    if (S) S[i] = s;
    nrm[i] = rsqrtf(s);
}

// ------------------------------------------------------------------------------------------------ bilateral kernel
struct BilArgs {
    const float* feat;     // (N, 8): x, y, R, G, B
    const float* V;        // (N, CP) operand; columns >= C are zero
    int N, C, CP;
    float a_xy, a_rgb;     // log2(e) / (2 sigma^2)
    int mode;              // 0: S = acc[label 0] -> S[i], nrm[i] = S^-1/2;  1: msg (C, N) = nrm[i] acc;  2: mean-field update
    float* S;
    float* nrm;            // mode 0: written; modes 1, 2: n_bil (read)
    float* msg;
    // mode 2: Q = softmax(-U + w_bil n_bil acc + w_pos n_pos G); Vb_out (N, CP) = n_bil Q, Vp_out (C, N) = n_pos Q
    const float* U;
    const float* G;
    const float* npos;
    float w_bil, w_pos;
    float* Q;
    float* Vb_out;
    float* Vp_out;
};

template <int CT>
__global__ __launch_bounds__(BIL_NT, 2) void dcrf_bil_kernel(BilArgs A) {
    constexpr int CP = 32 * CT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int N = A.N;
    const int qi = blockIdx.x * BIL_NT / 2 + wave * 32 + l31;
    const int qc = qi < N ? qi : N - 1;
    f32x16 tot[CT];
    bil_exact_sum<CT>(A.feat, A.V, N, qc, A.a_xy, A.a_rgb, tot);

    // epilogue: tot[c][r] = M^T(label bil_label(c, r, h), query qi)
    if (A.mode == 0) {
        if (h == 0 && qi < N) {
            A.S[qi] = tot[0][0];
            A.nrm[qi] = rsqrtf(tot[0][0]);
        }
        return;
    }
    const int C = A.C;
    const float nb = A.nrm[qc];
    if (A.mode == 1) {
        if (qi < N) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int l = bil_label(c, r, h);
                    if (l < C) A.msg[(long)l * N + qi] = nb * tot[c][r];
                }
        }
        return;
    }
    const float np = A.npos[qc];
    const float sb = A.w_bil * nb, sp = A.w_pos * np;
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int l = bil_label(c, r, h);
            const long o = (long)min(l, C - 1) * N + qc;
            const float z = fmaf(sp, A.G[o], fmaf(sb, tot[c][r], -A.U[o]));
            tot[c][r] = l < C ? z : -INFINITY;
            mx = fmaxf(mx, tot[c][r]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            tot[c][r] = __builtin_amdgcn_exp2f((tot[c][r] - mx) * LOG2E);
            sum += tot[c][r];
        }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    if (qi < N) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int l = bil_label(c, r, h);
                if (l < C) {
                    const float q = tot[c][r] * inv;
                    A.Q[(long)l * N + qi] = q;
                    A.Vp_out[(long)l * N + qi] = np * q;
                    A.Vb_out[(long)qi * CP + l] = nb * q;
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

struct Plan {
    int N, C, CT, CP, R;
    float a_pos, a_xy, a_rgb;
};

bool finite_pos(float v) { return v > 0.f && v < INFINITY; }

int plan(Plan& p, int C, int H, int W, float pos_xy_std, float bi_xy_std, float bi_rgb_std, const char* who) {
    WC_CHECK_ARG(C >= 1 && C <= DCRF_MAX_C, "%s: bad argument: C = %d outside [1, %d]", who, C, DCRF_MAX_C);
    WC_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= DCRF_MAX_N, "%s: bad argument: H x W = %d x %d outside [1, 640*640] pixels",
                 who, H, W);
    WC_CHECK_ARG(finite_pos(pos_xy_std) && finite_pos(bi_xy_std) && finite_pos(bi_rgb_std),
                 "%s: bad argument: standard deviations must be finite and > 0", who);
    p.N = H * W;
    p.C = C;
    p.CT = (C + 31) / 32;
    p.CP = 32 * p.CT;
    const double r = ceil((double)pos_xy_std * sqrt(60.0 * log(2.0)));   // 2^(-R^2 / (2 sigma^2)) <= 2^-30
    p.R = (int)fmin(r, (double)(H > W ? H : W));
    p.a_pos = (float)(1.4426950408889634 / (2.0 * (double)pos_xy_std * pos_xy_std));
    p.a_xy = (float)(1.4426950408889634 / (2.0 * (double)bi_xy_std * bi_xy_std));
    p.a_rgb = (float)(1.4426950408889634 / (2.0 * (double)bi_rgb_std * bi_rgb_std));
    return WC_OK;
}

int launch_bil(const Plan& p, BilArgs a, hipStream_t st) {
    const dim3 grid(wc_cdiv(p.N, BIL_NT / 2)), block(BIL_NT);
    const int idx = wc_prof_begin(st);
    switch (a.mode == 0 ? 1 : p.CT) {
        case 1: hipLaunchKernelGGL(dcrf_bil_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(dcrf_bil_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(dcrf_bil_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(dcrf_bil_kernel<4>, grid, block, 0, st, a); break;
    }
    WC_LAUNCH_CHECK("dcrf_bil_kernel");
    const int cols = a.mode == 0 ? 32 : p.CP;
    wc_prof_end(idx, "dcrf_bil_kernel", 2.0 * p.N * (double)p.N * cols, st);
    return WC_OK;
}

// Gaussian message of the (C, N) planes `in` -> out (C, N), through tmp (C, N)
int gauss_message(const Plan& p, int H, int W, const float* in, float* tmp, float* out, hipStream_t st) {
    const long total = (long)p.C * p.N;
    hipLaunchKernelGGL(dcrf_gauss_pass_kernel, dim3(wc_cdiv(total, 256)), dim3(256), 0, st, in, tmp, total, W, 1, p.R, p.a_pos);
    WC_LAUNCH_CHECK("dcrf_gauss_pass_kernel");
    hipLaunchKernelGGL(dcrf_gauss_pass_kernel, dim3(wc_cdiv(total, 256)), dim3(256), 0, st, tmp, out, total, H, W, p.R, p.a_pos);
    WC_LAUNCH_CHECK("dcrf_gauss_pass_kernel");
    return WC_OK;
}

// workspace carve-up shared by the two entries (floats): feat 8N | nrm 2N (n_pos, n_bil) | S 2N | Vb 2 x N CP | Vp, tmp, G 3 x C N
struct Ws {
    float *feat, *nrm, *S, *Vb[2], *Vp, *tmp, *G;
};

Ws carve(const Plan& p, void* ws) {
    Ws w;
    float* f = (float*)ws;
    const long N = p.N, CN = (long)p.C * p.N;
    w.feat = f;
    w.nrm = w.feat + 8 * N;
    w.S = w.nrm + 2 * N;
    w.Vb[0] = w.S + 2 * N;
    w.Vb[1] = w.Vb[0] + N * p.CP;
    w.Vp = w.Vb[1] + N * p.CP;
    w.tmp = w.Vp + CN;
    w.G = w.tmp + CN;
    return w;
}

// features, S_pos / n_pos, S_bil / n_bil (the bilateral pass on V = ones, written into Vb[1])
int normalisers(const Plan& p, const void* img, int img_is_u8, int H, int W, const Ws& w, float* S_out, hipStream_t st) {
    hipLaunchKernelGGL(dcrf_feat_kernel, dim3(wc_cdiv(p.N, 256)), dim3(256), 0, st, img, img_is_u8, w.feat, H, W);
    WC_LAUNCH_CHECK("dcrf_feat_kernel");
    hipLaunchKernelGGL(dcrf_gauss_norm_kernel, dim3(wc_cdiv(p.N, 256)), dim3(256), 0, st, S_out, w.nrm, H, W, p.R, p.a_pos);
    WC_LAUNCH_CHECK("dcrf_gauss_norm_kernel");
    // V = ones in column 0 only (the S pass reads a 32-column operand)
    if (hipMemsetAsync(w.Vb[1], 0, sizeof(float) * 32L * p.N, st) != hipSuccess) {
        wc_set_error("dcrf: hipMemsetAsync failed");
        return WC_ERR_HIP;
    }
    hipLaunchKernelGGL(dcrf_ones_col_kernel, dim3(wc_cdiv(p.N, 256)), dim3(256), 0, st, w.Vb[1], p.N);
    WC_LAUNCH_CHECK("dcrf_ones_col_kernel");
    BilArgs a = {};
    a.feat = w.feat, a.V = w.Vb[1], a.N = p.N, a.C = 1, a.CP = 32, a.a_xy = p.a_xy, a.a_rgb = p.a_rgb, a.mode = 0;
    a.S = S_out ? S_out + p.N : w.S + p.N;
    a.nrm = w.nrm + p.N;
    return launch_bil(p, a, st);
}

}  // namespace

extern "C" int wc_dcrf_unary_prob(const float* probs, float* unary, int C, int H, int W, void* stream) {
    WC_CHECK_ARG(probs && unary, "wc_dcrf_unary_prob: bad argument: null pointer");
    Plan p;
    if (int rc = plan(p, C, H, W, 1.f, 1.f, 1.f, "wc_dcrf_unary_prob")) return rc;
    const long n = (long)C * p.N;
    hipLaunchKernelGGL(dcrf_unary_prob_kernel, dim3(wc_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, probs, unary, n);
    WC_LAUNCH_CHECK("dcrf_unary_prob_kernel");
    return WC_OK;
}

extern "C" int wc_dcrf_unary_label(const int64_t* labels, float* unary, int C, int H, int W, float gt_prob, void* stream) {
    WC_CHECK_ARG(labels && unary, "wc_dcrf_unary_label: bad argument: null pointer");
    WC_CHECK_ARG(gt_prob > 0.f && gt_prob < 1.f && C >= 2, "wc_dcrf_unary_label: bad argument: gt_prob in (0, 1) and C >= 2 needed");
    Plan p;
    if (int rc = plan(p, C, H, W, 1.f, 1.f, 1.f, "wc_dcrf_unary_label")) return rc;
    const float u_on = (float)-log((double)gt_prob), u_off = (float)-log((1.0 - gt_prob) / (C - 1));
    hipLaunchKernelGGL(dcrf_unary_label_kernel, dim3(wc_cdiv(p.N, 256)), dim3(256), 0, (hipStream_t)stream, labels, unary, C, p.N,
                       u_on, u_off);
    WC_LAUNCH_CHECK("dcrf_unary_label_kernel");
    return WC_OK;
}

extern "C" int wc_dcrf_unary_logits(const float* logits, float* unary, int C, int h, int w, int H, int W, void* stream) {
    WC_CHECK_ARG(logits && unary, "wc_dcrf_unary_logits: bad argument: null pointer");
    WC_CHECK_ARG(h >= 1 && w >= 1 && (long)h * w <= DCRF_MAX_N, "wc_dcrf_unary_logits: bad argument: logit grid %d x %d", h, w);
    Plan p;
    if (int rc = plan(p, C, H, W, 1.f, 1.f, 1.f, "wc_dcrf_unary_logits")) return rc;
    hipLaunchKernelGGL(dcrf_unary_logits_kernel, dim3(wc_cdiv(p.N, 256)), dim3(256), 0, (hipStream_t)stream, logits, unary, C, h, w,
                       H, W, (float)h / H, (float)w / W);
    WC_LAUNCH_CHECK("dcrf_unary_logits_kernel");
    return WC_OK;
}

extern "C" int wc_dcrf_workspace_floats(int C, int H, int W, long* n_floats) {
    WC_CHECK_ARG(n_floats, "wc_dcrf_workspace_floats: bad argument: null pointer");
    Plan p;
    if (int rc = plan(p, C, H, W, 1.f, 1.f, 1.f, "wc_dcrf_workspace_floats")) return rc;
    *n_floats = (long)p.N * (12 + 2 * p.CP + 3L * p.C);
    return WC_OK;
}

extern "C" int wc_dcrf_message(const void* img, int img_is_u8, const float* Q, float* msg_pos, float* msg_bil, float* S, void* ws,
                               int C, int H, int W, float pos_xy_std, float bi_xy_std, float bi_rgb_std, void* stream) {
    WC_CHECK_ARG(img && Q && msg_pos && msg_bil && S && ws, "wc_dcrf_message: bad argument: null pointer");
    Plan p;
    if (int rc = plan(p, C, H, W, pos_xy_std, bi_xy_std, bi_rgb_std, "wc_dcrf_message")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(p, ws);
    if (int rc = normalisers(p, img, img_is_u8, H, W, w, S, st)) return rc;
    // operands from the given Q: Vp = n_pos Q (C, N), Vb = n_bil Q (N, CP)
    if (hipMemsetAsync(w.Vb[0], 0, sizeof(float) * (long)p.N * p.CP, st) != hipSuccess) {
        wc_set_error("wc_dcrf_message: hipMemsetAsync failed");
        return WC_ERR_HIP;
    }
    hipLaunchKernelGGL(dcrf_operands_kernel, dim3(wc_cdiv((long)p.C * p.N, 256)), dim3(256), 0, st, Q, w.nrm, w.Vb[0], w.Vp, p.C,
                       p.CP, p.N);
    WC_LAUNCH_CHECK("dcrf_operands_kernel");
    if (int rc = gauss_message(p, H, W, w.Vp, w.tmp, w.G, st)) return rc;
    hipLaunchKernelGGL(dcrf_scale_kernel, dim3(wc_cdiv((long)p.C * p.N, 256)), dim3(256), 0, st, w.G, w.nrm, msg_pos, p.C, p.N);
    WC_LAUNCH_CHECK("dcrf_scale_kernel");
    BilArgs a = {};
    a.feat = w.feat, a.V = w.Vb[0], a.N = p.N, a.C = p.C, a.CP = p.CP, a.a_xy = p.a_xy, a.a_rgb = p.a_rgb, a.mode = 1;
    a.nrm = w.nrm + p.N;
    a.msg = msg_bil;
    return launch_bil(p, a, st);
}

extern "C" int wc_dcrf_inference(const void* img, int img_is_u8, const float* unary, float* Q, void* ws, int C, int H, int W,
                                 int iter_max, float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std,
                                 void* stream) {
    WC_CHECK_ARG(img && unary && Q && ws, "wc_dcrf_inference: bad argument: null pointer");
    WC_CHECK_ARG(iter_max >= 0, "wc_dcrf_inference: bad argument: iter_max = %d < 0", iter_max);
    WC_CHECK_ARG(pos_w >= 0.f && pos_w < INFINITY && bi_w >= 0.f && bi_w < INFINITY,
                 "wc_dcrf_inference: bad argument: weights must be finite and >= 0");
    Plan p;
    if (int rc = plan(p, C, H, W, pos_xy_std, bi_xy_std, bi_rgb_std, "wc_dcrf_inference")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(p, ws);
    if (int rc = normalisers(p, img, img_is_u8, H, W, w, nullptr, st)) return rc;
    // padded label columns of both operand buffers stay zero
    if (hipMemsetAsync(w.Vb[0], 0, sizeof(float) * 2L * p.N * p.CP, st) != hipSuccess) {
        wc_set_error("wc_dcrf_inference: hipMemsetAsync failed");
        return WC_ERR_HIP;
    }
    hipLaunchKernelGGL(dcrf_init_kernel, dim3(wc_cdiv(p.N, 256)), dim3(256), 0, st, unary, w.nrm, Q, w.Vb[0], w.Vp, p.C, p.CP, p.N);
    WC_LAUNCH_CHECK("dcrf_init_kernel");
    for (int it = 0; it < iter_max; ++it) {
        if (int rc = gauss_message(p, H, W, w.Vp, w.tmp, w.G, st)) return rc;
        BilArgs a = {};
        a.feat = w.feat, a.V = w.Vb[it & 1], a.N = p.N, a.C = p.C, a.CP = p.CP, a.a_xy = p.a_xy, a.a_rgb = p.a_rgb, a.mode = 2;
        a.nrm = w.nrm + p.N;
        a.U = unary, a.G = w.G, a.npos = w.nrm, a.w_bil = bi_w, a.w_pos = pos_w;
        a.Q = Q, a.Vb_out = w.Vb[(it + 1) & 1], a.Vp_out = w.Vp;
        if (int rc = launch_bil(p, a, st)) return rc;
    }
    return WC_OK;
}

// ------------------------------------------------------------------------------------------------ shared with dcrf_lattice.hip
#include "dcrf_shared.h"

namespace dcrf_shared {

int limits(int C, int H, int W, float pos_xy_std, float bi_xy_std, float bi_rgb_std, const char* who) {
    Plan p;
    return plan(p, C, H, W, pos_xy_std, bi_xy_std, bi_rgb_std, who);
}

int pos_norm(int H, int W, float pos_xy_std, float* S, float* nrm, hipStream_t st) {
    Plan p;
    if (int rc = plan(p, 1, H, W, pos_xy_std, 1.f, 1.f, "dcrf")) return rc;
    hipLaunchKernelGGL(dcrf_gauss_norm_kernel, dim3(wc_cdiv(p.N, 256)), dim3(256), 0, st, S, nrm, H, W, p.R, p.a_pos);
    WC_LAUNCH_CHECK("dcrf_gauss_norm_kernel");
    return WC_OK;
}

int gauss_message(int C, int H, int W, float pos_xy_std, const float* in, float* tmp, float* out, hipStream_t st) {
    Plan p;
    if (int rc = plan(p, C, H, W, pos_xy_std, 1.f, 1.f, "dcrf")) return rc;
    return ::gauss_message(p, H, W, in, tmp, out, st);
}

int init(const float* U, const float* nrm, float* Q, float* Vb, float* Vp, int C, int CP, int N, hipStream_t st) {
    hipLaunchKernelGGL(dcrf_init_kernel, dim3(wc_cdiv(N, 256)), dim3(256), 0, st, U, nrm, Q, Vb, Vp, C, CP, N);
    WC_LAUNCH_CHECK("dcrf_init_kernel");
    return WC_OK;
}

int operands(const float* Q, const float* nrm, float* Vb, float* Vp, int C, int CP, int N, hipStream_t st) {
    hipLaunchKernelGGL(dcrf_operands_kernel, dim3(wc_cdiv((long)C * N, 256)), dim3(256), 0, st, Q, nrm, Vb, Vp, C, CP, N);
    WC_LAUNCH_CHECK("dcrf_operands_kernel");
    return WC_OK;
}

int scale(const float* G, const float* nrm, float* msg, int C, int N, hipStream_t st) {
    hipLaunchKernelGGL(dcrf_scale_kernel, dim3(wc_cdiv((long)C * N, 256)), dim3(256), 0, st, G, nrm, msg, C, N);
    WC_LAUNCH_CHECK("dcrf_scale_kernel");
    return WC_OK;
}

}  // namespace dcrf_shared
