// Dense energy (regularised CRF) loss: the energy of the fully connected bilateral kernel over the soft-max output, the device
// form of the reference's utils/losses.py:52-116 (`DenseEnergyLossFunction`, `DenseEnergyLoss`), whose `bilateralfilter`
// extension (a permutohedral lattice, not shipped) only approximates the sums that are formed exactly here
// (DESIGN.md section 15).
//
//   energy_prep_kernel   : per image n, 64 pixels per workgroup: features (x, y, R, G, B) -> (N, HW, 8) f32 rows from the NCHW
//                          image; the operand V (N, HW, CP) = P * ROI, CP = 32 ceil(K / 32), padding columns zero; the Gate
//                          (N, HW) = ROI - max_k P, 1 where unlabelled, 0 where negative.  P is read along the pixels (the
//                          contiguous side of a (K, HW) plane set), turned in LDS, and the 64 x CP tile -- one contiguous
//                          stretch of V -- is written in order: both sides of the transpose are coalesced.
//   energy_filter_kernel : AS(n, l, i) = sum_j k_n(i, j) V(n, j, l), the hot path: the exact all-pairs sum bil_exact_sum of
//                          csrc/bilateral_exact.h (which csrc/dcrf.hip's dcrf_bil_kernel runs too) with the image index in the
//                          grid and without normalisers.  Epilogue: A = Gate * AS -> (N, K, H, W), and this workgroup's
//                          partial of sum S * A (S re-read from V) -> partials[n][workgroup].
//   energy_finish_kernel : loss = -(1/N) sum of the partials, one workgroup, fixed order, f64 accumulation.
//   energy_bwd_kernel    : grad_P = (-2/N) g A ROI, g read from device memory.
// No atomics anywhere: every output is a fixed-order sum, bit-identical from run to run.
// Error model (per element of AS, relative to sum_j k |V_j|): bil_exact_sum's, stated in csrc/bilateral_exact.h: eps = 2^-10.
#include "common.h"
#include "bilateral_exact.h"
#include "energy_shared.h"        // what csrc/energy_lattice.hip (the opt-in lattice form of the filter) runs of this file

#define EN_MAX_K 128
#define EN_MAX_HW (640 * 640)
#define EN_MAX_N 65535            // the image index is a grid dimension
#define EN_QW (BIL_NT / 2)        // queries per workgroup
#define EN_PP 64                  // pixels per prep workgroup

// ------------------------------------------------------------------------------------------------ prep
__global__ __launch_bounds__(256) void energy_prep_kernel(const float* __restrict__ img, const float* __restrict__ P,
                                                          const float* __restrict__ roi, const uint8_t* __restrict__ unl,
                                                          float* __restrict__ feat, float* __restrict__ V, float* __restrict__ gate,
                                                          int K, int CP, int HW, int W) {
    __shared__ float tile[EN_PP * (EN_MAX_K + 1)];
    __shared__ float smx[4 * EN_PP];
    const int tid = threadIdx.x, pix = tid & (EN_PP - 1), kg = tid >> 6, n = blockIdx.y;
    const int p0 = blockIdx.x * EN_PP, p = p0 + pix, pc = min(p, HW - 1);
    const int st = CP + 1;
    const long io = (long)n * HW + pc;
    const float r = roi ? roi[io] : 1.f;
    float mx = -INFINITY;
    const float* Pn = P + (long)n * K * HW + pc;
    for (int k = kg; k < CP; k += 4) {
        const float v = Pn[(long)min(k, K - 1) * HW];
        mx = fmaxf(mx, v);                                 // (k >= K re-reads plane K - 1: the maximum is unchanged)
        tile[pix * st + k] = k < K ? v * r : 0.f;
    }
    smx[kg * EN_PP + pix] = mx;
    if (kg == 1) {
        const float* in = img + (long)n * 3 * HW + pc;
        const float cr = in[0], cg = in[HW], cb = in[2L * HW];
        if (p < HW) {
            const int y = p / W;
            float4* f = reinterpret_cast<float4*>(feat + 8 * ((long)n * HW + p));
            f[0] = make_float4((float)(p - y * W), (float)y, cr, cg);
            f[1] = make_float4(cb, 0.f, 0.f, 0.f);
        }
    }
    __syncthreads();
    if (kg == 0 && gate) {
        const float m = fmaxf(fmaxf(smx[pix], smx[EN_PP + pix]), fmaxf(smx[2 * EN_PP + pix], smx[3 * EN_PP + pix]));
        const uint8_t u = unl[io];
        float g = r - m;
        if (u) g = 1.f;
        if (g < 0.f) g = 0.f;
        if (p < HW) gate[io] = g;
    }
    const int ne = min(EN_PP, HW - p0) * CP;               // the tile is one contiguous stretch of V
    float* Vt = V + ((long)n * HW + p0) * CP;
    for (int e = tid; e < ne; e += 256) {
        const int row = e / CP;
        Vt[e] = tile[row * st + (e - row * CP)];
    }
}

// ------------------------------------------------------------------------------------------------ filter
struct EnergyFilterArgs {
    const float* feat;     // (N, HW, 8): x, y, R, G, B
    const float* V;        // (N, HW, CP) operand; columns >= K are zero
    const float* gate;     // (N, HW), or null: no gate
    float* out;            // (N, K, HW)
    float* part;           // (N, gridDim.x) partials of sum V * out, or null
    int HW, K;
    float a_xy, a_rgb;     // log2(e) / (2 sigma^2)
};

template <int CT>
__global__ __launch_bounds__(BIL_NT, 2) void energy_filter_kernel(EnergyFilterArgs A) {
    constexpr int CP = 32 * CT;
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int N = A.HW, n = blockIdx.y;
    const float* V = A.V + (long)n * N * CP;
    const int qi = blockIdx.x * EN_QW + wave * 32 + l31;
    const int qc = qi < N ? qi : N - 1;
    f32x16 tot[CT];
    bil_exact_sum<CT>(A.feat + 8L * n * N, V, N, qc, A.a_xy, A.a_rgb, tot);

    // epilogue: tot[c][r] = AS(label bil_label(c, r, h), query qi); a lane's labels come in runs of four
    const int K = A.K;
    const float g = A.gate ? A.gate[(long)n * N + qc] : 1.f;
    float4 sq[CT * 4];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) sq[c * 4 + q] = *reinterpret_cast<const float4*>(V + (long)qc * CP + 32 * c + 8 * q + 4 * h);
    float ps = 0.f;
    if (qi < N) {
        float* out = A.out + (long)n * K * N + qi;
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int l = bil_label(c, r, h);
                if (l < K) {
                    const float a = g * tot[c][r];
                    out[(long)l * N] = a;
                    const float4 s4 = sq[c * 4 + (r >> 2)];
                    const float sv_ = (r & 3) == 0 ? s4.x : (r & 3) == 1 ? s4.y : (r & 3) == 2 ? s4.z : s4.w;
                    ps = fmaf(sv_, a, ps);
                }
            }
    }
    if (A.part) {                                           // fixed order: lane chain, xor tree, four waves
        ps = wave_sum(ps);
        if (lane == 0) red[wave] = ps;
        __syncthreads();
        if (tid == 0) A.part[(long)n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// loss = -(1/N) sum part[0 .. n): one workgroup, thread t sums elements t, t + 256, ... in f64, then a fixed tree
__global__ __launch_bounds__(256) void energy_finish_kernel(const float* __restrict__ part, long n, double scale,
                                                            float* __restrict__ loss) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc += (double)part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(scale * red[0]);
}

// grad (N, K, HW) = ((c g) A) ROI, c = -2 / N; grid (pixels, K, N)
__global__ __launch_bounds__(256) void energy_bwd_kernel(const float* __restrict__ A, const float* __restrict__ roi,
                                                         const float* __restrict__ g, float* __restrict__ grad, float c, int HW) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const long e = ((long)blockIdx.z * gridDim.y + blockIdx.y) * HW + p;
    const float a = A[e], r = roi[(long)blockIdx.z * HW + p], s = c * g[0];
    grad[e] = (s * a) * r;
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

struct EPlan {
    int N, K, HW, W, CT, CP, nwg;
    float a_xy, a_rgb;
};

bool finite_pos(float v) { return v > 0.f && v < INFINITY; }

int eplan(EPlan& p, int N, int K, int H, int W, float sigma_rgb, float sigma_xy, const char* who) {
    WC_CHECK_ARG(N >= 1 && N <= EN_MAX_N, "%s: bad argument: N = %d outside [1, %d]", who, N, EN_MAX_N);
    WC_CHECK_ARG(K >= 1 && K <= EN_MAX_K, "%s: bad argument: K = %d outside [1, %d]", who, K, EN_MAX_K);
    WC_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= EN_MAX_HW, "%s: bad argument: H x W = %d x %d outside [1, 640*640] pixels", who,
                 H, W);
    WC_CHECK_ARG(finite_pos(sigma_rgb) && finite_pos(sigma_xy), "%s: bad argument: sigmas must be finite and > 0", who);
    p.N = N, p.K = K, p.HW = H * W, p.W = W;
    p.CT = (K + 31) / 32;
    p.CP = 32 * p.CT;
    p.nwg = wc_cdiv(p.HW, EN_QW);
    p.a_xy = (float)(1.4426950408889634 / (2.0 * (double)sigma_xy * sigma_xy));
    p.a_rgb = (float)(1.4426950408889634 / (2.0 * (double)sigma_rgb * sigma_rgb));
    return WC_OK;
}

// workspace carve-up (floats): feat 8 N HW | V N HW CP | partials N nwg
struct EWs {
    float *feat, *V, *part;
};

EWs ecarve(const EPlan& p, void* ws) {
    EWs w;
    w.feat = (float*)ws;
    w.V = w.feat + 8L * p.N * p.HW;
    w.part = w.V + (long)p.N * p.HW * p.CP;
    return w;
}

// prep + filter: out (N, K, HW) = gate * AS; partials when `part` is given
int prep_and_filter(const EPlan& p, const EWs& w, const float* images, const float* segs, const float* rois, const void* unlabel,
                    float* gate, float* out, float* part, hipStream_t st) {
    hipLaunchKernelGGL(energy_prep_kernel, dim3(wc_cdiv(p.HW, EN_PP), p.N), dim3(256), 0, st, images, segs, rois,
                       (const uint8_t*)unlabel, w.feat, w.V, gate, p.K, p.CP, p.HW, p.W);
    WC_LAUNCH_CHECK("energy_prep_kernel");
    EnergyFilterArgs a = {};
    a.feat = w.feat, a.V = w.V, a.gate = gate, a.out = out, a.part = part, a.HW = p.HW, a.K = p.K, a.a_xy = p.a_xy, a.a_rgb = p.a_rgb;
    const dim3 grid(p.nwg, p.N), block(BIL_NT);
    const int idx = wc_prof_begin(st);
    switch (p.CT) {
        case 1: hipLaunchKernelGGL(energy_filter_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(energy_filter_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(energy_filter_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(energy_filter_kernel<4>, grid, block, 0, st, a); break;
    }
    WC_LAUNCH_CHECK("energy_filter_kernel");
    wc_prof_end(idx, "energy_filter_kernel", 2.0 * p.N * (double)p.HW * (double)p.HW * p.CP, st);
    return WC_OK;
}

}  // namespace

extern "C" int wc_energy_workspace_floats(int N, int K, int H, int W, long* n_floats) {
    WC_CHECK_ARG(n_floats, "wc_energy_workspace_floats: bad argument: null pointer");
    EPlan p;
    if (int rc = eplan(p, N, K, H, W, 1.f, 1.f, "wc_energy_workspace_floats")) return rc;
    *n_floats = (long)p.N * ((long)p.HW * (8 + p.CP) + p.nwg);
    return WC_OK;
}

extern "C" int wc_bilateral_filter_batch(const float* images, const float* segs, float* AS, void* ws, int N, int K, int H, int W,
                                         float sigma_rgb, float sigma_xy, void* stream) {
    WC_CHECK_ARG(images && segs && AS && ws, "wc_bilateral_filter_batch: bad argument: null pointer");
    EPlan p;
    if (int rc = eplan(p, N, K, H, W, sigma_rgb, sigma_xy, "wc_bilateral_filter_batch")) return rc;
    return prep_and_filter(p, ecarve(p, ws), images, segs, nullptr, nullptr, nullptr, AS, nullptr, (hipStream_t)stream);
}

extern "C" int wc_dense_energy_fwd(const float* images, const float* segs, const float* rois, const void* unlabel_u8, float* A,
                                   float* gate, float* loss, void* ws, int N, int K, int H, int W, float sigma_rgb, float sigma_xy,
                                   void* stream) {
    WC_CHECK_ARG(images && segs && rois && unlabel_u8 && A && gate && loss && ws, "wc_dense_energy_fwd: bad argument: null pointer");
    EPlan p;
    if (int rc = eplan(p, N, K, H, W, sigma_rgb, sigma_xy, "wc_dense_energy_fwd")) return rc;
    const EWs w = ecarve(p, ws);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = prep_and_filter(p, w, images, segs, rois, unlabel_u8, gate, A, w.part, st)) return rc;
    hipLaunchKernelGGL(energy_finish_kernel, dim3(1), dim3(256), 0, st, w.part, (long)p.N * p.nwg, -1.0 / p.N, loss);
    WC_LAUNCH_CHECK("energy_finish_kernel");
    return WC_OK;
}

extern "C" int wc_dense_energy_bwd(const float* A, const float* rois, const float* grad_out, float* grad_segs, int N, int K, int H,
                                   int W, void* stream) {
    WC_CHECK_ARG(A && rois && grad_out && grad_segs, "wc_dense_energy_bwd: bad argument: null pointer");
    EPlan p;
    if (int rc = eplan(p, N, K, H, W, 1.f, 1.f, "wc_dense_energy_bwd")) return rc;
    hipLaunchKernelGGL(energy_bwd_kernel, dim3(wc_cdiv(p.HW, 256), p.K, p.N), dim3(256), 0, (hipStream_t)stream, A, rois, grad_out,
                       grad_segs, (float)(-2.0 / p.N), p.HW);
    WC_LAUNCH_CHECK("energy_bwd_kernel");
    return WC_OK;
}

// ---- what csrc/energy_lattice.hip shares (energy_shared.h)
int energy_shared::limits(int N, int K, int H, int W, float sigma_rgb, float sigma_xy, const char* who) {
    EPlan p;
    return eplan(p, N, K, H, W, sigma_rgb, sigma_xy, who);
}

int energy_shared::prep(const float* images, const float* segs, const float* rois, const void* unlabel_u8, float* feat, float* V,
                        float* gate, int N, int K, int H, int W, hipStream_t st) {
    const int HW = H * W, CP = 32 * ((K + 31) / 32);
    hipLaunchKernelGGL(energy_prep_kernel, dim3(wc_cdiv(HW, EN_PP), N), dim3(256), 0, st, images, segs, rois,
                       (const uint8_t*)unlabel_u8, feat, V, gate, K, CP, HW, W);
    WC_LAUNCH_CHECK("energy_prep_kernel");
    return WC_OK;
}

int energy_shared::finish(const float* part, long n, double scale, float* loss, hipStream_t st) {
    hipLaunchKernelGGL(energy_finish_kernel, dim3(1), dim3(256), 0, st, part, n, scale, loss);
    WC_LAUNCH_CHECK("energy_finish_kernel");
    return WC_OK;
}
