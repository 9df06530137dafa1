// The exact all-pairs bilateral sum, device code shared as text by dcrf_bil_kernel (csrc/dcrf.hip) and energy_filter_kernel
// (csrc/energy.hip): tot(l, i) = sum_j k(i, j) V(j, l) over every pixel j of one image, k(i, j) = exp(-|p_i - p_j|^2 /
// (2 sigma_xy^2) - |I_i - I_j|^2 / (2 sigma_rgb^2)).  The two kernels differ in where their image lies and in their epilogues.
//
// A wave owns 32 query pixels, a workgroup 4 waves; 64-key tiles of features and of the operand V stream through LDS with the
// next tile's loads in flight in registers.  Per pair the exponent is formed in f32 from DIFFERENCES of raw features (integer
// pixel offsets and colour differences are exact in f32, so no cancellation at any std or image size), log2(e) / (2 sigma^2) is
// folded into the two coefficients so that a bare v_exp_f32 gives k, and an f32-input MFMA (v_mfma_f32_32x32x2_f32: A = V^T,
// 32 labels x 2 keys; B = K, 2 keys x 32 queries) accumulates M^T = V^T K.  A lane computes exactly the one k(i, j) its B operand
// needs (query lane & 31, key 2s + lane / 32).  Each 64-key tile is summed in its own accumulator and then added to the running
// total (two-level summation).  No atomics: every output is one wave's fixed-order sum, bit-identical from run to run.
// Error model (per element, relative to the sum of its terms' magnitudes sum_j k_ij |V_j(l)|):
//   operands are f32 (V rounded once, 2^-24); exponent from exact differences, <= 3 roundings of a value |e| <= 40 that
//   matters (2^-19 of k through exp2); v_exp_f32 <= 2^-22; accumulation: a 64-key tile chain (<= 63 u) plus the running
//   sum over <= 6400 tiles (N <= 640^2): <= 6500 * 2^-24 < 2^-11.3.  Total eps = 2^-10 (include/weclip_hip.h), with the terms
//   k < 2^-126 flushed by exp2's range (an absolute 2^-126 N per element, far below the 2^-24 of the tests).
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define BIL_KT 64           // keys per LDS tile
#define BIL_NT 256          // 4 waves x 32 queries; a workgroup owns BIL_NT / 2 queries

// the label of accumulator register r of column tile c in half-wave h: tot[c][r] = M^T(bil_label(c, r, h), query)
__device__ __forceinline__ int bil_label(int c, int r, int h) { return 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h; }

// feat (N, 8): x, y, R, G, B rows and V (N, 32 CT): the operand, columns past the labels zero, both of the image being filtered;
// qc: this lane's query pixel, clamped to N - 1; a_xy, a_rgb: log2(e) / (2 sigma^2).  Called by all BIL_NT threads of the
// workgroup (it synchronises); tot is overwritten.
template <int CT>
__device__ __forceinline__ void bil_exact_sum(const float* __restrict__ feat, const float* __restrict__ V, int N, int qc, float axy,
                                              float argb, f32x16 (&tot)[CT]) {
    constexpr int CP = 32 * CT;
    constexpr int VST = CP + ((CT & 1) ? 0 : 32);      // LDS row stride: the two half-waves read rows 32 banks apart
    constexpr int NVL = BIL_KT * CP / 4 / BIL_NT;      // float4 of V per thread per tile
    __shared__ __attribute__((aligned(16))) float sf[BIL_KT * 8];
    __shared__ __attribute__((aligned(16))) float sv[BIL_KT * VST];

    const int tid = threadIdx.x, lane = tid & 63;
    const int h = lane >> 5, l31 = lane & 31;
    const float4 qf = *reinterpret_cast<const float4*>(feat + 8L * qc);
    const float qb = feat[8L * qc + 4];

#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[c][r] = 0.f;

    // register staging of the next tile (out-of-range keys: zero features and zero V rows)
    float4 rf;
    float4 rv[NVL];
    auto gload = [&](int t) {
        const int k0 = t * BIL_KT;
        if (tid < BIL_KT * 2) {
            const int key = min(k0 + (tid >> 1), N - 1);
            rf = *reinterpret_cast<const float4*>(feat + 8L * key + 4 * (tid & 1));
            if (k0 + (tid >> 1) >= N) rf = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < NVL; ++u) {
            const int e = tid + BIL_NT * u;                 // float4 index in the 64 x CP tile
            const int kr = e / (CP / 4);
            const int key = min(k0 + kr, N - 1);
            rv[u] = *reinterpret_cast<const float4*>(V + (long)key * CP + 4 * (e % (CP / 4)));
        }
#pragma unroll
        for (int u = 0; u < NVL; ++u)
            if (k0 + (tid + BIL_NT * u) / (CP / 4) >= N) rv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto lstore = [&]() {
        if (tid < BIL_KT * 2) *reinterpret_cast<float4*>(sf + 4 * tid) = rf;
#pragma unroll
        for (int u = 0; u < NVL; ++u) {
            const int e = tid + BIL_NT * u;
            const int kr = e / (CP / 4);
            *reinterpret_cast<float4*>(sv + kr * VST + 4 * (e % (CP / 4))) = rv[u];
        }
    };

    const int ntiles = (N + BIL_KT - 1) / BIL_KT;
    gload(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                                    // previous tile consumed
        lstore();
        __syncthreads();
        if (t + 1 < ntiles) gload(t + 1);                   // in flight during the tile's arithmetic
        f32x16 acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
#pragma unroll 4
        for (int s = 0; s < BIL_KT / 2; ++s) {
            const int key = 2 * s + h;
            const float4 kf = *reinterpret_cast<const float4*>(sf + 8 * key);
            const float kb = sf[8 * key + 4];
            const float dx = qf.x - kf.x, dy = qf.y - kf.y;
            const float dr = qf.z - kf.z, dg = qf.w - kf.w, db = qb - kb;
            float pxy = dx * dx;
            pxy = fmaf(dy, dy, pxy);
            float prgb = dr * dr;
            prgb = fmaf(dg, dg, prgb);
            prgb = fmaf(db, db, prgb);
            const float k = __builtin_amdgcn_exp2f(-fmaf(pxy, axy, prgb * argb));
#pragma unroll
            for (int c = 0; c < CT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[key * VST + 32 * c + l31], k, acc[c], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) tot[c] += acc[c];
    }
}
