// Multi-bandwidth RBF maximum mean discrepancy: the device form of the reference's utils/mmdloss.py:4-35 (`rbf_kernel`) and
// :38-59 (`mmd_rbf`), without the (N, N, d) expansion of :19-23 and -- for the loss and its gradient -- without the N x N matrix
// (DESIGN.md section 18).  X = cat(source, target), N = 2 B rows of width d.
//
//   mmd_colsum_kernel  : partial column sums of X over 32 row slices of the source and 32 of the target, f64.
//   mmd_mean_kernel    : the two blocks' means mu_s, mu_t = (sum of a block's slices, fixed order) / B.
//   mmd_centre_kernel  : Xc (N, dp) = a_i = x_i - (its own block's mean) in f32, dp = 32 ceil(d / 32), padding columns zero;
//                        nrm_i = |a_i|^2; mrow_i = nrm_i + 2 s_i delta . a_i, delta = mu_s - mu_t.  One wave per row.  With these
//                        |x_i - x_j|^2 = nrm_i + nrm_j - 2 a_i . a_j inside a block and mrow_i + mrow_j + |delta|^2 - 2 a_i . a_j
//                        across the blocks: no term is larger than the blocks' own spread or the distance itself, wherever the
//                        data sits and however far apart the two sets lie (one common mean would leave |delta|^2 / 4 in every
//                        norm, to cancel inside a block).
//   mmd_scal_kernel    : bandwidth = fix_sigma, or 2 sum_i |c_i|^2 / (N - 1) with c centred on the mean of all rows
//                        (= sum_ij L2_ij / (N^2 - N): L2 is translation invariant and sum_ij |c_i - c_j|^2 = 2 N sum_i |c_i|^2
//                        when sum_i c_i = 0), sum_i |c_i|^2 = sum_i nrm_i + (N / 4) |delta|^2; divided by mul^(num / 2); then
//                        log2(e) / bw_b and 1 / bw_b, widest bandwidth first, and |delta|^2, as 17 device floats.  One
//                        workgroup, f64.  The bandwidth never leaves the device.
//   mmd_main_kernel    : the hot path.  A workgroup (4 waves) owns a 64-row tile i and walks 64-row tiles j; a wave owns a 32 x 32
//                        block of S^T(j, i) = Xc_j . Xc_i, formed over all of d on v_mfma_f32_32x32x2_f32 from 32-column LDS
//                        stages of both operands.  Epilogue in registers: L2 as above, clamped at 0 (diagonal forced
//                        to 0), the kernel_num exponentials (kernel_mul == 2: one v_exp_f32 at the widest bandwidth and
//                        kernel_num - 1 squarings), K = sum_b e_b and W = sum_b e_b / bw_b.
//                        <0>  : loss only.  K is symmetric: tiles j < i are skipped, tiles j > i count twice; grid
//                               (row tiles, j slices).
//                        <CT> : loss and gradient.  P(j, i) = s_j W_ij stays in the accumulator's registers and is the B operand
//                               of a second MFMA whose A operand is the j tile's 32 CT columns of Xc (LDS): O^T(c, i) +=
//                               sum_j Xc(j, c) P(j, i), attention's P V.  Grid (row tiles, ceil(dp / (32 CT))): a column chunk
//                               per workgroup, S recomputed per chunk.  grad_i = -(4 / B^2) s_i (r_i x_i - sum_j P x_j), r_i =
//                               sum_j P, = -(4 / B^2) s_i (r_i a_i - O_i + q_i delta), q_i = the target rows' share of r_i on a
//                               source row and minus the source rows' share on a target row.
//                        Partial sums of s_i s_j K_ij per workgroup, f64.
//   mmd_finish_kernel  : loss = (1 / B^2) sum of the partials, one workgroup, fixed order, f64.
//   mmd_matrix_kernel  : K (N, N) f32 for `rbf_kernel`: the same tile arithmetic; an element with j >= i is computed once and
//                        stored at (i, j) and (j, i), so the matrix is symmetric bit for bit and its diagonal is kernel_num.
// No atomics anywhere: every output is a fixed-order sum, bit-identical from run to run.
// All rows identical: bandwidth 0, 0 * inf in the exponent, a NaN loss, as in the reference.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));        // (native: arrays of HIP's struct float4 stay in scratch)

#define MM_MAX_B (1 << 20)
#define MM_MAX_D 8192
#define MM_MAX_NUM 8
#define MM_T 64                   // rows per tile, both sides
#define MM_KC 32                  // columns of d per LDS stage
#define MM_KST (MM_KC + 4)        // LDS row stride of a stage: float4 aligned
#define MM_CT 4                   // 32-column blocks of the gradient chunk
#define MM_DC (32 * MM_CT)        // gradient chunk width
#define MM_VST (MM_DC + 8)        // LDS row stride of the chunk: rows 4 apart (the two half-waves) land 32 banks apart
#define MM_RS 64                  // row slices of the column sum
#define MM_LOG2E 1.4426950408889634

template <bool HALF>
__device__ __forceinline__ float mm_load(const void* src, const void* tgt, int B, int d, int row, int col) {
    const void* p = row < B ? src : tgt;
    const long e = (long)(row < B ? row : row - B) * d + col;
    if (HALF) return __half2float(reinterpret_cast<const __half*>(p)[e]);
    return reinterpret_cast<const float*>(p)[e];
}

// ------------------------------------------------------------------------------------------------ prep
template <bool HALF>
__global__ __launch_bounds__(256) void mmd_colsum_kernel(const void* __restrict__ src, const void* __restrict__ tgt,
                                                         double* __restrict__ pm, int B, int d, int dp) {
    __shared__ double red[256];
    const int tid = threadIdx.x, col = blockIdx.x * 64 + (tid & 63), rg = tid >> 6;
    const int blk = blockIdx.y / (MM_RS / 2), per = (B + MM_RS / 2 - 1) / (MM_RS / 2);      // slices 0..31: source, 32..63: target
    const int r0 = blk * B + (blockIdx.y % (MM_RS / 2)) * per, r1 = min(blk * B + B, r0 + per);
    double acc = 0.0;
    if (col < d)
        for (int r = r0 + rg; r < r1; r += 4) acc += (double)mm_load<HALF>(src, tgt, B, d, r, col);
    red[tid] = acc;
    __syncthreads();
    if (rg == 0 && col < dp) pm[(long)blockIdx.y * dp + col] = (red[tid] + red[tid + 64]) + (red[tid + 128] + red[tid + 192]);
}

// mean (2, dp): the source rows' and the target rows' column means
__global__ __launch_bounds__(256) void mmd_mean_kernel(const double* __restrict__ pm, float* __restrict__ mean, int B, int dp) {
    const int col = blockIdx.x * 256 + threadIdx.x, blk = blockIdx.y;
    if (col >= dp) return;
    double acc = 0.0;
    for (int s = 0; s < MM_RS / 2; ++s) acc += pm[(long)(blk * (MM_RS / 2) + s) * dp + col];
    mean[blk * dp + col] = (float)(acc / B);
}

template <bool HALF>
__global__ __launch_bounds__(256) void mmd_centre_kernel(const void* __restrict__ src, const void* __restrict__ tgt,
                                                         const float* __restrict__ mean, float* __restrict__ Xc,
                                                         float* __restrict__ nrm, float* __restrict__ mrow, int B, int d, int dp) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= 2 * B) return;
    const float* own = mean + (row < B ? 0 : dp);
    float acc = 0.f, lin = 0.f;
    for (int c = lane; c < dp; c += 64) {
        const float v = c < d ? mm_load<HALF>(src, tgt, B, d, row, c) - own[c] : 0.f;
        Xc[(long)row * dp + c] = v;
        acc = fmaf(v, v, acc);
        lin = fmaf(v, mean[c] - mean[dp + c], lin);
    }
    acc = wave_sum(acc);
    lin = wave_sum(lin);
    if (lane == 0) {
        nrm[row] = acc;
        mrow[row] = row < B ? acc + 2.f * lin : acc - 2.f * lin;
    }
}

// scal[t] = log2(e) / bw_(num-1-t), scal[8 + t] = 1 / bw_(num-1-t): widest bandwidth first
__global__ __launch_bounds__(256) void mmd_scal_kernel(const float* __restrict__ nrm, const float* __restrict__ mean,
                                                       float* __restrict__ scal, int N, int dp, int num, double mul,
                                                       double fix_sigma) {
    __shared__ double red[256], red2[256];
    double acc = 0.0, dd = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) acc += (double)nrm[i];
    for (int c = threadIdx.x; c < dp; c += 256) {
        const double dl = (double)(mean[c] - mean[dp + c]);      // (the f32 difference: the one mmd_centre_kernel used)
        dd += dl * dl;
    }
    red[threadIdx.x] = acc, red2[threadIdx.x] = dd;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s], red2[threadIdx.x] += red2[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // sum_i |x_i - mean of all|^2 = sum_i nrm_i + (N / 4) |delta|^2: the two blocks' means lie delta / 2 either side of it
        const double ssq = red[0] + 0.25 * N * red2[0];
        scal[16] = (float)red2[0];
        double bw = fix_sigma != 0.0 ? fix_sigma : 2.0 * ssq / (double)(N - 1);
        for (int b = 0; b < num / 2; ++b) bw /= mul;
        for (int b = 0; b < num; ++b) {
            scal[num - 1 - b] = (float)(MM_LOG2E / bw);
            scal[8 + num - 1 - b] = (float)(1.0 / bw);
            bw *= mul;
        }
        for (int t = num; t < 8; ++t) scal[t] = scal[8 + t] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ tiles
struct MmdArgs {
    const float* Xc;       // (N, dp) centred rows
    const float* nrm;      // (N) |a_i|^2, a = the rows centred on their own block's mean
    const float* mrow;     // (N) |a_i|^2 + 2 s_i delta . a_i, delta = source mean - target mean
    const float* mean;     // (2, dp) the two means
    const float* scal;     // mmd_scal_kernel's: 8 x log2(e) / bw, 8 x 1 / bw, |delta|^2
    double* part;          // loss partials, or null
    float* grad;           // (N, d) f32, gradient kernels only
    float* K;              // (N, N) f32, matrix kernel only
    int N, B, d, dp, num, pow2;
    float gscale;          // -4 / B^2
};

// row of S^T held by accumulator register r of a lane in half-wave h
__device__ __forceinline__ int mm_jrow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// one wave's 32 x 32 block of S^T(j, i) over all of d; sxi / sxj: MM_T x MM_KST stages.  All 256 threads call this together.
__device__ __forceinline__ f32x16 mm_gram(const MmdArgs& A, int i0, int j0, float* sxi, float* sxj, int tid, int ih, int jh) {
    const int lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int N = A.N, dp = A.dp;
    f32x4 ri[2], rj[2];
    auto gload = [&](int kc) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + 256 * u, row = e >> 3, c4 = e & 7;
            ri[u] = *reinterpret_cast<const f32x4*>(A.Xc + (long)min(i0 + row, N - 1) * dp + kc + 4 * c4);
            rj[u] = *reinterpret_cast<const f32x4*>(A.Xc + (long)min(j0 + row, N - 1) * dp + kc + 4 * c4);
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    gload(0);
    for (int kc = 0; kc < dp; kc += MM_KC) {
        __syncthreads();                                    // previous stage consumed
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + 256 * u, row = e >> 3, c4 = e & 7;
            *reinterpret_cast<f32x4*>(sxi + row * MM_KST + 4 * c4) = ri[u];
            *reinterpret_cast<f32x4*>(sxj + row * MM_KST + 4 * c4) = rj[u];
        }
        __syncthreads();
        if (kc + MM_KC < dp) gload(kc + MM_KC);             // in flight during the stage's arithmetic
#pragma unroll
        for (int g = 0; g < MM_KC / 8; ++g) {               // a lane's four k of this group: 8 g + 4 h + (0..3), same on both sides
            const float4 a = *reinterpret_cast<const float4*>(sxj + (jh * 32 + l31) * MM_KST + 8 * g + 4 * h);
            const float4 b = *reinterpret_cast<const float4*>(sxi + (ih * 32 + l31) * MM_KST + 8 * g + 4 * h);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    return acc;
}

struct MmdScal {
    float a[MM_MAX_NUM], ib[MM_MAX_NUM];
};

__device__ __forceinline__ MmdScal mm_scal(const MmdArgs& A) {
    MmdScal s;
#pragma unroll
    for (int t = 0; t < MM_MAX_NUM; ++t) s.a[t] = A.scal[t], s.ib[t] = A.scal[8 + t];
    return s;
}

// K = sum_b exp(-l2 / bw_b), W = sum_b exp(-l2 / bw_b) / bw_b
__device__ __forceinline__ void mm_kw(const MmdScal& s, int num, int pow2, float l2, float& k, float& w) {
    if (pow2) {                                             // bw_b = bw_(b+1) / 2: e_b = e_(b+1)^2
        float e = __builtin_amdgcn_exp2f(-l2 * s.a[0]);
        k = e, w = e * s.ib[0];
#pragma unroll
        for (int t = 1; t < MM_MAX_NUM; ++t)
            if (t < num) {
                e *= e;
                k += e;
                w = fmaf(e, s.ib[t], w);
            }
    } else {
        k = 0.f, w = 0.f;
#pragma unroll
        for (int t = 0; t < MM_MAX_NUM; ++t)
            if (t < num) {
                const float e = __builtin_amdgcn_exp2f(-l2 * s.a[t]);
                k += e;
                w = fmaf(e, s.ib[t], w);
            }
    }
}

template <int CT>
__global__ __launch_bounds__(256) void mmd_main_kernel(MmdArgs A) {
    constexpr bool GRAD = CT > 0;
    constexpr int NV = GRAD ? MM_T * MM_VST : 4;
    __shared__ __attribute__((aligned(16))) float sxi[MM_T * MM_KST];
    __shared__ __attribute__((aligned(16))) float sxj[MM_T * MM_KST];
    __shared__ __attribute__((aligned(16))) float sv[NV];   // the j tile's chunk columns; the epilogue's 64 x chunk transpose
    __shared__ float snj[MM_T], smj[MM_T];
    __shared__ float srs[2 * 4 * 64];
    __shared__ double sred[256];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31, ih = wave & 1, jh = wave >> 1;
    const int N = A.N, B = A.B, dp = A.dp, num = A.num, pow2 = A.pow2;
    const int ti = blockIdx.x, i0 = ti * MM_T, nt = gridDim.x;
    const int c0 = GRAD ? blockIdx.y * (32 * CT) : 0;
    const int gi = i0 + ih * 32 + l31;
    const float ni = A.nrm[min(gi, N - 1)], mi = A.mrow[min(gi, N - 1)] + A.scal[16];
    const float si = gi < B ? 1.f : -1.f;
    const MmdScal sc = mm_scal(A);

    f32x16 tot[GRAD ? CT : 1];
#pragma unroll
    for (int c = 0; c < (GRAD ? CT : 1); ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[c][r] = 0.f;
    double lsum = 0.0;
    float rsum_s = 0.f, rsum_t = 0.f;                       // sum_j P over the source rows j and over the target rows j

    const int tj0 = GRAD ? 0 : ti + ((int)blockIdx.y - ti % (int)gridDim.y + (int)gridDim.y) % (int)gridDim.y;
    const int tjs = GRAD ? 1 : gridDim.y;                   // loss only: slice y takes the tiles j >= i with j % slices == y
    for (int tj = tj0; tj < nt; tj += tjs) {
        const int j0 = tj * MM_T;
        __syncthreads();                                    // previous tile's sv / snj reads are done
        if (tid < MM_T) snj[tid] = A.nrm[min(j0 + tid, N - 1)], smj[tid] = A.mrow[min(j0 + tid, N - 1)];
        if constexpr (GRAD) {
#pragma unroll
            for (int u = 0; u < MM_T * CT * 8 / 256; ++u) {
                const int e = tid + 256 * u, row = e / (CT * 8), c4 = e % (CT * 8), col = c0 + 4 * c4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (col < dp) v = *reinterpret_cast<const float4*>(A.Xc + (long)min(j0 + row, N - 1) * dp + col);
                *reinterpret_cast<float4*>(sv + row * MM_VST + 4 * c4) = v;
            }
        }
        const f32x16 S = mm_gram(A, i0, j0, sxi, sxj, tid, ih, jh);   // (its barriers publish sv and snj)
        float tl = 0.f;
        float P[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jr = jh * 32 + mm_jrow(r, h), gj = j0 + jr;
            const float sj = gj < B ? 1.f : -1.f;
            float l2 = fmaxf((si == sj ? ni + snj[jr] : mi + smj[jr]) - 2.f * S[r], 0.f);
            if (gi == gj) l2 = 0.f;
            float k, w;
            mm_kw(sc, num, pow2, l2, k, w);
            const bool ok = gi < N && gj < N;
            tl += ok ? si * sj * k : 0.f;
            P[r] = ok ? sj * w : 0.f;
            rsum_s += gj < B ? P[r] : 0.f;
            rsum_t += gj < B ? 0.f : P[r];
        }
        lsum += (double)(!GRAD && tj > ti ? 2.f * tl : tl);
        if constexpr (GRAD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* vr = sv + (jh * 32 + mm_jrow(r, h)) * MM_VST + l31;
#pragma unroll
                for (int c = 0; c < CT; ++c) tot[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32 * c], P[r], tot[c], 0, 0, 0);
            }
        }
    }

    // loss partial: fixed tree over the 256 lanes
    if (A.part && (!GRAD || blockIdx.y == 0)) {
        sred[tid] = lsum;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) sred[tid] += sred[tid + s];
            __syncthreads();
        }
        if (tid == 0) A.part[(long)blockIdx.y * gridDim.x + blockIdx.x] = sred[0];
    }
    if constexpr (GRAD) {
        // tot[c][r] = O^T(column c0 + 32 c + mm_jrow(r, h), row i0 + 32 ih + l31) of this wave's half of the j rows
        srs[wave * 64 + lane] = rsum_s, srs[256 + wave * 64 + lane] = rsum_t;
        __syncthreads();                                    // (also: the last tile's sv reads are done)
        if (jh == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) sv[(ih * 32 + l31) * MM_VST + 32 * c + mm_jrow(r, h)] = tot[c][r];
        }
        __syncthreads();
        if (jh == 1) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) sv[(ih * 32 + l31) * MM_VST + 32 * c + mm_jrow(r, h)] += tot[c][r];
        }
        __syncthreads();
        const int d = A.d;
        for (int e = tid; e < MM_T * 32 * CT; e += 256) {
            const int row = e / (32 * CT), c = e % (32 * CT), g = i0 + row, gc = c0 + c;
            if (g < N && gc < d) {
                const int w0 = row >> 5, l = row & 31;      // row sums: the two half-waves of the two waves that own the row, fixed order
                const float* q = srs + w0 * 64 + l;
                const float rs = (q[0] + q[32]) + (q[128] + q[160]), rt = (q[256] + q[288]) + (q[384] + q[416]);
                const float s = g < B ? A.gscale : -A.gscale;
                // x_j = a_j + its block's mean: r x_i - sum_j P x_j = r a_i - sum_j P a_j + (rt on a source row, -rs on a target row) delta
                const float dl = A.mean[gc] - A.mean[dp + gc];
                A.grad[(long)g * d + gc] = s * (((rs + rt) * A.Xc[(long)g * dp + gc] - sv[row * MM_VST + c]) + (g < B ? rt : -rs) * dl);
            }
        }
    }
}

__global__ __launch_bounds__(256) void mmd_matrix_kernel(MmdArgs A) {
    __shared__ __attribute__((aligned(16))) float sxi[MM_T * MM_KST];
    __shared__ __attribute__((aligned(16))) float sxj[MM_T * MM_KST];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj < ti) return;                                    // the mirror tile stores both halves
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31, ih = wave & 1, jh = wave >> 1;
    const int N = A.N, i0 = ti * MM_T, j0 = tj * MM_T;
    const int gi = i0 + ih * 32 + l31;
    const float ni = A.nrm[min(gi, N - 1)], mi = A.mrow[min(gi, N - 1)] + A.scal[16];
    const MmdScal sc = mm_scal(A);
    const f32x16 S = mm_gram(A, i0, j0, sxi, sxj, tid, ih, jh);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gj = j0 + jh * 32 + mm_jrow(r, h);
        if (gi < N && gj < N && gj >= gi) {
            float l2 = fmaxf(((gi < A.B) == (gj < A.B) ? ni + A.nrm[gj] : mi + A.mrow[gj]) - 2.f * S[r], 0.f);
            if (gi == gj) l2 = 0.f;
            float k, w;
            mm_kw(sc, A.num, A.pow2, l2, k, w);
            A.K[(long)gi * N + gj] = k;
            A.K[(long)gj * N + gi] = k;
        }
    }
}

// loss = scale * sum part[0 .. n): one workgroup, thread t sums elements t, t + 256, ... then a fixed tree, f64
__global__ __launch_bounds__(256) void mmd_finish_kernel(const double* __restrict__ part, long n, double scale,
                                                         float* __restrict__ loss) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc += part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(scale * red[0]);
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

struct MPlan {
    int B, N, d, dp, nt, js, nchunk, num, pow2;
    double mul, fix;
};

long up256(long b) { return (b + 255) / 256 * 256; }

int mplan(MPlan& p, int B, int d, int num, double mul, double fix, const char* who) {
    WC_CHECK_ARG(B >= 1 && B <= MM_MAX_B, "%s: bad argument: B = %d outside [1, %d]", who, B, MM_MAX_B);
    WC_CHECK_ARG(d >= 1 && d <= MM_MAX_D, "%s: bad argument: d = %d outside [1, %d]", who, d, MM_MAX_D);
    WC_CHECK_ARG(num >= 1 && num <= MM_MAX_NUM, "%s: bad argument: kernel_num = %d outside [1, %d]", who, num, MM_MAX_NUM);
    WC_CHECK_ARG(mul > 0.0 && mul < INFINITY, "%s: bad argument: kernel_mul must be finite and > 0", who);
    WC_CHECK_ARG(fix == fix && fix < INFINITY && fix > -INFINITY, "%s: bad argument: fix_sigma must be finite (0: from the data)", who);
    p.B = B, p.N = 2 * B, p.d = d, p.dp = 32 * wc_cdiv(d, 32);
    p.nt = wc_cdiv(p.N, MM_T);
    p.js = 1024 / p.nt < 1 ? 1 : (1024 / p.nt > p.nt ? p.nt : 1024 / p.nt);
    p.nchunk = wc_cdiv(p.dp, MM_DC);
    p.num = num, p.mul = mul, p.fix = fix, p.pow2 = mul == 2.0;
    return WC_OK;
}

// workspace carve-up, every piece rounded up to 256 bytes:
//   f64 column-sum slices 64 dp | f64 loss partials nt * js | f32 means 2 dp | f32 nrm N | f32 mrow N | f32 scal 17 | f32 Xc N dp
struct MWs {
    double *pm, *part;
    float *mean, *nrm, *mrow, *scal, *Xc;
    long bytes;
};

MWs mcarve(const MPlan& p, void* ws) {
    MWs w;
    char* b = (char*)ws;
    long o = 0;
    w.pm = (double*)(b + o), o += up256(8L * MM_RS * p.dp);
    w.part = (double*)(b + o), o += up256(8L * p.nt * p.js);
    w.mean = (float*)(b + o), o += up256(8L * p.dp);
    w.nrm = (float*)(b + o), o += up256(4L * p.N);
    w.mrow = (float*)(b + o), o += up256(4L * p.N);
    w.scal = (float*)(b + o), o += up256(4L * 17);
    w.Xc = (float*)(b + o), o += up256(4L * p.N * p.dp);
    w.bytes = o;
    return w;
}

template <bool HALF>
int mprep_t(const MPlan& p, const MWs& w, const void* src, const void* tgt, hipStream_t st) {
    hipLaunchKernelGGL(mmd_colsum_kernel<HALF>, dim3(wc_cdiv(p.dp, 64), MM_RS), dim3(256), 0, st, src, tgt, w.pm, p.B, p.d, p.dp);
    WC_LAUNCH_CHECK("mmd_colsum_kernel");
    hipLaunchKernelGGL(mmd_mean_kernel, dim3(wc_cdiv(p.dp, 256), 2), dim3(256), 0, st, w.pm, w.mean, p.B, p.dp);
    WC_LAUNCH_CHECK("mmd_mean_kernel");
    hipLaunchKernelGGL(mmd_centre_kernel<HALF>, dim3(wc_cdiv(p.N, 4)), dim3(256), 0, st, src, tgt, w.mean, w.Xc, w.nrm, w.mrow, p.B,
                       p.d, p.dp);
    WC_LAUNCH_CHECK("mmd_centre_kernel");
    hipLaunchKernelGGL(mmd_scal_kernel, dim3(1), dim3(256), 0, st, w.nrm, w.mean, w.scal, p.N, p.dp, p.num, p.mul, p.fix);
    WC_LAUNCH_CHECK("mmd_scal_kernel");
    return WC_OK;
}

int mprep(const MPlan& p, const MWs& w, const void* src, const void* tgt, int is_half, hipStream_t st) {
    return is_half ? mprep_t<true>(p, w, src, tgt, st) : mprep_t<false>(p, w, src, tgt, st);
}

MmdArgs margs(const MPlan& p, const MWs& w) {
    MmdArgs a = {};
    a.Xc = w.Xc, a.nrm = w.nrm, a.mrow = w.mrow, a.mean = w.mean, a.scal = w.scal;
    a.N = p.N, a.B = p.B, a.d = p.d, a.dp = p.dp, a.num = p.num, a.pow2 = p.pow2;
    a.gscale = (float)(-4.0 / ((double)p.B * p.B));
    return a;
}

}  // namespace

extern "C" int wc_mmd_workspace_bytes(int B, int d, long* n_bytes) {
    WC_CHECK_ARG(n_bytes, "wc_mmd_workspace_bytes: bad argument: null pointer");
    MPlan p;
    if (int rc = mplan(p, B, d, 1, 2.0, 0.0, "wc_mmd_workspace_bytes")) return rc;
    *n_bytes = mcarve(p, nullptr).bytes;
    return WC_OK;
}

extern "C" int wc_mmd_rbf(const void* source, const void* target, int is_half, float* loss, float* grad, void* ws, int B, int d,
                          int kernel_num, double kernel_mul, double fix_sigma, void* stream) {
    WC_CHECK_ARG(source && target && loss && ws, "wc_mmd_rbf: bad argument: null pointer");
    WC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "wc_mmd_rbf: bad argument: workspace not 256-byte aligned");
    MPlan p;
    if (int rc = mplan(p, B, d, kernel_num, kernel_mul, fix_sigma, "wc_mmd_rbf")) return rc;
    const MWs w = mcarve(p, ws);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = mprep(p, w, source, target, is_half, st)) return rc;
    MmdArgs a = margs(p, w);
    a.part = w.part, a.grad = grad;
    const double tile_s = 2.0 * MM_T * MM_T * p.dp;         // issued MFMA FLOPs of one tile's S
    const int idx = wc_prof_begin(st);
    long npart;
    if (grad) {
        hipLaunchKernelGGL(mmd_main_kernel<MM_CT>, dim3(p.nt, p.nchunk), dim3(256), 0, st, a);
        npart = p.nt;
        WC_LAUNCH_CHECK("mmd_main_kernel");
        wc_prof_end(idx, "mmd_main_kernel<grad>", (double)p.nchunk * p.nt * p.nt * (tile_s + 2.0 * MM_T * MM_T * MM_DC), st);
    } else {
        hipLaunchKernelGGL(mmd_main_kernel<0>, dim3(p.nt, p.js), dim3(256), 0, st, a);
        npart = (long)p.nt * p.js;
        WC_LAUNCH_CHECK("mmd_main_kernel");
        wc_prof_end(idx, "mmd_main_kernel<loss>", 0.5 * p.nt * (p.nt + 1.0) * tile_s, st);
    }
    hipLaunchKernelGGL(mmd_finish_kernel, dim3(1), dim3(256), 0, st, w.part, npart, 1.0 / ((double)p.B * p.B), loss);
    WC_LAUNCH_CHECK("mmd_finish_kernel");
    return WC_OK;
}

extern "C" int wc_mmd_rbf_kernel(const void* source, const void* target, int is_half, float* K, void* ws, int B, int d,
                                 int kernel_num, double kernel_mul, double fix_sigma, void* stream) {
    WC_CHECK_ARG(source && target && K && ws, "wc_mmd_rbf_kernel: bad argument: null pointer");
    WC_CHECK_ARG(((uintptr_t)ws & 255) == 0, "wc_mmd_rbf_kernel: bad argument: workspace not 256-byte aligned");
    MPlan p;
    if (int rc = mplan(p, B, d, kernel_num, kernel_mul, fix_sigma, "wc_mmd_rbf_kernel")) return rc;
    const MWs w = mcarve(p, ws);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = mprep(p, w, source, target, is_half, st)) return rc;
    MmdArgs a = margs(p, w);
    a.K = K;
    hipLaunchKernelGGL(mmd_matrix_kernel, dim3(p.nt, p.nt), dim3(256), 0, st, a);
    WC_LAUNCH_CHECK("mmd_matrix_kernel");
    return WC_OK;
}
