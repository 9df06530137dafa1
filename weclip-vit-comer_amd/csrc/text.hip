// CLIP text tower pieces for gfx950: token embedding, causal self-attention for short prompts, EOT pooling and the
// zero-shot classifier rows.  The block GEMMs and LayerNorms of the tower are the vision path's (gemm.hip, norm.hip).
//
// Replaces reference clip/model.py:392-403 (`CLIP.encode_text`: embedding, causal blocks, ln_final, EOT row @
// text_projection), clip/model.py:375-381 + clip/myAtt.py:57-58 (the -inf causal mask added to the scores) and
// WeCLIP_model/model_attn_aff_voc.py:34-46 (`zeroshot_classifier` after encode_text).
//
//   text_embed_kernel        : one workgroup per prompt: eot[n] = first argmax of the ids, a flag for ids outside [0, V)
//                              (they read row 0 instead: never out of bounds), rows x = token_embedding[id] + pos[l].
//   text_attn_causal_kernel  : one workgroup per prompt, heads looped; the whole (prompt, head) K and V^T sit in LDS
//                              (L <= 128, DH = 64).  Wave w owns queries [32w, 32w + 32) and computes S^T = K Q^T only for
//                              key tiles 0..w (the tiles right of the diagonal tile are all masked), masks the diagonal
//                              tile before the row maximum, then O^T = V^T P^T with the S^T accumulators as B operand
//                              (same fragment algebra as attention.hip).  The head-mean map is summed over the heads in
//                              registers and written once, zeros above the diagonal included.
//   text_pool_kernel         : one workgroup per prompt: row eot[n] of the last block, ln_final in fp32, @ text_projection.
//   text_zeroshot_kernel     : one workgroup per class: L2-normalise each of its T rows, average, renormalise.
//
// MFMA layouts (v_mfma_f32_32x32x16_f16): A[i=lane&31][k=8*(lane>>5)+j], B[k][j=lane&31],
// D col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define TXT_LMAX 128                 // longest causal sequence (4 waves x 32 queries)
#define TXT_DH 64
#define TXT_KROW (TXT_DH * 2 + 16)   // bytes per K row in LDS (16-B pad: rows l31 and l31 + 1 on different banks)
#define TXT_VTROW (TXT_LMAX + 8)     // halves per V^T row in LDS (272 B: 16-B aligned rows)
#define TXT_NEG_BIG (-1.0e30f)

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ tok, int Lctx,
                                                        const float* __restrict__ emb, int V,
                                                        const float* __restrict__ pos, int W, int L,
                                                        float* __restrict__ x, int* __restrict__ eot,
                                                        int* __restrict__ bad) {
    __shared__ int s_val[256], s_idx[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int* row = tok + (long)n * Lctx;
    int best = -2147483647 - 1, bi = 0x7fffffff, oob = 0;
    for (int l = tid; l < Lctx; l += 256) {
        const int id = row[l];
        if (id < 0 || id >= V) oob = 1;
        if (id > best) { best = id; bi = l; }          // ascending l per thread: keeps the first maximum
    }
    s_val[tid] = best;
    s_idx[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const int v2 = s_val[tid + s], i2 = s_idx[tid + s];
            if (v2 > s_val[tid] || (v2 == s_val[tid] && i2 < s_idx[tid])) { s_val[tid] = v2; s_idx[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid == 0) eot[n] = s_idx[0];
    if (oob) *bad = 1;
    if (x == nullptr) return;
    for (long i = tid; i < (long)L * W; i += 256) {
        const int l = (int)(i / W), c = (int)(i - (long)l * W);
        int id = row[l];
        if (id < 0 || id >= V) id = 0;                 // flagged above; the host raises
        x[((long)n * L + l) * W + c] = emb[(long)id * W + c] + pos[(long)l * W + c];
    }
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void text_attn_causal_kernel(const __half* __restrict__ qkv, __half* __restrict__ out,
                                                              float* __restrict__ out32, float* __restrict__ lse,
                                                              float* __restrict__ mean, int L, int H, int E) {
    __shared__ __attribute__((aligned(16))) char kbuf[TXT_LMAX * TXT_KROW];     // K [key][dh], 18 KiB
    __shared__ __attribute__((aligned(16))) _Float16 vt[TXT_DH * TXT_VTROW];     // V^T [dh][key], 17 KiB
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int hh = lane >> 5, l31 = lane & 31;
    const int nkt = (L + 31) >> 5, Lp = nkt * 32;
    const bool active = w < nkt;                      // wave-uniform
    const long ldq = 3L * E;
    const __half* base = qkv + (long)n * L * ldq;
    const int q = 32 * w + l31;
    const int qr = q < L ? q : L - 1;

    f32x16 macc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[kt][r] = 0.f;

    for (int h = 0; h < H; ++h) {
        // stage K and V^T of head h; rows L .. Lp-1 are zero so masked products stay finite
        for (int c = tid; c < Lp * 8; c += 256) {
            const int key = c >> 3, ch = c & 7;
            u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
            if (key < L) {
                const __half* kr = base + (long)key * ldq + E + (long)h * TXT_DH + ch * 8;
                kv = *reinterpret_cast<const u32x4*>(kr);
                vv = *reinterpret_cast<const u32x4*>(kr + E);
            }
            *reinterpret_cast<u32x4*>(kbuf + key * TXT_KROW + ch * 16) = kv;
            const f16x8 v8 = __builtin_bit_cast(f16x8, vv);
#pragma unroll
            for (int j = 0; j < 8; ++j) vt[(ch * 8 + j) * TXT_VTROW + key] = v8[j];
        }
        __syncthreads();
        if (active) {
            f16x8 qf[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                qf[ks] = *reinterpret_cast<const f16x8*>(base + (long)qr * ldq + (long)h * TXT_DH + 16 * ks + 8 * hh);
            f32x16 s[4];
            float m = TXT_NEG_BIG;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                if (kt > w) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const f16x8 a = *reinterpret_cast<const f16x8*>(kbuf + (32 * kt + l31) * TXT_KROW + ks * 32 + hh * 16);
                    s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[ks], s[kt], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    if (key > q || key >= L) s[kt][r] = TXT_NEG_BIG;       // causal mask, before the maximum
                    m = fmaxf(m, s[kt][r]);
                }
            }
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float lsum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                if (kt > w) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(s[kt][r] - m);    // masked: exactly 0
                    s[kt][r] = p;
                    lsum += p;
                }
            }
            lsum += __shfl_xor(lsum, 32, 64);
            const float inv = 1.0f / lsum;
            f32x16 o[2];
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                if (kt > w) break;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    // B = P^T: element j of lane half hh is key 32 kt + 16 s2 + 8 (j >> 2) + 4 hh + (j & 3)
                    f16x8 pb;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pb[j] = (_Float16)s[kt][s2 * 8 + j];
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        // A = V^T: dh row 32 d + l31, the same keys as pb's elements
                        const _Float16* vr = vt + (32 * d + l31) * TXT_VTROW + 32 * kt + 16 * s2 + 4 * hh;
                        const f16x4 v0 = *reinterpret_cast<const f16x4*>(vr);
                        const f16x4 v1 = *reinterpret_cast<const f16x4*>(vr + 8);
                        const f16x8 va = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                        o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb, o[d], 0, 0, 0);
                    }
                }
            }
            if (mean) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    if (kt > w) break;
#pragma unroll
                    for (int r = 0; r < 16; ++r) macc[kt][r] += s[kt][r] * inv;
                }
            }
            if (q < L) {
                const long oi = ((long)n * L + q) * E + (long)h * TXT_DH;
#pragma unroll
                for (int d = 0; d < 2; ++d)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        // o[d][4g + k] is dh 32 d + 8 g + 4 hh + k of query q
                        __half hv[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) hv[k] = __float2half(o[d][g * 4 + k] * inv);
                        *reinterpret_cast<uint2*>(out + oi + d * 32 + 8 * g + 4 * hh) = *reinterpret_cast<uint2*>(hv);
                        if (out32)
                            *reinterpret_cast<float4*>(out32 + oi + d * 32 + 8 * g + 4 * hh) =
                                make_float4(o[d][g * 4] * inv, o[d][g * 4 + 1] * inv, o[d][g * 4 + 2] * inv, o[d][g * 4 + 3] * inv);
                    }
                if (lse && hh == 0) lse[((long)n * H + h) * L + q] = m + log2f(lsum);
            }
        }
        __syncthreads();          // K / V^T of the next head overwrite the buffers
    }
    if (mean && active && q < L) {
        const float invh = 1.0f / H;
        float* mrow = mean + ((long)n * L + q) * L;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (kt >= nkt) break;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (key < L) mrow[key] = kt <= w ? macc[kt][r] * invh : 0.f;     // tiles right of the diagonal: zero
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// lds: W floats (the normalised row) + 16 reduction slots
__global__ __launch_bounds__(256) void text_pool_kernel(const float* __restrict__ x, const int* __restrict__ eot, int L, int W,
                                                       const float* __restrict__ lnw, const float* __restrict__ lnb, float eps,
                                                       const float* __restrict__ proj, int Ed, float* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* y = sm;
    float* red = sm + W;
    const int n = blockIdx.x, tid = threadIdx.x;
    int e = eot[n];
    e = e < 0 ? 0 : (e >= L ? L - 1 : e);
    const float* row = x + ((long)n * L + e) * W;
    float s = 0.f;
    for (int c = tid; c < W; c += 256) {
        const float v = row[c];
        y[c] = v;
        s += v;
    }
    const float mu = block_sum(s, red) / W;
    float s2 = 0.f;
    for (int c = tid; c < W; c += 256) {
        const float d = y[c] - mu;
        s2 += d * d;
    }
    const float rstd = rsqrtf(block_sum(s2, red) / W + eps);
    for (int c = tid; c < W; c += 256) y[c] = (y[c] - mu) * rstd * lnw[c] + lnb[c];
    __syncthreads();
    for (int j = tid; j < Ed; j += 256) {
        float acc = 0.f;
        for (int c = 0; c < W; ++c) acc = fmaf(y[c], proj[(long)c * Ed + j], acc);
        feat[(long)n * Ed + j] = acc;
    }
}

// lds: Ed floats (the running class sum) + 16 reduction slots
__global__ __launch_bounds__(256) void text_zeroshot_kernel(const float* __restrict__ feat, int T, int Ed, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* acc = sm;
    float* red = sm + Ed;
    const int c = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < Ed; j += 256) acc[j] = 0.f;
    for (int t = 0; t < T; ++t) {
        const float* f = feat + ((long)c * T + t) * Ed;
        float s = 0.f;
        for (int j = tid; j < Ed; j += 256) s = fmaf(f[j], f[j], s);
        const float nrm = sqrtf(block_sum(s, red));
        for (int j = tid; j < Ed; j += 256) acc[j] += f[j] / nrm;       // each thread owns its j: no barrier needed
    }
    float s = 0.f;
    for (int j = tid; j < Ed; j += 256) {
        acc[j] /= T;
        s = fmaf(acc[j], acc[j], s);
    }
    const float nrm = sqrtf(block_sum(s, red));
    for (int j = tid; j < Ed; j += 256) out[(long)c * Ed + j] = acc[j] / nrm;
}

// ------------------------------------------------------------------------------------------------
extern "C" int wc_text_embed(const int* tokens, int N, int Lctx, const float* tok_emb, int V, const float* pos, int W, int L,
                             float* x, int* eot, int* bad, void* stream) {
    WC_CHECK_ARG(tokens && tok_emb && pos && eot && bad && N > 0 && N <= 65535 && Lctx > 0 && V > 0 && W > 0,
                 "wc_text_embed: bad argument");
    WC_CHECK_ARG(x ? (L > 0 && L <= Lctx) : L == 0, "wc_text_embed: need 0 < L <= Lctx with x, L == 0 without (got L=%d)", L);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) {
        wc_set_error("wc_text_embed: hipMemsetAsync failed");
        return WC_ERR_HIP;
    }
    hipLaunchKernelGGL(text_embed_kernel, dim3(N), dim3(256), 0, st, tokens, Lctx, tok_emb, V, pos, W, L, x, eot, bad);
    WC_LAUNCH_CHECK("text_embed_kernel");
    return WC_OK;
}

extern "C" int wc_attn_fwd_causal(const void* qkv, void* out, float* out32, float* lse, float* mean, int N, int L, int H,
                                  int DH, void* stream) {
    WC_CHECK_ARG(qkv && out && N > 0 && N <= 65535 && H > 0 && H <= 4096, "wc_attn_fwd_causal: bad argument");
    WC_CHECK_ARG(L >= 1 && L <= TXT_LMAX, "wc_attn_fwd_causal: need 1 <= L <= %d (got %d)", TXT_LMAX, L);
    WC_CHECK_ARG(DH == TXT_DH, "wc_attn_fwd_causal: head dim must be 64 (got %d)", DH);
    WC_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)out32) % 16 == 0,
                 "wc_attn_fwd_causal: operands must be 16-byte aligned");
    const int E = H * DH;
    hipStream_t st = (hipStream_t)stream;
    const int pr = wc_prof_begin(stream);
    hipLaunchKernelGGL(text_attn_causal_kernel, dim3(N), dim3(256), 0, st, (const __half*)qkv, (__half*)out, out32, lse, mean,
                       L, H, E);
    wc_prof_end(pr, "text_attn_causal_kernel", 2.0 * N * H * (double)L * (L + 1) * DH, stream);
    WC_LAUNCH_CHECK("text_attn_causal_kernel");
    return WC_OK;
}

extern "C" int wc_text_pool(const float* x, const int* eot, int N, int L, int W, const float* ln_w, const float* ln_b, float eps,
                            const float* proj, int Ed, float* feat, void* stream) {
    WC_CHECK_ARG(x && eot && ln_w && ln_b && proj && feat && N > 0 && N <= 65535 && L > 0 && Ed > 0,
                 "wc_text_pool: bad argument");
    WC_CHECK_ARG(W > 0 && W <= 8192, "wc_text_pool: need 0 < W <= 8192 (got %d)", W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(text_pool_kernel, dim3(N), dim3(256), (W + 16) * sizeof(float), st, x, eot, L, W, ln_w, ln_b, eps, proj,
                       Ed, feat);
    WC_LAUNCH_CHECK("text_pool_kernel");
    return WC_OK;
}

extern "C" int wc_text_zeroshot(const float* feat, int C, int T, int Ed, float* out, void* stream) {
    WC_CHECK_ARG(feat && out && C > 0 && C <= 65535 && T > 0, "wc_text_zeroshot: bad argument");
    WC_CHECK_ARG(Ed > 0 && Ed <= 8192, "wc_text_zeroshot: need 0 < Ed <= 8192 (got %d)", Ed);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(text_zeroshot_kernel, dim3(C), dim3(256), (Ed + 16) * sizeof(float), st, feat, T, Ed, out);
    WC_LAUNCH_CHECK("text_zeroshot_kernel");
    return WC_OK;
}
