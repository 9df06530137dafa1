// Losses of the training steps.
// Soft-max cross-entropy of the bilinearly up-sampled logits, with its gradient pulled back to the low-resolution map:
// reference scripts/dist_clip_voc.py:250 (F.interpolate(segs, size=(H,W), bilinear, align_corners=False)) followed by
//   get_seg_loss :105-113:  0.5 * (CE(pred, label with fg->ignore) + CE(pred, label with bg->ignore)), each CE a mean over
//                           its non-ignored pixels (the weakly supervised step), or
//   F.cross_entropy(pred, label, ignore_index)  (the supervised variant's step).
// The reference materialises the (B, nc, H, W) up-sampled logits (352 MB at 16x21x512x512) for log_softmax forward and
// backward; here every high-res pixel interpolates its nc logits from the low-res map on the fly.
//   seg_loss_kernel              : forward only (no gradient requested): per pixel nll, block sums of
//                                  (nll_bg, n_bg, nll_fg, n_fg) -> seg_loss_reduce_kernel                 wc_seg_loss_fwd
//   ce_loss_fused_kernel<CH, MULTI, TWO_TERM> : TRAINING: loss and gradient in one pixel pass, 1..128 classes in register
//                                  chunks of CH, + seg_bwd_x2_kernel (X pass of the separable bilinear backward)
//       TWO_TERM = true          : get_seg_loss weighting; seg_count_kernel first, seg_loss_reduce_kernel  wc_seg_loss_fwd_bwd
//       TWO_TERM = false         : plain cross-entropy; ce_loss_reduce_kernel, X pass scaled by 1/N_valid wc_ce_loss_fwd_bwd
// and the affinity loss fused with the affinity-label construction (aff_loss_kernel, wc_aff_loss_fwd / wc_aff_loss_bwd).
#include "common.h"
#include "resample.h"

#define LOSS_MAX_C 128   // class limit of every entry of this file

__global__ __launch_bounds__(256) void seg_loss_kernel(const float* __restrict__ seg, const long* __restrict__ label,
                                                        float* __restrict__ part, int nc, int h, int w, int H, int W,
                                                        float sy, float sx, int ignore) {
    __shared__ float red[16];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    float nll = 0.f;
    int cls = -1;   // -1: outside / ignored, 0: background pixel, 1: foreground pixel
    if (x < W && y < H) {
        const long lab = label[((long)b * H + y) * W + x];
        int y0, y1, x0, x1;
        float ly, lx;
        wc_bil_src(y, h, sy, y0, y1, ly);
        wc_bil_src(x, w, sx, x0, x1, lx);
        const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
        const float* S = seg + (long)b * nc * h * w;
        const long o00 = (long)y0 * w + x0, o01 = (long)y0 * w + x1, o10 = (long)y1 * w + x0, o11 = (long)y1 * w + x1;
        float mx = -INFINITY, sum = 0.f, zl = 0.f;
        for (int c = 0; c < nc; ++c) {
            const float* Sc = S + (long)c * h * w;
            const float z = w00 * Sc[o00] + w01 * Sc[o01] + w10 * Sc[o10] + w11 * Sc[o11];
            if (c == lab) zl = z;
            const float nm = fmaxf(mx, z);
            sum = sum * __expf(mx - nm) + __expf(z - nm);
            mx = nm;
        }
        if (lab != ignore && lab >= 0 && lab < nc) {
            cls = lab == 0 ? 0 : 1;
            nll = mx + __logf(sum) - zl;
        }
    }
    const float a0 = block_sum(cls == 0 ? nll : 0.f, red), a1 = block_sum(cls == 0 ? 1.f : 0.f, red);
    const float a2 = block_sum(cls == 1 ? nll : 0.f, red), a3 = block_sum(cls == 1 ? 1.f : 0.f, red);
    if (threadIdx.x == 0) {
        const long blk = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[blk * 4] = a0; part[blk * 4 + 1] = a1; part[blk * 4 + 2] = a2; part[blk * 4 + 3] = a3;
    }
}

// sums[k] = sum over blocks of part[blk*4 + k]  (deterministic second stage), then the scalar tail of the loss so
// that no elementwise torch launches follow: sums[4] = the loss, sums[5..6] = d loss / d (per-pixel term) for the two
// classes of terms (the backward kernels' weights for an upstream gradient of 1).
//   mode 0 (segmentation, get_seg_loss):  0.5 * (s0 / s1 + s2 / s3);                 0.5 / s1,  0.5 / s3
//   mode 1 (affinity, get_aff_loss):      0.5 * s0 / (s1 + 1) + 0.5 * s2 / (s3 + 1); -0.5 / (s1 + 1), 0.5 / (s3 + 1)
__global__ __launch_bounds__(1024) void seg_loss_reduce_kernel(const float* __restrict__ part, float* __restrict__ sums, long nblk,
                                                               int mode) {
    __shared__ float red[16];
    __shared__ float tot[4];
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (long i = threadIdx.x; i < nblk; i += 1024) {          // one 16-byte load per partial block
        const float4 v = *reinterpret_cast<const float4*>(part + i * 4);
        s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
    }
    for (int k = 0; k < 4; ++k) {
        const float t = block_sum(s[k], red);
        if (threadIdx.x == 0) { sums[k] = t; tot[k] = t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (mode == 0) {
            sums[4] = 0.5f * (tot[0] / tot[1] + tot[2] / tot[3]);
            sums[5] = 0.5f / tot[1];
            sums[6] = 0.5f / tot[3];
        } else {
            sums[4] = 0.5f * tot[0] / (tot[1] + 1.0f) + 0.5f * tot[2] / (tot[3] + 1.0f);
            sums[5] = -0.5f / (tot[1] + 1.0f);
            sums[6] = 0.5f / (tot[3] + 1.0f);
        }
        sums[7] = 0.f;
    }
}

extern "C" int wc_seg_loss_fwd(const float* seg, const int64_t* label, float* part, float* sums, int B, int nc, int h,
                               int w, int H, int W, int ignore, void* stream) {
    WC_CHECK_ARG(seg && label && part && sums && B > 0 && nc > 0 && nc <= LOSS_MAX_C && h > 0 && w > 0 && H >= h && W >= w,
                 "wc_seg_loss_fwd: bad argument");
    dim3 grid(wc_cdiv(W, 64), wc_cdiv(H, 4), B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg_loss_kernel, grid, dim3(256), 0, st, seg, (const long*)label, part, nc, h, w, H, W, (float)h / H,
                       (float)w / W, ignore);
    WC_LAUNCH_CHECK("seg_loss_kernel");
    hipLaunchKernelGGL(seg_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, part, sums, (long)grid.x * grid.y * grid.z, 0);
    WC_LAUNCH_CHECK("seg_loss_reduce_kernel");
    return WC_OK;
}

// ---------------------------------------------------------------------------------------------
// Training form: loss AND its gradient in one pass over the pixels (the soft-max of a pixel is formed once; separate
// forward + gradient passes form it three times: once for the loss and once for each of the two low-resolution rows a
// pixel contributes to), without the (B, nc, H, W) high-resolution gradient: bilinear interpolation is separable.
// Thread (x, ys): the pixels of column x whose upper source row is ys.  Their logits are a_c + ly * (b_c - a_c) with
// a_c, b_c = the x-interpolated logits of rows ys, ys + 1 (registers); their gradient goes to row ys with weight 1 - ly
// (tmpA) and to row ys + 1 with ly (tmpB); the X pass adds the two in a fixed order.  H and W are free (down-sampling too:
// a thread with no rows writes zeros).  Up to LOSS_MAX_C classes in chunks of CH per workgroup (blockIdx.z = image * nchunk
// + chunk).  MULTI (nc > CH): the pixel's log-sum-exp runs over all classes from memory, CE_LSE_G classes' loads at a time;
// the chunk's own logits stay in registers for the gradient.  Only chunk 0 contributes to the block partials.
// A label outside [0, nc) that is not `ignore` is treated as ignored; it is compared, never used as an index.
//   TWO_TERM = false (F.cross_entropy): every valid pixel weighs 1 (the 1 / N_valid is applied by the X pass from a device
//     scalar, so no count pass runs first).  Block partials: (sum nll, n_valid, n_bad, 0), n_bad = the out-of-range labels.
//   TWO_TERM = true (get_seg_loss): a valid pixel weighs 0.5 / n_bg or 0.5 / n_fg by its label.  The gradient needs these
//     before the pass: a label count runs first (SEG_CNT_BLOCKS block partials, summed in a fixed order by every workgroup
//     of the main pass).  Block partials: (nll_bg, n_bg, nll_fg, n_fg), as seg_loss_kernel's.
#define SEG_CNT_BLOCKS 1024
#define SEG_CNT_BLOCKS 1024
__global__ __launch_bounds__(256) void seg_count_kernel(const long* __restrict__ label, float* __restrict__ cnt, long n, int nc,
                                                         int ignore) {
    __shared__ float red[16];
    float nb = 0.f, nf = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long lab = label[i];
        const bool valid = lab != ignore && lab >= 0 && lab < nc;
        nb += (valid && lab == 0) ? 1.f : 0.f;
        nf += (valid && lab != 0) ? 1.f : 0.f;
    }
    const float a = block_sum(nb, red), b = block_sum(nf, red);      // integers < 2^24: exact
    if (threadIdx.x == 0) { cnt[2 * blockIdx.x] = a; cnt[2 * blockIdx.x + 1] = b; }
}

#define CE_LSE_G 4       // classes whose logits the MULTI log-sum-exp requests together (8: the register file overflows, loads serialise)
template <int CH, bool MULTI, bool TWO_TERM>
__global__ __launch_bounds__(256) void ce_loss_fused_kernel(const float* __restrict__ seg, const long* __restrict__ label,
                                                             const float* __restrict__ cnt, float* __restrict__ part,
                                                             float* __restrict__ tmpA, float* __restrict__ tmpB, int nc,
                                                             int nchunk, int h, int w, int H, int W, float sy, float sx,
                                                             int ignore) {
    __shared__ float red[16];
    float wbg = 1.f, wfg = 1.f;
    if constexpr (TWO_TERM) {
        float pb = 0.f, pf = 0.f;
        for (int i = threadIdx.x; i < SEG_CNT_BLOCKS; i += 256) { pb += cnt[2 * i]; pf += cnt[2 * i + 1]; }
        const float nbg = block_sum(pb, red), nfg = block_sum(pf, red);
        wbg = nbg > 0.f ? 0.5f / nbg : 0.f;
        wfg = nfg > 0.f ? 0.5f / nfg : 0.f;
    }
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), ys = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.z / nchunk, ck = blockIdx.z - b * nchunk, c0 = ck * CH;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;     // this thread's share of the block partials
    if (x < W && ys < h) {
        int x0, x1;
        float lx;
        wc_bil_src(x, w, sx, x0, x1, lx);
        const int y1s = ys + (ys < h - 1 ? 1 : 0);
        const float* S = seg + (long)b * nc * h * w;
        const long r0 = (long)ys * w, r1 = (long)y1s * w;
        float av[CH], dv[CH], accT[CH], accB[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            accT[c] = accB[c] = 0.f;
            // clamped class: no branch around the loads (behind an `if (c < nc)` hipcc waited for the four loads of a class
            // before issuing the next class's -- CH dependent latencies at the head of every thread)
            const float* Sc = S + (long)min(c0 + c, nc - 1) * h * w;
            const float a = (1.f - lx) * Sc[r0 + x0] + lx * Sc[r0 + x1];
            const float bb = (1.f - lx) * Sc[r1 + x0] + lx * Sc[r1 + x1];
            av[c] = a;
            dv[c] = bb - a;
        }
        const float iy = 1.0f / sy;
        int y_lo = ys == 0 ? 0 : (int)floorf((ys + 0.5f) * iy - 0.5f) - 1;
        int y_hi = ys == h - 1 ? H - 1 : (int)ceilf((ys + 1.5f) * iy - 0.5f) + 1;
        if (y_lo < 0) y_lo = 0;
        if (y_hi > H - 1) y_hi = H - 1;
        long labs[8];
        for (int y = y_lo; y <= y_hi; ++y) {
            if (((y - y_lo) & 7) == 0) {               // the labels of the next 8 rows: 8 independent loads in flight
#pragma unroll
                for (int u = 0; u < 8; ++u) labs[u] = label[((long)b * H + min(y + u, H - 1)) * W + x];
            }
            int y0, y1;
            float ly;
            wc_bil_src(y, h, sy, y0, y1, ly);
            long lab = labs[0];
#pragma unroll
            for (int u = 1; u < 8; ++u) lab = ((y - y_lo) & 7) == u ? labs[u] : lab;
            if (y0 != ys) continue;                      // wave-uniform
            float zc[CH];
            float mx = -INFINITY, sum = 0.f, zl = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) zc[c] = c0 + c < nc ? fmaf(ly, dv[c], av[c]) : -INFINITY;
            if constexpr (!MULTI) {
                // maximum first, then independent exponentials (an online form's max -> rescale -> add chain is serial over
                // the classes)
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    mx = fmaxf(mx, zc[c]);
                    zl = c == lab ? zc[c] : zl;
                }
            } else {
                // online log-sum-exp over all nc classes, CE_LSE_G at a time (loads from clamped class indices, issued together)
                for (int cb = 0; cb < nc; cb += CE_LSE_G) {
                    float zz[CE_LSE_G];
#pragma unroll
                    for (int u = 0; u < CE_LSE_G; ++u) {
                        const float* Sc = S + (long)min(cb + u, nc - 1) * h * w;
                        const float a = (1.f - lx) * Sc[r0 + x0] + lx * Sc[r0 + x1];
                        const float bb = (1.f - lx) * Sc[r1 + x0] + lx * Sc[r1 + x1];
                        zz[u] = cb + u < nc ? fmaf(ly, bb - a, a) : -INFINITY;
                    }
                    float m8 = mx;
#pragma unroll
                    for (int u = 0; u < CE_LSE_G; ++u) {
                        m8 = fmaxf(m8, zz[u]);
                        zl = cb + u == lab ? zz[u] : zl;
                    }
                    float s8 = 0.f;
#pragma unroll
                    for (int u = 0; u < CE_LSE_G; ++u) s8 += __expf(zz[u] - m8);
                    sum = sum * __expf(mx - m8) + s8;
                    mx = m8;
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                zc[c] = __expf(zc[c] - mx);                // class past nc: exp(-inf) = 0
                if constexpr (!MULTI) sum += zc[c];
            }
            const bool valid = lab != ignore && lab >= 0 && lab < nc;
            if (ck == 0) {
                const float nll = mx + __logf(sum) - zl;
                if constexpr (TWO_TERM) {
                    if (valid && lab == 0) { p0 += nll; p1 += 1.f; }
                    if (valid && lab != 0) { p2 += nll; p3 += 1.f; }
                } else {
                    p0 += valid ? nll : 0.f;
                    p1 += valid ? 1.f : 0.f;
                    p2 += (!valid && lab != ignore) ? 1.f : 0.f;
                }
            }
            const float wp = valid ? (TWO_TERM ? (lab == 0 ? wbg : wfg) : 1.f) : 0.f;
            const float u = wp / sum;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const float gval = fmaf(u, zc[c], c0 + c == lab ? -wp : 0.f);   // wp * (softmax_c - [c == label])
                accT[c] += gval;
                accB[c] = fmaf(ly, gval, accB[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (c0 + c < nc) {
                const long o = (((long)b * nc + c0 + c) * h) * W + x;
                if (y1s == ys) tmpA[o + (long)ys * W] = accT[c];               // last row: both weights land on it
                else {
                    tmpA[o + (long)ys * W] = accT[c] - accB[c];
                    tmpB[o + (long)y1s * W] = accB[c];
                }
            }
    }
    const float a0 = block_sum(p0, red), a1 = block_sum(p1, red), a2 = block_sum(p2, red);
    const float a3 = TWO_TERM ? block_sum(p3, red) : 0.f;
    if (threadIdx.x == 0) {
        const long blk = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        *reinterpret_cast<float4*>(part + blk * 4) = make_float4(a0, a1, a2, a3);
    }
}

// X pass over tmpA (+ tmpB for rows > 0: row 0 receives nothing from above).  One wave per (image, class, row): the Wd
// values are read coalesced and parked in LDS (index x + x/16: the 32 output lanes then read their windows, 16 apart, from
// different banks); each output lane sums its window in ascending x, the order of the per-thread form (which read global
// memory at a 64-byte lane stride: 51 us for 22 MB).
// SCALED (wc_ce_loss_fwd_bwd): every output is multiplied by the device scalar scale[0] (1 / N_valid, known only after the
// pixel pass), so the per-pixel gradient is accumulated unscaled and no host synchronisation is needed.
template <bool SCALED>
__global__ __launch_bounds__(256) void seg_bwd_x2_kernel(const float* __restrict__ tmpA, const float* __restrict__ tmpB,
                                                          float* __restrict__ gsrc, long rows, int Hs, int Ws, int Wd, float sx,
                                                          const float* __restrict__ scale) {
    extern __shared__ float xrow[];                       // 4 waves x (Wd + Wd/16 + 1)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;         // (image * nc + class) * Hs + ys
    if (row >= rows) return;                              // wave-uniform; no block-wide barrier below
    const int ys = (int)(row % Hs);
    float* v = xrow + wave * (Wd + (Wd >> 4) + 1);
    const float* TA = tmpA + row * Wd;
    const float* TB = tmpB + row * Wd;
    for (int x = lane; x < Wd; x += 64) v[x + (x >> 4)] = ys > 0 ? TA[x] + TB[x] : TA[x];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the LDS writes of this wave are done before its lanes read them
    __builtin_amdgcn_wave_barrier();
    const float ix = 1.0f / sx;
    const float sc = SCALED ? scale[0] : 1.f;
    for (int xs = lane; xs < Ws; xs += 64) {
        int x_lo = (int)floorf((xs - 1.5f) * ix) - 1, x_hi = (int)ceilf((xs + 1.5f) * ix) + 1;
        if (x_lo < 0) x_lo = 0;
        if (x_hi > Wd - 1) x_hi = Wd - 1;
        float acc = 0.f;
        for (int x = x_lo; x <= x_hi; ++x) {
            int x0, x1;
            float lx;
            wc_bil_src(x, Ws, sx, x0, x1, lx);
            const float wx = (x0 == xs ? 1.f - lx : 0.f) + (x1 == xs ? lx : 0.f);
            acc = fmaf(wx, v[x + (x >> 4)], acc);
        }
        gsrc[row * Ws + xs] = SCALED ? acc * sc : acc;
    }
}

// sums = [loss = s0 / s1 (NaN when no pixel is valid, as F.cross_entropy), 1 / s1 (0 when s1 == 0: the gradient is then 0,
// as torch's), n_valid, n_bad]: block partials in a fixed order, accumulated in double.
__global__ __launch_bounds__(1024) void ce_loss_reduce_kernel(const float* __restrict__ part, float* __restrict__ sums, long nblk) {
    __shared__ double red[3][1024];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long i = threadIdx.x; i < nblk; i += 1024) {
        const float4 v = *reinterpret_cast<const float4*>(part + i * 4);
        s0 += v.x; s1 += v.y; s2 += v.z;
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if (threadIdx.x < k) {
            red[0][threadIdx.x] += red[0][threadIdx.x + k];
            red[1][threadIdx.x] += red[1][threadIdx.x + k];
            red[2][threadIdx.x] += red[2][threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double nll = red[0][0], n = red[1][0];
        sums[0] = (float)(nll / n);
        sums[1] = n > 0.0 ? (float)(1.0 / n) : 0.f;
        sums[2] = (float)n;
        sums[3] = (float)red[2][0];
    }
}

// The unscaled X pass alone (resample.h), for a pixel pass of another file that leaves the same tmpA / tmpB rows
// (csrc/energy_prep.hip): rows = (images * classes) * h.
int wc_bilinear_bwd_x(const float* tmpA, const float* tmpB, float* grad, long rows, int h, int w, int W, void* stream) {
    hipLaunchKernelGGL(seg_bwd_x2_kernel<false>, dim3((unsigned)wc_cdiv(rows, 4)), dim3(256), 4 * (W + (W >> 4) + 1) * sizeof(float),
                       (hipStream_t)stream, tmpA, tmpB, grad, rows, h, w, W, (float)w / W, nullptr);
    WC_LAUNCH_CHECK("seg_bwd_x2_kernel");
    return WC_OK;
}

// Both training entries: [label count,] pixel pass, one-block reduce, X pass.
template <bool TWO_TERM>
static int up_ce_fwd_bwd(const char* who, const float* seg, const int64_t* label, float* cnt, float* part, float* sums,
                         float* tmp, float* grad, int B, int nc, int h, int w, int H, int W, int ignore, void* stream) {
    WC_CHECK_ARG(seg && label && (cnt || !TWO_TERM) && part && sums && tmp && grad, "%s: null pointer", who);
    WC_CHECK_ARG(B > 0 && nc >= 1 && nc <= LOSS_MAX_C && h > 0 && w > 0 && H > 0 && W > 0 && W <= 8192,
                 "%s: bad size (1 <= nc <= 128, W <= 8192)", who);
    const int nchunk = nc <= 32 ? 1 : (nc + 31) / 32;
    WC_CHECK_ARG((long)B * nchunk <= 65535 && (long)B * nc * h * W < (1L << 40), "%s: batch too large", who);
    WC_CHECK_ARG((uintptr_t)part % 16 == 0 && ((uintptr_t)seg | (uintptr_t)cnt | (uintptr_t)sums | (uintptr_t)tmp | (uintptr_t)grad) % 4 == 0 &&
                 (uintptr_t)label % 8 == 0, "%s: misaligned pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (TWO_TERM) {
        hipLaunchKernelGGL(seg_count_kernel, dim3(SEG_CNT_BLOCKS), dim3(256), 0, st, (const long*)label, cnt, (long)B * H * W, nc,
                           ignore);
        WC_LAUNCH_CHECK("seg_count_kernel");
    }
    dim3 grid(wc_cdiv(W, 64), wc_cdiv(h, 4), B * nchunk);
    float* tmpB = tmp + (long)B * nc * h * W;
    const float sy = (float)h / H, sx = (float)w / W;
    const auto pass = nc <= 24 ? ce_loss_fused_kernel<24, false, TWO_TERM>
                    : nc <= 32 ? ce_loss_fused_kernel<32, false, TWO_TERM> : ce_loss_fused_kernel<32, true, TWO_TERM>;
    hipLaunchKernelGGL(pass, grid, dim3(256), 0, st, seg, (const long*)label, cnt, part, tmp, tmpB, nc, nchunk, h, w, H, W, sy, sx,
                       ignore);
    WC_LAUNCH_CHECK("ce_loss_fused_kernel");
    const long nblk = (long)grid.x * grid.y * grid.z;
    if (TWO_TERM) hipLaunchKernelGGL(seg_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, part, sums, nblk, 0);
    else hipLaunchKernelGGL(ce_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, part, sums, nblk);
    WC_LAUNCH_CHECK("loss reduce kernel");
    const long rows = (long)B * nc * h;
    // two-term: the pixel weights are final before the pass; cross-entropy: 1 / N_valid = sums[1] after it
    hipLaunchKernelGGL(seg_bwd_x2_kernel<!TWO_TERM>, dim3((unsigned)wc_cdiv(rows, 4)), dim3(256), 4 * (W + (W >> 4) + 1) * sizeof(float),
                       st, tmp, tmpB, grad, rows, h, w, W, sx, TWO_TERM ? nullptr : sums + 1);
    WC_LAUNCH_CHECK("seg_bwd_x2_kernel");
    return WC_OK;
}

// get_seg_loss: sums (8) as wc_seg_loss_fwd and d loss / d seg for an upstream gradient of 1 (grad, (B,nc,h,w)).
// cnt: 2 * SEG_CNT_BLOCKS floats; part, tmp: as wc_ce_loss_fwd_bwd.
extern "C" int wc_seg_loss_fwd_bwd(const float* seg, const int64_t* label, float* cnt, float* part, float* sums, float* tmp,
                                   float* grad, int B, int nc, int h, int w, int H, int W, int ignore, void* stream) {
    return up_ce_fwd_bwd<true>("wc_seg_loss_fwd_bwd", seg, label, cnt, part, sums, tmp, grad, B, nc, h, w, H, W, ignore, stream);
}

// F.cross_entropy(F.interpolate(seg, (H, W), bilinear, align_corners=False), label, ignore_index=ignore), the supervised
// WeCLIP variant's loss (WeCLIP_model/model_attn_aff_voc_seg.py in this package): sums (4) from ce_loss_reduce_kernel.
// part: 4 floats per workgroup of the pixel pass; tmp: 2 * B*nc*h*W floats.
extern "C" int wc_ce_loss_fwd_bwd(const float* seg, const int64_t* label, float* part, float* sums, float* tmp, float* grad, int B,
                                  int nc, int h, int w, int H, int W, int ignore, void* stream) {
    return up_ce_fwd_bwd<false>("wc_ce_loss_fwd_bwd", seg, label, nullptr, part, sums, tmp, grad, B, nc, h, w, H, W, ignore, stream);
}

// ---------------------------------------------------------------------------------------------
// Affinity loss of the training step, fused with the label -> affinity-label construction.
// reference utils/camutils.py:226-247 (cams_to_affinity_label: nearest down-sampling of the pseudo labels by 16,
// pairwise equality, ignore where either token is ignored or the pair is outside the radius mask of
// scripts/dist_clip_voc.py:116-133) + utils/losses.py:11-22 (get_aff_loss):
//   loss = 0.5 * sum_pos(1 - p) / (n_pos + 1) + 0.5 * sum_neg(p) / (n_neg + 1)
// The reference materialises the (B, hw, hw) affinity label, the two masks and their products (six passes over
// 67 MB at hw = 1024); here one pass reads attn_pred and the hw low-res labels of the image (LDS).
__device__ __forceinline__ int aff_lowres_label(const long* __restrict__ cam, int b, int t, int h, int w, int H, int W) {
    const int y = t / w, x = t - y * w;
    // F.interpolate(mode="nearest"): src = min(floor(dst * in / out), in - 1)
    int sy = (int)floorf(y * ((float)H / h)), sx = (int)floorf(x * ((float)W / w));
    sy = sy > H - 1 ? H - 1 : sy;
    sx = sx > W - 1 ? W - 1 : sx;
    return (int)cam[((long)b * H + sy) * W + sx];
}

#define AFF_ROWS 32      // rows of the (hw, hw) matrix per workgroup
template <bool BWD>
__global__ __launch_bounds__(256) void aff_loss_kernel(const float* __restrict__ ap, const long* __restrict__ cam,
                                                        float* __restrict__ part, const float* __restrict__ coef,
                                                        float* __restrict__ dap, int h, int w, int H, int W, int radius,
                                                        int ignore) {
    extern __shared__ int lab[];          // [hw] low-res labels of image b | [hw] (y << 16 | x) of every token
    __shared__ float red[16];
    const int hw = h * w, b = blockIdx.y;
    int* yx = lab + hw;                   // token coordinates once per block: the sweep below has no integer division
    for (int t = threadIdx.x; t < hw; t += 256) {
        lab[t] = aff_lowres_label(cam, b, t, h, w, H, W);
        const int ty = t / w;
        yx[t] = (ty << 16) | (t - ty * w);
    }
    __syncthreads();
    // block = ROWS rows i of the (hw, hw) matrix, threads sweep j (four consecutive j per thread and 16-byte access when
    // hw % 4 == 0; the low-resolution label table above is rebuilt per block, so the rows per block amortise it)
    constexpr int ROWS = AFF_ROWS;
    float ps = 0.f, pc = 0.f, ns = 0.f, nc = 0.f;
    float cp = 0.f, cn = 0.f;
    if (BWD) { cp = coef[0]; cn = coef[1]; }
    const bool vec = (hw & 3) == 0;
    if (!BWD && vec && (blockIdx.x + 1) * ROWS <= hw) {
        // forward, full block: the 16-byte loads of 8 rows are issued before any of them is consumed (the row loop
        // below keeps one load per thread in flight: 32 dependent round trips per thread)
        for (int r0 = 0; r0 < ROWS; r0 += 8) {
            for (int j0 = threadIdx.x * 4; j0 < hw; j0 += 1024) {
                float4 pv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    pv[u] = *reinterpret_cast<const float4*>(ap + ((long)b * hw + blockIdx.x * ROWS + r0 + u) * hw + j0);
                int lj[4], yj[4], xj[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { lj[k] = lab[j0 + k]; yj[k] = yx[j0 + k] >> 16; xj[k] = yx[j0 + k] & 0xffff; }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = blockIdx.x * ROWS + r0 + u;
                    const int li = lab[i], yi = yx[i] >> 16, xi = yx[i] & 0xffff;
                    const float p4[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int dy = yi - yj[k], dx = xi - xj[k];
                        const bool ok = li != ignore && lj[k] != ignore && dy <= radius && -dy <= radius && dx <= radius && -dx <= radius;
                        const bool pos = ok && li == lj[k], neg = ok && li != lj[k];
                        if (pos) { ps += 1.f - p4[k]; pc += 1.f; }
                        if (neg) { ns += p4[k]; nc += 1.f; }
                    }
                }
            }
        }
    } else
    for (int r = 0; r < ROWS; ++r) {
        const int i = blockIdx.x * ROWS + r;
        if (i >= hw) break;
        const int li = lab[i], yi = i / w, xi = i - yi * w;
        const float* row = ap + ((long)b * hw + i) * hw;
        if (vec) {
            for (int j0 = threadIdx.x * 4; j0 < hw; j0 += 1024) {
                float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!BWD) pv = *reinterpret_cast<const float4*>(row + j0);
                const float p4[4] = {pv.x, pv.y, pv.z, pv.w};
                float o4[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j0 + k;
                    const int lj = lab[j], yj = yx[j] >> 16, xj = yx[j] & 0xffff;
                    const int dy = yi - yj, dx = xi - xj;
                    const bool ok = li != ignore && lj != ignore && dy <= radius && -dy <= radius && dx <= radius && -dx <= radius;
                    const bool pos = ok && li == lj, neg = ok && li != lj;
                    o4[k] = pos ? cp : (neg ? cn : 0.f);
                    if (!BWD) {
                        if (pos) { ps += 1.f - p4[k]; pc += 1.f; }
                        if (neg) { ns += p4[k]; nc += 1.f; }
                    }
                }
                if (BWD) *reinterpret_cast<float4*>(dap + ((long)b * hw + i) * hw + j0) = make_float4(o4[0], o4[1], o4[2], o4[3]);
            }
            continue;
        }
        for (int j = threadIdx.x; j < hw; j += 256) {
            const int lj = lab[j], yj = yx[j] >> 16, xj = yx[j] & 0xffff;
            const int dy = yi - yj, dx = xi - xj;
            const bool ok = li != ignore && lj != ignore && dy <= radius && -dy <= radius && dx <= radius && -dx <= radius;
            const bool pos = ok && li == lj, neg = ok && li != lj;
            if (BWD) {
                dap[((long)b * hw + i) * hw + j] = pos ? cp : (neg ? cn : 0.f);
            } else {
                const float p = row[j];
                if (pos) { ps += 1.f - p; pc += 1.f; }
                if (neg) { ns += p; nc += 1.f; }
            }
        }
    }
    if (!BWD) {
        const float a0 = block_sum(ps, red), a1 = block_sum(pc, red), a2 = block_sum(ns, red), a3 = block_sum(nc, red);
        if (threadIdx.x == 0) {
            const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
            part[blk * 4] = a0; part[blk * 4 + 1] = a1; part[blk * 4 + 2] = a2; part[blk * 4 + 3] = a3;
        }
    }
}

// sums (4) = [sum_pos(1-p), n_pos, sum_neg(p), n_neg]; part: workspace 4 * B * ceil(hw/8) floats.
extern "C" int wc_aff_loss_fwd(const float* attn_pred, const int64_t* cam_label, float* part, float* sums, int B, int h,
                               int w, int H, int W, int radius, int ignore, void* stream) {
    WC_CHECK_ARG(attn_pred && cam_label && part && sums && B > 0 && h > 0 && w > 0 && H >= h && W >= w && radius >= 0,
                 "wc_aff_loss_fwd: bad argument");
    WC_CHECK_ARG((size_t)h * w * 8 <= 64 * 1024 && B <= 65535 && h < 32768 && w < 65536, "wc_aff_loss_fwd: h*w <= 8192");
    dim3 grid(wc_cdiv(h * w, AFF_ROWS), B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aff_loss_kernel<false>, grid, dim3(256), (size_t)h * w * 8, st, attn_pred, (const long*)cam_label, part,
                       nullptr, nullptr, h, w, H, W, radius, ignore);
    WC_LAUNCH_CHECK("aff_loss_kernel<fwd>");
    hipLaunchKernelGGL(seg_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, part, sums, (long)grid.x * grid.y, 1);
    WC_LAUNCH_CHECK("seg_loss_reduce_kernel");
    return WC_OK;
}

// dap (B, hw, hw) = coef[0] on positive pairs, coef[1] on negative pairs, 0 elsewhere (coef: 2 device floats,
// = upstream gradient * [-0.5 / (n_pos + 1), 0.5 / (n_neg + 1)]).
extern "C" int wc_aff_loss_bwd(const int64_t* cam_label, const float* coef, float* dap, int B, int h, int w, int H, int W,
                               int radius, int ignore, void* stream) {
    WC_CHECK_ARG(cam_label && coef && dap && B > 0 && h > 0 && w > 0 && H >= h && W >= w && radius >= 0,
                 "wc_aff_loss_bwd: bad argument");
    WC_CHECK_ARG((size_t)h * w * 8 <= 64 * 1024 && B <= 65535 && h < 32768 && w < 65536, "wc_aff_loss_bwd: h*w <= 8192");
    hipLaunchKernelGGL(aff_loss_kernel<true>, dim3(wc_cdiv(h * w, AFF_ROWS), B), dim3(256), (size_t)h * w * 8, (hipStream_t)stream,
                       nullptr, (const long*)cam_label, nullptr, coef, dap, h, w, H, W, radius, ignore);
    WC_LAUNCH_CHECK("aff_loss_kernel<bwd>");
    return WC_OK;
}
