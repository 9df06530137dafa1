/* weclip_hip.h -- C ABI of libweclip_hip.so (MI355X / gfx950 HIP kernels for the WeCLIP
 * forward/CAM hot path).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed, or a torch CUDA tensor's data_ptr())
 *     unless the parameter name starts with `h_` (host array, read during the call);
 *   - tensors are dense row-major in the stated shape; inputs are never written;
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work, never sync;
 *   - return value: 0 = ok, non-zero = error (WC_ERR_ARG 1: rejected argument, nothing was
 *     launched; WC_ERR_HIP 2: HIP runtime error); wc_last_error() gives the message
 *     (thread-local).  The Python host raises RuntimeError, like the stock torch ops the
 *     reference calls do.
 *   - no global state except thread-local error text and the kernel form set by wc_par_sweep_form (results do not depend
 *     on it); re-entrant per device.
 *
 * Each entry cites the reference interface it replaces (paths relative to the reference
 * repository dayae1204/WeCLIP-ViT-CoMer).
 */
#ifndef WECLIP_HIP_H
#define WECLIP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------- */
int wc_version(void);
const char* wc_last_error(void);
int wc_device_count(void);
int wc_device_arch(int dev, char* buf, int buflen);

/* Per-kernel HIP-event timing of the dominant kernels (GEMMs, attention, PAR), for bench.py's roofline leg.
 * wc_prof_enable(n) clears the records and records one of every n instrumented launches on average (a fixed pseudo-random
 * pick, so that the sample does not alias with the step; n = 1: all; an event pair fences its launch, ~6 us), (0) stops.
 * The sweeps of a PAR.forward group share ONE pair (always recorded).  wc_prof_report synchronises the device and writes one
 * "kernel name \t launches \t total ms \t algorithmic work (flop or bytes) \t ms scaled by each record's sampling weight"
 * line per kernel. */
void wc_prof_enable(int stride);
/* Group tag appended to the kernel names of the launches that follow ("@vit_attn": in-projection, attention, head-mean
 * maps and out-projection of an encoder block, the north star's "ViT attention" group); NULL / "" clears it. */
void wc_prof_tag(const char* tag);
int wc_prof_report(char* buf, int cap);

/* ---- PAR: pixel-adaptive refinement -------------------------------------------------- */
/* WeCLIP_model/PAR.py:64-88 (`PAR.forward` up to `aff`, incl. get_dilated_neighbors :39-49 and
 * get_pos :51-62).  img (B,3,H,W) f32 -> aff (B, 8*n_dil, H, W) f32. */
int wc_par_affinity(const float* img, float* aff, int B, int H, int W,
                    const int* h_dilations, int n_dil, void* stream);
/* WeCLIP_model/PAR.py:88-91, one iteration: masks_out = sum_t aff_t * masks_in(nbr_t).
 * masks (B,C,H,W) f32; in and out must differ. */
int wc_par_iterate(const float* aff, const float* masks_in, float* masks_out, int B, int C,
                   int H, int W, const int* h_dilations, int n_dil, void* stream);
/* WeCLIP_model/PAR.py:64-92, whole `PAR.forward` for imgs already at mask resolution.
 * out/tmp: (B,C,H,W) f32 workspaces (result in out); aff_ws: min(group,B)*8*n_dil*H*ceil64(W) f32.
 * Images are swept in groups of `group` so a group's aff planes stay cache resident. */
int wc_par_forward(const float* img, const float* masks, float* out, float* tmp, float* aff_ws,
                   int B, int C, int H, int W, const int* h_dilations, int n_dil, int num_iter,
                   int group, void* stream);
/* Same sweep with the affinities stored as 16-bit fixed-point pairs + one fp32 scale per pixel between the iterations
 * (half the HBM bytes per sweep; |rounding error| <= max_t a_t * 7.7e-6 per weight, error-diffused so a pixel's weights
 * keep their sum): the `fast` precision mode.  6 dilations (48 taps) only; aff_ws as for wc_par_forward. */
int wc_par_forward_h(const float* img, const float* masks, float* out, float* tmp, float* aff_ws,
                   int B, int C, int H, int W, const int* h_dilations, int n_dil, int num_iter,
                   int group, void* stream);
/* Kernel form of the sweeps of wc_par_forward_h (process-wide; both forms give bit-identical masks): 0 = the 64 x 8 tile with
 * a 12-pixel halo and gathered far taps (the comparator of tests/test_par_strip_gpu.py and of A/B timings), 1 = the strip walk
 * with a rolling 24-pixel-halo window in LDS, -1 = the default: WECLIP_PAR_SWEEP from the environment, else form 1, for
 * launches of at least one 64-row segment of a 64-pixel strip per CU, and form 0 below that.  Dilations above 24 always run
 * form 0.  seg_rows: rows of a strip per workgroup, 0 = planned from the CU count. */
int wc_par_sweep_form(int form, int seg_rows);
/* WeCLIP_model/model_attn_aff_voc.py:49-57 (`_refine_cams` tail): labels = valid_key[argmax_c].
 * valid_key (B,C) i64, nch (B) i32 channels in use per image (NULL = C), labels (B,H,W) i64. */
int wc_par_labels(const float* masks, const int64_t* valid_key, const int* nch, int64_t* labels,
                  int B, int C, int H, int W, void* stream);

/* ---- bilinear plane resize ------------------------------------------------------------ */
/* cv2.resize(INTER_LINEAR) in clip/clip_tool.py:202-216 (align_corners=0);
 * F.interpolate(..., bilinear, align_corners=True) in WeCLIP_model/PAR.py:67;
 * F.interpolate(segs, bilinear, align_corners=False) in scripts/dist_clip_voc.py:250.
 * src (planes,Hs,Ws) f32 -> dst (planes,Hd,Wd) f32. */
int wc_bilinear_resize(const float* src, float* dst, int planes, int Hs, int Ws, int Hd, int Wd,
                       int align_corners, void* stream);
/* backward of the same (up-sampling): gsrc (planes,Hs,Ws) = sum over destination pixels of their
 * gradient gdst (planes,Hd,Wd) times the interpolation weight; separable two-pass gather, no atomics
 * (tmp: planes*Hs*Wd f32 workspace)
 * (autograd of F.interpolate at scripts/dist_clip_voc.py:250). */
int wc_bilinear_resize_bwd(const float* gdst, float* gsrc, float* tmp, int planes, int Hs, int Ws, int Hd,
                           int Wd, int align_corners, void* stream);

/* ---- segmentation loss fused with the logit up-sampling -------------------------------- */
/* scripts/dist_clip_voc.py:250 (bilinear up-sampling of seg to H x W) + get_seg_loss :105-113.
 * seg (B,nc,h,w) f32 low-res logits, label (B,H,W) i64 (ignore = 255).
 * wc_seg_loss_fwd: sums (8) = [sum nll over label==0, #label==0, sum nll over fg labels, #fg,
 *                  loss = 0.5*(sums[0]/sums[1] + sums[2]/sums[3]), 0.5/sums[1], 0.5/sums[3], 0]
 *                  (sums[5..6]: the backward weights wts for an upstream gradient of 1);
 *                  part: ceil(W/64)*ceil(H/4)*B*4 f32.  Forward only; 1 <= nc <= 128, H >= h, W >= w. */
int wc_seg_loss_fwd(const float* seg, const int64_t* label, float* part, float* sums, int B, int nc, int h, int w,
                    int H, int W, int ignore, void* stream);

/* Training form: loss sums (as wc_seg_loss_fwd) AND d loss / d seg for an upstream gradient of 1 in ONE pass over the
 * pixels (a label count first gives the class weights), a one-block reduce and the X pass of the separable bilinear
 * backward; no host synchronisation, no atomics (bit-identical between calls).  The pixel pass is that of
 * wc_ce_loss_fwd_bwd with the two-term weighting, and the sizes are its sizes: 1 <= nc <= 128, label at any H x W,
 * W <= 8192.  cnt: 2048 floats; part: 4 * ceil(W/64) * ceil(h/4) * B * nchunk floats, 16-byte aligned, nchunk = 1 for
 * nc <= 32, else ceil(nc/32); tmp: 2*B*nc*h*W floats; grad: (B,nc,h,w).  (scripts/dist_clip_voc.py:105-113,250) */
int wc_seg_loss_fwd_bwd(const float* seg, const int64_t* label, float* cnt, float* part, float* sums, float* tmp, float* grad,
                        int B, int nc, int h, int w, int H, int W, int ignore, void* stream);

/* Cross-entropy with an ignore index fused with the bilinear up-sampling of the logits, training form (the supervised
 * variant's loss: F.cross_entropy(F.interpolate(seg, (H,W), bilinear, align_corners=False), label, ignore_index=ignore)).
 * seg (B,nc,h,w) f32, label (B,H,W) i64 at any H x W (up- or down-sampling), 1 <= nc <= 128, W <= 8192.
 * Loss AND d loss / d seg for an upstream gradient of 1 in one pixel pass, a one-block reduce and the X pass of the
 * separable bilinear backward; no host synchronisation, no atomics (bit-identical between calls).
 * A label outside [0, nc) that is not `ignore` counts as ignored and is reported in sums[3].
 * Workspaces:
 *   part: 4 f32 per workgroup of the pixel pass = 4 * ceil(W/64) * ceil(h/4) * B * nchunk floats, 16-byte aligned,
 *         nchunk = 1 for nc <= 32, else ceil(nc/32);
 *   sums: 4 f32 = [loss (NaN when no pixel is valid, as F.cross_entropy), 1/N_valid (0 when N_valid == 0), N_valid,
 *         N_bad (labels outside [0, nc) that are not ignore)] -- counts exact below 2^24;
 *   tmp:  2 * B*nc*h*W f32;
 *   grad: (B,nc,h,w) f32 output, (softmax - onehot) / N_valid pulled back through the up-sampling (all zero when N_valid == 0,
 *         as torch's). */
int wc_ce_loss_fwd_bwd(const float* seg, const int64_t* label, float* part, float* sums, float* tmp, float* grad, int B, int nc,
                       int h, int w, int H, int W, int ignore, void* stream);

/* Affinity loss fused with the affinity-label construction (reference utils/camutils.py:226-247 +
 * scripts/dist_clip_voc.py:116-133 radius mask + utils/losses.py:11-22): attn_pred (B,hw,hw) f32, cam_label (B,H,W)
 * int64 pseudo labels (nearest down-sampled to h x w inside), Chebyshev `radius`.
 * fwd: sums (8) = [sum_pos(1-p), n_pos, sum_neg(p), n_neg, loss = 0.5*s0/(s1+1) + 0.5*s2/(s3+1),
 *      -0.5/(s1+1), 0.5/(s3+1), 0]  (sums[5..6]: the backward coef for an upstream gradient of 1);
 *      part: workspace 4*B*ceil(hw/8) f32.
 * bwd: dap (B,hw,hw) = coef[0] on positive pairs, coef[1] on negative pairs, 0 elsewhere (coef: 2 device floats). */
int wc_aff_loss_fwd(const float* attn_pred, const int64_t* cam_label, float* part, float* sums, int B, int h,
                    int w, int H, int W, int radius, int ignore, void* stream);
int wc_aff_loss_bwd(const int64_t* cam_label, const float* coef, float* dap, int B, int h, int w, int H, int W,
                    int radius, int ignore, void* stream);

/* ---- MFMA GEMM ------------------------------------------------------------------------ */
/* C[M,N] = epilogue(sum_{s<nseg} A_s[M,K] * W_s[N,K]^T), fp16 operands (K contiguous), fp32
 * accumulate on v_mfma_f32_32x32x16_f16.  Replaces F.linear / nn.Linear / 1x1 Conv2d / bmm at
 * clip/myAtt.py:201 (in-proj), :321 (fp16 out-proj), clip/model.py:198-202 (MLP), :264-268
 * (patch-embed conv k16 s16 == GEMM), :420 (visual.proj), WeCLIP_model/segformer_head.py:22-28,76,
 * WeCLIP_model/Decoder/TransDecoder.py:122, WeCLIP_model/model_attn_aff_voc.py:136 (bmm).
 * nseg 2/3 = split precision (x = hi + lo): extra (A,W) pairs are accumulated into the same tile.
 * epilogue: v = acc + bias[n]; if round16: v = fp16(v); if n < scale_cols: v *= scale;
 *           v = act(v) (0 none, 1 QuickGELU, 2 ReLU, 3 sigmoid); v += resid[m*ldr + n];
 *           C32[m,n] = v; C16[m,n] = fp16(v); C16lo[m,n] = fp16(v - C16).
 *           P32 (optional) receives the pre-activation value.  act 4 (backward of QuickGELU,
 *           clip/model.py:186-188): v *= d/du[u*sigmoid(1.702u)] at u = aux[arow*ldaux + n],
 *           arow = rowmap[m / rpg]*rpg + m % rpg (rowmap NULL: arow = m).
 *           act 5 (backward of ReLU, segformer_head.py:26): v *= (auxh[m*ldaux + n] > 0), auxh fp16.
 *           act 6: exact GELU 0.5 v (1 + erf(v / sqrt 2)) (nn.GELU of the ViT-CoMer inserts); act 7: its backward,
 *           v *= Phi(u) + u phi(u) at u = aux[...] as for act 4.
 *           cscale (optional): v *= cscale[z*sCS + n] after the bias (Dropout2d mask/(1-p) of image z,
 *           segformer_head.py:78).
 * batch > 1: operand/output/residual batch strides sA/sW/sC/sR in elements.  K % 64 == 0, lda/ldw % 8 == 0. */
int wc_gemm_f16(const void* A0, const void* A1, const void* A2, const void* W0, const void* W1,
                const void* W2, int nseg, int M, int N, int K, long lda, long ldw, int batch,
                long sA, long sW, long sC, const float* bias, const float* resid, long ldr, long sR,
                float* C32,
                void* C16, void* C16lo, long ldc, int act, int round16, float scale,
                int scale_cols, float* P32, const float* aux, const int* rowmap, int rpg,
                long ldaux, const void* auxh, const float* cscale, long sCS, void* stream);

/* Grouped form of wc_gemm_f16: several small GEMMs of one shape in ONE launch -- the 11 adapter MLPs of
 * WeCLIP_model/segformer_head.py:58-76 (one nn.Linear pair per encoder block, the reference loops over them) times
 * the B images.  Batch index z splits into z2 = z / zdiv (group: adapter) and z1 = z % zdiv (image): A, W and the
 * outputs move by z1*s? + z2*s?2 elements, the bias by z2*sB2 and the act-5 aux by z2*sX2; everything else as
 * wc_gemm_f16 (which is this entry with zdiv = batch and zero second-level strides). */
int wc_gemm_f16_grouped(const void* A0, const void* A1, const void* A2, const void* W0, const void* W1,
                        const void* W2, int nseg, int M, int N, int K, long lda, long ldw, int batch,
                        long sA, long sW, long sC, const float* bias, const float* resid, long ldr, long sR,
                        float* C32, void* C16, void* C16lo, long ldc, int act, int round16, float scale,
                        int scale_cols, float* P32, const float* aux, const int* rowmap, int rpg,
                        long ldaux, const void* auxh, const float* cscale, long sCS, int zdiv, long sA2, long sW2,
                        long sC2, long sB2, long sX2, void* stream);

/* Row-streaming GEMM for tall, narrow products: C[M, N <= 256] = epilogue(A[M, K] W[N, K]^T), K = 128 | 256, fp16 operands,
 * fp32 accumulate (csrc/gemm_row.hip).  Replaces the same F.linear / 1x1-conv call sites as wc_gemm_f16 where the output row is
 * one complete channel vector: the Linear layers of the ViT-CoMer inserts (no reference code: ViT_CoMer.pdf section 3.2-3.3,
 * SURVEY.md section 8 row a-9) and WeCLIP_model/segformer_head.py:22-28, Decoder/TransDecoder.py:98-125 at N = 256.  The launch
 * is bound by HBM bytes, not flops: weights stay in registers, A and the side input stream through LDS once, every output row
 * leaves as whole coalesced rows.  Epilogue, in this order:  v = (acc + bias[n]) * cscale[n];  P32 = v;  act (0 none, 2 ReLU,
 * 6 GELU(erf); 5: v *= (auxh[m, n] > 0); 7: v *= GELU'(aux[m, n]));  v += resid[m, n];  C32 = v;  C16 = fp16(v);  and, for
 * N == 256, up to two LayerNorms of the finished row (fp32 statistics, clip/model.py:177-183 arithmetic) written as fp16:
 * ln_o{0,1}[m, :] = LN(v; ln_g, ln_b, eps) -- the operand of the next GEMM, without a LayerNorm launch.  At most ONE side input
 * per launch (resid, or aux with act 7, or auxh with act 5).  Any subset of outputs; null pointers = absent.
 * ldc = row pitch of C32 / P32, ldc16 = row pitch of C16 (it may be a column slice of a wider buffer).
 * lda, ldw % 8 == 0; ldc, ldc16, ldr, ldaux % 4 == 0 (ldaux % 8 for act 5); fp32 buffers 16-byte, fp16 outputs 8-byte aligned.
 * wc_gemm_row_supported: 1 when (M, N, K) is a shape this entry accepts. */
int wc_gemm_row_supported(int M, int N, int K);
int wc_gemm_row_f16(const void* A, long lda, const void* W, long ldw, int M, int N, int K, const float* bias,
                    const float* cscale, int act, const float* aux, const void* auxh, long ldaux, const float* resid, long ldr,
                    float* C32, void* C16, float* P32, long ldc, long ldc16, const float* ln_g0, const float* ln_b0, void* ln_o0,
                    const float* ln_g1, const float* ln_b1, void* ln_o1, float eps, void* stream);

/* `groups` products of one shape in one launch of the row-streaming kernel (the eleven adapter MLPs' second Linear and its input
 * gradient, WeCLIP_model/segformer_head.py:22-28,69-80): group i reads A + i*gA, W + i*gW, bias + i*gB, auxh + i*gX and writes
 * C32 / C16 + i*gC (element offsets; e.g. gC = 256 with ldc16 = 11*256 drops every adapter's output into its column slice of the
 * fuse input).  act 0 | 2 | 5. */
int wc_gemm_row_f16_grouped(const void* A, long lda, const void* W, long ldw, int M, int N, int K, const float* bias, int act,
                            const void* auxh, long ldaux, float* C32, void* C16, long ldc, long ldc16, int groups, long gA,
                            long gW, long gB, long gC, long gX, void* stream);

/* Which kernel wc_gemm_f16 runs for a shape (for profiling / roofline bookkeeping only):
 * 0 = 128x128x64 kernel, 1 = 256x256x64 ping-pong kernel, 2 = ping-pong kernel + 128x128 kernel on the ragged
 * last M % 256 rows (two launches). */
int wc_gemm_plan(int M, int N, int K, int nseg, int batch);
/* Per-shape timing of the GEMM entry points when WECLIP_GEMM_LOG=1 (an event pair around every call): writes
 * "entry M= N= K= seg= batch= plan= act=\tcalls\tms\tflop" lines into buf, clears the log, returns the number of lines. */
int wc_gemm_log_report(char* buf, int cap);
/* out[i] = alpha * sum_s part[s*n + i]: reduction of split-K partial products (the slices are a
 * batched wc_gemm_f16 over K ranges: sA = sW = K/slices, sC = M*N). */
int wc_sum_slices(const float* part, float* out, int nslices, long n, float alpha, void* stream);

/* Split-K reduction of a weight-gradient GEMM whose X^T operand carried a ones row (the bias-gradient column):
 * part (nslices, rows, cols+1) -> out_w (rows, cols) dense and out_b (rows); replaces the autograd-produced
 * .weight/.bias gradients of nn.Linear / 1x1 nn.Conv2d (reference WeCLIP_model/segformer_head.py:22-28). */
int wc_sum_slices_wb(const float* part, float* out_w, float* out_b, int nslices, int rows, int cols,
                     float alpha, void* stream);
/* `groups` such reductions of one shape in one launch: part (groups, nslices, rows, cols+1); group i writes
 * out_w + i*gW and out_b + i*gB (elements) -- the per-adapter gradient views of a flat gradient bucket. */
int wc_sum_slices_wb_grouped(const float* part, float* out_w, float* out_b, int nslices, int rows, int cols,
                             float alpha, int groups, long gW, long gB, void* stream);
/* Many split-K reductions in one launch.  jobs: HOST array of count x 8 int64 {part, out_w, out_b (device pointers), nslices,
 * rows, cols, alpha as IEEE float bits, slice stride in elements (0 = rows * (cols + 1); larger when the job reduces a row
 * range of a wider partial matrix)}; each job = one wc_sum_slices_wb (same summation order).  The jobs travel by value
 * in the kernel arguments (graph-capturable, no device table). */
int wc_sum_slices_wb_multi(const int64_t* jobs, int count, void* stream);

/* Weight-gradient GEMM on row-major operands: part[z, n, k] = sum over the tokens m of slice z of dY[m, n] * X[m, k]
 * (and, with bias != 0, one more column k = K holding sum_m dY[m, n]); z = 0 .. ceil(M / mslice) - 1, mslice a multiple
 * of 64.  fp16 operands (M, lda) / (M, ldx), fp32 partials (nslices, N, K + bias) to be summed by wc_sum_slices(_wb).
 * Replaces the autograd weight/bias gradients of nn.Linear / 1x1 nn.Conv2d (reference
 * WeCLIP_model/segformer_head.py:22-28,69-80; Decoder/TransDecoder.py:98-125) without transposed operand copies.
 * The X row of token m is (m / x_rpg) * x_gs + m % x_rpg + x_off (use x_rpg = M, x_gs = 0, x_off = 0 for a
 * dense matrix) -- lets X be the patch rows of a (B, 1 + hw, C) token tensor.  zeros: >= 16 zero bytes. */
int wc_gemm_km_f16(const void* dY, long lda, const void* X, long ldx, const void* zeros, int M, int N, int K,
                   int x_rpg, int x_gs, int x_off, int mslice, int bias, float* part, void* stream);
/* `groups` weight gradients of one shape in one launch (the 11 adapter Linears, segformer_head.py:58-76): group i
 * reads dY + i*gA and X + i*gX (elements) and writes part + i*nslices*N*(K+bias). */
int wc_gemm_km_f16_grouped(const void* dY, long lda, const void* X, long ldx, const void* zeros, int M, int N, int K,
                           int x_rpg, int x_gs, int x_off, int mslice, int bias, float* part, int groups, long gA,
                           long gX, void* stream);
/* Many weight-gradient GEMMs in one grid (all Linear / 1x1 conv weight gradients of a backward pass, reference
 * WeCLIP_model/segformer_head.py:22-28,58-80; Decoder/TransDecoder.py:98-125: nothing reads one before the optimizer).
 * jobs: HOST array of count x 16 int64 {dY, X, part (device pointers), M, N, K, lda, ldx, x_rpg, x_gs, x_off, mslice, bias,
 * groups, gA, gX}; each job = one wc_gemm_km_f16_grouped call and writes the partials that call would write (same kernel
 * form, bit-identical).  Jobs run longest K loop first; the table travels by value in the kernel arguments
 * (graph-capturable), 32 jobs per launch and one launch per kernel form. */
int wc_gemm_km_f16_multi(const int64_t* jobs, int count, const void* zeros, void* stream);
/* The launches wc_gemm_km_f16_multi would make, without a GPU.  cus: CU count the kernel form is chosen for (<= 0: the
 * current device's).  Per job i: launch[i], first[i] = its first workgroup id there (a multiple of 8), pos[i] = its place
 * in that launch's table; per launch l < *nlaunches: grids[l] workgroups and forms[l] (1: 4 waves, 2: 8 waves). */
int wc_gemm_km_multi_plan(const int64_t* jobs, int count, int cus, int* launch, int* first, int* pos, int* grids,
                          int* forms, int max_launches, int* nlaunches);
/* The kernel's job search and index arithmetic for workgroup wg of launch l, run on the host:
 * out[0] = job (input order; -1: a padding id that exits at once), out[1] = unit (group * slices + slice), out[2] = tile. */
int wc_gemm_km_multi_locate(const int64_t* jobs, int count, int cus, int l, int wg, int* out);
/* fp32 -> fp16 hi (+ lo = fp16(x - hi), may be NULL): `.half()` casts of weights/activations
 * (clip/model.py:457-478 convert_weights; clip/myAtt.py:321). */
int wc_split_f16(const float* x, void* hi, void* lo, long n, void* stream);

/* Many fp32 weight matrices -> fp16 operands in one launch: row-major hi[,lo] (R,C) and transposed hiT[,loT]
 * (C, ldT >= R; padding columns are left untouched -- keep them zero).  table (device): count rows of 8 int64
 * {src, hi, lo|0, hiT|0, loT|0, R, C, ldT}.  Replaces the per-layer `.half()` / `.t()` of the trainable weights. */
int wc_convert_weights(const int64_t* table, int count, int blocks_per_tensor, void* stream);

/* One AdamW step over many fp32 parameter tensors in one launch (reference utils/optimizer.py:3-33: torch.optim.AdamW
 * with the poly-warm-up lr written per group).  table (device): count rows of 8 int64 {param, grad, exp_avg, exp_avg_sq,
 * numel, 0, 0, 0}.  p *= 1 - lr*wd; m = lerp(m, g, 1-b1); v = v*b2 + (1-b2) g^2; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 * with bias_correction{1,2} = 1 - beta^step > 0 (the update order of torch._multi_tensor_adam).  0 < count <= 65535 (also for
 * wc_convert_weights), blocks_per_tensor > 0.  A tensor with numel % 4 == 0 whose four pointers are 16-byte aligned is walked
 * with 16-byte accesses, any other one element by element: the arithmetic is the same. */
int wc_adamw_multi(const int64_t* table, int count, double lr, double beta1, double beta2, double eps,
                   double weight_decay, double bias_correction1, double bias_correction2, int blocks_per_tensor,
                   void* stream);

/* One SGD-with-momentum step over many fp32 parameter tensors in one launch (reference utils/optimizer.py:35-65:
 * torch.optim.SGD with momentum 0.9 and the poly-warm-up lr written per group).  table (device): count rows of 8 int64
 * {param, grad, momentum_buffer, numel, 0, 0, 0, 0}.  g' = g + weight_decay*p; buf = momentum*buf + g'; p -= lr*buf (the order
 * of torch.optim.SGD with dampening 0, no Nesterov, no maximize); grad is only read.  A first step is a zero momentum_buffer:
 * momentum*0 + g' = g' exactly, which is torch's clone(g').  lr, momentum and weight_decay are each rounded once to fp32.
 * 0 < count <= 65535, blocks_per_tensor > 0, 0 <= momentum < 1, lr and weight_decay finite and >= 0 (WC_ERR_ARG otherwise).
 * A tensor with numel % 4 == 0 whose three pointers are 16-byte aligned is walked with 16-byte accesses, any other one
 * element by element: the arithmetic is the same. */
int wc_sgd_multi(const int64_t* table, int count, double lr, double momentum, double weight_decay, int blocks_per_tensor,
                 void* stream);

/* ---- LayerNorm ------------------------------------------------------------------------ */
/* clip/model.py:177-183 (`LayerNorm.forward`, fp32 math).  x (rows, D) f32 with row stride ldx;
 * outputs (each optional, at least one of y32 / y16; y16lo only with y16): y32 f32, y16 fp16 hi, y16lo fp16 residual; all dense
 * (rows, D).  D % 4 == 0, D <= 4096, ldx >= D, ldx % 4 == 0 (WC_ERR_ARG otherwise).  The kernels use 16-byte (fp16: 8-byte)
 * accesses: keep every buffer aligned to that (not checked). */
int wc_layernorm(const float* x, long ldx, const float* w, const float* b, float eps, float* y32,
                 void* y16, void* y16lo, long rows, int D, void* stream);

/* ---- multi-head attention -------------------------------------------------------------- */
/* Packed in-projection output qkv (B*L, 3E) fp16, E = H*DH, q pre-scaled by log2(e)/sqrt(DH)
 * (wc_gemm_f16 scale/scale_cols).  DH in {32, 64}.
 * wc_attn_fwd:  clip/myAtt.py:21-64 without materialising the scores: out (B*L, E) fp16 =
 *               softmax(QK^T)V with heads merged (the `.half()` input of the out-projection,
 *               myAtt.py:319-321); out32 (optional) the same before fp16 rounding;
 *               lse (B,H,L) f32 = log2-sum-exp2 of each score row.  V is read row-major from qkv.
 * wc_attn_mean: clip/myAtt.py:325-326: mean (B,L,L) f32 = (1/H) sum_h softmax_h.
 * qkv, out and out32 must be 16-byte aligned (WC_ERR_ARG otherwise); so must qkv, dO and o32 of wc_attn_bwd_colsum. */
int wc_attn_fwd(const void* qkv, void* out, float* out32, float* lse, int B, int L, int H, int DH,
                void* stream);
int wc_attn_mean(const void* qkv, const float* lse, float* mean, int B, int L, int H, int DH,
                 void* stream);

/* ---- ViT patch embedding ---------------------------------------------------------------- */
/* clip/model.py:264-272.  wc_patchify: img (B,3,H,W) f32 -> im2col rows (B*h*w, 3*P*P) fp16 hi
 * (+lo, may be NULL) in the conv weight's (c,ky,kx) order, so conv1 == wc_gemm_f16.
 * wc_cls_rows: x[b,0,:] = class_embedding + pos[0] for the token tensor x (B,L,E) f32. */
int wc_patchify(const float* img, void* hi, void* lo, int B, int H, int W, int P, void* stream);
int wc_cls_rows(float* x, const float* cls, const float* pos0, int B, int L, int E, void* stream);

/* ---- GradCAM on the last CLIP block (analytic, batched over (image, class) pairs) ------- */
/* Replaces pytorch_grad_cam/base_cam.py:62-154, grad_cam.py:16-23,
 * activations_and_gradients.py:19-47 (autograd through CLIP.forward_last_layer,
 * clip/model.py:407-429).  P pairs; pair_img[p] = image of pair p, pair_cls[p] = index of the
 * target row among that pair's text rows.  L tokens, E width, Ed joint embedding width.
 *
 * wc_cam_head: x2 (B,L,E) f32 block output -> ln_post, mean over patch tokens, @proj (E,Ed),
 *   cosine logits against pre-normalised text rows text[text_idx[p,t]] (t < n_text[p], row
 *   stride Tmax), softmax -> probs (P,Tmax); df (P,E) = d probs[p,cls] / d pooled feature.
 *   partial: workspace B*ceil(L/16)*E f32.  logit_scale = exp(CLIP.logit_scale).
 *   Three launches behind the pooling, none with a workgroup per pair on the projection: y (B,Ed) = pooled feature @ proj
 *   per (image, 64 columns), the soft-max part per pair -> dy (P,Ed), df per (pair, 64 rows).  y, dy: those workspaces.
 * wc_lnpost_bwd: dx2 (P,L,E) = gs * backward of ln_post+mean-pool (token 0 gets 0);
 *   written as f32 and as fp16 hi/lo GEMM operands.
 * wc_ln2_bwd_add: g16 = fp16((dx2 + LN2_bwd(da2; x1)) / gs): the gradient arriving at the fp16
 *   out-projection output (autograd rounds it to fp16, clip/myAtt.py:321).
 * wc_attn_bwd_colsum: column sums over tokens of dq,dk,dv -> c (P,3E) f32 from the packed
 *   qkv (B*L,3E fp16, q pre-scaled), dO (P*L,E fp16), o32 (B*L,E), lse (B,H,L).
 *   Workspaces: delta,u,dS0,P0 each (P,H,L) f32.
 * wc_rowvec_matmul: out (P,E) = scale * c (P,N) @ W (N,E), fp32 FMA; ws: workspace 16*P*E f32.
 * wc_cam_map: cam (P,L-1) = scale_cam(scale_cam(relu(A w))) with A = a32[img, 1:, :]
 *   (base_cam.py:56-60,144-154; utils/image.py:51-61). */
int wc_cam_head(const float* x2, const float* lnw, const float* lnb, const float* proj,
                const float* text, const int* text_idx, const int* n_text, const int* pair_img,
                const int* pair_cls, float logit_scale, float* partial, float* probs, float* df,
                float* y, float* dy, int B, int P, int L, int E, int Ed, int Tmax, void* stream);
/* wc_cam_head in its earlier form, one workgroup per pair for everything behind the pooling: bit-identical probs and df.
 * Kept as the comparator of tests/test_cam_head_wide_gpu.py and of A/B timings; y and dy are required and left alone. */
int wc_cam_head_single(const float* x2, const float* lnw, const float* lnb, const float* proj,
                       const float* text, const int* text_idx, const int* n_text, const int* pair_img,
                       const int* pair_cls, float logit_scale, float* partial, float* probs, float* df,
                       float* y, float* dy, int B, int P, int L, int E, int Ed, int Tmax, void* stream);
int wc_lnpost_bwd(const float* df, const float* x2, const float* lnw, float gs, const int* pair_img,
                  float* d32, void* dhi, void* dlo, int P, int L, int E, void* stream);
int wc_ln2_bwd_add(const float* da2, const float* dx2, const float* x1, const float* lnw, float gs,
                   const int* pair_img, void* g16, int P, int L, int E, void* stream);
int wc_attn_bwd_colsum(const void* qkv, const void* dO, const float* o32, const float* lse,
                       const int* pair_img, float* delta, float* u, float* dS0, float* P0, float* c,
                       int P, int L, int H, int DH, void* stream);
int wc_rowvec_matmul(const float* c, const float* W, float* out, float* ws, int P, int N, int E, float scale,
                     void* stream);
int wc_cam_map(const float* a32, const float* w, const int* pair_img, float* cam, int P, int L, int E,
               void* stream);

/* ---- attention-affinity CAM refinement -------------------------------------------------- */
/* clip/clip_tool.py:152-191, compute_trans_mat :64-80, clip/utils.py:115-142 (scoremap2bbox),
 * generate_cam_label :202-216, WeCLIP_model/model_attn_aff_voc.py:158-163.  hw = L-1 patch tokens.
 * wc_aff_weight:      W (B,hw,hw) = sum_l wgt[b,l] * maps[l][b,1:,1:] (* seg[b] if seg != NULL);
 *                     h_maps: HOST array of nmaps (<=12) device pointers to (B,L,L) head-mean maps.
 * wc_aff_seg_weights: seg-trans layer selection (:158-167): rowsum (B,nmaps,hw) workspace (the row sums of maps[l][b,1:,1:]),
 *                     diff (B,nmaps) = -sum of them, wgt[b,l] = [diff <= mean diff] / (count + 1e-5).
 * wc_matvec:          out (B,hw,K) = f(W x) (transpose=0) or f(W^T x) (transpose=1),
 *                     x = X * sin[:,None]; f = 1/v if recip else alpha*v*sout[:,None] + add.
 *                     Sinkhorn (:64-75) as scale vectors: c = 1/(W^T r), r = 1/(W c), 3 rounds;
 *                     T_sym x = (r*(W(c*x)) + c*(W^T(r*x)))/2; refined = T_sym(T_sym(mask*cam)).
 * wc_tsym:            materialise T_sym (B,hw,hw) (public compute_trans_mat only).
 * wc_box_mask:        per pair p (cam (P,h*w) in [0,1]): u8 quantise, > int(thr*max), 8-connected
 *                     components, boxes [x0,y0,min(x1+1,w-1),min(y1+1,h-1)], half-open fill;
 *                     V[pair_img[p], :, pair_slot[p]] = mask*cam (V is (B,hw,K));
 *                     optional mask_out (P,hw) f32, boxes (P,maxbox,4) i32 + nbox (P).
 * wc_cam_upsample:    R (B,hw,K) refined maps -> cams (B,C,H,W): channel 1+k = bilinear(half-pixel)
 *                     of min-max(R_k) for k < nk[b] (0 beyond), channel 0 = 1 - max_k.
 *                     2 <= C <= K + 1; nk is read on the device, unchecked: 1 <= nk[b] <= C - 1 is the caller's duty.
 *                     stats: workspace B*K*2 f32. */
int wc_aff_weight(const float* const* h_maps, int nmaps, const float* wgt, const float* seg, float* W,
                  int B, int L, void* stream);
int wc_aff_seg_weights(const float* const* h_maps, int nmaps, float* rowsum, float* diff, float* wgt,
                       int B, int L, void* stream);
int wc_matvec(const float* W, const float* X, const float* sin, const float* sout, const float* add,
              float* out, int B, int hw, int K, int transpose, int recip, float alpha, void* stream);
/* Fused forms for hw %% 4 == 0 (wc_aff_fused_supported): a workgroup owns 32 complete rows of W, so one read of W serves a
 * Sinkhorn row pass AND the next column pass, or both halves of T_sym X; W is read 5 times per batch instead of 10.
 * wc_aff_weight_c1:     W as wc_aff_weight + c1 = 1 / colsum(W).                ws: B*ceil(hw/8)*hw f32
 * wc_aff_sinkhorn_step: r = 1/(W c); unless last: c_next = 1/(W^T r).            ws: B*ceil(hw/32)*hw f32
 * wc_aff_tsym_apply:    out (B,hw,K) = T_sym X, K <= 4.  y1: B*hw*K f32; ws: B*ceil(hw/32)*hw*K f32. */
int wc_aff_fused_supported(int hw);
int wc_aff_weight_c1(const float* const* h_maps, int nmaps, const float* wgt, const float* seg, float* W, float* c1,
                     float* ws, int B, int L, void* stream);
/* wc_attn_aff_weight: clip/clip_tool.py:169-173 (the branch without seg-trans) straight from the layers' attention operands:
 *   W (B,hw,hw) = sum_l wgt[b,l] * ((1/H) sum_h softmax_h(Q_l K_l^T))[1:,1:] and c1 = 1 / colsum(W), bit-identical to
 *   wc_attn_mean per layer followed by wc_aff_weight_c1 (seg == NULL), in one launch that writes no (B,L,L) map.
 *   h_qkv / h_lse: HOST arrays of nmaps (<=12) device pointers to the layers' packed qkv (B*L, 3E) fp16 (as wc_attn_fwd takes it,
 *   16-byte aligned) and lse (B,H,L) f32 (as wc_attn_fwd wrote it), in layer order; wgt (B,nmaps) f32; DH in {32, 64};
 *   hw = L-1 with wc_aff_fused_supported(hw).  ws: B*ceil(hw/8)*hw f32. */
int wc_attn_aff_weight(const void* const* h_qkv, const float* const* h_lse, int nmaps, const float* wgt, float* W, float* c1,
                       float* ws, int B, int L, int H, int DH, void* stream);
int wc_aff_sinkhorn_step(const float* W, const float* c, float* r, float* c_next, float* ws, int B, int hw, int last,
                         void* stream);
int wc_aff_tsym_apply(const float* W, const float* r, const float* c, const float* X, float* out, float* y1, float* ws,
                      int B, int hw, int K, void* stream);
int wc_tsym(const float* W, const float* r, const float* c, float* T, int B, int hw, void* stream);
int wc_box_mask(const float* cam, const int* pair_img, const int* pair_slot, float* V, float* mask_out,
                int* boxes, int* nbox, int maxbox, int P, int h, int w, int K, double thr, void* stream);
/* wc_box_mask in its earlier form (256 threads per pair, a box fill that walks every box per pixel): the same mask_out, V, nbox
 * and set of boxes.  Kept as the comparator of tests/test_box_mask_wide_gpu.py and of A/B timings. */
int wc_box_mask_single(const float* cam, const int* pair_img, const int* pair_slot, float* V, float* mask_out,
                       int* boxes, int* nbox, int maxbox, int P, int h, int w, int K, double thr, void* stream);
int wc_cam_upsample(const float* R, const int* nk, float* stats, float* cams, int B, int h, int w, int K,
                    int C, int H, int W, void* stream);

/* ---- backward helpers of the trainable adapters / decoder ------------------------------ */
/* autograd through WeCLIP_model/segformer_head.py:69-80, Decoder/TransDecoder.py:63-125,
 * model_attn_aff_voc.py:134-137 (all run by torch.autograd in the reference).
 * wc_transpose_f16:  out[c, b*oR + r] = fp16(scale*src[b,r,c]) (hi[,lo]); src f32 or f16 (src_f32),
 *                    row stride ld, batch stride sSrc; out row stride ldo: operands of dW = dY^T X.
 *                    ld >= C, oR >= R, ldo >= (batch-1)*oR + R, batch <= 65535; the columns of out that no (b, r) maps to are
 *                    left untouched (keep them zero).
 * wc_colsum:         out[c] = alpha * sum_r src[r,c] (bias gradients), rounded through fp16 if round16; src f32 or f16
 *                    (src_f32), row stride ld >= C; part: ceil(R/256)*C f32; R <= 256*65535.
 * wc_layernorm_bwd:  dx = add (may be NULL) + LN_bwd(dy; x, w) as f32 and/or fp16(dx*out_scale) (at least one of dx32 / dx16);
 *                    dgb (2,D) = alpha*[sum dy*xhat ; sum dy]; part: ceil(rows/16)*2*D f32.  D % 4 == 0, D <= 1024; dy, x, w,
 *                    add, dx32 16-byte aligned, dx16 (and dy16 of wc_layernorm_bwd_h) 8-byte (WC_ERR_ARG otherwise).
 * wc_sigmoid_gram_bwd: S[b] = scale*(Z + Z^T), Z = dAP*AP*(1-AP) (fp16 hi[,lo], row stride ldo >= n; columns [n, ldo) are left
 *                    untouched) so dF = S F.  n <= 65535.
 * wc_colscale_split: y = alpha * x * cs[row / rows_per_batch, col] (cs may be NULL) -> f32 (optional), fp16 hi[,lo]. */
/* wc_attn_bwd: backward of clip/myAtt.py:21-64 without storing L x L tensors: from the packed qkv
 * (q pre-scaled), dO (B*L,E) fp16, o32, lse -> dqkv (B*L,3E) fp16 hi (+lo, may be NULL), gradients
 * w.r.t. the UNSCALED in-projection output.  Workspaces qt, kt, dot: B*H*DH*Lp halves each;
 * delta: B*H*L floats.  qkv, dO, o32, qt, kt, dot 16-byte aligned, dqkv_hi / dqkv_lo 8-byte. */
int wc_attn_bwd(const void* qkv, const void* dO, const float* o32, const float* lse, void* qt, void* kt,
                void* dot, float* delta, void* dqkv_hi, void* dqkv_lo, int B, int L, int Lp, int H, int DH,
                void* stream);
int wc_transpose_f16(const void* src, int src_f32, long ld, long sSrc, void* hi, void* lo, long ldo,
                     long oR, int batch, int R, int C, float scale, void* stream);
int wc_colsum(const void* src, int src_f32, long ld, float* part, float* out, long R, int C, float alpha,
              int round16, void* stream);
int wc_layernorm_bwd(const float* dy, const float* x, const float* w, const float* add, float eps,
                     float* dx32, void* dx16, float out_scale, float* part, float* dgb, float alpha,
                     long rows, int D, void* stream);
/* the same with the incoming gradient as fp16 rows dy16 (rows, D) */
int wc_layernorm_bwd_h(const void* dy16, const float* x, const float* w, const float* add, float eps,
                       float* dx32, void* dx16, float out_scale, float* part, float* dgb, float alpha,
                       long rows, int D, void* stream);
/* two LayerNorms of ONE input x (the ViT-CoMer CTI normalises c1 once for the values of one deformable attention and once
 * for the queries of the other: this package's own WeCLIP_model/comer.py CTI.forward; no reference code) back-propagated in one
 * pass: dx = LN_bwd_a(dya16) + LN_bwd_b(dyb16) [+ add]; dgba / dgbb (2, D) = alpha * [dgamma; dbeta] of each; D % 4 == 0,
 * D <= 256; part: >= min(ceil(rows / 16), 2048) * 4 * D floats; alignment as for wc_layernorm_bwd_h (wa, wb 16-byte, dya16,
 * dyb16 8-byte) */
int wc_layernorm_bwd2_h(const void* dya16, const float* wa, const void* dyb16, const float* wb, const float* x,
                        const float* add, float eps, float* dx32, void* dx16, float out_scale, float* part, float* dgba,
                        float* dgbb, float alpha, long rows, int D, void* stream);
int wc_sigmoid_gram_bwd(const float* dAP, const float* AP, void* hi, void* lo, int B, int n, int ldo,
                        float scale, void* stream);
int wc_colscale_split(const float* x, const float* cs, float* out32, void* hi, void* lo, long rows, int C,
                      int rows_per_batch, float alpha, void* stream);

/* ---- ViT-CoMer: multi-scale deformable attention core ---------------------------------- */
/* No reference code exists for the CoMer inserts (paper ViT_CoMer.pdf 3.3 / Deformable-DETR eq. 2-3).
 * value (N,S,M,D) f32, S = sum_l H_l*W_l (h_shapes: HOST array of n_levels (H,W) pairs);
 * loc (N,Lq,M,nL,P,2) f32 in [0,1] as (x,y); attn (N,Lq,M,nL,P) f32; out (N,Lq,M*D) f32:
 * out = sum_l sum_p attn * bilinear_zero_pad(value_l, loc*size - 0.5).
 * wc_msda_bwd: gvalue (every element written once: no initialisation needed), gloc, gattn.  grad_value is a bucketed
 *              gather (count / scan / fill per pixel, then a per-pixel sum in 64-bit fixed point): every product
 *              gout * attn * bilinear weight is rounded to a multiple of the quantum q = max|gout| max(1, max|attn|) 2^-24,
 *              so |error| <= (pairs / 2 + 1) q + fp32 rounding per element (pairs: (sample, corner) pairs on the pixel);
 *              holds for any finite gout / attn.  No float atomics anywhere, the result is independent of the execution
 *              order.  gmax: workspace of two uint32 (max|gout|, max|attn|); ws: workspace of N*M*S*2 + N*M*n_levels*Lq*P*8
 *              int32; a level may have at most 16384 pixels (checked before anything is launched). */
int wc_msda_fwd(const float* value, const int* h_shapes, int n_levels, const float* loc, const float* attn,
                float* out, int N, int Lq, int M, int D, int P, void* stream);
/* The same with the value tensor as f32 or f16 (value_is_f16: half the gather traffic; needs D % 4 == 0 and M*D/4 dividing
 * 256) and an optional fp16 copy of the output (the MFMA operand of MSDeformAttn's output projection); out or out16 may be
 * NULL. */
int wc_msda_fwd_h(const void* value, int value_is_f16, const int* h_shapes, int n_levels, const float* loc,
                  const float* attn, float* out, void* out16, int N, int Lq, int M, int D, int P, void* stream);
int wc_msda_bwd(const float* value, const int* h_shapes, int n_levels, const float* loc, const float* attn,
                const float* gout, float* gvalue, float* gloc, float* gattn, void* gmax, void* ws, int N, int Lq, int M,
                int D, int P, void* stream);
/* The same with value and / or the output gradient gout as f16 (*_is_f16) and the value gradient as f32 (gvalue) and / or
 * f16 (gvalue16: the operand of the value projection's gradient GEMMs); either of the two may be NULL. */
int wc_msda_bwd_h(const void* value, int value_is_f16, const int* h_shapes, int n_levels, const float* loc,
                  const float* attn, const void* gout, int gout_is_f16, float* gvalue, void* gvalue16, float* gloc,
                  float* gattn, void* gmax, void* ws, int N, int Lq, int M, int D, int P, void* stream);

/* Depth-wise conv2d (stride 1, zero "same" padding k/2, odd k <= 7) of the MRFP block of the ViT-CoMer inserts
 * (nn.Conv2d(C, C, k, padding=k//2, groups=C); no reference code).  x, y, dy, dx: (N, C, H, W) f32;
 * w, dw: (C, 1, k, k); bias, db: (C) (bias / db may be NULL); part: workspace N*C*(k*k+1) f32. */
int wc_dwconv_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int k,
                  void* stream);
int wc_dwconv_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, float* part,
                  int N, int C, int H, int W, int k, void* stream);

/* ---- ViT-CoMer spatial-prior conv stem on token rows (no reference code) ---- */
/* Activations are rows x[(n*H + y)*W + x][c] (NHWC).  A 3x3 / stride-s / pad-1 convolution = wc_im2col3x3 + wc_gemm_f16
 * against Wmat[o][(ky*3+kx)*C + c] = w[o][c][ky][kx] (zero padded to Kp); its input gradient = wc_gemm_f16 (dY W) +
 * wc_col2im3x3 (a deterministic gather).  wc_groupnorm_relu_*: nn.GroupNorm(G, C) followed by ReLU, all reductions in
 * a fixed order.  stats: N*G*2 f32 (mean, rstd); part: N*ceil(HW/64)*G*2 f32; gpart like part; cpart:
 * N*ceil(HW/64)*C*2 f32; gsum: N*G*2 f32. */
int wc_im2col3x3(const float* x, void* cols_hi, void* cols_lo, int N, int H, int W, int C, int stride, int Kp,
                 void* stream);
int wc_col2im3x3(const float* dcols, float* dx, int N, int H, int W, int C, int stride, int Kp, void* stream);
int wc_groupnorm_relu_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, float* part,
                          int N, int HW, int C, int G, float eps, void* stream);
int wc_groupnorm_relu_bwd(const float* x, const float* y, const float* dy, const float* stats, const float* gamma,
                          float* dx, float* dgamma, float* dbeta, float* gpart, float* cpart, float* gsum, int N,
                          int HW, int C, int G, void* stream);

/* ---- multi-scale + flip inference and the confusion histogram ----------------------------- */
/* test_msc_flip_coco.py:61-96 (`validate`: [img, flip] at every scale, flip-average, mean over scales, bilinear to
 * the label size, argmax) and utils/evaluate.py:10-16 (_fast_hist), per image, on the device.
 * wc_scale_flip_pair: dst (2,C,Hd,Wd) = [bilinear(src (C,Hs,Ws)), its horizontal flip]; scale_y/x = the source step
 *                     per destination pixel (in/out for F.interpolate(size=), 1/s for F.interpolate(scale_factor=s));
 *                     plain copy + flip when nothing is resized.
 * wc_flip_avg:        out (C,Hd,Wd) = (accumulate ? out : 0) + weight * (R(segs[0]) + flip(R(segs[1]))) / 2 with
 *                     segs (2,C,Hs,Ws) and R = F.interpolate(size=(Hd,Wd), bilinear, align_corners=False).
 * wc_resize_argmax:   pred (Hd,Wd) int64 = argmax_c R(seg (C,Hs,Ws)); the (C,Hd,Wd) logits are never materialised.
 * wc_confusion_hist:  hist (nc,nc) int64 += counts of (true, pred) pairs over n pixels whose true label is in
 *                     [0,nc); *flag is set to 1 if a prediction is outside [0,nc) (int32, caller-zeroed). */
int wc_scale_flip_pair(const float* src, float* dst, int C, int Hs, int Ws, int Hd, int Wd, float scale_y,
                       float scale_x, void* stream);
int wc_flip_avg(const float* segs, float* out, int C, int Hs, int Ws, int Hd, int Wd, float weight, int accumulate,
                void* stream);
int wc_resize_argmax(const float* seg, long* pred, int C, int Hs, int Ws, int Hd, int Wd, void* stream);
int wc_confusion_hist(const long* label_true, const long* label_pred, long* hist, int* flag, long n, int nc,
                      void* stream);

/* Fused forms of the two calls above for the CTI configurations ((n_levels, P) = (3, 4) or (1, 4); wc_msda_fused_supported
 * returns 1): the sampling locations and soft-maxed weights are computed inside the forward kernel from the raw rows
 * ow (N*Lq, ld) = [M*nL*P*2 offsets | M*nL*P logits] of the fused sampling_offsets | attention_weights Linear, their biases
 * (optional) and the reference points ref (Lq, nl_ref, 2); loc / attn are written for the backward.  The backward writes the
 * gradient of the raw rows as the f16 GEMM operand dow16 (N*Lq, ld), padding columns zeroed. */
int wc_msda_fused_supported(int n_levels, int M, int D, int P);
int wc_msda_fwd_f(const void* value, int value_is_f16, const int* h_shapes, int n_levels, const float* ow, int ld,
                  const float* bias_off, const float* bias_aw, const float* ref, int nl_ref, float* loc, float* attn,
                  float* out, void* out16, int N, int Lq, int M, int D, int P, void* stream);
int wc_msda_bwd_f(const void* value, int value_is_f16, const int* h_shapes, int n_levels, const float* loc,
                  const float* attn, const void* gout, int gout_is_f16, float* gvalue, void* gvalue16, void* dow16,
                  int ld, void* gmax, void* ws, int N, int Lq, int M, int D, int P, void* stream);

/* ---- fused glue of the ViT-CoMer insert engine (csrc/comer.hip; no reference code exists: ViT_CoMer.pdf §3.2-3.3) ---- */
/* MRFP's depth-wise convolutions on token rows x (N, S, C) f32, S = sum of the n_levels maps h_shapes = {H0, W0, H1, W1, ...}:
 * 3x3 filters w3 (C/2, 9) + b3 on channels [0, C/2), 5x5 filters w5 (C/2, 25) + b5 on [C/2, C), zero padding, all levels in
 * one launch.  y (f32, may be NULL) = conv + bias; g16 (f16, may be NULL) = GELU(y) (erf form), the next FC's operand. */
int wc_mrfp_dwconv_fwd(const float* x, const float* w3, const float* b3, const float* w5, const float* b5, float* y,
                       void* g16, const int* h_shapes, int n_levels, int N, int C, void* stream);
/* Backward: dy (f16 if dy_is_f16 else f32); dx32 / dx16 (either may be NULL) = gradient w.r.t. x; dw3 / db3 / dw5 / db5 =
 * alpha * filter / bias gradients (two-stage fixed-order reduction); part: workspace of n_parts * C * 26 floats with n_parts
 * from wc_mrfp_dwconv_parts (HOST out-parameter). */
int wc_mrfp_dwconv_parts(const int* h_shapes, int n_levels, int N, int C, long* n_parts);
int wc_mrfp_dwconv_bwd(const void* dy, int dy_is_f16, const float* x, const float* w3, const float* w5, float* dx32, void* dx16,
                       float* dw3, float* db3, float* dw5, float* db5, float* part, float alpha, const int* h_shapes,
                       int n_levels, int N, int C, void* stream);
/* MSDeformAttn's sampling_offsets | attention_weights outputs ow (N*Lq, ld) [M*nL*P*2 offsets, then M*nL*P logits per row]
 * -> loc (N,Lq,M,nL,P,2) = ref + offset / (W_l, H_l) and attn (N,Lq,M,nL,P) = softmax over nL*P.  ref (Lq, nl_ref, 2),
 * nl_ref = 1 (one point for all levels) or n_levels.  bias_off (M*nL*P*2) / bias_aw (M*nL*P), optional: the two Linears'
 * biases, added here when the fused GEMM ran without one. */
int wc_msda_prep_fwd(const float* ow, const float* bias_off, const float* bias_aw, const float* ref, float* loc, float* attn,
                     const int* h_shapes, int n_levels, int N, int Lq, int M, int P, int ld, int nl_ref, void* stream);
/* Its backward: dow (N*Lq, ld) as f32 and / or f16 from the gradients of loc and attn; columns >= 3*M*nL*P are zeroed. */
int wc_msda_prep_bwd(const float* gloc, const float* gattn, const float* attn, float* dow32, void* dow16,
                     const int* h_shapes, int n_levels, int N, int Lq, int M, int P, int ld, void* stream);
/* dst[b][r][0:C] (f16; row stride ld_dst, batch stride s_dst) = src[b][r][0:C] (f32 if src_is_f32 else f16; ld_src, s_src). */
int wc_rows_copy_f16(const void* src, int src_is_f32, void* dst, int B, int R, int C, long ld_src, long s_src,
                     long ld_dst, long s_dst, void* stream);
/* dst[b][r][0:C] (f32, dense rows of C, batch stride s_dst) += alpha * src[b][r][0:C] (f32; ld_src, s_src). */
int wc_rows_add_f32(const float* src, float* dst, int B, int R, int C, long ld_src, long s_src, long s_dst, float alpha,
                    void* stream);

/* Gradients of the gated CTI output projection v1 = v + gamma * (o1 Wop^T + bop) from the un-gated weight-gradient products
 * G (C, K) = dv1^T o1 and gs (C) = dv1^T 1:  dWop = diag(gamma) G, dbop = gamma * gs, dgamma = rowsum(Wop * G) + bop * gs
 * (all f32; no reference code: ViT_CoMer.pdf section 3.3, the gate of the CNN -> ViT injection). */
int wc_cti_gate_grads(const float* G, const float* gs, const float* gamma, const float* Wop, const float* bop, float* dWop,
                      float* dbop, float* dgamma, int C, int K, void* stream);

/* ---- device-side input pipeline ------------------------------------------------------------ */
/* datasets/transforms.py:26-49 (random_scaling), :70-84 (random_fliplr), :119-176 (random_crop, zero padding),
 * :8-15 (normalize_img) + HWC->CHW (datasets/voc.py:137-143) for a batch in one gather kernel.
 * src_u8 (B,Hs,Ws,3) uint8; params: B records of 8 x 32 bit {float scale; int flip, rh, rw, pad_y, pad_x, crop_y, crop_x}
 * (device memory; the random draws are made on the host); dst (B,3,crop,crop) f32; mean3 / std3: HOST float[3];
 * coeff_ws: device scratch of *n_ints ints as reported by wc_augment_workspace_ints(B, crop, &n_ints) (the per-coordinate filter tables).
 * The rescale is Pillow's Image.BILINEAR for 8-bit images reproduced exactly (transforms.py:41: triangle filter of support
 * max(in/out, 1), double-precision coefficients rounded to 22-bit fixed point, uint8 rounding after the horizontal and after
 * the vertical pass).  PRECONDITION, checked on the device: in/out <= 4 on both axes (Hs <= 4 rh, Ws <= 4 rw; the reference's
 * rescale_range is [0.5, 2.0]).  The filter tables hold 9 taps; an output coordinate that would need more makes every pixel
 * it touches NaN instead of applying a truncated (non-Pillow) filter.  data.DeviceAugment also rejects it on the host when
 * the params are host-resident. */
int wc_augment_workspace_ints(int B, int crop, long* n_ints);       /* HOST out-parameter */
int wc_augment_normalize(const void* src_u8, const void* params, float* dst, int* coeff_ws, int B, int Hs, int Ws, int crop,
                         const float* mean3, const float* std3, void* stream);
/* The same chain for a batch of images of DIFFERENT sizes, as files of VOC / COCO are (datasets/voc.py:48-67, :160-180 and
 * datasets/coco.py:54-76, :156-167 hand every image to the transforms at its own size; datasets/transforms.py:26-49, :70-84,
 * :119-176, :8-15 as above).  src_u8: src_bytes bytes, the images uint8 HWC back to back; offsets (B) int64: byte offset of
 * each image (a multiple of 3); sizes (B,2) int32 {H, W}; both tables are device memory, like params.  The kernels are the
 * ones of wc_augment_normalize instantiated with a per-image extent (csrc/augment_shape.h): a batch of equal sizes gives the
 * same bits.  The workspace is wc_augment_workspace_ints(B, crop): it does not depend on the source sizes.
 * Checked on the device: an image with H or W outside [1, 16384], an offset that is negative or no multiple of 3, or an
 * extent beyond src_bytes is not read at all and its output is NaN; in/out <= 4 as above. */
int wc_augment_normalize_ragged(const void* src_u8, long src_bytes, const int64_t* offsets, const int* sizes, const void* params,
                                float* dst, int* coeff_ws, int B, int crop, const float* mean3, const float* std3, void* stream);
/* The un-augmented path (aug=False: datasets/transforms.py:8-15 normalize_img + HWC->CHW, datasets/voc.py:137-143, :247-249;
 * the label as the collated LongTensor of a stock DataLoader): src_u8 (H,W,3) uint8 -> dst (3,H,W) f32; lab_u8 (H,W) uint8 ->
 * dst_label (H,W) int64, both NULL when there is no label.  mean3 / std3: HOST double[3] -- numpy evaluates
 * (uint8 - float) / float in double precision and rounds once into the float32 array; this does the same. */
int wc_normalize_u8(const void* src_u8, const void* lab_u8, float* dst, int64_t* dst_label, int H, int W, const double* mean3,
                    const double* std3, void* stream);

/* Label-aware variant for the fully supervised model (csrc/augment_seg.hip): the chain of
 * `VOC12SegDataset.__transforms` (datasets/voc.py:216-251) = _img_rescaling(image, label) when enabled (datasets/transforms.py:35-51:
 * PIL BILINEAR image, PIL NEAREST label) -> random_fliplr(image, label) (:75-88) -> PhotoMetricDistortion (:178-264) ->
 * random_crop(image, label) (:119-176, label padded with ignore_index, crop box from get_random_cropbox :137-156) ->
 * normalize_img (:8-15) + HWC->CHW, with every random draw made on the host and nothing read back.
 * src_u8 (B,Hs,Ws,3) / lab_u8 (B,Hs,Ws) uint8.  params: B records of 16 x 32 bit (device memory)
 *   {float scale; int flip, rh, rw, pad_y, pad_x; int photo; float beta, alpha_c, alpha_s; int hue; int reserved[5]}
 *   photo: bit 0 brightness, 1 contrast, 2 saturation, 3 hue gate; bit 4 = `mode` (1: contrast before saturation, :247-251);
 *   beta / alpha_c / alpha_s: the random.uniform amounts as float32 (`convert`, :191-195, works in float32); hue in [-18, 18).
 * cand (B, n_cand, 2) int32 {H_start, W_start}: the candidate boxes in draw order.  For every candidate the classes of the
 * label inside the window (flipped, rescaled, padded) are counted; the first with n_valid > 0 and 4 * max_count < 3 * n_valid
 * is taken (np.max(cnt) / np.sum(cnt) < 0.75 over the non-ignored classes, :150-154), else the last one.
 * Out: dst (B,3,crop,crop) f32; dst_label (B,crop,crop) int64; sel (B,4) int32 {H_start, W_start, chosen candidate, accepted};
 * img_box (B,4) int32 as :162-166.  ws: *n_ints ints from wc_seg_augment_workspace_ints.  canvas_max: upper bound of
 * max(crop, rh, rw) over the batch (sizes the per-coordinate tables).
 * Saturation / hue use OpenCV's 8-bit COLOR_BGR2HSV / COLOR_HSV2BGR (mmcv.bgr2hsv / hsv2bgr) as restated in tests/photo_ref.py,
 * applied to the RGB triple as if it were BGR like the reference does.
 * PRECONDITIONS, refused with WC_ERR_ARG: n_cand in [1,16], crop in [1,4096], crop <= canvas_max <= 65536, Hs, Ws <= 16384,
 * ignore_index in [0,255].  Checked on the device (records are device memory): candidates are clamped into the canvas;
 * rh / rw outside [1, canvas_max] or down-scaling beyond 4x make the image NaN, as wc_augment_normalize does. */
int wc_seg_augment_workspace_ints(int B, int crop, int canvas_max, int n_cand, long* n_ints);       /* HOST out-parameter */
int wc_seg_augment(const void* src_u8, const void* lab_u8, const void* params, const int* cand, float* dst, int64_t* dst_label,
                   int* sel, int* img_box, int* ws, int B, int Hs, int Ws, int crop, int canvas_max, int n_cand, int ignore_index,
                   const float* mean3, const float* std3, void* stream);
/* wc_seg_augment for a batch of images of different sizes (datasets/voc.py:253-271, datasets/coco.py:232-239: every image and
 * its label map reach `__transforms` at their own size).  src_u8 / offsets / sizes as wc_augment_normalize_ragged; lab_u8: the
 * label maps (H,W) uint8 packed in the same order, image b's map at byte offsets[b] / 3, so the buffer holds at least
 * src_bytes / 3 bytes.  canvas_max: max(crop, rh, rw) over the batch, which also sizes the workspace
 * (wc_seg_augment_workspace_ints: no term depends on the source sizes, so it serves both forms).  Same kernels as
 * wc_seg_augment (csrc/augment_shape.h).  An image that fails the device check of wc_augment_normalize_ragged comes out as
 * NaN with an all-ignore label. */
int wc_seg_augment_ragged(const void* src_u8, const void* lab_u8, long src_bytes, const int64_t* offsets, const int* sizes,
                          const void* params, const int* cand, float* dst, int64_t* dst_label, int* sel, int* img_box, int* ws,
                          int B, int crop, int canvas_max, int n_cand, int ignore_index, const float* mean3, const float* std3,
                          void* stream);
/* The candidate histogram + select stage of wc_seg_augment alone (transforms.py:137-156, :162-166): sel and img_box only. */
int wc_seg_crop_select(const void* lab_u8, const void* params, const int* cand, int* sel, int* img_box, int* ws, int B, int Hs,
                       int Ws, int crop, int canvas_max, int n_cand, int ignore_index, void* stream);
/* n uint8 triples through the 8-bit BGR -> HSV (inverse = 0) or HSV -> BGR (inverse = 1) conversion used above. */
int wc_hsv8_convert(const void* src_u8, void* dst_u8, long n, int inverse, void* stream);

/* ---- dense CRF (csrc/dcrf.hip; DESIGN.md "Dense CRF") -------------------------------------------------------------- */
/* utils/dcrf.py (`DenseCRF`, `crf_inference`, `crf_inference_label`: pydensecrf's DenseCRF2D with one Gaussian and one
 * bilateral Potts term) as the EXACT mean-field inference of the fully connected CRF (no permutohedral lattice; parity
 * with pydensecrf: unpinned).  Pixel i = y * W + x; img (H,W,3) HWC, uint8 (img_is_u8 = 1) or f32; every (C,H,W) plane set
 * is f32.  k_pos(i,j) = exp(-|p_i - p_j|^2 / (2 pos_xy_std^2)), k_bil(i,j) = exp(-|p_i - p_j|^2 / (2 bi_xy_std^2)
 * - |c_i - c_j|^2 / (2 bi_rgb_std^2)), summed over every j (j = i included); S_m(i) = sum_j k_m(i,j), n_m = S_m^-1/2.
 * Q0 = softmax(-U); each iteration Q = softmax_l(-U + sum_m w_m n_m(i) sum_j k_m(i,j) n_m(j) Q(l,j)).
 * Limits (WC_ERR_ARG, nothing launched): 1 <= C <= 128, 1 <= H*W <= 640*640, every std finite and > 0, iter_max >= 0,
 * weights finite and >= 0, non-null pointers.
 * Error model of a message element M_m(l,i) = n_m(i) sum_j k_m(i,j) n_m(j) Q(l,j) against fp64:
 *   |M - M64| <= eps * M64 + 2^-24 with eps = 2^-10 (all terms are non-negative).  Bilateral: f32 features, exponent from
 *   exact feature differences, v_exp_f32, f32-input MFMA, per-64-key-tile then running f32 sums (bound ~2^-11.3 at 640^2).
 *   Gaussian: separable passes truncated at R = ceil(pos_xy_std sqrt(60 ln 2)) (dropped mass < 2^-29 S_pos(i), also in
 *   S_pos itself), f32 taps.  Deterministic: no atomics, bit-identical results from run to run.
 * wc_dcrf_unary_prob:   unary (C,H,W) = -ln clamp(probs (C,H,W), 1e-5, 1)   (pydensecrf.utils.unary_from_softmax).
 * wc_dcrf_unary_label:  labels (H,W) int64: unary = -ln gt_prob where l == label, else -ln((1 - gt_prob) / (C - 1))
 *                       (labels outside [0,C) get the second value for every l); 0 < gt_prob < 1, C >= 2.
 * wc_dcrf_unary_logits: logits (C,h,w) -> F.interpolate to (H,W) (bilinear, align_corners=False), softmax over C, clamp,
 *                       -ln: the crf_proc composition of test_msc_flip_voc.py:153-157; the resized logits are never written.
 * wc_dcrf_workspace_floats: *n_floats (HOST out-parameter) = H*W*(12 + 2*CP + 3*C), CP = 32*ceil(C/32): the f32 workspace
 *                       `ws` of the two calls below.
 * wc_dcrf_inference:    Q (C,H,W) after iter_max mean-field updates (iter_max = 0: softmax(-U)).
 * wc_dcrf_message:      for the given Q (C,H,W): msg_pos / msg_bil (C,H,W) = M_pos / M_bil, S (2,H,W) = [S_pos, S_bil]. */
int wc_dcrf_unary_prob(const float* probs, float* unary, int C, int H, int W, void* stream);
int wc_dcrf_unary_label(const int64_t* labels, float* unary, int C, int H, int W, float gt_prob, void* stream);
int wc_dcrf_unary_logits(const float* logits, float* unary, int C, int h, int w, int H, int W, void* stream);
int wc_dcrf_workspace_floats(int C, int H, int W, long* n_floats);
int wc_dcrf_inference(const void* img, int img_is_u8, const float* unary, float* Q, void* ws, int C, int H, int W,
                      int iter_max, float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, void* stream);
int wc_dcrf_message(const void* img, int img_is_u8, const float* Q, float* msg_pos, float* msg_bil, float* S, void* ws,
                    int C, int H, int W, float pos_xy_std, float bi_xy_std, float bi_rgb_std, void* stream);

/* ---- dense CRF, lattice bilateral term (csrc/dcrf_lattice.hip; DESIGN.md "Dense CRF", "The lattice") --------------- */
/* utils/dcrf.py wraps pydensecrf, which filters the bilateral term on the permutohedral lattice (Adams, Baek, Davis 2010).
 * These entries are that filter (d = 5, features (x, y) / bi_xy_std and (R, G, B) / bi_rgb_std) as an OPT-IN second way to the
 * bilateral message; the wc_dcrf_* entries above stay exact.  The algorithm is the one restated in fp64 by
 * tests/dcrf_lattice_ref.py: fp64 build (weights stored f32), splat, d + 1 blur passes new = old + (n1 + n2) / 2 over the
 * vertices the image touches, slice with alpha = 1 / (1 + 2^-d).  Built by sorting packed vertex keys: no hash table, no float
 * atomics, bit-identical from call to call.
 * Key bound: a key packs the d stored coordinates at 12 bits each.  With c_max = ((W-1) / bi_xy_std) s_0, ((H-1) / bi_xy_std) s_1,
 *   (256 / bi_rgb_std) s_2..4 and s_j = sqrt(2/3) (d+1) / sqrt((j+1)(j+2)), the elevated coordinate e_j = sum_{m>=j} c_m - j c_{j-1}
 *   satisfies |e_j| <= E = max_j max(sum_{m>=j} c_max,m, j c_max,j-1); a vertex or blur-neighbour coordinate is within 20 of it.
 *   E + 20 <= 2047 is required (WC_ERR_ARG otherwise, nothing launched).  Colours outside [0, 256] (f32 images) are clamped for the
 *   keys and set flag = 1.
 * Limits (WC_ERR_ARG, nothing launched): those of wc_dcrf_inference, the key bound, 1 <= M <= 6 H W, non-null pointers.
 * Error model of a filter or message element against the fp64 restatement: |M - M64| <= eps * M64 + 2^-24, eps = 2^-10
 *   (f32 weights, f32 splat / blur / slice sums in fixed order, at most 6 * 3^6 terms, all non-negative up to weight rounding).
 * wc_dcrf_lattice_key_bound:       *h_bound (HOST) = E + 20 for the given shape and stds; WC_ERR_ARG when it exceeds 2047.
 * wc_dcrf_lattice_workspace_bytes: HOST out-parameters: bytes of the structure `lat` (depends on H W only) and of the f32
 *                                  workspace `ws` of the three calls below.
 * wc_dcrf_lattice_build:           img (H,W,3) -> lat.  lat begins with int32 meta[16]: meta[0] = M (unique vertices), meta[1] =
 *                                  flag.  The host may read these once to size `vals`; nothing else is read back.
 * vals: 2 * (M + 1) * CP f32, CP = 32 * ceil(C / 32): the value rows and their ping-pong partner.  M is passed back by the host;
 *                                  a call whose M differs from meta[0] writes nothing.
 * wc_dcrf_lattice_filter:          out (C,H,W) = the un-normalised filter of in (C,H,W).
 * wc_dcrf_lattice_message:         the outputs of wc_dcrf_message with M_bil = n filter(n Q), n = (filter(1) + 1e-20)^-1/2,
 *                                  S[1] = filter(1) (about half the exact S_bil; the symmetric normalisation absorbs it).
 * wc_dcrf_lattice_inference:       wc_dcrf_inference with that bilateral message; the image and the bilateral stds are in lat. */
int wc_dcrf_lattice_key_bound(int H, int W, float bi_xy_std, float bi_rgb_std, double* h_bound);
int wc_dcrf_lattice_workspace_bytes(int C, int H, int W, long* h_lat_bytes, long* h_ws_bytes);
int wc_dcrf_lattice_build(const void* img, int img_is_u8, void* lat, int H, int W, float bi_xy_std, float bi_rgb_std,
                          void* stream);
int wc_dcrf_lattice_filter(const void* lat, const float* in, float* out, float* vals, void* ws, int C, int H, int W, long M,
                           void* stream);
int wc_dcrf_lattice_message(const void* lat, const float* Q, float* msg_pos, float* msg_bil, float* S, float* vals, void* ws,
                            int C, int H, int W, long M, float pos_xy_std, void* stream);
int wc_dcrf_lattice_inference(const void* lat, const float* unary, float* Q, float* vals, void* ws, int C, int H, int W, long M,
                              int iter_max, float pos_w, float pos_xy_std, float bi_w, void* stream);

/* ---- dense energy loss (csrc/energy.hip) ------------------------------------------------------ */
/* utils/losses.py:52-116 (`DenseEnergyLossFunction`, `DenseEnergyLoss`) with the `bilateralfilter_batch` call of :75 as the
 * EXACT all-pairs sum (the extension's permutohedral lattice is not built by these entries -- the opt-in lattice entries
 * follow below --; parity with the extension: unpinned).  Pixel i = y * W + x;
 * images (N,3,H,W) f32 on the 0..255 scale, segs P (N,K,H,W) f32, rois (N,H,W) f32 in {0,1}, unlabel_u8 (N,H,W) bytes
 * (non-zero = unlabelled).  k_n(i,j) = exp(-|p_i - p_j|^2 / (2 sigma_xy^2) - |I_n,i - I_n,j|^2 / (2 sigma_rgb^2)), j = i
 * included; S = P * ROI; AS(n,k,i) = sum_j k_n(i,j) S(n,k,j); Gate = ROI - max_k P, then 1 where unlabelled, then 0 where
 * negative; A = Gate * AS; loss = -(1/N) sum_{n,k,i} S A.
 * Limits (WC_ERR_ARG, nothing launched): non-null pointers, 1 <= N <= 65535, 1 <= K <= 128, 1 <= H*W <= 640*640, sigmas
 * finite and > 0.  No allocation, no host synchronisation, every launch on `stream`.
 * Error model of an element of AS against fp64: |AS - AS64| <= eps * sum_j k |S_j| + 2^-24, eps = 2^-10 (the arithmetic of
 * the dense CRF's bilateral message above).  Deterministic: no atomics, fixed-order sums, bit-identical from run to run.
 * wc_energy_workspace_floats: *n_floats (HOST out-parameter) = N * (H*W*(8 + CP) + ceil(H*W / 128)), CP = 32*ceil(K/32): the
 *                       f32 workspace `ws` of the two calls below (features, the pixel-major operand, loss partials).
 * wc_bilateral_filter_batch: losses.py:75 alone: AS (N,K,H,W) of segs as given (no ROI, no Gate; segs may be signed).
 * wc_dense_energy_fwd:  losses.py:55-84: A (N,K,H,W) = Gate * AS, gate (N,H,W), loss (1) f32.
 * wc_dense_energy_bwd:  losses.py:87-91: grad_segs (N,K,H,W) = (-2/N) * grad_out[0] * A * ROI, grad_out (1) f32 in DEVICE
 *                       memory.  The Gate is a constant here, as in the reference. */
int wc_energy_workspace_floats(int N, int K, int H, int W, long* n_floats);
int wc_bilateral_filter_batch(const float* images, const float* segs, float* AS, void* ws, int N, int K, int H, int W,
                              float sigma_rgb, float sigma_xy, void* stream);
int wc_dense_energy_fwd(const float* images, const float* segs, const float* rois, const void* unlabel_u8, float* A, float* gate,
                        float* loss, void* ws, int N, int K, int H, int W, float sigma_rgb, float sigma_xy, void* stream);
int wc_dense_energy_bwd(const float* A, const float* rois, const float* grad_out, float* grad_segs, int N, int K, int H, int W,
                        void* stream);

/* ---- dense energy loss, lattice filter (csrc/energy_lattice.hip) ----------------------------- */
/* (Added to the paragraph above: "the extension's permutohedral lattice is not built" was true of the exact entries and still
 * is; these entries are the opt-in second way.  Parity with the extension itself stays unpinned: it is not shipped.)
 * utils/losses.py:75 with the filter as the permutohedral lattice (Adams, Baek, Davis 2010; d = 5), un-normalised, as the
 * lineage's `bilateralfilter` extension uses it: per image n, AS(n) = filter(build(image_n, H, W, sigma_xy, sigma_rgb), S(n))
 * of tests/dcrf_lattice_ref.py (forward blur order 0..d, alpha = 1 / (1 + 2^-d)), composed with the loss, Gate and gradient of
 * tests/energy_ref.py in tests/energy_lattice_ref.py.  Shapes, S, Gate, A and loss as for the exact entries above; the backward
 * is the unchanged wc_dense_energy_bwd / wc_energy_prep_bwd (the factor 2 is an approximation here: the lattice filter is not a
 * symmetric matrix).  The lattice AS is about half the exact AS: a weight tuned for one does not carry
 * over to the other.
 * The images are read as NCHW f32 (no HWC copy); every build decision is made in fp64; colours outside [0, 256] are clamped
 * for the key and reported by OR-ing 1 into int32 meta[1] of `lat`, which the caller may read whenever it likes (the entries
 * never do).  `lat` begins with int32 meta[16 + N]: meta[0] = M of the last image, meta[1] = the flag, meta[16 + n] = M (the
 * number of lattice vertices) of image n.  M never crosses to the host: the kernels read it on the device, their grids cover
 * the worst case M <= 6 H W (every pixel touches d + 1 = 6 vertices) and workgroups beyond M exit at once.  The images go one
 * after another through one shared structure.  No allocation, no host synchronisation, every launch and every rocPRIM call
 * on `stream`: an entry can be captured into a graph and replayed on other contents.  No floating-point atomics, fixed-order
 * sums: bit-identical from run to run.
 * Limits (WC_ERR_ARG, nothing launched): those of the exact entries (non-null pointers, 1 <= N <= 65535: N is looped over
 * inside the entry, but the shared operand kernel keeps the image index in its grid; 1 <= K <= 128, 1 <= H*W <= 640*640,
 * sigmas finite and > 0), lat and ws 256-byte aligned, and wc_dcrf_lattice_key_bound(H, W, sigma_xy, sigma_rgb) <= 2047,
 * checked on the host before any launch.
 * Error model of an element of AS against the fp64 restatement: |AS - AS64| <= eps * filter64(|S|) + 2^-24, eps = 2^-10.
 * wc_energy_lattice_workspace_bytes: HOST out-parameters, the only source of sizes.  With HW = H*W, NE = 6*HW, CP = 32*ceil(K/32),
 *     XC = NE/256 + 2 (integer division) and every piece rounded up to 256 bytes:
 *     lat_bytes = 4*(16 + N) + 4*NE*6 + 8*NE*2 + 8*(NE+1) + 4*(NE+2) + 4*XC*2 + 48*(NE+1) + rocPRIM's temporary storage
 *                 (the larger of a 60-bit pair sort and a scan of NE entries);
 *     ws_bytes  = 4 * (8*N*HW + N*HW*CP + N*ceil(HW/32) + 2*(NE+1)*CP + XC*CP): features, operand, loss partials, the two value
 *                 row sets of ONE image (the worst case, 100 MB at 256x256 and CP = 32) and the long-segment partial rows.
 * wc_bilateral_filter_batch_lattice: wc_bilateral_filter_batch with that filter (segs may be signed).
 * wc_dense_energy_fwd_lattice: wc_dense_energy_fwd with that filter: A = Gate * AS, gate, loss. */
int wc_energy_lattice_workspace_bytes(int N, int K, int H, int W, long* h_lat_bytes, long* h_ws_bytes);
int wc_bilateral_filter_batch_lattice(const float* images, const float* segs, float* AS, void* lat, void* ws, int N, int K, int H,
                                      int W, float sigma_rgb, float sigma_xy, void* stream);
int wc_dense_energy_fwd_lattice(const float* images, const float* segs, const float* rois, const void* unlabel_u8, float* A,
                                float* gate, float* loss, void* lat, void* ws, int N, int K, int H, int W, float sigma_rgb,
                                float sigma_xy, void* stream);

/* ---- dense energy loss as a term of the training step (csrc/energy_prep.hip) ------------------ */
/* get_energy_loss (utils/losses.py:35-50) on F.interpolate(seg, (H,W), bilinear, align_corners=False) followed by
 * DenseEnergyLoss.forward (:102-111) at scale_factor = 2^-e, e in {0,1,2}, around the unchanged wc_dense_energy_fwd: the
 * up-sampled logits, their soft-max and the full-resolution gradient are never written.  Hs = H >> e, Ws = W >> e.
 * Limits (WC_ERR_ARG, nothing launched): non-null pointers (img_box may be NULL), 1 <= K <= 128, 0 <= e <= 2, Hs, Ws >= 1,
 * Hs*Ws <= 640*640, W <= 8192, 1 <= N <= 65535 / ceil(K/32).  No allocation, no host synchronisation, every launch on `stream`; no
 * atomics, fixed-order sums: bit-identical from run to run.
 * wc_energy_prep_fwd: img (N,3,H,W) f32 normalised, seg (N,K,h,w) f32, label (N,H,W) int64, img_box (N,4) int32 rows
 *                     (y0, y1, x0, x1) in DEVICE memory, 16-byte aligned, or NULL = the whole image; mean, std: 3 HOST floats.
 *                     Out, at the scaled size: images_s (N,3,Hs,Ws) = img * std + mean (two roundings) at the nearest source
 *                     (Y << e, X << e); rois_s (N,Hs,Ws) = 1 inside the box at the nearest source, else 0; unlabel_u8 (N,Hs,Ws)
 *                     = 1 where the low byte of the label at the nearest source is 255; P_s (N,K,Hs,Ws) = the bilinear
 *                     down-sample of soft-max_k of the up-sampled logits.  |P_s - P64| <= (16 max|logit| + K + 16) * 2^-24.
 * wc_energy_prep_workspace_floats: *n_floats (HOST out-parameter) = 2*N*K*h*W: the workspace of wc_energy_prep_bwd.
 * wc_energy_prep_bwd: A (N,K,Hs,Ws) as wc_dense_energy_fwd wrote it, rois_s as above, seg as above, coef a host float
 *                     (-2 * weight / N) -> grad_seg (N,K,h,w): G_s = coef * A * rois_s pulled back through the down-sample,
 *                     the soft-max Jacobian (soft-max recomputed) and the up-sample.  The Gate is a constant. */
int wc_energy_prep_fwd(const float* img, const float* seg, const int64_t* label, const int* img_box, const float* mean,
                       const float* std, float* images_s, float* P_s, float* rois_s, void* unlabel_u8, int N, int K, int h, int w,
                       int H, int W, int e, void* stream);
int wc_energy_prep_workspace_floats(int N, int K, int h, int W, long* n_floats);
int wc_energy_prep_bwd(const float* A, const float* rois_s, const float* seg, float* grad_seg, void* ws, float coef, int N, int K,
                       int h, int w, int H, int W, int e, void* stream);

/* ---- CLIP text tower (csrc/text.hip; DESIGN.md "Text tower") -------------------------------------------------------- */
/* wc_text_embed:      clip/model.py:393-395 (token_embedding(text) + positional_embedding) and :403 (`text.argmax(-1)`).
 *                     tokens (N, Lctx) int32; tok_emb (V, W) f32; pos (>= L, W) f32.  eot (N) int32 = index of the first
 *                     maximum id of each row (over all Lctx ids); x (N*L, W) f32 = rows 0..L-1 of every prompt, or NULL
 *                     (then L must be 0: only eot and the flag).  *bad (int32) = 1 if any id lies outside [0, V), else 0;
 *                     such ids read embedding row 0 (never out of bounds) and the caller raises.
 * wc_attn_fwd_causal: clip/myAtt.py:21-64 with the causal `attn_mask` of clip/model.py:333,375-381 (-inf above the
 *                     diagonal, myAtt.py:57-58): qkv as for wc_attn_fwd (q pre-scaled by log2(e)/sqrt(DH)); out (N*L, E)
 *                     fp16; optional out32 (N*L, E) f32, lse (N, H, L) f32 (base 2), mean (N, L, L) f32 = head-mean
 *                     probabilities, exactly 0 above the diagonal.  1 <= L <= 128, DH == 64, H >= 1; qkv, out, out32
 *                     16-byte aligned.
 * wc_text_pool:       clip/model.py:399-403: feat (N, Ed) f32 = LayerNorm(x[n*L + eot[n]]; ln_w, ln_b, eps) @ proj (W, Ed)
 *                     in fp32; x (N*L, W) f32 (eot clamped to [0, L)).  W <= 8192.
 * wc_text_zeroshot:   WeCLIP_model/model_attn_aff_voc.py:34-46 (`zeroshot_classifier` after encode_text): feat (C*T, Ed)
 *                     f32, T rows per class -> out (C, Ed) f32 = normalise(mean_t(normalise(feat row))).  Ed <= 8192. */
int wc_text_embed(const int* tokens, int N, int Lctx, const float* tok_emb, int V, const float* pos, int W, int L,
                  float* x, int* eot, int* bad, void* stream);
int wc_attn_fwd_causal(const void* qkv, void* out, float* out32, float* lse, float* mean, int N, int L, int H, int DH,
                       void* stream);
int wc_text_pool(const float* x, const int* eot, int N, int L, int W, const float* ln_w, const float* ln_b, float eps,
                 const float* proj, int Ed, float* feat, void* stream);
int wc_text_zeroshot(const float* feat, int C, int T, int Ed, float* out, void* stream);

/* ---- stand-alone CAM generation (csrc/preprocess.hip) ----------------------------------------- */
/* wc_clip_preprocess: clip/generate_cams_voc12.py:76-93 (`_transform_resize`, `img_ms_and_flip`; the same lines of
 *   generate_cams_coco14.py): Resize((h, w), BICUBIC) -> ToTensor -> Normalize(mean, std), and torch.flip(image, [-1]).
 *   src_u8 (B,H0,W0,3) uint8 HWC RGB, every image of one source size.  dst (B,3,h,w) f32; dst_flip (B,3,h,w) f32 or NULL;
 *   out_u8 (B,h,w,3) uint8 or NULL: the image after the resize alone.  The resize is Pillow's 8-bit
 *   `Image.resize((w, h), BICUBIC)` (Resample.c: separable, horizontal pass first into a uint8 intermediate; window
 *   support = 2 * max(1, in / out) around (x + 0.5) * in / out; cubic kernel with a = -0.5; weights normalised in double
 *   precision, then 22-bit fixed point rounded half away from zero; pixel = clip8((2^21 + sum w_i p_i) >> 22)), bit for bit.
 *   Then x / 255, - mean, / std as three separately rounded fp32 operations.  mean3 / std3: HOST arrays of 3 floats.
 *   ws: *n_bytes bytes of device memory from wc_clip_preprocess_workspace_bytes (weight tables + the intermediate);
 *   ws_bytes: the size of the buffer passed, refused with WC_ERR_ARG when it is smaller than that.
 *   Limits (WC_ERR_ARG, nothing launched): B in [1,65535], every size in [1,16384], down-scaling by at most 8 per axis.
 * wc_cam_scale_resize_f16: pytorch_grad_cam/utils/image.py:51-61 (`scale_cam_image([cam], (ori_w, ori_h))`) followed by the
 *   dumpers' `.astype(np.float16)` (generate_cams_voc12.py:198,215).  cam (P, gh*gw) f32, P (image, class) pairs of one
 *   token grid; per pair m = min, (v - m) / (1e-7 + (max - m)) in fp32, bilinear resize to the pair's own (ori_h, ori_w):
 *   src = max((dst + 0.5) * in / out - 0.5, 0), second tap clamped (OpenCV INTER_LINEAR on a float image), in fp32, stored
 *   as fp16 (round to nearest even).  sizes (P,2) int32 {ori_h, ori_w}, offsets (P) int64 = first element of pair p in
 *   out_f16 (both device memory); out_elems = number of fp16 elements of out_f16 (nothing is written outside it);
 *   max_pixels >= max_p ori_h * ori_w sizes the grid.  gh * gw <= 4096, P <= 65535.
 * wc_cam_resize_f32: the bilinear resize alone, f32 -> f32 (`cv2.resize(grayscale_cam, (ori_w, ori_h))`,
 *   generate_cams_voc12.py:159, and GradCAM.__call__(target_size=...)); same tables. */
int wc_clip_preprocess_workspace_bytes(int B, int H0, int W0, int h, int w, long* n_bytes);          /* HOST out-parameter */
int wc_clip_preprocess(const void* src_u8, float* dst, float* dst_flip, void* out_u8, void* ws, long ws_bytes, int B, int H0, int W0, int h,
                       int w, const float* mean3, const float* std3, void* stream);
int wc_cam_scale_resize_f16(const float* cam, const int* sizes, const int64_t* offsets, void* out_f16, long out_elems, int P, int gh,
                            int gw, int max_pixels, void* stream);
int wc_cam_resize_f32(const float* cam, const int* sizes, const int64_t* offsets, float* out, long out_elems, int P, int gh, int gw,
                      int max_pixels, void* stream);

/* ---- training driver: validation histograms and the step metric (csrc/trainlog.hip) ----------- */
/* wc_val_pair_hist: one validated image of scripts/dist_clip_voc.py:71-102 in one launch.  seg (C,Hs,Ws) f32 low-resolution
 *   logits, cam (Hl,Wl) int64 or NULL, gt (Hl,Wl) int64.  Over the pixels with 0 <= gt < nc:
 *   seg_hist[gt*nc + p] += 1 with p = argmax_c bilinear(seg)[c] (align_corners=False, scale = in / out, first maximum wins:
 *   the value wc_resize_argmax writes, which is never stored here) and, when cam is given, cam_hist[gt*nc + cam] += 1.
 *   A p or cam value outside [0, nc) is skipped in its own histogram and sets flag[0] (wc_confusion_hist's contract).
 *   seg_hist / cam_hist (nc,nc) int64, accumulated with integer atomics (per-workgroup LDS histograms while both fit in
 *   64 KiB, global atomics otherwise); cam_hist may be NULL when cam is.  nc <= 4096.
 * wc_label_match_count: the pseudo_seg_mAcc of :274-277.  seg (B,C,Hs,Ws) f32, label (B,H,W) int64 (255 = ignore, which no
 *   arg-max equals).  counts int64[2] is OVERWRITTEN: counts[0] = #pixels with argmax_c bilinear(seg)[c] == label,
 *   counts[1] = B*H*W.  The entry zeroes counts on `stream` and launches one kernel: no allocation, no host read, so it may
 *   be called while `stream` is being captured into a HIP graph.
 * wc_step_pair_hist: the confusion counts of one supervised train step, wc_val_pair_hist's seg leg over a batch.  seg
 *   (B,C,Hs,Ws) f32 low-resolution logits, label (B,H,W) int64 ground-truth masks.  Over the pixels with 0 <= label < nc:
 *   hist[label*nc + p] += 1 with p = argmax_c bilinear(seg[b])[c] on the (H,W) grid (the arithmetic above).  Every other label
 *   value (255, negative, >= nc) is skipped; p >= nc (C > nc) is skipped and sets flag[0].  hist (nc,nc) int64 is ADDED to and
 *   never zeroed: the caller owns the window.  Integer atomics only (per-workgroup LDS histogram while nc*nc*4 <= 64 KiB,
 *   global atomics otherwise; the counts of a wave's leading cell are summed across its lanes and added once), so the result
 *   does not depend on their order.  One launch, no allocation, no host read: capturable into a HIP graph.  nc <= 4096. */
int wc_val_pair_hist(const float* seg, const long* cam, const long* gt, long* seg_hist, long* cam_hist, int* flag, int C, int Hs,
                     int Ws, int Hl, int Wl, int nc, void* stream);
int wc_label_match_count(const float* seg, const long* label, long* counts, int B, int C, int Hs, int Ws, int H, int W,
                         void* stream);
int wc_step_pair_hist(const float* seg, const long* label, long* hist, int* flag, int B, int C, int Hs, int Ws, int H, int W,
                      int nc, void* stream);

/* ---- evaluation entry point: the per-image tail (csrc/evalfinish.hip) -------------------------- */
/* wc_eval_finish: one evaluated image of test_msc_flip_voc.py:92-107 in one launch over the (Hl,Wl) label grid.
 *   seg1 (C,Hs,Ws) f32 scale-1 logits; msc (C,Hs,Ws) f32 multi-scale average on the same grid, or NULL; cam (Hl,Wl) int64 or
 *   NULL; gt (Hl,Wl) int64 or NULL.  p1 / pm = argmax_c bilinear(seg1 / msc)[c] (align_corners=False, scale = in / out, first
 *   maximum wins: the value wc_resize_argmax writes, bit for bit).  Outputs, each NULL-able and written for EVERY pixel:
 *   pred1_u8 / predm_u8 (Hl,Wl) uint8 = p1 / pm; cmap_rgb (Hl,Wl,3) uint8 HWC = the PASCAL VOC colour (utils/imutils.py:136-154
 *   `colormap`, computed from the label) of pm, of p1 when msc is NULL.  Over the pixels with 0 <= gt < nc:
 *   hist[gt*nc + p1] += 1, msc_hist[gt*nc + pm] += 1, cam_hist[gt*nc + cam] += 1, each (nc,nc) int64 and NULL-able (cam given
 *   with gt needs cam_hist; predm_u8 / msc_hist need msc); a prediction or CAM value outside [0, nc) is skipped in its own
 *   histogram and sets flag[0] (wc_confusion_hist's contract).  Integer atomics; the entry puts as many of the counted
 *   histograms as fit 64 KiB into per-workgroup LDS cells and counts the rest with global atomics (same counts either way).
 *   C <= 256 (the maps are uint8), nc <= 4096: WC_ERR_ARG otherwise, nothing launched.
 * wc_label_finish: the same outputs for a ready int64 arg-max map (the CRF leg, :158-161).  pred (H,W) int64, gt (H,W) int64
 *   or NULL; out_u8 (H,W) uint8 and cmap_rgb (H,W,3) uint8, each NULL-able; hist (nc,nc) int64, required with gt.  A pred
 *   outside [0, 255] is written as 255 and sets flag[0]; a pred outside [0, nc) where 0 <= gt < nc is skipped and sets flag[0]. */
int wc_eval_finish(const float* seg1, const float* msc, const long* cam, const long* gt, void* pred1_u8, void* predm_u8,
                   void* cmap_rgb, long* hist, long* msc_hist, long* cam_hist, int* flag, int C, int Hs, int Ws, int Hl, int Wl,
                   int nc, void* stream);
int wc_label_finish(const long* pred, const long* gt, void* out_u8, void* cmap_rgb, long* hist, int* flag, int H, int W, int nc,
                    void* stream);

/* ---- predict entry point: the per-image tail without a label map (csrc/predict.hip) ------------ */
/* wc_predict_finish: one predicted image in one launch over its own (H,W) grid: the resize + arg-max of
 *   test_msc_flip_voc.py:92-96, or the arg-max of the CRF's Q of :146-161, the colour image of utils/imutils.py:136-154, and
 *   the confidence of the arg-max, which the reference does not keep.
 *   src (C,Hs,Ws) f32: mode 0 logits on the model's grid, mode 1 probabilities with Hs == H and Ws == W (the CRF's Q).
 *   image (H,W,3) uint8 HWC or NULL.  Per pixel v_c = bilinear(src)[c] (align_corners=False, scale = in / out), best = the first
 *   maximum over c: the value wc_resize_argmax / wc_eval_finish write, bit for bit.  conf = 1 / sum_c exp(v_c - v_best) (mode 0,
 *   f32, one pass with a running maximum) or clamp(v_best, 0, 1) (mode 1); conf8 = (int)(255 * conf + 0.5f).  Written label =
 *   best, or 255 where ignore_below > 0 and conf8 < ignore_below.  Outputs, each NULL-able, written for EVERY pixel:
 *   pred_u8 (H,W) uint8 = the written label; cmap_rgb (H,W,3) uint8 = its PASCAL VOC colour; conf_u8 (H,W) uint8 = conf8
 *   (never affected by ignore_below); overlay_rgb (H,W,3) uint8 = (alpha256 * colour + (256 - alpha256) * image + 128) >> 8 per
 *   channel (needs image).  stats int64[2C + 1], ADDED to and never zeroed: [c] += pixels whose written label is c,
 *   [C + c] += the sum of their conf8, [2C] += ignored pixels.  Integer atomics only (32-bit LDS cells per workgroup, flushed
 *   once): two calls give the same bits.  64-bit pixel indices.  One launch, no allocation, no host read.
 *   WC_ERR_ARG, nothing launched: src NULL; C outside [1,255] (255 is the ignore label); a size <= 0; mode outside {0,1};
 *   mode 1 with another grid; alpha256 outside [0,256]; ignore_below outside [0,255]; overlay_rgb without image. */
int wc_predict_finish(const float* src, const unsigned char* image, void* pred_u8, void* cmap_rgb, void* conf_u8,
                      void* overlay_rgb, long* stats, int C, int Hs, int Ws, int H, int W, int mode, int alpha256, int ignore_below,
                      void* stream);

/* ---- the AFA pseudo-label chain of utils/camutils.py (csrc/camlabel.hip) ----------------------- */
/* Every entry checks its limits first and returns WC_ERR_ARG with nothing launched; everything runs on `stream`; no entry
 * allocates, reads device memory on the host or uses an atomic (two calls on the same input give the same bits).
 * A box is a row (y0, y1, x0, x1) of int32 in device memory, applied as the Python slices [y0:y1, x0:x1] are (clamped to the
 * axis, a negative bound counted from its end).
 * wc_aff_propagate: utils/camutils.py:249-275 (with_bkg = 0) and :277-317 (with_bkg = 1), the random walk of the CAMs over the
 *   learned affinity.  aff (B,n,n) f32, read once and NOT modified (the reference zeroes it in place); mask (n,n) f32 or NULL;
 *   cams (B,C,n) f32; cls (B,C) f32, needed with with_bkg and ignored without; out (B,C+with_bkg,n) f32.
 *     A[b,i,j] = (aff[b,i,j] * [mask[i,j] != 0])^2,  s[b,j] = sum_i A[b,i,j],  out[b,k,j] = (sum_i X[b,k,i] A[b,i,j]) / (s[b,j] + eps)
 *   with_bkg = 1: eps = 1e-1, rows k in {0} + {1 + c : cls[b,c] != 0}, X = soft-max over exactly those rows of [bkg_score, cams],
 *   every other row of out is 0.  with_bkg = 0: eps = 1e-4, X = cams.  f32-input MFMA products, |error| <= 2^-20 of the value.
 *   ws: *n_floats floats from wc_aff_propagate_workspace_floats (the operand X, transposed and padded).
 *   Limits: non-null pointers, B in [1,65535], n in [1,4096], C + with_bkg in [1,128], finite bkg_score.
 * wc_cam_to_label: utils/camutils.py:8-28.  cam (B,C,H,W) f32, cls (B,C) f32, box (B,4) or NULL, label (B,H,W) int64,
 *   valid_cam (B,C,H,W) f32 = cls * cam or NULL.  v = max_c cls * cam (the first maximum wins), label = 1 + argmax, 0 where
 *   v <= bkg_score; with a box and ignore_mid: ignore_index where v <= high_thre, then 0 where v <= low_thre; with a box:
 *   ignore_index outside it.  Without a box the thresholds of ignore_mid are not applied, as in the reference (:17-18).
 * wc_box_ignore: utils/camutils.py:30-37.  label / out (B,H,W) int64 (is_f32 = 0) or f32 (is_f32 = 1): ignore_index outside the box.
 * wc_bkg_refine_prep / wc_bkg_refine_finish: utils/camutils.py:149-198 on either side of ONE refinement call for the batch.
 *   meta (B, 1 + Kmax) int32 per image: its channel count nch in [1,Kmax], then the label value of each channel (0 = background,
 *   1 + class, ascending).  prep: cams (B,C,H,W) -> stack (B, 2 Kmax, h2, w2): per pixel of the (h2,w2) grid the bilinear
 *   (align_corners=False) down-sample of the image's channels, the background being the constant high_thre (first half) or
 *   low_thre (second half), and the soft-max over the image's nch channels; channels >= nch are 0.  finish: stack as refined,
 *   bilinear up-sample to (H,W) of both halves, arg-max over nch channels (first maximum), label values lh / ll through meta;
 *   out (B,H,W) f32 = lh where lh != 0, ignore_index where lh == 0, 0 where lh == ll == 0, ignore_index outside the box.
 * wc_box_gather / wc_box_scatter: utils/camutils.py:200-223 for G images whose boxes have one size (hb,wb).  meta (G, 3 + Kg)
 *   int32 per member: image index, y0, x0 of the (already clamped) box, the channel of each compact slot or -1.  gather:
 *   cams_out (G,Kg,hb,wb) = the crop of the listed channels, 0 in padding slots; img_out (G,3,hb/2,wb/2) = the bilinear
 *   (align_corners=False) down-sample of the image crop.  scatter: out[image, channel, box] = src (G,Kg,hb,wb); out is zeroed by
 *   the caller.  A member that does not fit (B,C,H,W) is skipped.  hb, wb >= 2. */
int wc_aff_propagate_workspace_floats(int B, int n, int C, int with_bkg, long* n_floats);           /* HOST out-parameter */
int wc_aff_propagate(const float* aff, const float* mask, const float* cams, const float* cls, float* out, void* ws, int B, int n,
                     int C, float bkg_score, int with_bkg, void* stream);
int wc_cam_to_label(const float* cam, const float* cls, const int* box, long* label, float* valid_cam, int B, int C, int H, int W,
                    float bkg_score, float high_thre, float low_thre, int ignore_mid, long ignore_index, void* stream);
int wc_box_ignore(const void* label, const int* box, void* out, int B, int H, int W, int is_f32, long ignore_index, void* stream);
int wc_bkg_refine_prep(const float* cams, const int* meta, float* stack, int B, int C, int H, int W, int h2, int w2, int Kmax,
                       float high_thre, float low_thre, void* stream);
int wc_bkg_refine_finish(const float* stack, const int* meta, const int* box, float* out, int B, int H, int W, int h2, int w2,
                         int Kmax, float ignore_index, void* stream);
int wc_box_gather(const float* cams, const float* images, const int* meta, float* cams_out, float* img_out, int G, int B, int C,
                  int H, int W, int hb, int wb, int Kg, void* stream);
int wc_box_scatter(const float* src, const int* meta, float* out, int G, int B, int C, int H, int W, int hb, int wb, int Kg,
                   void* stream);

/* ---- training image panels of utils/imutils.py (csrc/panels.hip) ------------------------------ */
/* Every entry paints B tiles of (H,W) pixels straight into `out`, a (3,canvas_h,canvas_w) uint8 CHW canvas that the caller has
 * zeroed: the grid of `torchvision.utils.make_grid(nrow, padding=2, pad_value=0)` (utils/imutils.py:30,38,49,83,131) without a
 * grid pass.  Tile k0 + i (i = 0..B-1, k = k0 + i) has its first pixel at
 *   (oy + (k / xmaps) * (H + pad), ox + (k % xmaps) * (W + pad)),   with colmajor != 0 at
 *   (oy + (k % xmaps) * (H + pad), ox + (k / xmaps) * (W + pad)):   tiles run down the columns first, the net effect of the two
 * transposes of tensorboard_attn (:79 `permute([0,3,2,1])`, :83 `.permute(0,2,1)`).  Only the tiles' bytes are written.  Each
 * entry checks that every tile lies inside the canvas and returns WC_ERR_ARG with nothing launched otherwise; no entry
 * allocates or reads device memory on the host.  A float becomes a uint8 by truncation toward zero (`.type(torch.uint8)`).
 * mean3 / std3: HOST arrays of 3 floats.
 * wc_panel_images: utils/imutils.py:11-18 (`denormalize_img`) + :30.  img (B,3,H,W) f32; pixel = uint8(x * std + mean), the
 *   product and the sum rounded separately in fp32.
 * wc_panel_labels: utils/imutils.py:7-9 (`encode_cmap`) + :125-133 (`tensorboard_label`).  label (B,H,W) int64 (is_u8 = 0; taken
 *   modulo 256) or uint8 (is_u8 = 1) -> the PASCAL VOC colour of :136-154, 255 -> (224,224,192).
 * wc_panel_heat: the heat-map tiles of utils/imutils.py:32-38 (`tensorboard_image`'s overlay), :44-47 (`tensorboard_edge`) and
 *   :59-79 (`tensorboard_attn`).  Image b's source is C maps of (h,w) f32 at src + b * sB + c * sC (elements).  Per pixel:
 *   bilinear up-sampling to (H,W) (aligned = 0: align_corners=False, scale = in / out; aligned = 1: align_corners=True), the
 *   maximum over the C maps (a NaN wins), then with minmax != NULL (device workspace of 3 * B floats, written by a reduction
 *   launch of this entry) x = (x - min_b) / (max_b - min_b) over image b's up-sampled map (:71-76; a constant map gives 0 / 0),
 *   then matplotlib's look-up of cmap (0 jet, 1 viridis): entry int(x * 256), x == 1 -> 255, x < 0 -> 0, x > 1 -> 255, NaN ->
 *   (0,0,0).  img == NULL: pixel = uint8(lut * 255) (fp64).  img (B,3,H,W) f32: pixel = uint8(0.5 * lut * 255 + 0.5 * u), u =
 *   wc_panel_images' pixel, in fp64 (:37).
 * wc_panel_snapshot: what a later render of a train step needs, copied out of the step's memory in ONE launch (no allocation,
 *   no memset, no host read: capturable into a HIP graph).  seg_out[0..n_seg) = seg; label_out[0..n_label) uint8 = the low
 *   byte of label (int64; torch's cast); with attn (B,hw,hw) f32 != NULL: rows_out (B,4,hw) = attn[b, rows4[q], :], rows4 a
 *   HOST array of the 4 rows tensorboard_attn reads (:64).  label 16-byte, label_out 4-byte aligned. */
int wc_panel_images(const float* img, const float* mean3, const float* std3, int B, int H, int W, void* out, int canvas_h,
                    int canvas_w, int oy, int ox, int xmaps, int pad, int colmajor, int k0, void* stream);
int wc_panel_labels(const void* label, int is_u8, int B, int H, int W, void* out, int canvas_h, int canvas_w, int oy, int ox,
                    int xmaps, int pad, int colmajor, int k0, void* stream);
int wc_panel_heat(const float* src, long sB, long sC, int C, int h, int w, int aligned, float* minmax, int cmap,
                  const float* img, const float* mean3, const float* std3, int B, int H, int W, void* out, int canvas_h,
                  int canvas_w, int oy, int ox, int xmaps, int pad, int colmajor, int k0, void* stream);
int wc_panel_snapshot(const float* seg, long n_seg, const long* label, long n_label, const float* attn, int B, int hw,
                      const int* rows4, float* seg_out, void* label_out, float* rows_out, void* stream);

/* ---- multi-bandwidth RBF MMD loss of utils/mmdloss.py (csrc/mmd.hip) ---------------------------- */
/* source, target (B, d) row-major, both f32 (is_half = 0) or both fp16 (is_half = 1); X = cat(source, target), N = 2 B rows.
 * All arithmetic in f32 (sums that cross rows in f64).  With L2_ij = |x_i - x_j|^2:
 *   bandwidth = fix_sigma, or sum_ij L2_ij / (N^2 - N) when fix_sigma == 0 (utils/mmdloss.py:25-28; formed as
 *   2 sum_i |x_i - mean|^2 / (N - 1), no N x N pass), then / kernel_mul^(kernel_num / 2) (:30); bw_b = bandwidth * kernel_mul^b
 *   (:31); K_ij = sum_b exp(-L2_ij / bw_b) (:33-35); W_ij = sum_b exp(-L2_ij / bw_b) / bw_b.
 * The bandwidth is a device scalar and never read on the host.  With a_i = x_i minus the mean of its own block (source or
 * target) and delta = source mean - target mean, L2 is formed on the f32-input MFMA as |a_i|^2 + |a_j|^2 - 2 a_i.a_j inside a
 * block and (|a_i|^2 + 2 s_i delta.a_i) + (|a_j|^2 + 2 s_j delta.a_j) + |delta|^2 - 2 a_i.a_j across the blocks, clamped at 0,
 * and is exactly 0 on the diagonal (K_ii = kernel_num exactly): neither a common offset of the data nor the distance between
 * the two sets enters a cancellation.  kernel_mul == 2
 * takes one exponential and kernel_num - 1 squarings, every other kernel_mul kernel_num exponentials.
 * Limits (WC_ERR_ARG "bad argument", nothing launched): non-null pointers (grad may be NULL), 1 <= B <= 2^20, 1 <= d <= 8192,
 * 1 <= kernel_num <= 8, kernel_mul finite and > 0, fix_sigma finite, ws 256-byte aligned.  No allocation, no host
 * synchronisation, every launch on `stream`; no atomics, fixed-order sums: bit-identical from run to run.  All rows identical
 * with fix_sigma == 0: bandwidth 0 and a NaN loss, as in the reference.
 * Error model against fp64 on the same inputs, eps = 2^-16: |loss - loss64| <= eps * A + 2^-24, A = (1/B^2) sum_ij K_ij;
 * |K_ij - K64_ij| <= eps * K64_ij + 2^-24; |g_ic - g64_ic| <= eps * G_ic + 2^-24,
 * G_ic = (4/B^2) (sum_j W_ij |x_ic| + sum_j W_ij |x_jc|).
 * wc_mmd_workspace_bytes: *n_bytes (HOST out-parameter), with dp = 32 ceil(d/32), nt = ceil(N/64), js = min(nt, max(1, 1024/nt))
 *                    and every piece rounded up to 256 bytes: 8*64*dp + 8*nt*js + 8*dp + 4*N + 4*N + 68 + 4*N*dp: O(N d + tiles).
 * wc_mmd_rbf:        utils/mmdloss.py:38-59 for n == m == B: loss (1) f32 = (1/B^2) sum_ij s_i s_j K_ij, s = +1 on source rows,
 *                    -1 on target rows.  grad (N, d) f32 or NULL: rows 0..B-1 = d loss / d source, rows B..N-1 = d loss / d target,
 *                    with the bandwidth a constant as in the reference (:28 `.data`):
 *                    grad_i = -(4/B^2) s_i ((sum_j s_j W_ij) x_i - sum_j s_j W_ij x_j).  With grad the d columns are processed in
 *                    chunks of 128, S = X X^T recomputed per chunk; without it the second product is skipped and only the upper
 *                    triangle of tiles is visited.
 * wc_mmd_rbf_kernel: utils/mmdloss.py:4-35: K (N, N) f32, symmetric bit for bit. */
int wc_mmd_workspace_bytes(int B, int d, long* n_bytes);
int wc_mmd_rbf(const void* source, const void* target, int is_half, float* loss, float* grad, void* ws, int B, int d,
               int kernel_num, double kernel_mul, double fix_sigma, void* stream);
int wc_mmd_rbf_kernel(const void* source, const void* target, int is_half, float* K, void* ws, int B, int d, int kernel_num,
                      double kernel_mul, double fix_sigma, void* stream);

/* ---- CAM seeds: threshold sweep, seed label maps and their scores (csrc/camseed.hip) ----------- */
/* Common inputs: cam_f16 (P, HW) fp16, the bucket buffer of clip/generate_cams.py (the (image, class) pairs of an image
 * consecutive; 16-byte aligned base, a pair itself only 2-byte aligned when HW is odd); first (B+1) int32 = first pair of every
 * image; keys (P) int32 = 0-based foreground class id of every pair, distinct within an image, in any order; gt_u8 (B, HW)
 * uint8 (4-byte aligned base).  All device memory.  Per pixel v = max_k cam[k] and c = 1 + the class id attaining it, the
 * smallest class id on a tie: the arg-max over the class axis of the dense `cls_label * cam` of utils/camutils.py:11-14 (equal
 * to it for maps >= 0, which scale_cam_image's are).  fp16 widens to f32 exactly; every comparison is f32.
 * Every entry: integer atomics only, no allocation, no host read, limits checked before anything is launched (WC_ERR_ARG);
 * flag (int32, caller-zeroed) is set by a pair table that leaves [0, P) or gives an image no pair or more than Kmax, by a
 * class id outside [0, nc - 1) and by a slot outside the table; such pixels are not counted.
 * wc_cam_seed_sweep: utils/camutils.py:13-15 (`cam_value <= bkg_score` -> 0: a value equal to the threshold is background) +
 *   utils/evaluate.py:9-16 (`_fast_hist`; gt >= nc skipped) for T thresholds in one pass.  thresholds: HOST array of T floats,
 *   finite and strictly ascending, 1 <= T <= 64; 2 <= nc <= 256; Kmax >= the largest number of pairs of an image.  With
 *   j* = #{j : t_j < v}: bins[gt][c][j*] += 1, bins (nc, nc, T+1) int64, ADDED to and never zeroed.  Per-workgroup 32-bit LDS
 *   cells over (gt, the image's slot, j*) while they and the thresholds fit 64 KiB (nc * Kmax * (T+1) * 4 + 256 bytes), flushed by
 *   64-bit global atomics; global
 *   atomics per pixel otherwise or with force_global != 0 (same counts).  1 <= HW <= 2^28, 1 <= B <= 65535.
 * wc_cam_seed_sweep_path: *use_lds (HOST out-parameter) = 1 when the sweep stages in LDS for (nc, Kmax, T).
 *   The per-threshold confusion matrices follow from bins by two cumulative sums (clip/cam_seeds.py confusion_from_bins).
 * wc_cam_seed_labels: the two slot maps of the per-image body of utils/camutils.py:55-79 at the image's own size:
 *   lab_low / lab_high (B, HW) int64 (what wc_dcrf_unary_label reads) = 1 + rank of c's class id among the image's ids
 *   ascending (:56 `nonzero`) where v > low_thre / high_thre, else 0 (:61-65: the threshold plane is channel 0 and wins a tie).
 *   At most 255 pairs per image.
 * wc_cam_seed_merge: utils/camutils.py:77-79 for B images in one launch: label_u8 (B, HW) = slot_class[b][high], then 255
 *   where high == 0, then 0 where high == 0 and low == 0; slot_class (B, S) int32, entry 0 = 0, entry s = 1 + the s-th smallest
 *   class id.  On un-refined slot maps this is cam_to_label(..., ignore_mid=True) of :20-22.  cmap_rgb (B, HW, 3) uint8 or NULL:
 *   the VOC colour (utils/imutils.py:136-154).  gt_u8 or NULL; with it `pseudo_scores` (utils/evaluate.py:38-45): hist (nc, nc)
 *   int64 += (gt, label) over gt < nc and label != 255, cover[0] += those pixels, cover[1] += the pixels with gt < nc (int64[2]).
 */
int wc_cam_seed_sweep_path(int nc, int Kmax, int T, int* use_lds);
int wc_cam_seed_sweep(const void* cam_f16, const int* first, const int* keys, const void* gt_u8, const float* thresholds, long* bins,
                      int* flag, int B, int P, long HW, int nc, int T, int Kmax, int force_global, void* stream);
int wc_cam_seed_labels(const void* cam_f16, const int* first, const int* keys, long* lab_low, long* lab_high, int* flag, int B, int P,
                       long HW, float low_thre, float high_thre, void* stream);
int wc_cam_seed_merge(const long* lab_low, const long* lab_high, const int* slot_class, const void* gt_u8, void* label_u8,
                      void* cmap_rgb, long* hist, long* cover, int* flag, int B, long HW, int S, int nc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
