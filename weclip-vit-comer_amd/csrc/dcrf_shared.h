// The parts of csrc/dcrf.hip that csrc/dcrf_lattice.hip runs unchanged: the limits, the separable Gaussian term and the
// operand / initialisation kernels.  Thin host wrappers over dcrf.hip's own kernels (defined at the end of dcrf.hip), so the
// exact path and the lattice path share one Gaussian message and one Q0.
#pragma once
#include "common.h"

namespace dcrf_shared {

// the limits of wc_dcrf_inference (C, H x W, finite stds > 0); `who` prefixes the error text
int limits(int C, int H, int W, float pos_xy_std, float bi_xy_std, float bi_rgb_std, const char* who);
// S_pos -> S (N floats, may be NULL) and n_pos = S_pos^-1/2 -> nrm (N floats)
int pos_norm(int H, int W, float pos_xy_std, float* S, float* nrm, hipStream_t st);
// Gaussian message of the (C, N) planes `in` -> out (C, N), through tmp (C, N)
int gauss_message(int C, int H, int W, float pos_xy_std, const float* in, float* tmp, float* out, hipStream_t st);
// Q0 = softmax(-U), Vb (N, CP) = n_bil Q0, Vp (C, N) = n_pos Q0; nrm = [n_pos (N) | n_bil (N)]
int init(const float* U, const float* nrm, float* Q, float* Vb, float* Vp, int C, int CP, int N, hipStream_t st);
// the same operands from a given Q (C, N)
int operands(const float* Q, const float* nrm, float* Vb, float* Vp, int C, int CP, int N, hipStream_t st);
// msg (C, N) = nrm[i] G
int scale(const float* G, const float* nrm, float* msg, int C, int N, hipStream_t st);

}  // namespace dcrf_shared
