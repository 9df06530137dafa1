// The parts of csrc/energy.hip that csrc/energy_lattice.hip runs unchanged: the limits, the operand / Gate kernel and the loss
// reduction.  Thin host wrappers over energy.hip's own kernels (defined at the end of energy.hip), so the exact path and the
// lattice path share one operand V, one Gate and one fixed-order sum of the partials.
#pragma once
#include "common.h"

namespace energy_shared {

// the limits of wc_dense_energy_fwd (N, K, H x W, finite sigmas > 0); `who` prefixes the error text
int limits(int N, int K, int H, int W, float sigma_rgb, float sigma_xy, const char* who);
// energy_prep_kernel: feat (N, HW, 8), V (N, HW, CP) = P * ROI (rois NULL: P), gate (N, HW) when given (then unlabel too)
int prep(const float* images, const float* segs, const float* rois, const void* unlabel_u8, float* feat, float* V, float* gate,
         int N, int K, int H, int W, hipStream_t st);
// energy_finish_kernel: loss[0] = scale * (part[0] + ... + part[n - 1]), fixed order, f64
int finish(const float* part, long n, double scale, float* loss, hipStream_t st);

}  // namespace energy_shared
