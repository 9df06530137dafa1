// Dense energy loss, second way to the bilateral filter: the permutohedral lattice of csrc/dcrf_lattice.hip in place of the exact
// all-pairs sum of csrc/energy.hip.  Opt-in: the exact sum stays the default.  The reference's utils/losses.py:75 calls a
// `bilateralfilter` extension that is this lattice, used un-normalised, and does not ship it; the filter here is pinned to
// tests/dcrf_lattice_ref.py (build + filter per image) composed with tests/energy_ref.py in tests/energy_lattice_ref.py
// (DESIGN.md section 15.3).
//
// One entry call is: energy_prep_kernel (csrc/energy.hip, unchanged: the operand V (N, HW, CP), the Gate), then image after
// image through ONE shared structure, then energy_finish_kernel (unchanged).  Per image:
//   el_build_kernel  : one thread per pixel reads the three NCHW f32 planes (no HWC copy) and runs lat_point (lattice_shared.h):
//                      fp64 keys and weights, colours outside 0..256 clamped for the key and reported by an integer OR.
//   structure        : lattice_shared::structure, dcrf_lattice.hip's own kernels around rocPRIM's sort and scans.
//   filter_rows      : lattice_shared::filter_rows, dcrf_lattice.hip's splat, extra-chunk splat and blur kernels over V's rows of
//                      this image (segments over 256 entries chunk by chunk; d + 1 ping-pong blur passes, forward order 0..d),
//                      called with M < 0.
//   el_slice_kernel  : 32 lanes own a pixel, a workgroup 32 pixels: AS = alpha sum_r b_r val[vertex_r] (lat_slice_gather,
//                      lattice_shared.h); epilogue A = Gate * AS -> (K, HW) planes and this workgroup's partial of sum S * A
//                      (S re-read from V).
// The vertex count M never reaches the host: every kernel that needs it reads meta[0] on the device, the grids cover the proven
// worst case M <= 6 HW (every pixel touches d + 1 = 6 vertices) and workgroups beyond M exit at the top.  No host
// synchronisation, no allocation, every launch and every rocPRIM call on the caller's stream: an entry can be captured into a
// graph and replayed on other image contents.  No floating-point atomics, fixed-order sums, no loop without a compile-time or
// segment-length bound, no waiting between workgroups (rocPRIM's sort and scan are used as they ship): two calls on the same
// input are bit-identical.  Error model: include/weclip_hip.h (wc_*_lattice of the dense energy loss).
#include "common.h"
#include "energy_shared.h"
#include "lattice_shared.h"

#define EL_PIX 32                 // pixels per slice workgroup: 4 rounds of 8
#define EL_META 16                // meta[0..15] as in dcrf_lattice.hip; meta[16 + n] = M of image n of the last call

// ------------------------------------------------------------------------------------------------ build
// A.img: the R plane of one image; G and B lie HW and 2 HW floats further
__global__ __launch_bounds__(256) void el_build_kernel(BuildArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int HW = A.H * A.W;
    if (i >= HW) return;
    const float* p = (const float*)A.img + i;
    double col[3];
    col[0] = p[0], col[1] = p[HW], col[2] = p[2L * HW];
    const int flag = lat_point(A, i, col);
    if (flag) atomicOr(A.meta + 1, flag);          // an integer OR over all images of the call
}

// ------------------------------------------------------------------------------------------------ slice
struct ElSliceArgs {
    const float* val;         // (M + 1, CP)
    const u32* pixvert;
    const float* bary;
    const float* V;           // (HW, CP) operand of this image
    const float* gate;        // (HW), or null: no gate
    float* out;               // (K, HW)
    float* part;              // (gridDim.x) partials of sum V * out, or null
    int* meta;
    int n, HW, K, CP;
};

template <int CT>
__global__ __launch_bounds__(256) void el_slice_kernel(ElSliceArgs A) {
    __shared__ float red[4];
    const int tid = threadIdx.x, l31 = tid & 31;
    const int HW = A.HW, K = A.K, CP = A.CP;
    float ps = 0.f;
#pragma unroll 1
    for (int it = 0; it < EL_PIX / 8; ++it) {
        const int i = blockIdx.x * EL_PIX + it * 8 + (tid >> 5);
        const int ic = min(i, HW - 1);
        float acc[CT], sv[CT];
#pragma unroll
        for (int k = 0; k < CT; ++k) sv[k] = A.V[(long)ic * CP + 32 * k + l31];
        lat_slice_gather<CT>(A.val, A.pixvert, A.bary, ic, CP, l31, acc);
        const float g = A.gate ? A.gate[ic] : 1.f;
        if (i < HW) {
#pragma unroll
            for (int k = 0; k < CT; ++k) {
                const int l = 32 * k + l31;
                if (l < K) {
                    const float a = g * (acc[k] * LAT_ALPHA);
                    A.out[(long)l * HW + i] = a;
                    ps = fmaf(sv[k], a, ps);
                }
            }
        }
    }
    if (A.part) {                                           // fixed order: lane chain, xor tree, four waves
        ps = wave_sum(ps);
        if ((tid & 63) == 0) red[tid >> 6] = ps;
        __syncthreads();
        if (tid == 0) A.part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    if (blockIdx.x == 0 && tid == 0) A.meta[EL_META + A.n] = A.meta[0];
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

// f32 workspace: feat 8 N HW | V N HW CP | part N nwg | vals 2 (6 HW + 1) CP | partial (6 HW / 256 + 2) CP, 256-byte pieces
struct ElWs {
    float *feat, *V, *part, *vals, *partial;
    long total;
    int nwg;
};

ElWs el_carve(void* base, long N, int K, long HW) {
    ElWs w;
    const long CP = 32L * ((K + 31) / 32), NE = HW * LAT_D1, XC = NE / LAT_CHUNK + 2;
    float* f = (float*)base;
    long o = 0;
    auto take = [&](long n) { float* r = f + o; o += (n + 63) & ~63L; return r; };
    w.nwg = wc_cdiv(HW, EL_PIX);
    w.feat = take(8 * N * HW);
    w.V = take(N * HW * CP);
    w.part = take(N * w.nwg);
    w.vals = take(2 * (NE + 1) * CP);
    w.partial = take(XC * CP);
    w.total = o;
    return w;
}

long el_meta_bytes(int N) { return 4L * (EL_META + N); }

int el_slice(ElSliceArgs a, int nwg, hipStream_t st) {
    const dim3 grid(nwg), block(256);
    switch (a.CP / 32) {
        case 1: hipLaunchKernelGGL(el_slice_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(el_slice_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(el_slice_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(el_slice_kernel<4>, grid, block, 0, st, a); break;
    }
    WC_LAUNCH_CHECK("el_slice_kernel");
    return WC_OK;
}

// prep, then per image build + filter with the fused epilogue: out (N, K, HW) = gate * AS; partials when `want_part`
int el_run(const char* who, const float* images, const float* segs, const float* rois, const void* unlabel, float* gate, float* out,
           float* loss, void* lat, void* ws, int N, int K, int H, int W, float sigma_rgb, float sigma_xy, hipStream_t st) {
    if (int rc = energy_shared::limits(N, K, H, W, sigma_rgb, sigma_xy, who)) return rc;
    BuildArgs b;
    if (int rc = lattice_shared::check_bound(H, W, sigma_xy, sigma_rgb, b.s, who)) return rc;      // before any launch
    WC_CHECK_ARG((uintptr_t)lat % 256 == 0 && (uintptr_t)ws % 256 == 0, "%s: bad argument: lat and ws must be 256-byte aligned", who);
    const long HW = (long)H * W;
    const int NE = (int)(HW * LAT_D1), CP = 32 * ((K + 31) / 32);
    size_t tb = 0;
    if (int rc = lattice_shared::temp_bytes(NE, &tb, who)) return rc;
    const Lat L = lat_carve(lat, HW, tb, el_meta_bytes(N));
    const ElWs w = el_carve(ws, N, K, HW);
    if (hipMemsetAsync(L.meta, 0, el_meta_bytes(N), st) != hipSuccess) {
        wc_set_error("%s: hipMemsetAsync failed", who);
        return WC_ERR_HIP;
    }
    if (int rc = energy_shared::prep(images, segs, rois, unlabel, w.feat, w.V, gate, N, K, H, W, st)) return rc;
    b.is_u8 = 0, b.H = H, b.W = W, b.xy_std = sigma_xy, b.rgb_std = sigma_rgb;
    b.keys = L.keys[1], b.slots = L.slots[1], b.bary = L.bary, b.meta = L.meta;
    for (int n = 0; n < N; ++n) {
        int idx = wc_prof_begin_always(st);
        b.img = images + (long)n * 3 * HW;
        hipLaunchKernelGGL(el_build_kernel, dim3(wc_cdiv(HW, 256)), dim3(256), 0, st, b);
        WC_LAUNCH_CHECK("el_build_kernel");
        if (int rc = lattice_shared::structure(L, NE, st, who)) return rc;
        wc_prof_end_n(idx, "energy_lattice_build", 0.0, st, 1);
        idx = wc_prof_begin_always(st);
        // M = -1: the vertex count stays on the device
        if (int rc = lattice_shared::filter_rows(L, w.V + (long)n * HW * CP, w.vals, w.partial, HW, CP, -1, st)) return rc;
        ElSliceArgs s;
        s.val = w.vals, s.pixvert = L.pixvert, s.bary = L.bary, s.V = w.V + (long)n * HW * CP;
        s.gate = gate ? gate + (long)n * HW : nullptr, s.out = out + (long)n * K * HW;
        s.part = loss ? w.part + (long)n * w.nwg : nullptr;
        s.meta = L.meta, s.n = n, s.HW = (int)HW, s.K = K, s.CP = CP;
        if (int rc = el_slice(s, w.nwg, st)) return rc;
        wc_prof_end_n(idx, "energy_lattice_filter", 0.0, st, 1);
    }
    if (loss) return energy_shared::finish(w.part, (long)N * w.nwg, -1.0 / N, loss, st);
    return WC_OK;
}

}  // namespace

extern "C" int wc_energy_lattice_workspace_bytes(int N, int K, int H, int W, long* h_lat_bytes, long* h_ws_bytes) {
    const char* who = "wc_energy_lattice_workspace_bytes";
    WC_CHECK_ARG(h_lat_bytes && h_ws_bytes, "%s: bad argument: null pointer", who);
    if (int rc = energy_shared::limits(N, K, H, W, 1.f, 1.f, who)) return rc;
    const long HW = (long)H * W;
    size_t tb = 0;
    if (int rc = lattice_shared::temp_bytes(HW * LAT_D1, &tb, who)) return rc;
    *h_lat_bytes = lat_carve(nullptr, HW, tb, el_meta_bytes(N)).total;
    *h_ws_bytes = 4 * el_carve(nullptr, N, K, HW).total;
    return WC_OK;
}

extern "C" int wc_bilateral_filter_batch_lattice(const float* images, const float* segs, float* AS, void* lat, void* ws, int N, int K,
                                                 int H, int W, float sigma_rgb, float sigma_xy, void* stream) {
    const char* who = "wc_bilateral_filter_batch_lattice";
    WC_CHECK_ARG(images && segs && AS && lat && ws, "%s: bad argument: null pointer", who);
    return el_run(who, images, segs, nullptr, nullptr, nullptr, AS, nullptr, lat, ws, N, K, H, W, sigma_rgb, sigma_xy,
                  (hipStream_t)stream);
}

extern "C" int wc_dense_energy_fwd_lattice(const float* images, const float* segs, const float* rois, const void* unlabel_u8, float* A,
                                           float* gate, float* loss, void* lat, void* ws, int N, int K, int H, int W, float sigma_rgb,
                                           float sigma_xy, void* stream) {
    const char* who = "wc_dense_energy_fwd_lattice";
    WC_CHECK_ARG(images && segs && rois && unlabel_u8 && A && gate && loss && lat && ws, "%s: bad argument: null pointer", who);
    return el_run(who, images, segs, rois, unlabel_u8, gate, A, loss, lat, ws, N, K, H, W, sigma_rgb, sigma_xy, (hipStream_t)stream);
}
