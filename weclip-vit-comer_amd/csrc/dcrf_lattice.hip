// Dense CRF, second way to the bilateral message: the permutohedral lattice (Adams, Baek, Davis 2010; d = 5) that the
// reference's utils/dcrf.py gets from pydensecrf, here without a hash table and without atomics.  Opt-in: the exact all-pairs
// sum of dcrf.hip stays the default.  The algorithm is pinned, op for op in its fp64 part, to tests/dcrf_lattice_ref.py.
//
//   lat_build_kernel  : one thread per pixel, fp64, no FP contraction (the build's -ffp-contract=off): scale, elevate, nearest
//                       zero-remainder point, rank, barycentric weights (stored f32) and the d + 1 vertex keys.  A key packs the
//                       d stored coordinates, 12 bits each with bias 2048, into 60 bits of a uint64.  The host proves before any
//                       launch that every coordinate fits (key_bound below); colours outside 0..256 (float images) are clamped
//                       for the keys and reported through a device flag, so no key is ever corrupt.
//   structure         : rocPRIM radix sort of the (key, slot) pairs (slot = pixel * 6 + vertex; LSD radix sort: stable), head
//                       flags + inclusive scan -> vertex index 1..M of every entry, each vertex's segment of the sorted entries
//                       and its key; a second flag + scan numbers the 256-entry chunks of long segments after their first.  The
//                       2 (d + 1) blur neighbours of a vertex are found by binary search (23 fixed steps) in the sorted unique
//                       keys.  Vertex 0 is "absent": its value row is all zeros, so the blur has no branch.
//   splat             : value rows (M + 1, CP), vertex-major; a group of CP / 4 lanes owns a vertex and a lane 4 channels, and
//                       sums the vertex's segment in sorted order.  Segments longer than 256 entries (a flat image puts 1e5
//                       entries on one vertex) are cut into 256-entry chunks summed by other groups into `partial` rows, which
//                       the owner adds in chunk order.  No float atomics: two calls are bit-identical.
//   blur              : d + 1 ping-pong passes new = old + (n1 + n2) / 2, 16-byte loads of whole rows.
//   slice             : 32 lanes own a pixel; out = alpha sum_r b_r val[vertex_r] (lat_slice_gather, lattice_shared.h); the
//                       inference form fuses dcrf.hip's epilogue (n(i) w_bil, the Gaussian message, -U, the softmax over labels,
//                       the writes of Q and of n Q).
// The structure, splat and blur kernels here are the only ones: csrc/energy_lattice.hip (the dense energy loss) runs them through
// lattice_shared::structure and lattice_shared::filter_rows, defined at the end of this file.  A vertex count M >= 0 in the
// arguments is the one the host read back (this file's entries: a structure whose count differs is left alone); M < 0 means
// that the count stays on the device (the energy loss: grids cover the worst case 6 HW, rows past meta[0] exit).
// The kernels of this file contain no loop without a compile-time or segment-length bound, never wait on another workgroup and
// never retry; rocPRIM's device sort and scan are used as they ship.
// Error model: include/weclip_hip.h (wc_dcrf_lattice_*).
#include "common.h"
#include "dcrf_shared.h"
#include "lattice_shared.h"       // the layout and the device code shared as text with csrc/energy_lattice.hip

#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

// f32 workspace of the filter / message / inference entries: nrm 2N | Vb N CP | Vp, tmp, G 3 C N | partial (NE / 256 + 2) CP
struct LatWs {
    float *nrm, *Vb, *Vp, *tmp, *G, *partial;
    long total;
};

static LatWs ws_carve(void* base, long N, int C) {
    LatWs w;
    const long CP = 32L * ((C + 31) / 32), CN = (long)C * N, XC = N * LAT_D1 / LAT_CHUNK + 2;
    float* f = (float*)base;
    long o = 0;
    auto take = [&](long n) { float* r = f + o; o += (n + 63) & ~63L; return r; };      // 256-byte pieces: float4 access
    w.nrm = take(2 * N);
    w.Vb = take(N * CP);
    w.Vp = take(CN);
    w.tmp = take(CN);
    w.G = take(CN);
    w.partial = take(XC * CP);
    w.total = o;
    return w;
}

// ------------------------------------------------------------------------------------------------ build
__global__ __launch_bounds__(256) void lat_build_kernel(BuildArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.H * A.W) return;
    double col[3];
    if (A.is_u8) {
        const uint8_t* p = (const uint8_t*)A.img + 3L * i;
        col[0] = p[0], col[1] = p[1], col[2] = p[2];
    } else {
        const float* p = (const float*)A.img + 3L * i;
        col[0] = p[0], col[1] = p[1], col[2] = p[2];
    }
    const int flag = lat_point(A, i, col);
    if (flag) A.meta[1] = flag;
}

// head flag of every sorted entry
__global__ __launch_bounds__(256) void lat_head_kernel(const u64* __restrict__ keys, u32* __restrict__ flags, int NE) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    flags[e] = (e == 0 || keys[e] != keys[e - 1]) ? 1u : 0u;
}

// vertex index of every slot; key and segment start of every vertex; M
__global__ __launch_bounds__(256) void lat_vertex_kernel(const u64* __restrict__ keys, const u32* __restrict__ slots,
                                                         const u32* __restrict__ vid, u32* __restrict__ pixvert,
                                                         u64* __restrict__ ukeys, u32* __restrict__ segstart,
                                                         int* __restrict__ meta, int NE) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const u32 v = vid[e];
    const u64 key = keys[e];
    pixvert[slots[e]] = v;
    if (e == 0 || key != keys[e - 1]) {
        ukeys[v] = key;
        segstart[v] = (u32)e;
    }
    if (e == NE - 1) {
        segstart[v + 1] = (u32)NE;
        meta[0] = (int)v;
    }
}

// an entry starts an extra chunk when it lies a positive multiple of LAT_CHUNK past its segment's start
__device__ __forceinline__ bool lat_is_xstart(int e, u32 start) { return (u32)e > start && (((u32)e - start) % LAT_CHUNK) == 0; }

__global__ __launch_bounds__(256) void lat_xflag_kernel(const u32* __restrict__ vid, const u32* __restrict__ segstart,
                                                        u32* __restrict__ flags, int NE) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    flags[e] = lat_is_xstart(e, segstart[vid[e]]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void lat_xchunk_kernel(const u32* __restrict__ vid, const u32* __restrict__ segstart,
                                                         const u32* __restrict__ xid, u32* __restrict__ xstart,
                                                         u32* __restrict__ xvert, int* __restrict__ meta, int NE) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const u32 v = vid[e];
    if (lat_is_xstart(e, segstart[v])) {
        const u32 xi = xid[e] - 1;
        xstart[xi] = (u32)e;
        xvert[xi] = v;
    }
    if (e == NE - 1) meta[2] = (int)xid[e];
}

// blur neighbours: thread per (vertex 0..cap, n = 2 j + s); row 0 and absent neighbours are 0
__global__ __launch_bounds__(256) void lat_nbr_kernel(const u64* __restrict__ ukeys, const int* __restrict__ meta,
                                                      u32* __restrict__ nbr, long cap) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long v = g / LAT_NBR;
    const int n = (int)(g - v * LAT_NBR);
    const int M = meta[0];
    if (v > cap || v > M) return;
    if (v == 0) {
        nbr[n] = 0;
        return;
    }
    const int j = n >> 1;
    // n1: every stored coordinate - 1, coordinate j (< d) + d; n2: the opposite
    long long dp = 0;
#pragma unroll
    for (int k = 0; k < LAT_D; ++k) dp += (long long)(k == j ? LAT_D : -1) << (LAT_BITS * (LAT_D - 1 - k));
    const u64 want = (u64)((long long)ukeys[v] + ((n & 1) ? -dp : dp));
    int lo = 1, hi = M + 1;                         // first index with ukeys[index] >= want
#pragma unroll 1
    for (int it = 0; it < 23; ++it) {               // 2^23 > 6 * 640^2 + 1
        if (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ukeys[mid] < want) lo = mid + 1;
            else hi = mid;
        }
    }
    nbr[v * LAT_NBR + n] = (lo <= M && ukeys[lo] == want) ? (u32)lo : 0u;
}

// ------------------------------------------------------------------------------------------------ operands
// V (N, CP) = nrm[i] in (C, N)   (nrm may be NULL); columns >= C stay as the caller's memset left them
__global__ __launch_bounds__(256) void lat_operand_kernel(const float* __restrict__ in, const float* __restrict__ nrm,
                                                          float* __restrict__ V, int C, int CP, int N) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * N) return;
    const int l = (int)(e / N), i = (int)(e - (long)l * N);
    V[(long)i * CP + l] = nrm ? nrm[i] * in[e] : in[e];
}

// V (N, 32): 1 in column 0
__global__ __launch_bounds__(256) void lat_ones_kernel(float* __restrict__ V, long n) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) V[e] = (e & 31) == 0 ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------ splat

// the chunks of long segments after their first -> partial rows; grid covers the a-priori bound on X
__global__ __launch_bounds__(256) void lat_splat_extra_kernel(SplatArgs A, long cap) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long xi = g / A.q;
    const int c4 = (int)(g - xi * A.q);
    if ((A.M >= 0 && A.meta[0] != A.M) || xi >= cap || xi >= A.meta[2]) return;
    const u32 start = A.xstart[xi];
    const u32 end = min(start + LAT_CHUNK, A.segstart[A.xvert[xi] + 1]);
    A.partial[xi * A.q + c4] = lat_chunk_sum(A, start, end, c4);
}

// val[v] = first chunk + the partial rows in chunk order; val[0] = 0
__global__ __launch_bounds__(256) void lat_splat_kernel(SplatArgs A) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long v = g / A.q;
    const int c4 = (int)(g - v * A.q);
    if (lat_row_idle(A.meta, A.M, v)) return;
    if (v == 0) {
        A.val[c4] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const u32 start = A.segstart[v], endall = A.segstart[v + 1];
    float4 acc = lat_chunk_sum(A, start, min(endall, start + LAT_CHUNK), c4);
    const u32 len = endall - start;
    if (len > LAT_CHUNK) {
        const long x0 = (long)A.xid[start + LAT_CHUNK] - 1;
        const int n = (int)((len - 1) / LAT_CHUNK);
        for (int k = 0; k < n; ++k) {
            const float4 p = A.partial[(x0 + k) * A.q + c4];
            acc.x += p.x, acc.y += p.y, acc.z += p.z, acc.w += p.w;
        }
    }
    A.val[v * A.q + c4] = acc;
}

// ------------------------------------------------------------------------------------------------ blur
__global__ __launch_bounds__(256) void lat_blur_kernel(const float4* __restrict__ in, float4* __restrict__ out,
                                                       const u32* __restrict__ nbr, const int* __restrict__ meta, int j, int q,
                                                       int M) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long v = g / q;
    const int c4 = (int)(g - v * q);
    if (lat_row_idle(meta, M, v)) return;
    const u32 n1 = nbr[v * LAT_NBR + 2 * j], n2 = nbr[v * LAT_NBR + 2 * j + 1];
    const float4 a = in[v * q + c4], b = in[(long)n1 * q + c4], c = in[(long)n2 * q + c4];
    out[v * q + c4] = make_float4(a.x + 0.5f * (b.x + c.x), a.y + 0.5f * (b.y + c.y), a.z + 0.5f * (b.z + c.z),
                                  a.w + 0.5f * (b.w + c.w));
}

// ------------------------------------------------------------------------------------------------ slice
struct SliceArgs {
    const float* val;         // (M + 1, CP)
    const u32* pixvert;
    const float* bary;
    const int* meta;
    int M, N, C, CP;
    int mode;                 // 0: S, n = (S + 1e-20)^-1/2;  1: out = nb ? nb[i] f : f;  2: mean-field update
    float* S;
    float* nrm;               // mode 0: written
    float* out;
    const float* nb;          // modes 1, 2: n_bil
    const float* U;
    const float* G;
    const float* npos;
    float w_bil, w_pos;
    float* Q;
    float* Vb_out;
    float* Vp_out;
};

template <int CT>
__global__ __launch_bounds__(256) void lat_slice_kernel(SliceArgs A) {
    if (A.meta[0] != A.M) return;
    const int l31 = threadIdx.x & 31;
    const int i = blockIdx.x * 8 + (threadIdx.x >> 5);
    const int N = A.N, C = A.C, CP = A.CP;
    const int ic = min(i, N - 1);
    float acc[CT];
    lat_slice_gather<CT>(A.val, A.pixvert, A.bary, ic, CP, l31, acc);
#pragma unroll
    for (int k = 0; k < CT; ++k) acc[k] *= LAT_ALPHA;
    if (A.mode == 0) {
        if (l31 == 0 && i < N) {
            A.S[i] = acc[0];
            A.nrm[i] = rsqrtf(acc[0] + 1e-20f);
        }
        return;
    }
    if (A.mode == 1) {
        const float nb = A.nb ? A.nb[ic] : 1.f;
        if (i < N) {
#pragma unroll
            for (int k = 0; k < CT; ++k) {
                const int l = 32 * k + l31;
                if (l < C) A.out[(long)l * N + i] = nb * acc[k];
            }
        }
        return;
    }
    // dcrf_bil_kernel's mode-2 epilogue
    const float nb = A.nb[ic], np = A.npos[ic];
    const float sb = A.w_bil * nb, sp = A.w_pos * np;
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < CT; ++k) {
        const int l = 32 * k + l31;
        const long o = (long)min(l, C - 1) * N + ic;
        const float z = fmaf(sp, A.G[o], fmaf(sb, acc[k], -A.U[o]));
        acc[k] = l < C ? z : -INFINITY;
        mx = fmaxf(mx, acc[k]);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CT; ++k) {
        acc[k] = __builtin_amdgcn_exp2f((acc[k] - mx) * LAT_LOG2E);
        sum += acc[k];
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = 1.f / sum;
    if (i < N) {
#pragma unroll
        for (int k = 0; k < CT; ++k) {
            const int l = 32 * k + l31;
            if (l < C) {
                const float q = acc[k] * inv;
                A.Q[(long)l * N + i] = q;
                A.Vp_out[(long)l * N + i] = np * q;
                A.Vb_out[(long)i * CP + l] = nb * q;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {

// |e_j| of every stored coordinate for features in [0, max]: e_j = sum_{m >= j} c_m - j c_{j-1} with c >= 0
double key_bound(int H, int W, double xy_std, double rgb_std, double* s_out) {
    double s[LAT_D], cmax[LAT_D];
    for (int j = 0; j < LAT_D; ++j) s[j] = sqrt(2.0 / 3.0) * (LAT_D + 1) / sqrt((double)((j + 1) * (j + 2)));
    cmax[0] = (double)(W - 1) / xy_std * s[0];
    cmax[1] = (double)(H - 1) / xy_std * s[1];
    for (int k = 2; k < LAT_D; ++k) cmax[k] = LAT_CMAX / rgb_std * s[k];
    double E = 0.0;
    for (int j = 0; j < LAT_D; ++j) {
        double up = 0.0;
        for (int m = j; m < LAT_D; ++m) up += cmax[m];
        const double dn = j ? j * cmax[j - 1] : 0.0;
        E = fmax(E, fmax(up, dn));
    }
    if (s_out)
        for (int j = 0; j < LAT_D; ++j) s_out[j] = s[j];
    return E + LAT_MARGIN;
}

int check_bound(int H, int W, float bi_xy_std, float bi_rgb_std, double* s_out, const char* who) {
    WC_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= LAT_MAX_N, "%s: bad argument: H x W = %d x %d outside [1, 640*640] pixels", who,
                 H, W);
    WC_CHECK_ARG(bi_xy_std > 0.f && bi_xy_std < INFINITY && bi_rgb_std > 0.f && bi_rgb_std < INFINITY,
                 "%s: bad argument: standard deviations must be finite and > 0", who);
    const double b = key_bound(H, W, bi_xy_std, bi_rgb_std, s_out);
    WC_CHECK_ARG(b <= LAT_BIAS - 1, "%s: bad argument: lattice key bound %.1f > %d (bi_xy_std = %g, bi_rgb_std = %g at %d x %d)", who,
                 b, LAT_BIAS - 1, (double)bi_xy_std, (double)bi_rgb_std, H, W);
    return WC_OK;
}

int temp_bytes(long NE, size_t* bytes, const char* who) {
    size_t a = 0, b = 0;
    rocprim::double_buffer<u64> dk((u64*)nullptr, (u64*)nullptr);
    rocprim::double_buffer<u32> dv((u32*)nullptr, (u32*)nullptr);
    if (rocprim::radix_sort_pairs(nullptr, a, dk, dv, (size_t)NE, 0, LAT_BITS * LAT_D, (hipStream_t)0) != hipSuccess ||
        rocprim::inclusive_scan(nullptr, b, (u32*)nullptr, (u32*)nullptr, (size_t)NE, rocprim::plus<u32>(), (hipStream_t)0) !=
            hipSuccess) {
        (void)hipGetLastError();
        wc_set_error("%s: rocPRIM temporary-storage query failed (no device?)", who);
        return WC_ERR_HIP;
    }
    *bytes = a > b ? a : b;
    return WC_OK;
}

int check_values(int C, int H, int W, long M, const char* who) {
    WC_CHECK_ARG(C >= 1 && C <= LAT_MAX_C, "%s: bad argument: C = %d outside [1, %d]", who, C, LAT_MAX_C);
    WC_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= LAT_MAX_N, "%s: bad argument: H x W = %d x %d outside [1, 640*640] pixels", who,
                 H, W);
    WC_CHECK_ARG(M >= 1 && M <= (long)H * W * LAT_D1, "%s: bad argument: M = %ld outside [1, 6 H W]", who, M);
    return WC_OK;
}

int launch_slice(SliceArgs a, hipStream_t st) {
    const dim3 grid(wc_cdiv(a.N, 8)), block(256);
    switch (a.CP / 32) {
        case 1: hipLaunchKernelGGL(lat_slice_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(lat_slice_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(lat_slice_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(lat_slice_kernel<4>, grid, block, 0, st, a); break;
    }
    WC_LAUNCH_CHECK("lat_slice_kernel");
    return WC_OK;
}

SliceArgs slice_args(const Lat& L, const float* vals, long N, int C, int CP, long M) {
    SliceArgs a = {};
    a.val = vals, a.pixvert = L.pixvert, a.bary = L.bary, a.meta = L.meta;
    a.M = (int)M, a.N = (int)N, a.C = C, a.CP = CP;
    return a;
}

// S_bil = filter(1) -> S (may be NULL: then into w.tmp), n_bil -> w.nrm + N
int bil_norm(const Lat& L, const LatWs& w, float* vals, float* S, long N, long M, hipStream_t st) {
    hipLaunchKernelGGL(lat_ones_kernel, dim3(wc_cdiv(32 * N, 256)), dim3(256), 0, st, w.Vb, 32 * N);
    WC_LAUNCH_CHECK("lat_ones_kernel");
    if (int rc = lattice_shared::filter_rows(L, w.Vb, vals, w.partial, N, 32, M, st)) return rc;
    SliceArgs a = slice_args(L, vals, N, 1, 32, M);
    a.mode = 0, a.S = S ? S : w.tmp, a.nrm = w.nrm + N;
    return launch_slice(a, st);
}

int zero(float* p, long n, hipStream_t st, const char* who) {
    if (hipMemsetAsync(p, 0, sizeof(float) * n, st) != hipSuccess) {
        wc_set_error("%s: hipMemsetAsync failed", who);
        return WC_ERR_HIP;
    }
    return WC_OK;
}

}  // namespace

extern "C" int wc_dcrf_lattice_key_bound(int H, int W, float bi_xy_std, float bi_rgb_std, double* h_bound) {
    WC_CHECK_ARG(h_bound, "wc_dcrf_lattice_key_bound: bad argument: null pointer");
    if (int rc = check_bound(H, W, bi_xy_std, bi_rgb_std, nullptr, "wc_dcrf_lattice_key_bound")) {
        if (H >= 1 && W >= 1 && bi_xy_std > 0.f && bi_rgb_std > 0.f) *h_bound = key_bound(H, W, bi_xy_std, bi_rgb_std, nullptr);
        return rc;
    }
    *h_bound = key_bound(H, W, bi_xy_std, bi_rgb_std, nullptr);
    return WC_OK;
}

extern "C" int wc_dcrf_lattice_workspace_bytes(int C, int H, int W, long* h_lat_bytes, long* h_ws_bytes) {
    WC_CHECK_ARG(h_lat_bytes && h_ws_bytes, "wc_dcrf_lattice_workspace_bytes: bad argument: null pointer");
    if (int rc = check_values(C, H, W, 1, "wc_dcrf_lattice_workspace_bytes")) return rc;
    const long N = (long)H * W;
    size_t tb = 0;
    if (int rc = temp_bytes(N * LAT_D1, &tb, "wc_dcrf_lattice_workspace_bytes")) return rc;
    *h_lat_bytes = lat_carve(nullptr, N, tb).total;
    *h_ws_bytes = 4 * ws_carve(nullptr, N, C).total;
    return WC_OK;
}

extern "C" int wc_dcrf_lattice_build(const void* img, int img_is_u8, void* lat, int H, int W, float bi_xy_std, float bi_rgb_std,
                                     void* stream) {
    WC_CHECK_ARG(img && lat, "wc_dcrf_lattice_build: bad argument: null pointer");
    BuildArgs b;
    if (int rc = check_bound(H, W, bi_xy_std, bi_rgb_std, b.s, "wc_dcrf_lattice_build")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long N = (long)H * W;
    const int NE = (int)(N * LAT_D1);
    size_t tb = 0;
    if (int rc = temp_bytes(NE, &tb, "wc_dcrf_lattice_build")) return rc;
    const Lat L = lat_carve(lat, N, tb);
    if (hipMemsetAsync(L.meta, 0, 64, st) != hipSuccess) {
        wc_set_error("wc_dcrf_lattice_build: hipMemsetAsync failed");
        return WC_ERR_HIP;
    }
    b.img = img, b.is_u8 = img_is_u8, b.H = H, b.W = W, b.xy_std = bi_xy_std, b.rgb_std = bi_rgb_std;
    b.keys = L.keys[1], b.slots = L.slots[1], b.bary = L.bary, b.meta = L.meta;
    hipLaunchKernelGGL(lat_build_kernel, dim3(wc_cdiv(N, 256)), dim3(256), 0, st, b);
    WC_LAUNCH_CHECK("lat_build_kernel");
    return lattice_shared::structure(L, NE, st, "wc_dcrf_lattice_build");
}

// ---- what csrc/energy_lattice.hip shares (lattice_shared.h)
int lattice_shared::check_bound(int H, int W, float bi_xy_std, float bi_rgb_std, double* s_out, const char* who) {
    return ::check_bound(H, W, bi_xy_std, bi_rgb_std, s_out, who);
}

int lattice_shared::temp_bytes(long NE, size_t* bytes, const char* who) { return ::temp_bytes(NE, bytes, who); }

int lattice_shared::structure(const Lat& L, int NE, hipStream_t st, const char* who) {
    const dim3 ge(wc_cdiv(NE, 256)), blk(256);
    // sort into keys[0] / slots[0], whichever buffer rocPRIM finishes in
    rocprim::double_buffer<u64> dk(L.keys[1], L.keys[0]);
    rocprim::double_buffer<u32> dv(L.slots[1], L.slots[0]);
    size_t tbytes = L.temp_bytes;
    if (rocprim::radix_sort_pairs(L.temp, tbytes, dk, dv, (size_t)NE, 0, LAT_BITS * LAT_D, st) != hipSuccess) {
        wc_set_error("%s: rocPRIM radix sort failed", who);
        return WC_ERR_HIP;
    }
    if (dk.current() != L.keys[0]) {
        if (hipMemcpyAsync(L.keys[0], dk.current(), 8L * NE, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(L.slots[0], dv.current(), 4L * NE, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            wc_set_error("%s: hipMemcpyAsync failed", who);
            return WC_ERR_HIP;
        }
    }
    u32* flags = L.slots[1];
    hipLaunchKernelGGL(lat_head_kernel, ge, blk, 0, st, L.keys[0], flags, NE);
    WC_LAUNCH_CHECK("lat_head_kernel");
    tbytes = L.temp_bytes;
    if (rocprim::inclusive_scan(L.temp, tbytes, flags, L.vid, (size_t)NE, rocprim::plus<u32>(), st) != hipSuccess) {
        wc_set_error("%s: rocPRIM scan failed", who);
        return WC_ERR_HIP;
    }
    hipLaunchKernelGGL(lat_vertex_kernel, ge, blk, 0, st, L.keys[0], L.slots[0], L.vid, L.pixvert, L.ukeys, L.segstart, L.meta, NE);
    WC_LAUNCH_CHECK("lat_vertex_kernel");
    hipLaunchKernelGGL(lat_xflag_kernel, ge, blk, 0, st, L.vid, L.segstart, flags, NE);
    WC_LAUNCH_CHECK("lat_xflag_kernel");
    tbytes = L.temp_bytes;
    if (rocprim::inclusive_scan(L.temp, tbytes, flags, L.xid, (size_t)NE, rocprim::plus<u32>(), st) != hipSuccess) {
        wc_set_error("%s: rocPRIM scan failed", who);
        return WC_ERR_HIP;
    }
    hipLaunchKernelGGL(lat_xchunk_kernel, ge, blk, 0, st, L.vid, L.segstart, L.xid, L.xstart, L.xvert, L.meta, NE);
    WC_LAUNCH_CHECK("lat_xchunk_kernel");
    hipLaunchKernelGGL(lat_nbr_kernel, dim3(wc_cdiv((long)(NE + 1) * LAT_NBR, 256)), blk, 0, st, L.ukeys, L.meta, L.nbr, (long)NE);
    WC_LAUNCH_CHECK("lat_nbr_kernel");
    return WC_OK;
}

int lattice_shared::filter_rows(const Lat& L, const float* V, float* vals, float* partial, long N, int CP, long M, hipStream_t st) {
    const long rows = M >= 0 ? M : N * LAT_D1;
    float* va = vals;
    float* vb = vals + (rows + 1) * CP;
    SplatArgs a;
    a.V = (const float4*)V, a.val = (float4*)va, a.partial = (float4*)partial;
    a.slots = L.slots[0], a.bary = L.bary, a.segstart = L.segstart, a.xid = L.xid, a.xstart = L.xstart, a.xvert = L.xvert;
    a.meta = L.meta, a.q = CP / 4, a.M = M >= 0 ? (int)M : -1;
    const long XC = N * LAT_D1 / LAT_CHUNK + 1;
    hipLaunchKernelGGL(lat_splat_extra_kernel, dim3(wc_cdiv(XC * a.q, 256)), dim3(256), 0, st, a, XC);
    WC_LAUNCH_CHECK("lat_splat_extra_kernel");
    const dim3 grid(wc_cdiv((rows + 1) * a.q, 256));
    hipLaunchKernelGGL(lat_splat_kernel, grid, dim3(256), 0, st, a);
    WC_LAUNCH_CHECK("lat_splat_kernel");
    for (int j = 0; j < LAT_D1; ++j) {
        hipLaunchKernelGGL(lat_blur_kernel, grid, dim3(256), 0, st, (const float4*)((j & 1) ? vb : va), (float4*)((j & 1) ? va : vb),
                           L.nbr, L.meta, j, a.q, a.M);
        WC_LAUNCH_CHECK("lat_blur_kernel");
    }
    return WC_OK;             // LAT_D1 is even: the result is back in vals
}

#define LAT_OPEN(who)                                                    \
    if (int rc = check_values(C, H, W, M, who)) return rc;               \
    hipStream_t st = (hipStream_t)stream;                                \
    const long N = (long)H * W;                                          \
    const int CP = 32 * ((C + 31) / 32);                                 \
    const Lat L = lat_carve((void*)lat, N, 0); /* rocPRIM's temporary storage lies last and is the build's alone */ \
    const LatWs w = ws_carve(ws, N, C);

extern "C" int wc_dcrf_lattice_filter(const void* lat, const float* in, float* out, float* vals, void* ws, int C, int H, int W,
                                      long M, void* stream) {
    WC_CHECK_ARG(lat && in && out && vals && ws, "wc_dcrf_lattice_filter: bad argument: null pointer");
    LAT_OPEN("wc_dcrf_lattice_filter")
    if (int rc = zero(w.Vb, N * CP, st, "wc_dcrf_lattice_filter")) return rc;
    hipLaunchKernelGGL(lat_operand_kernel, dim3(wc_cdiv((long)C * N, 256)), dim3(256), 0, st, in, (const float*)nullptr, w.Vb, C, CP,
                       (int)N);
    WC_LAUNCH_CHECK("lat_operand_kernel");
    if (int rc = lattice_shared::filter_rows(L, w.Vb, vals, w.partial, N, CP, M, st)) return rc;
    SliceArgs a = slice_args(L, vals, N, C, CP, M);
    a.mode = 1, a.out = out, a.nb = nullptr;
    return launch_slice(a, st);
}

extern "C" int wc_dcrf_lattice_message(const void* lat, const float* Q, float* msg_pos, float* msg_bil, float* S, float* vals,
                                       void* ws, int C, int H, int W, long M, float pos_xy_std, void* stream) {
    WC_CHECK_ARG(lat && Q && msg_pos && msg_bil && S && vals && ws, "wc_dcrf_lattice_message: bad argument: null pointer");
    if (int rc = dcrf_shared::limits(C, H, W, pos_xy_std, 1.f, 1.f, "wc_dcrf_lattice_message")) return rc;
    LAT_OPEN("wc_dcrf_lattice_message")
    if (int rc = dcrf_shared::pos_norm(H, W, pos_xy_std, S, w.nrm, st)) return rc;
    if (int rc = bil_norm(L, w, vals, S + N, N, M, st)) return rc;
    if (int rc = zero(w.Vb, N * CP, st, "wc_dcrf_lattice_message")) return rc;
    if (int rc = dcrf_shared::operands(Q, w.nrm, w.Vb, w.Vp, C, CP, (int)N, st)) return rc;
    if (int rc = dcrf_shared::gauss_message(C, H, W, pos_xy_std, w.Vp, w.tmp, w.G, st)) return rc;
    if (int rc = dcrf_shared::scale(w.G, w.nrm, msg_pos, C, (int)N, st)) return rc;
    if (int rc = lattice_shared::filter_rows(L, w.Vb, vals, w.partial, N, CP, M, st)) return rc;
    SliceArgs a = slice_args(L, vals, N, C, CP, M);
    a.mode = 1, a.out = msg_bil, a.nb = w.nrm + N;
    return launch_slice(a, st);
}

extern "C" int wc_dcrf_lattice_inference(const void* lat, const float* unary, float* Q, float* vals, void* ws, int C, int H, int W,
                                         long M, int iter_max, float pos_w, float pos_xy_std, float bi_w, void* stream) {
    WC_CHECK_ARG(lat && unary && Q && vals && ws, "wc_dcrf_lattice_inference: bad argument: null pointer");
    WC_CHECK_ARG(iter_max >= 0, "wc_dcrf_lattice_inference: bad argument: iter_max = %d < 0", iter_max);
    WC_CHECK_ARG(pos_w >= 0.f && pos_w < INFINITY && bi_w >= 0.f && bi_w < INFINITY,
                 "wc_dcrf_lattice_inference: bad argument: weights must be finite and >= 0");
    if (int rc = dcrf_shared::limits(C, H, W, pos_xy_std, 1.f, 1.f, "wc_dcrf_lattice_inference")) return rc;
    LAT_OPEN("wc_dcrf_lattice_inference")
    if (int rc = dcrf_shared::pos_norm(H, W, pos_xy_std, nullptr, w.nrm, st)) return rc;
    if (int rc = bil_norm(L, w, vals, nullptr, N, M, st)) return rc;
    if (int rc = zero(w.Vb, N * CP, st, "wc_dcrf_lattice_inference")) return rc;       // padded label columns stay zero
    if (int rc = dcrf_shared::init(unary, w.nrm, Q, w.Vb, w.Vp, C, CP, (int)N, st)) return rc;
    for (int it = 0; it < iter_max; ++it) {
        if (int rc = dcrf_shared::gauss_message(C, H, W, pos_xy_std, w.Vp, w.tmp, w.G, st)) return rc;
        if (int rc = lattice_shared::filter_rows(L, w.Vb, vals, w.partial, N, CP, M, st)) return rc;
        SliceArgs a = slice_args(L, vals, N, C, CP, M);
        a.mode = 2, a.nb = w.nrm + N, a.U = unary, a.G = w.G, a.npos = w.nrm, a.w_bil = bi_w, a.w_pos = pos_w;
        a.Q = Q, a.Vb_out = w.Vb, a.Vp_out = w.Vp;
        if (int rc = launch_slice(a, st)) return rc;
    }
    return WC_OK;
}
