// The one permutohedral lattice under the dense CRF (csrc/dcrf_lattice.hip) and the dense energy loss (csrc/energy_lattice.hip):
// the structure's layout; device code shared as text, so that both files form the same bits: the per-pixel fp64 build
// (lat_point), the in-order chunk sum of the splat (lat_chunk_sum) and the slice's gather (lat_slice_gather); and host entries
// over the kernels that dcrf_lattice.hip alone holds (defined at its end): the structure behind the per-pixel build, and the
// filter itself, filter_rows: splat, extra-chunk splat and blur.  Each file keeps its own build kernel (the image layouts differ)
// and its own slice kernel (the epilogues differ).  The algorithm is pinned to tests/dcrf_lattice_ref.py.
#pragma once
#include "common.h"

#define LAT_D 5
#define LAT_D1 6
#define LAT_BITS 12
#define LAT_BIAS 2048
#define LAT_MARGIN 20            // nearest point 3 + rank wrap 6 + canonical offset 5 + blur neighbour 5, rounded up
#define LAT_CHUNK 256
#define LAT_CMAX 256.0           // colours lie in [0, 256): 8-bit values, or 8-bit values plus a fraction
#define LAT_NBR (2 * LAT_D1)
#define LAT_MAX_C 128
#define LAT_MAX_N (640 * 640)
#define LAT_ALPHA (1.0f / (1.0f + 0.03125f))
#define LAT_LOG2E 1.4426950408889634f

typedef unsigned long long u64;
typedef unsigned int u32;

// ------------------------------------------------------------------------------------------------ structure layout
// meta[0] = M, meta[1] = flag (1: a colour outside 0..256 was clamped, 2: a key coordinate left the packing), meta[2] = X, the
// number of extra chunks
struct Lat {
    int* meta;
    float* bary;        // (N, 6) f32 weights, by slot
    u32* pixvert;       // (N, 6) vertex index of every slot
    u64* keys[2];       // sort double buffer
    u32* slots[2];
    u32* vid;           // vertex index of every sorted entry
    u32* xid;           // inclusive count of extra-chunk starts
    u64* ukeys;         // [1..M] sorted unique keys
    u32* segstart;      // [1..M+1]
    u32* xstart;        // [X] first entry of an extra chunk
    u32* xvert;         // [X] its vertex
    u32* nbr;           // (NE + 1, 12)
    void* temp;         // rocPRIM
    size_t temp_bytes;
    long total;
};

static inline long lat_align(long b) { return (b + 255) & ~255L; }

// N pixels; meta_bytes: the int32 block the structure begins with (64 for one image; the batched loss keeps more there)
static inline Lat lat_carve(void* base, long N, size_t temp_bytes, long meta_bytes = 64) {
    Lat L;
    const long NE = N * LAT_D1, XC = NE / LAT_CHUNK + 2;
    char* p = (char*)base;
    long o = 0;
    auto take = [&](long bytes) { char* r = p + o; o += lat_align(bytes); return r; };
    L.meta = (int*)take(meta_bytes);
    L.bary = (float*)take(4 * NE);
    L.pixvert = (u32*)take(4 * NE);
    L.keys[0] = (u64*)take(8 * NE);
    L.keys[1] = (u64*)take(8 * NE);
    L.slots[0] = (u32*)take(4 * NE);
    L.slots[1] = (u32*)take(4 * NE);
    L.vid = (u32*)take(4 * NE);
    L.xid = (u32*)take(4 * NE);
    L.ukeys = (u64*)take(8 * (NE + 1));
    L.segstart = (u32*)take(4 * (NE + 2));
    L.xstart = (u32*)take(4 * XC);
    L.xvert = (u32*)take(4 * XC);
    L.nbr = (u32*)take(4L * LAT_NBR * (NE + 1));
    L.temp = take((long)temp_bytes);
    L.temp_bytes = temp_bytes;
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------------------------------ build
struct BuildArgs {
    const void* img;
    int is_u8, H, W;
    double xy_std, rgb_std;
    double s[LAT_D];
    u64* keys;
    u32* slots;
    float* bary;
    int* meta;
};

// Pixel i with colour col (fp64, modified: clamped for the key): keys, slots and weights of its d + 1 vertices.  Returns the
// flag (0, 1: a colour was clamped, 2: a key coordinate left the packing).  Every decision in fp64, no FP contraction.
__device__ __forceinline__ int lat_point(const BuildArgs& A, int i, double* col) {
    const int y = i / A.W, x = i - y * A.W;
    int flag = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (!(col[k] >= 0.0 && col[k] <= LAT_CMAX)) {
            col[k] = col[k] > LAT_CMAX ? LAT_CMAX : 0.0;          // NaN -> 0
            flag = 1;
        }
    double c[LAT_D];
    c[0] = ((double)x / A.xy_std) * A.s[0];
    c[1] = ((double)y / A.xy_std) * A.s[1];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[2 + k] = (col[k] / A.rgb_std) * A.s[2 + k];
    // elevate
    double e[LAT_D1], sm = 0.0;
#pragma unroll
    for (int j = LAT_D; j >= 1; --j) {
        e[j] = sm - (double)j * c[j - 1];
        sm = sm + c[j - 1];
    }
    e[0] = sm;
    // nearest zero-remainder point
    double rem0[LAT_D1], sumd = 0.0;
#pragma unroll
    for (int k = 0; k < LAT_D1; ++k) {
        const double v = e[k] / (double)LAT_D1;
        const double up = ceil(v) * (double)LAT_D1, dn = floor(v) * (double)LAT_D1;
        rem0[k] = (up - e[k] < e[k] - dn) ? up : dn;
        sumd += rem0[k] / (double)LAT_D1;
    }
    const int sum = (int)rint(sumd);
    // rank
    int rank[LAT_D1];
    double delta[LAT_D1];
#pragma unroll
    for (int k = 0; k < LAT_D1; ++k) rank[k] = 0, delta[k] = e[k] - rem0[k];
#pragma unroll
    for (int a = 0; a < LAT_D1; ++a)
#pragma unroll
        for (int b = a + 1; b < LAT_D1; ++b) {
            const bool lt = delta[a] < delta[b];
            rank[a] += lt ? 1 : 0;
            rank[b] += lt ? 0 : 1;
        }
#pragma unroll
    for (int k = 0; k < LAT_D1; ++k) {
        rank[k] += sum;
        if (rank[k] < 0) {
            rank[k] += LAT_D1;
            rem0[k] += (double)LAT_D1;
        } else if (rank[k] > LAT_D) {
            rank[k] -= LAT_D1;
            rem0[k] -= (double)LAT_D1;
        }
    }
    // barycentric weights (the additions in the restatement's order; adding 0.0 to the other entries changes nothing)
    double b[LAT_D1 + 1];
#pragma unroll
    for (int m = 0; m <= LAT_D1; ++m) b[m] = 0.0;
#pragma unroll
    for (int k = 0; k < LAT_D1; ++k) {
        const double t = (e[k] - rem0[k]) / (double)LAT_D1;
#pragma unroll
        for (int m = 0; m <= LAT_D1; ++m) {
            if (m == LAT_D - rank[k]) b[m] += t;
            if (m == LAT_D1 - rank[k]) b[m] -= t;
        }
    }
    b[0] += 1.0 + b[LAT_D1];
    // keys
    int r0[LAT_D];
#pragma unroll
    for (int k = 0; k < LAT_D; ++k) r0[k] = (int)rem0[k];
#pragma unroll
    for (int r = 0; r < LAT_D1; ++r) {
        u64 key = 0;
#pragma unroll
        for (int k = 0; k < LAT_D; ++k) {
            int f = r0[k] + (rank[k] <= LAT_D - r ? r : r - LAT_D1) + LAT_BIAS;
            if (f < LAT_D1 || f > 2 * LAT_BIAS - 1 - LAT_D1) {          // cannot happen inside the host's bound
                f = min(max(f, LAT_D1), 2 * LAT_BIAS - 1 - LAT_D1);
                flag = 2;
            }
            key |= (u64)f << (LAT_BITS * (LAT_D - 1 - k));
        }
        const long s = (long)i * LAT_D1 + r;
        A.keys[s] = key;
        A.slots[s] = (u32)s;
        A.bary[s] = (float)b[r];
    }
    return flag;
}

// ------------------------------------------------------------------------------------------------ splat
struct SplatArgs {
    const float4* V;          // (N, q) float4
    float4* val;              // (M + 1, q)
    float4* partial;          // (X, q)
    const u32* slots;         // sorted
    const float* bary;
    const u32* segstart;
    const u32* xid;
    const u32* xstart;
    const u32* xvert;
    const int* meta;
    int q, M;                 // M >= 0: the vertex count the host read back; M < 0: the count stays on the device
};

// The one guard of the splat and blur kernels, for vertex row v.  M >= 0 (the CRF's entries): the grid covers M + 1 rows and a
// structure whose count is not the M the buffers were sized for is left alone (stale-structure check).  M < 0 (the energy
// loss's entries): the grid covers the proven worst case 6 HW + 1 rows and the rows past the device's count exit here.
__device__ __forceinline__ bool lat_row_idle(const int* meta, int M, long v) {
    const int m = meta[0];
    return (M >= 0 && m != M) || v > m;
}

// sum of entries [start, end) of the sorted list, in order, four loads in flight
__device__ __forceinline__ float4 lat_chunk_sum(const SplatArgs& A, u32 start, u32 end, int c4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (u32 e = start; e < end; e += 4) {
        float w[4];
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const u32 s = A.slots[min(e + u, end - 1)];
            w[u] = e + u < end ? A.bary[s] : 0.f;
            x[u] = A.V[(long)(s / LAT_D1) * A.q + c4];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc.x = fmaf(w[u], x[u].x, acc.x);
            acc.y = fmaf(w[u], x[u].y, acc.y);
            acc.z = fmaf(w[u], x[u].z, acc.z);
            acc.w = fmaf(w[u], x[u].w, acc.w);
        }
    }
    return acc;
}

// ------------------------------------------------------------------------------------------------ slice
// acc[k] = sum_r b_r val[vertex_r][32 k + l31] of pixel ic, in the order r = 0..d (alpha is the caller's to apply); 32 lanes own
// a pixel and a lane CT columns
template <int CT>
__device__ __forceinline__ void lat_slice_gather(const float* __restrict__ val, const u32* __restrict__ pixvert,
                                                 const float* __restrict__ bary, int ic, int CP, int l31, float (&acc)[CT]) {
    u32 vr[LAT_D1];
    float br[LAT_D1];
#pragma unroll
    for (int r = 0; r < LAT_D1; ++r) vr[r] = pixvert[(long)ic * LAT_D1 + r], br[r] = bary[(long)ic * LAT_D1 + r];
#pragma unroll
    for (int k = 0; k < CT; ++k) acc[k] = 0.f;
#pragma unroll
    for (int r = 0; r < LAT_D1; ++r)
#pragma unroll
        for (int k = 0; k < CT; ++k) acc[k] = fmaf(br[r], val[(long)vr[r] * CP + 32 * k + l31], acc[k]);
}

// ------------------------------------------------------------------------------------------------ host side
namespace lattice_shared {

// the limits and the key bound of wc_dcrf_lattice_key_bound; s_out (may be NULL): the d feature scales; `who` prefixes the text
int check_bound(int H, int W, float bi_xy_std, float bi_rgb_std, double* s_out, const char* who);
// bytes of rocPRIM's temporary storage for a sort and a scan of NE entries
int temp_bytes(long NE, size_t* bytes, const char* who);
// Everything of the build behind the per-pixel kernel: the (key, slot) pairs of L.keys[1] / L.slots[1] -> sorted entries,
// vertices, segments, extra chunks and blur neighbours; M -> L.meta[0], X -> L.meta[2].  No host synchronisation.
int structure(const Lat& L, int NE, hipStream_t st, const char* who);
// The filter up to the slice: vals[0 .. rows] (rows + 1, CP) = the blurred splat of V (N, CP), rows = M when M >= 0 (the count
// the host read back) and the worst case 6 N when M < 0 (the count stays on the device: SplatArgs).  The ping-pong partner
// is the (rows + 1, CP) block behind vals; partial: (6 N / 256 + 2, CP) for the extra chunks.  No host synchronisation.
int filter_rows(const Lat& L, const float* V, float* vals, float* partial, long N, int CP, long M, hipStream_t st);

}  // namespace lattice_shared
