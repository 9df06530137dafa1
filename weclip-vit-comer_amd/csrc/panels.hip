// The training image panels of the reference's utils/imutils.py on the device: every kernel writes uint8 CHW tiles straight into
// the canvas `torchvision.utils.make_grid(nrow, padding=2, pad_value=0)` would assemble (the caller zeroes the canvas once; there
// is no grid pass and no per-image launch), and one capturable launch snapshots what a later render needs out of a train step.
//   panel_images_kernel   : denormalize_img (:11-18): x * std + mean in fp32 (multiply, then add: the library is built with
//                           -ffp-contract=off), truncated toward zero to uint8
//   panel_labels_kernel   : tensorboard_label / encode_cmap (:7-9, :125-133): the VOC colour (voc_colour.h) of int64 / uint8 labels
//   panel_minmax_kernel   : the per-image min and max of the up-sampled map that tensorboard_attn's minmax_norm (:71-76) needs
//   panel_heat_kernel     : bilinear up-sampling (resample.h) -> max over channels -> [x - min, / max] -> matplotlib look-up
//                           (cmap_tables.h) -> [0.5 * colour + 0.5 * image in fp64] -> uint8: tensorboard_image's overlay (:32-38),
//                           tensorboard_attn's tiles (:59-79) and tensorboard_edge's (:44-47)
//   panel_snapshot_kernel : seg logits, the label map as uint8 and four rows of attn_pred -> caller-owned buffers
// A float becomes a uint8 as `(unsigned char)(int)v`: truncation toward zero, a value outside [0, 256) wraps as it does on the
// reference's host.
#include "common.h"
#include "resample.h"
#include "voc_colour.h"
#include "cmap_tables.h"

// Where tile k of a panel goes: canvas (3, canvas_h, canvas_w) uint8, tile 0 at (oy, ox), tiles (H + pad, W + pad) apart, xmaps
// tiles per row; colmajor: tiles run down the columns first (tile k in row k % xmaps, column k / xmaps), the net effect of
// tensorboard_attn's two transposes around make_grid (:79, :83).  k0: index of the launch's first tile.
struct PanelGrid {
    unsigned char* out;
    long plane;
    int pitch, oy, ox, xmaps, pad, colmajor, k0;
};

__device__ __forceinline__ long panel_tile_base(const PanelGrid& g, int k, int H, int W) {
    k += g.k0;
    const int a = k % g.xmaps, b = k / g.xmaps;
    const int ty = g.colmajor ? a : b, tx = g.colmajor ? b : a;
    return (long)(g.oy + ty * (H + g.pad)) * g.pitch + g.ox + tx * (W + g.pad);
}

__device__ __forceinline__ unsigned char panel_u8(float v) { return (unsigned char)(int)v; }
__device__ __forceinline__ unsigned char panel_u8(double v) { return (unsigned char)(int)v; }

struct PanelNorm {
    float m[3], s[3];
};

// one thread per pixel of one image, the three channels in turn: neighbouring lanes write neighbouring bytes
__global__ __launch_bounds__(256) void panel_images_kernel(const float* __restrict__ img, PanelGrid g, PanelNorm n, int B, int H, int W) {
    const long HW = (long)H * W, total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int b = (int)(i / HW);
        const long p = i - (long)b * HW;
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        unsigned char* o = g.out + panel_tile_base(g, b, H, W) + (long)y * g.pitch + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * g.plane] = panel_u8(img[((long)b * 3 + c) * HW + p] * n.s[c] + n.m[c]);
    }
}

__global__ __launch_bounds__(256) void panel_labels_kernel(const void* __restrict__ lab, int is_u8, PanelGrid g, int B, int H, int W) {
    const long HW = (long)H * W, total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int b = (int)(i / HW);
        const long p = i - (long)b * HW;
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const unsigned int v = is_u8 ? ((const unsigned char*)lab)[i] : (unsigned int)(((const long*)lab)[i] & 255);
        const unsigned int c = ef_colour(v);
        unsigned char* o = g.out + panel_tile_base(g, b, H, W) + (long)y * g.pitch + x;
        o[0] = (unsigned char)(c & 255u);
        o[g.plane] = (unsigned char)((c >> 8) & 255u);
        o[2 * g.plane] = (unsigned char)(c >> 16);
    }
}

// max over C channels of the bilinear up-sample at one destination pixel; a NaN in any channel wins, like torch.max
template <bool ALIGNED>
__device__ __forceinline__ float panel_heat_at(const float* __restrict__ S, long sC, int C, int h, int w, int y, int x, float sy, float sx) {
    int y0, y1, x0, x1;
    float ly, lx;
    if (ALIGNED) {
        wc_bil_src_aligned(y, h, sy, y0, y1, ly);
        wc_bil_src_aligned(x, w, sx, x0, x1, lx);
    } else {
        wc_bil_src(y, h, sy, y0, y1, ly);
        wc_bil_src(x, w, sx, x0, x1, lx);
    }
    float best = wc_bilerp(S, w, y0, y1, x0, x1, ly, lx);
    for (int c = 1; c < C; ++c) {
        const float v = wc_bilerp(S + c * sC, w, y0, y1, x0, x1, ly, lx);
        if (best == best && (v > best || v != v)) best = v;
    }
    return best;
}

// one workgroup per image: mm[3 b] = min, mm[3 b + 1] = max over the (H, W) up-sampled map, mm[3 b + 2] = 1 when it holds a NaN
// (torch's min / max then are NaN and the whole tile is painted with the "bad" colour)
template <bool ALIGNED>
__global__ __launch_bounds__(256) void panel_minmax_kernel(const float* __restrict__ src, long sB, long sC, int C, int h, int w,
                                                            float* __restrict__ mm, int H, int W, float sy, float sx) {
    __shared__ float red[16];
    const float* S = src + (long)blockIdx.x * sB;
    float mn = INFINITY, mx = -INFINITY, bad = 0.f;
    for (int p = threadIdx.x; p < H * W; p += 256) {
        const int y = p / W, x = p - y * W;
        const float v = panel_heat_at<ALIGNED>(S, sC, C, h, w, y, x, sy, sx);
        if (v != v) bad = 1.f;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    mn = block_min(mn, red);
    mx = block_max(mx, red);
    bad = block_max(bad, red);
    if (threadIdx.x == 0) {
        mm[3 * blockIdx.x] = mn;
        mm[3 * blockIdx.x + 1] = mx;
        mm[3 * blockIdx.x + 2] = bad;
    }
}

// matplotlib's Colormap.__call__ on a float: index int(x * 256); x == 1 -> 255; x < 0 -> entry 0; x * 256 >= 256 -> entry 255;
// NaN -> the "bad" colour (0, 0, 0): returns -1
__device__ __forceinline__ int panel_cmap_index(float x) {
    float xa = x * 256.f;
    if (xa == 256.f) xa = 255.f;
    if (xa != xa) return -1;
    if (xa < 0.f) return 0;
    if (xa >= 256.f) return 255;
    return (int)xa;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void panel_heat_kernel(const float* __restrict__ src, long sB, long sC, int C, int h, int w,
                                                          const float* __restrict__ mm, int cmap, const float* __restrict__ img,
                                                          PanelNorm n, PanelGrid g, int B, int H, int W, float sy, float sx) {
    const long HW = (long)H * W, total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int b = (int)(i / HW);
        const long p = i - (long)b * HW;
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        float v = panel_heat_at<ALIGNED>(src + (long)b * sB, sC, C, h, w, y, x, sy, sx);
        if (mm) {
            const float mn = mm[3 * b], mx = mm[3 * b + 1];
            v = (v - mn) / (mx - mn);                 // x - min, then / max(x - min): the rounding of fp32 is monotone
            if (mm[3 * b + 2] != 0.f) v = NAN;
        }
        const int k = panel_cmap_index(v);
        unsigned char* o = g.out + panel_tile_base(g, b, H, W) + (long)y * g.pitch + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double col = k < 0 ? 0.0 : WC_CMAP255[cmap][3 * k + c];
            if (img) {
                const unsigned char u = panel_u8(img[((long)b * 3 + c) * HW + p] * n.s[c] + n.m[c]);
                o[c * g.plane] = panel_u8(col * 0.5 + (double)u * 0.5);
            } else {
                o[c * g.plane] = panel_u8(col);
            }
        }
    }
}

// [0, n_seg): the logits as they are; then groups of 4 labels int64 -> uint8 (the low byte, torch's cast); then (B, 4, hw) rows of attn
typedef long panel_l2 __attribute__((ext_vector_type(2)));
struct PanelRows {
    int r[4];
};

__global__ __launch_bounds__(256) void panel_snapshot_kernel(const float* __restrict__ seg, long n_seg, const long* __restrict__ label,
                                                              long n_label, const float* __restrict__ attn, int B, int hw, PanelRows rows,
                                                              float* __restrict__ seg_out, unsigned char* __restrict__ label_out,
                                                              float* __restrict__ rows_out) {
    const long groups = (n_label + 3) >> 2, n_rows = attn ? (long)B * 4 * hw : 0, total = n_seg + groups + n_rows;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        if (i < n_seg) {
            seg_out[i] = seg[i];
        } else if (i < n_seg + groups) {
            const long j = (i - n_seg) << 2;
            if (n_label - j >= 4) {                   // label and label_out are 16- / 4-byte aligned (checked by the entry)
                const panel_l2 a = *reinterpret_cast<const panel_l2*>(label + j), b = *reinterpret_cast<const panel_l2*>(label + j + 2);
                *reinterpret_cast<unsigned int*>(label_out + j) = ((unsigned int)a.x & 255u) | (((unsigned int)a.y & 255u) << 8) |
                                                                  (((unsigned int)b.x & 255u) << 16) | (((unsigned int)b.y & 255u) << 24);
            } else {
                for (long k = j; k < n_label; ++k) label_out[k] = (unsigned char)label[k];
            }
        } else {
            const long r = i - n_seg - groups;
            const int e = (int)(r % hw), q = (int)((r / hw) & 3), b = (int)(r / (4L * hw));
            rows_out[r] = attn[((long)b * hw + rows.r[q]) * hw + e];
        }
    }
}

// ---------------------------------------------------------------------------------------------
static unsigned panel_blocks(long items) {
    long blocks = (items + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

// every tile of the launch lies inside the canvas
static bool panel_grid_ok(int B, int H, int W, const void* out, int canvas_h, int canvas_w, int oy, int ox, int xmaps, int pad,
                          int k0) {
    if (!out || B < 1 || B > 65535 || H < 1 || W < 1 || H > 16384 || W > 16384 || canvas_h < 1 || canvas_w < 1 || oy < 0 || ox < 0 ||
        xmaps < 1 || pad < 0 || pad > 16384 || k0 < 0 || k0 > 65535)
        return false;
    return true;
}

static bool panel_tiles_fit(int B, int H, int W, int canvas_h, int canvas_w, int oy, int ox, int xmaps, int pad, int colmajor, int k0) {
    for (int k = k0; k < k0 + B; ++k) {
        const int a = k % xmaps, b = k / xmaps;
        const long ty = colmajor ? a : b, tx = colmajor ? b : a;
        if (oy + ty * (H + pad) + H > canvas_h || ox + tx * (W + pad) + W > canvas_w) return false;
    }
    return true;
}

#define PANEL_CHECK_GRID(name)                                                                                                   \
    WC_CHECK_ARG(panel_grid_ok(B, H, W, out, canvas_h, canvas_w, oy, ox, xmaps, pad, k0), name ": bad argument");                \
    WC_CHECK_ARG(panel_tiles_fit(B, H, W, canvas_h, canvas_w, oy, ox, xmaps, pad, colmajor, k0),                                 \
                 name ": %d tiles of (%d, %d) from tile %d do not fit the (%d, %d) canvas", B, H, W, k0, canvas_h, canvas_w);    \
    const PanelGrid g = {(unsigned char*)out, (long)canvas_h * canvas_w, canvas_w, oy, ox, xmaps, pad, colmajor ? 1 : 0, k0}

static PanelNorm panel_norm(const float* mean3, const float* std3) {
    PanelNorm n = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    for (int c = 0; c < 3; ++c) {
        if (mean3) n.m[c] = mean3[c];
        if (std3) n.s[c] = std3[c];
    }
    return n;
}

extern "C" int wc_panel_images(const float* img, const float* mean3, const float* std3, int B, int H, int W, void* out, int canvas_h,
                               int canvas_w, int oy, int ox, int xmaps, int pad, int colmajor, int k0, void* stream) {
    WC_CHECK_ARG(img && mean3 && std3, "wc_panel_images: bad argument");
    PANEL_CHECK_GRID("wc_panel_images");
    hipLaunchKernelGGL(panel_images_kernel, dim3(panel_blocks((long)B * H * W)), dim3(256), 0, (hipStream_t)stream, img, g,
                       panel_norm(mean3, std3), B, H, W);
    WC_LAUNCH_CHECK("panel_images_kernel");
    return WC_OK;
}

extern "C" int wc_panel_labels(const void* label, int is_u8, int B, int H, int W, void* out, int canvas_h, int canvas_w, int oy, int ox,
                               int xmaps, int pad, int colmajor, int k0, void* stream) {
    WC_CHECK_ARG(label, "wc_panel_labels: bad argument");
    PANEL_CHECK_GRID("wc_panel_labels");
    hipLaunchKernelGGL(panel_labels_kernel, dim3(panel_blocks((long)B * H * W)), dim3(256), 0, (hipStream_t)stream, label,
                       is_u8 ? 1 : 0, g, B, H, W);
    WC_LAUNCH_CHECK("panel_labels_kernel");
    return WC_OK;
}

extern "C" int wc_panel_heat(const float* src, long sB, long sC, int C, int h, int w, int aligned, float* minmax, int cmap,
                             const float* img, const float* mean3, const float* std3, int B, int H, int W, void* out, int canvas_h,
                             int canvas_w, int oy, int ox, int xmaps, int pad, int colmajor, int k0, void* stream) {
    WC_CHECK_ARG(src && C >= 1 && C <= 65535 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384 && sB >= 0 && sC >= 0 &&
                     (cmap == 0 || cmap == 1) && (!img || (mean3 && std3)),
                 "wc_panel_heat: bad argument");
    PANEL_CHECK_GRID("wc_panel_heat");
    const PanelNorm n = panel_norm(img ? mean3 : nullptr, img ? std3 : nullptr);
    hipStream_t st = (hipStream_t)stream;
    if (aligned) {                                    // ATen's scale with align_corners=True: 0 for a one-sample output axis
        const float sy = H > 1 ? (float)(h - 1) / (H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (W - 1) : 0.f;
        if (minmax) {
            hipLaunchKernelGGL(panel_minmax_kernel<true>, dim3(B), dim3(256), 0, st, src, sB, sC, C, h, w, minmax, H, W, sy, sx);
            WC_LAUNCH_CHECK("panel_minmax_kernel");
        }
        hipLaunchKernelGGL(panel_heat_kernel<true>, dim3(panel_blocks((long)B * H * W)), dim3(256), 0, st, src, sB, sC, C, h, w,
                           (const float*)minmax, cmap, img, n, g, B, H, W, sy, sx);
    } else {
        const float sy = (float)h / H, sx = (float)w / W;
        if (minmax) {
            hipLaunchKernelGGL(panel_minmax_kernel<false>, dim3(B), dim3(256), 0, st, src, sB, sC, C, h, w, minmax, H, W, sy, sx);
            WC_LAUNCH_CHECK("panel_minmax_kernel");
        }
        hipLaunchKernelGGL(panel_heat_kernel<false>, dim3(panel_blocks((long)B * H * W)), dim3(256), 0, st, src, sB, sC, C, h, w,
                           (const float*)minmax, cmap, img, n, g, B, H, W, sy, sx);
    }
    WC_LAUNCH_CHECK("panel_heat_kernel");
    return WC_OK;
}

extern "C" int wc_panel_snapshot(const float* seg, long n_seg, const long* label, long n_label, const float* attn, int B, int hw,
                                 const int* rows4, float* seg_out, void* label_out, float* rows_out, void* stream) {
    WC_CHECK_ARG(seg && seg_out && label && label_out && n_seg >= 1 && n_label >= 1, "wc_panel_snapshot: bad argument");
    WC_CHECK_ARG(((size_t)label & 15) == 0 && ((size_t)label_out & 3) == 0,
                 "wc_panel_snapshot: label must be 16-byte and label_out 4-byte aligned");
    PanelRows rows = {{0, 0, 0, 0}};
    if (attn) {
        WC_CHECK_ARG(rows4 && rows_out && B >= 1 && B <= 65535 && hw >= 1 && hw <= 46340, "wc_panel_snapshot: bad argument");
        for (int q = 0; q < 4; ++q) {
            WC_CHECK_ARG(rows4[q] >= 0 && rows4[q] < hw, "wc_panel_snapshot: row %d lies outside the (%d, %d) map", rows4[q], hw, hw);
            rows.r[q] = rows4[q];
        }
    }
    const long total = n_seg + ((n_label + 3) >> 2) + (attn ? (long)B * 4 * hw : 0);
    hipLaunchKernelGGL(panel_snapshot_kernel, dim3(panel_blocks(total)), dim3(256), 0, (hipStream_t)stream, seg, n_seg, label, n_label,
                       attn, B, hw, rows, seg_out, (unsigned char*)label_out, rows_out);
    WC_LAUNCH_CHECK("panel_snapshot_kernel");
    return WC_OK;
}
