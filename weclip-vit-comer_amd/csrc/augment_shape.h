// Where image b of a batch lies and how large it is, for both forms of the device input pipeline (augment.hip,
// augment_seg.hip).  One set of kernels serves both; they are templates over RAGGED, so the uniform instantiation compiles
// to the code it was before the ragged form existed.
//   uniform: src (B, Hs, Ws, 3) dense, every image Hs x Ws (wc_augment_normalize, wc_seg_augment)
//   ragged:  src packed, image b is sizes[b] = {H, W} HWC at byte offsets[b]; its label map (H, W) lies at byte
//            offsets[b] / 3 of the label buffer (wc_augment_normalize_ragged, wc_seg_augment_ragged)
// The tables are device memory, so they are checked here, on the device: an image that does not lie inside the buffer is
// reported as !ok with a 1 x 1 extent at offset 0 -- the kernels then poison it (NaN image, ignore label) and never read
// outside [0, src_bytes).
#pragma once

#define AUG_MAX_SIDE 16384

struct AugShape {
    int H, W;
    long off;           // byte offset of the image; off / 3 is the pixel offset of its label map
    bool ok;
};

template <bool RAGGED>
__device__ __forceinline__ AugShape aug_shape(int b, int Hs, int Ws, const long long* __restrict__ offsets,
                                              const int* __restrict__ sizes, long src_bytes) {
    AugShape s;
    if constexpr (RAGGED) {
        s.H = sizes[2 * b];
        s.W = sizes[2 * b + 1];
        s.off = (long)offsets[b];
        s.ok = s.H >= 1 && s.W >= 1 && s.H <= AUG_MAX_SIDE && s.W <= AUG_MAX_SIDE && s.off >= 0 && s.off % 3 == 0 &&
               s.off <= src_bytes && (long)s.H * s.W * 3 <= src_bytes - s.off;
        if (!s.ok) {
            s.H = s.W = 1;
            s.off = 0;
        }
    } else {
        s.H = Hs;
        s.W = Ws;
        s.off = (long)b * Hs * Ws * 3;
        s.ok = true;
    }
    return s;
}
