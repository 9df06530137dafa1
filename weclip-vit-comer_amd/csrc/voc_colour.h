// The PASCAL VOC colour of a label, defined once for the kernel files that paint labels (evalfinish.hip, panels.hip, camseed.hip):
// bit j of v (j = 0..7) goes to bit 7 - j/3 of channel j % 3 (reference utils/imutils.py:136-154 `colormap`).
#pragma once
#include "common.h"

// (r, g, b) of label v packed as r | g << 8 | b << 16 (utils/imutils.py:142-151)
__device__ __forceinline__ unsigned int ef_colour(unsigned int v) {
    unsigned int r = 0, g = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        r |= ((v >> 0) & 1u) << (7 - j);
        g |= ((v >> 1) & 1u) << (7 - j);
        b |= ((v >> 2) & 1u) << (7 - j);
        v >>= 3;
    }
    return r | (g << 8) | (b << 16);
}

// 4 labels -> the uint8 map and the RGB image at pixels [i, i + n) of a row-major grid.  Full groups whose first pixel is
// 4-byte aligned in the output go out as one 32-bit and three 32-bit vector stores (neighbouring lanes write neighbouring words),
// the rest by bytes.
__device__ __forceinline__ void ef_store(const unsigned int* lab, int n, long i, unsigned char* __restrict__ u8,
                                         unsigned char* __restrict__ rgb) {
    if (u8) {
        if (n == 4 && ((size_t)(u8 + i) & 3) == 0) {
            *reinterpret_cast<unsigned int*>(u8 + i) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
        } else {
            for (int k = 0; k < n; ++k) u8[i + k] = (unsigned char)lab[k];
        }
    }
    if (rgb) {
        unsigned int c[4] = {0, 0, 0, 0};
        for (int k = 0; k < n; ++k) c[k] = ef_colour(lab[k]);
        if (n == 4 && ((size_t)(rgb + 3 * i) & 3) == 0) {
            unsigned int* o = reinterpret_cast<unsigned int*>(rgb + 3 * i);
            o[0] = c[0] | (c[1] << 24);
            o[1] = (c[1] >> 8) | (c[2] << 16);
            o[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
            for (int k = 0; k < n; ++k) {
                rgb[3 * (i + k) + 0] = (unsigned char)(c[k] & 255u);
                rgb[3 * (i + k) + 1] = (unsigned char)((c[k] >> 8) & 255u);
                rgb[3 * (i + k) + 2] = (unsigned char)(c[k] >> 16);
            }
        }
    }
}
