// The PASCAL VOC colour of a label, defined once for the kernel files that paint labels (evalfinish.hip, panels.hip):
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
