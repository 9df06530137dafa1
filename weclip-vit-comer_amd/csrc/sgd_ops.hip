// SGD-with-momentum step over many parameter tensors in ONE launch (reference utils/optimizer.py:35-65 = torch.optim.SGD
// with momentum 0.9 and a scheduled lr): the sibling of adamw_multi_kernel (train_ops.hip), same table form, same grid.
#include "common.h"

// the table's pointers are device allocations: typed as global memory, so that the accesses are global_load / global_store
// (a pointer made from an integer is generic otherwise, and its accesses flat ones, which also tie up lgkmcnt)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// table: count rows of 8 int64 {param, grad, momentum_buffer, n, 0, 0, 0, 0}.
// Update order of torch.optim.SGD with dampening 0, no Nesterov, no maximize:
//   g' = g + wd*p;  buf = mu*buf + g';  p -= lr*buf
// A first step is the same arithmetic on a zero buffer (mu*0 + g' = g' exactly, torch's clone(g')): no "first" flag.
// grad is only read.  12 bytes in and 8 out per element; every load of an iteration is issued before its arithmetic.
__global__ __launch_bounds__(256) void sgd_multi_kernel(const long* __restrict__ table, float lr, float mu, float wd) {
    const long* e = table + (long)blockIdx.y * 8;
    gf32* p = (gf32*)e[0];
    const gf32* g = (const gf32*)e[1];
    gf32* b = (gf32*)e[2];
    const long n = e[3];
    if (((n & 3) | (((uintptr_t)p | (uintptr_t)g | (uintptr_t)b) & 15)) == 0) {
        // four elements per thread and access (16-byte IO); element-wise arithmetic unchanged
        for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
            const f32x4 g4 = *(const gf32x4*)(g + i), p4 = *(const gf32x4*)(p + i);
            const f32x4 b4 = *(const gf32x4*)(b + i);
            const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, pp[4] = {p4.x, p4.y, p4.z, p4.w};
            const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
            float po[4], bo[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float gd = gg[k] + wd * pp[k];
                bo[k] = mu * bb[k] + gd;
                po[k] = pp[k] - lr * bo[k];
            }
            *(gf32x4*)(p + i) = f32x4{po[0], po[1], po[2], po[3]};
            *(gf32x4*)(b + i) = f32x4{bo[0], bo[1], bo[2], bo[3]};
        }
        return;
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float gi = g[i], pi = p[i], bi = b[i];
        const float gd = gi + wd * pi;
        const float bn = mu * bi + gd;
        p[i] = pi - lr * bn;
        b[i] = bn;
    }
}

// Hyper-parameters arrive as doubles and are rounded once to fp32 (the kernel uses lr, momentum and weight_decay as they are).
extern "C" int wc_sgd_multi(const int64_t* table, int count, double lr, double momentum, double weight_decay,
                            int blocks_per_tensor, void* stream) {
    WC_CHECK_ARG(table && count > 0 && count <= 65535 && blocks_per_tensor > 0 && momentum >= 0.0 && momentum < 1.0 &&
                     lr >= 0.0 && __builtin_isfinite(lr) && weight_decay >= 0.0 && __builtin_isfinite(weight_decay),
                 "wc_sgd_multi: bad argument");
    hipLaunchKernelGGL(sgd_multi_kernel, dim3(blocks_per_tensor, count), dim3(256), 0, (hipStream_t)stream, (const long*)table,
                       (float)lr, (float)momentum, (float)weight_decay);
    WC_LAUNCH_CHECK("sgd_multi_kernel");
    return WC_OK;
}
