// args_dev.h -- what the kernels of args.hip and xargs.hip share on the device side: the workgroup scan of a column build's
// block and scan launches, and what the scan and propagation launches read of a list.
#pragma once
#include <hip/hip_runtime.h>

#include "args_core.h"

// of a list the scan and propagation launches read the kinds alone; passed to the kernels by value
struct ArgsScanDev {
    uint32_t A, g_m;   // arguments; g in Montgomery form
    uint32_t kind[SMI_ARGS_MAX];
};

// the workgroup scan of args_core.h (args_scan_step) between barriers; returns the lane's EXCLUSIVE prefix and the
// workgroup's aggregate.  sc: 2 x 4 x PERM_BLOCK words of LDS.  perm is uniform over the workgroup.
__device__ __forceinline__ Fq args_wg_scan(bool perm, Fq v, uint32_t (*sc)[4][PERM_BLOCK], uint32_t tid, uint32_t g_m, const Fp &F, Fq *total) {
    __syncthreads();   // the buffers of the scan before are consumed
#pragma unroll
    for (int e = 0; e < 4; e++) sc[0][e][tid] = v.c[e];
    __syncthreads();
    int cur = 0;
    for (uint32_t off = 1; off < PERM_BLOCK; off <<= 1) {
        args_scan_step(perm, sc[cur], sc[cur ^ 1], tid, off, g_m, F);
        __syncthreads();
        cur ^= 1;
    }
    *total = perm_scan_at(sc[cur], PERM_BLOCK - 1);
    return tid ? perm_scan_at(sc[cur], tid - 1) : args_identity(perm, F);
}
