// row4_dev.h -- what the streaming kernels of perm.hip and lookup.hip share on the device side: four consecutive words of a
// column as one 16-byte access where the layout allows (VEC), word by word with a bound otherwise; the alignment tests of
// their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <bool VEC>
__device__ __forceinline__ void perm_load4(const uint32_t *__restrict__ src, uint64_t at, uint64_t len, uint32_t v[4]) {
    if (VEC) {
        const uint4 t = *(const uint4 *)(src + at);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = at + q < len ? src[at + q] : 0u;
    }
}
template <bool VEC>
__device__ __forceinline__ void perm_store4(uint32_t *__restrict__ dst, uint64_t at, uint64_t len, const uint32_t v[4]) {
    if (VEC) {
        *(uint4 *)(dst + at) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (at + q < len) dst[at + q] = v[q];
    }
}
inline bool al16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
