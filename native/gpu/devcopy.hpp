/*
 * binder-amd: the two device copy routines of the GPU batch resolver,
 * shared by the resolve kernels (resolve.cpp) and the update kernels
 * (update.cpp). Device code only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include "resolve.hpp"

namespace bamd::gpu {

/* A workgroup of kThreads copies nbytes from src to dst, where
 * dst - src is a multiple of 16 (dst is in LDS): 16-byte loads over
 * the aligned middle, bytes at both ends, nothing outside
 * [src, src + nbytes) read. */
template <int kThreads>
__device__ __forceinline__ void loadSpan(uint8_t* dst, const uint8_t* src,
                                         uint32_t nbytes) {
    uint32_t tid = threadIdx.x;
    uint32_t head = (16u - ((uint32_t)(uintptr_t)src & 15u)) & 15u;
    if (head > nbytes) head = nbytes;
    for (uint32_t k = tid; k < head; k += kThreads) dst[k] = src[k];
    uint32_t mid = (nbytes - head) / 16;
    const uint4* s4 = (const uint4*)(src + head);
    uint4* d4 = (uint4*)(dst + head);
    for (uint32_t k = tid; k < mid; k += kThreads) d4[k] = s4[k];
    for (uint32_t k = head + mid * 16 + tid; k < nbytes; k += kThreads)
        dst[k] = src[k];
}

/* kGroup lanes copy n bytes, both ends at any alignment: bytes up to
 * dst's dword boundary, whole dwords to the aligned middle of dst
 * (from two aligned source dwords when src sits off by `sh` bytes),
 * bytes for the rest. Reads at most 3 bytes before src, which the
 * callers keep inside the blob, and none past src + n. */
__device__ __forceinline__ void groupCopy(uint8_t* d, const uint8_t* s,
                                          uint32_t n, uint32_t lane) {
    uint32_t head = (uint32_t)(-(intptr_t)d) & 3u;
    if (head > n) head = n;
    if (lane < head) d[lane] = s[lane];
    d += head;
    s += head;
    n -= head;
    uint32_t m = n >> 2;
    uint32_t sh = (uint32_t)(uintptr_t)s & 3u;
    /* the last shifted dword would read 4 - sh bytes past its own end:
     * leave it to the tail when the source does not have them */
    if (sh != 0 && m != 0 && (n & 3u) < 4u - sh) --m;
    uint32_t* d4 = (uint32_t*)d;
    if (sh == 0) {
        const uint32_t* s4 = (const uint32_t*)s;
        for (uint32_t j = lane; j < m; j += kGroup) d4[j] = s4[j];
    } else {
        const uint32_t* s4 = (const uint32_t*)(s - sh);
        uint32_t r = 8 * sh;
        for (uint32_t j = lane; j < m; j += kGroup)
            d4[j] = (s4[j] >> r) | (s4[j + 1] << (32 - r));
    }
    uint32_t done = 4 * m;  /* n - done < 8 */
    if (lane < n - done) d[done + lane] = s[done + lane];
}

}  // namespace bamd::gpu
