/*
 * binder-amd: GPU batch resolver - the gfx950 kernels that update the
 * device answer table in place (see update.hpp for the work split).
 *
 * The CPU table deletes by shifting the rest of a probe chain back, a
 * serial walk. Here a removed slot is marked instead: { hash 0, off =
 * tomb, len = 2 }, where the two bytes at `tomb` are zero. The lookup
 * kernel needs no change for it - len != 0 keeps the chain unbroken,
 * and the blob's qtype byte 0 matches no query - and only compaction
 * takes tombstones out again; inserts never reuse them, so a chain
 * never loses a slot between two compactions.
 *
 * Concurrency inside one launch. Lanes of an invalidate launch only
 * ever write tombstones, and two that meet write the same bytes; the
 * write is an exchange, so only the lane that saw the live slot counts
 * it. Lanes of an insert launch claim an empty slot with one 64-bit
 * compare-and-swap on its { off, len } half and store the hash after
 * it. Every blob of the batch lies at or above `used`, so a walker
 * that finds off >= used knows the slot belongs to another lane of
 * this launch without reading its hash, which may not be there yet;
 * keys are distinct within a delta, so it is not the walker's key and
 * it steps on. A lane that loses the compare-and-swap gets the slot's
 * new value back and judges it again. Only len == 0 says empty: the
 * host table leaves old hash and off behind in the slots it clears.
 *
 * All stores are plain vector stores or HIP atomics.
 */
#include "update.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"

namespace bamd::gpu {

namespace {

using u64 = unsigned long long;

/* the { off, len } half of slot idx: off in the low word */
__device__ __forceinline__ u64* halfOf(uint4* slots, uint32_t idx) {
    return (u64*)slots + 2 * (size_t)idx + 1;
}
__device__ __forceinline__ u64 packHalf(uint32_t off, uint32_t len) {
    return ((u64)len << 32) | off;
}

/* op i's span [*o0, *o1) of a buffer of `bytes`, or false: its own two
 * offsets and the one before it must ascend inside the buffer */
__device__ __forceinline__ bool opSpan(const int32_t* off, int32_t i,
                                       int32_t bytes, int64_t* o0,
                                       int64_t* o1) {
    int64_t prev = i > 0 ? off[i - 1] : 0;
    *o0 = off[i];
    *o1 = off[i + 1];
    return prev >= 0 && prev <= *o0 && *o0 < *o1 && *o1 <= bytes;
}

/* Turn slot idx into a tombstone; blk[] takes the count and the bytes
 * if this lane was the one to end a live slot. */
__device__ __forceinline__ void bury(uint4* slots, uint32_t idx,
                                     uint32_t tomb, uint32_t* blk) {
    u64 old = atomicExch(halfOf(slots, idx), packHalf(tomb, kTombLen));
    ((u64*)slots)[2 * (size_t)idx] = 0;
    uint32_t len = (uint32_t)(old >> 32);
    if (len != kTombLen) {
        atomicAdd(&blk[kCntTombstones], 1u);
        atomicAdd(&blk[kCntDeadBytes], len);
    }
}

/* One domain: AnswerTable::remove(hashA, 1, dom) and removeSuffix(
 * hash33, 33, dom) with tombstones for the backward shift. */
__device__ __forceinline__ void invalidateOne(
    const uint8_t* dom, uint32_t slen, uint64_t hashA, uint64_t hash33,
    uint4* slots, uint32_t cap, const uint8_t* arena, uint32_t tomb,
    uint32_t* blk) {
    uint32_t mask = cap - 1;
    uint32_t lo = (uint32_t)hashA, hi = (uint32_t)(hashA >> 32);
    uint32_t idx = lo & mask;
    for (uint32_t step = 0; step < cap; ++step, idx = (idx + 1) & mask) {
        uint4 s = slots[idx];  /* hash lo, hash hi, off, len */
        if (s.w == 0) break;
        if (s.w == kTombLen || s.x != lo || s.y != hi) continue;
        const uint8_t* b = arena + s.z;
        if (b[0] != slen || b[1] != 1) continue;
        bool same = true;
        for (uint32_t k = 0; k < slen && same; ++k)
            same = b[2 + k] == dom[k];
        if (!same) continue;
        bury(slots, idx, tomb, blk);
        break;
    }
    lo = (uint32_t)hash33;
    hi = (uint32_t)(hash33 >> 32);
    idx = lo & mask;
    for (uint32_t step = 0; step < cap; ++step, idx = (idx + 1) & mask) {
        uint4 s = slots[idx];
        if (s.w == 0) break;
        if (s.w == kTombLen || s.x != lo || s.y != hi) continue;
        const uint8_t* b = arena + s.z;
        uint32_t klen = b[0];
        if (b[1] != 33 || klen < slen) continue;
        const uint8_t* tail = b + 2 + klen - slen;
        if (klen != slen && tail[-1] != '.') continue;
        bool same = true;
        for (uint32_t k = 0; k < slen && same; ++k)
            same = tail[k] == dom[k];
        if (same) bury(slots, idx, tomb, blk);
    }
}

/* One blob of the batch, `len` bytes at arena offset `at` (>= used). */
__device__ __forceinline__ void insertOne(
    uint32_t at, uint32_t len, uint64_t h, uint4* slots, uint32_t cap,
    const uint8_t* arena, uint32_t used, uint32_t* blk) {
    const uint8_t* nb = arena + at;
    uint32_t keyBytes = 2u + nb[0];  /* klen, qtype, key */
    if (len < keyBytes + 4) return;  /* verifyBlob's "short blob" */
    u64 mine = packHalf(at, len);
    uint32_t mask = cap - 1;
    uint32_t idx = (uint32_t)h & mask;
    u64* half = halfOf(slots, idx);
    u64 cur = __hip_atomic_load(half, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t step = 0; step < cap;) {
        uint32_t off = (uint32_t)cur, slen = (uint32_t)(cur >> 32);
        if (slen == 0) {
            u64 seen = atomicCAS(half, cur, mine);
            if (seen == cur) {
                ((u64*)slots)[2 * (size_t)idx] = h;
                atomicAdd(&blk[kCntClaims], 1u);
                return;
            }
            cur = seen;  /* lost: the same slot again, as it is now */
            continue;
        }
        /* a slot from before this batch: is it this key? */
        if (slen != kTombLen && off < used &&
            ((const u64*)slots)[2 * (size_t)idx] == h) {
            const uint8_t* b = arena + off;
            bool same = true;
            for (uint32_t k = 0; k < keyBytes && same; ++k)
                same = b[k] == nb[k];
            if (same) {
                __hip_atomic_store(half, mine, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                atomicAdd(&blk[kCntReplaced], 1u);
                atomicAdd(&blk[kCntDeadBytes], slen);
                return;
            }
        }
        ++step;
        idx = (idx + 1) & mask;
        half = halfOf(slots, idx);
        cur = __hip_atomic_load(half, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* a workgroup's counts, gathered in LDS, go out as one atomic each */
__device__ __forceinline__ void flushCounts(const uint32_t* blk,
                                            uint32_t* counters) {
    __syncthreads();
    uint32_t t = threadIdx.x;
    if (t < (uint32_t)kCounters && blk[t] != 0)
        atomicAdd(&counters[t], blk[t]);
}

}  // namespace

extern "C" __global__ __launch_bounds__(kOpBlock) void
bamd_update_invalidate(uint4* slots, uint32_t cap,
                       const uint8_t* __restrict__ arena, uint32_t tomb,
                       uint32_t* __restrict__ counters,
                       const uint8_t* __restrict__ ibuf,
                       const int32_t* __restrict__ ioff, int32_t ibytes,
                       const uint64_t* __restrict__ ihash, int32_t n) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kOpTileBytes + 16) / 16];
    __shared__ uint32_t blk[kCounters];
    uint8_t* tile = (uint8_t*)tile4;

    int32_t t0 = (int32_t)blockIdx.x * kOpBlock;
    int32_t t1 = t0 + kOpBlock < n ? t0 + kOpBlock : n;
    int64_t b0 = ioff[t0], b1 = ioff[t1];
    /* a span that is not one ascending stretch of ibuf stays in global
     * memory; its lanes check their own offsets below */
    bool staged = b0 >= 0 && b1 >= b0 && b1 <= ibytes &&
                  b1 - b0 <= kOpTileBytes;
    uint32_t shift = 0;
    if (staged) {
        shift = (uint32_t)(uintptr_t)(ibuf + b0) & 15u;
        loadSpan<kOpBlock>(tile + shift, ibuf + b0, (uint32_t)(b1 - b0));
    }
    if (threadIdx.x < (uint32_t)kCounters) blk[threadIdx.x] = 0;
    __syncthreads();

    int32_t i = t0 + (int32_t)threadIdx.x;
    int64_t o0, o1;
    if (i < t1 && opSpan(ioff, i, ibytes, &o0, &o1) &&
        o1 - o0 <= kMaxDomain) {
        uint32_t slen = (uint32_t)(o1 - o0);
        uint64_t hA = ihash[2 * (size_t)i], h33 = ihash[2 * (size_t)i + 1];
        if (staged && o0 >= b0 && o1 <= b1)
            invalidateOne(tile + shift + (uint32_t)(o0 - b0), slen, hA, h33,
                          slots, cap, arena, tomb, blk);
        else
            invalidateOne(ibuf + o0, slen, hA, h33, slots, cap, arena, tomb,
                          blk);
    }
    flushCounts(blk, counters);
}

extern "C" __global__ __launch_bounds__(kOpBlock) void bamd_update_insert(
    uint4* slots, uint32_t cap, const uint8_t* arena, uint32_t used,
    uint32_t* __restrict__ counters,
    const int32_t* __restrict__ uoff, int32_t ubytes,
    const uint64_t* __restrict__ uhash, int32_t n) {
    __shared__ uint32_t blk[kCounters];
    if (threadIdx.x < (uint32_t)kCounters) blk[threadIdx.x] = 0;
    __syncthreads();

    int32_t i = (int32_t)blockIdx.x * kOpBlock + (int32_t)threadIdx.x;
    int64_t o0, o1;
    if (i < n && opSpan(uoff, i, ubytes, &o0, &o1))
        insertOne(used + (uint32_t)o0, (uint32_t)(o1 - o0), uhash[i], slots,
                  cap, arena, used, blk);
    flushCounts(blk, counters);
}

extern "C" __global__ __launch_bounds__(kScanBlock) void bamd_update_scan(
    const uint4* __restrict__ slots, uint32_t cap,
    int32_t* __restrict__ lens, u64* __restrict__ totals) {
    __shared__ uint32_t blk[2];
    if (threadIdx.x < 2) blk[threadIdx.x] = 0;
    __syncthreads();
    uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    if (i < cap) {
        uint32_t len = slots[i].w;
        if (len == kTombLen) len = 0;
        lens[i] = (int32_t)len;
        if (len != 0) {
            atomicAdd(&blk[0], 1u);
            atomicAdd(&blk[1], len);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && blk[threadIdx.x] != 0)
        atomicAdd(&totals[threadIdx.x], (u64)blk[threadIdx.x]);
}

extern "C" __global__ __launch_bounds__(kEmitBlock) void bamd_update_move(
    const uint4* __restrict__ slots, uint32_t cap,
    const uint8_t* __restrict__ arena, const int32_t* __restrict__ lens,
    const int64_t* __restrict__ incl, uint4* __restrict__ nslots,
    uint32_t ncap, uint8_t* __restrict__ narena, uint32_t ntomb,
    uint32_t* __restrict__ counters) {
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)kCounters) {
        counters[threadIdx.x] = 0;
        if (threadIdx.x < kTombLen) narena[ntomb + threadIdx.x] = 0;
    }
    uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    uint64_t i = (uint64_t)blockIdx.x * kGroupsPerBlock + g;
    if (i >= cap) return;
    uint32_t len = (uint32_t)lens[i];
    if (len == 0) return;
    uint4 s = slots[i];
    uint32_t at = (uint32_t)(incl[i] - len);
    groupCopy(narena + at, arena + s.z, len, lane);
    if (lane != 0) return;
    /* keys are distinct: the first empty slot from home is the place */
    u64 mine = packHalf(at, len);
    uint32_t mask = ncap - 1;
    uint32_t idx = s.x & mask;
    for (uint32_t step = 0; step < ncap; ++step, idx = (idx + 1) & mask) {
        if (atomicCAS(halfOf(nslots, idx), 0ull, mine) != 0ull) continue;
        ((u64*)nslots)[2 * (size_t)idx] = ((u64)s.y << 32) | s.x;
        return;
    }
}

hipError_t launchInvalidate(const Table& t, const uint8_t* ibuf,
                            const int32_t* ioff, int32_t ibytes,
                            const uint64_t* ihash, int32_t n,
                            hipStream_t stream) {
    if (n <= 0 || t.cap == 0) return hipSuccess;
    uint32_t blocks = ((uint32_t)n + kOpBlock - 1) / kOpBlock;
    hipLaunchKernelGGL(bamd_update_invalidate, dim3(blocks), dim3(kOpBlock),
                       0, stream, (uint4*)t.slots, t.cap, t.arena, t.tomb,
                       t.counters, ibuf, ioff, ibytes, ihash, n);
    return hipGetLastError();
}

hipError_t launchInsert(const Table& t, uint32_t used, const int32_t* uoff,
                        int32_t ubytes, const uint64_t* uhash, int32_t n,
                        hipStream_t stream) {
    if (n <= 0 || t.cap == 0) return hipSuccess;
    uint32_t blocks = ((uint32_t)n + kOpBlock - 1) / kOpBlock;
    hipLaunchKernelGGL(bamd_update_insert, dim3(blocks), dim3(kOpBlock), 0,
                       stream, (uint4*)t.slots, t.cap, t.arena, used,
                       t.counters, uoff, ubytes, uhash, n);
    return hipGetLastError();
}

hipError_t launchScan(const Table& t, int32_t* lens,
                      unsigned long long* totals, hipStream_t stream) {
    if (t.cap == 0) return hipSuccess;
    uint32_t blocks = (t.cap + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(bamd_update_scan, dim3(blocks), dim3(kScanBlock), 0,
                       stream, (const uint4*)t.slots, t.cap, lens, totals);
    return hipGetLastError();
}

hipError_t launchMove(const Table& from, const int32_t* lens,
                      const int64_t* incl, const Table& to,
                      hipStream_t stream) {
    /* an empty table still gets its tombstone blob and counters */
    uint32_t blocks = (from.cap + kGroupsPerBlock - 1) / kGroupsPerBlock;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(bamd_update_move, dim3(blocks), dim3(kEmitBlock), 0,
                       stream, (const uint4*)from.slots, from.cap,
                       from.arena, lens, incl, (uint4*)to.slots, to.cap,
                       to.arena, to.tomb, to.counters);
    return hipGetLastError();
}

}  // namespace bamd::gpu
