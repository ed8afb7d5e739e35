/*
 * binder-amd: GPU batch resolver - the two gfx950 kernels.
 *
 * The CPU hit path (server.cpp: parseFast, answerHash, AnswerTable::
 * find, serveHit) done for a whole run of queries at once. Lookups are
 * independent reads of a static table, so one lane takes one query;
 * replies are short byte strings at arbitrary alignment on both ends,
 * so a 16-lane group takes one reply.
 *
 * Data movement of the lookup: a workgroup's kTile queries are one
 * contiguous span of qbuf, fetched into LDS once with 16-byte loads
 * (head and tail peeled bytewise, nothing outside the span is read).
 * Parsing, hashing and the key compare then read the query from LDS
 * bytewise. The dotted key is never materialised: key byte k is wire
 * byte 13 + k, except that an inner length byte reads as '.' (see
 * KeyReader). Slots are read one 16-byte load per probe step.
 *
 * Neither kernel trusts qoff: a tile or query whose offsets are not
 * ascending inside qbuf is left unserved. Both trust the image, which
 * the host has verified (answerimage.hpp).
 */
#include "resolve.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

extern "C" __global__ __launch_bounds__(kTile) void bamd_resolve_lookup(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int64_t qbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena,
    uint32_t* __restrict__ bodyOff, int32_t* __restrict__ rlen) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kTileBytes + 16) / 16];
    uint8_t* tile = (uint8_t*)tile4;

    int32_t t0 = (int32_t)blockIdx.x * kTile;
    int32_t t1 = t0 + kTile < n ? t0 + kTile : n;
    int64_t b0 = qoff[t0], b1 = qoff[t1];
    bool spanOk = b0 >= 0 && b1 >= b0 && b1 <= qbytes;
    /* a span above kTileBytes holds a query above kMaxQuery: leave it
     * in global memory, its lanes parse from there */
    bool staged = spanOk && b1 - b0 <= kTileBytes;
    uint32_t shift = 0;
    if (staged) {
        shift = (uint32_t)(uintptr_t)(qbuf + b0) & 15u;
        loadSpan<kTile>(tile + shift, qbuf + b0, (uint32_t)(b1 - b0));
    }
    __syncthreads();

    int32_t i = t0 + (int32_t)threadIdx.x;
    if (i >= t1) return;
    int64_t o0 = qoff[i], o1 = qoff[i + 1];
    uint32_t off = kUnserved;
    int32_t total = 0;
    if (cap != 0 && spanOk && o0 >= b0 && o1 >= o0 && o1 <= b1 &&
        o1 - o0 <= kMaxQuery) {
        uint32_t len = (uint32_t)(o1 - o0);
        if (staged)
            resolveOne(tile + shift + (uint32_t)(o0 - b0), len, slots, cap,
                       arena, &off, &total);
        else
            resolveOne(qbuf + o0, len, slots, cap, arena, &off, &total);
    }
    bodyOff[i] = off;
    rlen[i] = total;
}

extern "C" __global__ __launch_bounds__(kEmitBlock) void bamd_resolve_emit(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int32_t n, const uint8_t* __restrict__ arena,
    const uint32_t* __restrict__ bodyOff, const int32_t* __restrict__ rlen,
    const int64_t* __restrict__ roff, uint8_t* __restrict__ rbuf,
    uint64_t seed) {
    __shared__ uint8_t order[kGroupsPerBlock][64];
    __shared__ Job jobs[kGroupsPerBlock][kMaxJobs];

    uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    int64_t i = (int64_t)blockIdx.x * kGroupsPerBlock + g;
    uint32_t total = i < n ? (uint32_t)rlen[i] : 0;
    const uint8_t* body = nullptr;
    bool service = false;
    if (total != 0) {
        body = arena + bodyOff[i];
        service = body[0] == 1;
        if (service && lane == 0)
            planService(body, seed, (uint64_t)i, order[g], jobs[g]);
    }
    __syncthreads();  /* the plans are in LDS; no barrier below */
    if (total == 0) return;

    uint8_t* dst = rbuf + roff[i];
    const uint8_t* q = qbuf + qoff[i];
    /* the reply's header: id and RD come from the query */
    const uint8_t* first = service ? body + 6 + 8 * body[1] : body + 4;
    if (lane < 12) {
        uint32_t v = first[lane];
        if (lane < 2) v = q[lane];
        if (lane == 2) v |= q[2] & 1u;
        dst[lane] = (uint8_t)v;
    }
    if (!service) {
        groupCopy(dst + 12, first + 12, total - 12, lane);
        return;
    }
    uint32_t njobs = 1 + 2 * body[1];
    for (uint32_t j = 0; j < njobs; ++j) {
        Job jb = jobs[g][j];
        groupCopy(dst + jb.dst, body + jb.src, jb.len, lane);
    }
}

hipError_t launchLookup(const Batch& b, const Image& img,
                        uint32_t* bodyOff, int32_t* rlen,
                        hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    uint32_t blocks = ((uint32_t)b.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(bamd_resolve_lookup, dim3(blocks), dim3(kTile), 0,
                       stream, b.qbuf, b.qoff, b.qbytes, b.n,
                       (const uint4*)img.slots, img.cap, img.arena, bodyOff,
                       rlen);
    return hipGetLastError();
}

hipError_t launchEmit(const Batch& b, const Image& img,
                      const uint32_t* bodyOff, const int32_t* rlen,
                      const int64_t* roff, uint8_t* rbuf, uint64_t seed,
                      hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    uint32_t blocks =
        ((uint32_t)b.n + kGroupsPerBlock - 1) / kGroupsPerBlock;
    hipLaunchKernelGGL(bamd_resolve_emit, dim3(blocks), dim3(kEmitBlock), 0,
                       stream, b.qbuf, b.qoff, b.n, img.arena, bodyOff, rlen,
                       roff, rbuf, seed);
    return hipGetLastError();
}

}  // namespace bamd::gpu
