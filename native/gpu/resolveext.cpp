/*
 * binder-amd: GPU batch resolver - the opt-in kernel pair for EDNS0
 * and mixed-case queries (resolveext.hpp).
 *
 * The lookup is the base lookup (resolve.cpp) with three changes. The
 * label walk folds 'A'-'Z' when kAcceptAnycase is set and remembers
 * that it did; hash and key compare read the name through FoldReader,
 * so no lowercase copy of the name is made in LDS or registers. With
 * kAcceptEdns an ARCOUNT of 1 is let through, and the 11 fixed bytes
 * of an OPT record are checked right behind the question, from the
 * same staged bytes; every read is below the query's own length, so
 * the staged and the unstaged tile need no separate care. A hit is
 * then held against the advertised size, and its length grows by the
 * server's OPT. `accept` is a kernel argument: the branches on it are
 * the same for every lane.
 *
 * The emit keeps one 16-lane group per reply and the base copy
 * routine. What changes is the plan: the group's first lane lays out
 * every reply, wire or service, as jobs { source, src, dst, len } in
 * LDS, where source says which base `src` counts from - the answer
 * body in the arena, the query, or the constant OPT record. The 12
 * header bytes are still written by the lanes that own them, with
 * ARCOUNT's carry worked out from the stored bytes 10 and 11.
 *
 * Trust is the base pair's: qoff is checked per tile and per query,
 * the image is believed, and emit reads a query only where the lookup
 * served it and only below the name length the lookup found in it.
 */
#include "resolveext.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

extern "C" __global__ __launch_bounds__(kTile) void bamd_resolve_lookup_ext(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int64_t qbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena, uint32_t accept,
    uint32_t* __restrict__ bodyOff, int32_t* __restrict__ rlen,
    uint32_t* __restrict__ meta) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kTileBytes + 16) / 16];
    uint8_t* tile = (uint8_t*)tile4;

    lookupTileExt<false>(tile, qbuf, qoff, qbytes, n, slots, cap, arena,
                         accept, bodyOff, rlen, meta);
}

extern "C" __global__ __launch_bounds__(kEmitBlock)
void bamd_resolve_emit_ext(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int32_t n, const uint8_t* __restrict__ arena,
    const uint32_t* __restrict__ bodyOff, const int32_t* __restrict__ rlen,
    const uint32_t* __restrict__ meta, const int64_t* __restrict__ roff,
    uint8_t* __restrict__ rbuf, uint64_t seed) {
    __shared__ uint8_t order[kGroupsPerBlock][64];
    __shared__ ExtJob jobs[kGroupsPerBlock][kMaxExtJobs];
    __shared__ uint32_t njobs[kGroupsPerBlock];

    uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    int64_t i = (int64_t)blockIdx.x * kGroupsPerBlock + g;
    uint32_t total = i < n ? (uint32_t)rlen[i] : 0;
    const uint8_t* body = nullptr;
    bool edns = false;
    if (total != 0) {
        body = arena + bodyOff[i];
        uint32_t m = meta[i];
        edns = (m & kMetaEdns) != 0;
        if (lane == 0)
            njobs[g] = planReply(body, total - (edns ? kOptLen : 0), m, seed,
                                 (uint64_t)i, order[g], jobs[g]);
    }
    __syncthreads();  /* the plans are in LDS; no barrier below */
    if (total == 0) return;

    uint8_t* dst = rbuf + roff[i];
    const uint8_t* q = qbuf + qoff[i];
    /* the reply's header: id and RD come from the query, and an OPT
     * behind the reply counts in ARCOUNT, bytes 10 and 11, big-endian */
    const uint8_t* first = body[0] == 1 ? body + 6 + 8 * body[1] : body + 4;
    if (lane < 12) {
        uint32_t v = first[lane];
        if (lane < 2) v = q[lane];
        if (lane == 2) v |= q[2] & 1u;
        if (edns && lane == 11) v += 1;
        if (edns && lane == 10) v += first[11] == 0xFF;
        dst[lane] = (uint8_t)v;
    }
    uint32_t nj = njobs[g];
    for (uint32_t j = 0; j < nj; ++j) {
        ExtJob jb = jobs[g][j];
        const uint8_t* base = jb.source == kSrcBody    ? body
                              : jb.source == kSrcQuery ? q
                                                       : kOptSrc + 4;
        groupCopy(dst + jb.dst, base + jb.src, jb.len, lane);
    }
}

hipError_t launchLookupExt(const Batch& b, const Image& img,
                           uint32_t accept, uint32_t* bodyOff,
                           int32_t* rlen, uint32_t* meta,
                           hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if ((accept & ~kAcceptAll) != 0) return hipErrorInvalidValue;
    uint32_t blocks = ((uint32_t)b.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(bamd_resolve_lookup_ext, dim3(blocks), dim3(kTile), 0,
                       stream, b.qbuf, b.qoff, b.qbytes, b.n,
                       (const uint4*)img.slots, img.cap, img.arena, accept,
                       bodyOff, rlen, meta);
    return hipGetLastError();
}

hipError_t launchEmitExt(const Batch& b, const Image& img,
                         const uint32_t* bodyOff, const int32_t* rlen,
                         const uint32_t* meta, const int64_t* roff,
                         uint8_t* rbuf, uint64_t seed, hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    uint32_t blocks =
        ((uint32_t)b.n + kGroupsPerBlock - 1) / kGroupsPerBlock;
    hipLaunchKernelGGL(bamd_resolve_emit_ext, dim3(blocks), dim3(kEmitBlock),
                       0, stream, b.qbuf, b.qoff, b.n, img.arena, bodyOff,
                       rlen, meta, roff, rbuf, seed);
    return hipGetLastError();
}

}  // namespace bamd::gpu
