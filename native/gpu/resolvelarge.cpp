/*
 * binder-amd: GPU batch resolver - the kernel pair for replies above
 * 512 bytes and for truncation (resolvelarge.hpp).
 *
 * The lookup is the opt-in lookup (resolveext.cpp), the same code with
 * one decision changed: where that one leaves a hit unserved because of
 * its size, this one holds the reply against what the query may take
 * and serves it in full or truncated (resolveOneExtT<true>). A
 * truncated reply's length needs only the question name's wire length,
 * which the label walk has found by then.
 *
 * The emit has to write replies of 60 bytes and of 4 KiB side by side.
 * A 64-member service is 129 copies of 30 to 90 bytes and two small
 * ones; walked by the one 16-lane group that owns the reply they are
 * 131 rounds on a quarter of a wave while the other fifteen groups of
 * the workgroup, done with their host replies, wait for it. So the
 * copies of a long plan are dealt out to the whole workgroup:
 *
 *   plan   each group's first lane lays its reply out in LDS as the
 *          opt-in emit does (planReply), or as the two jobs of a
 *          truncated reply (planTruncated). A plan above `listAbove`
 *          jobs is listed: the lane leaves the reply's three offsets in
 *          LDS next to the plan. Meanwhile the lanes that own the 12
 *          header bytes write them, TC and the counts in place.
 *   own    behind the one barrier, a group whose plan is not listed
 *          walks it, as in the opt-in emit.
 *   drain  where the workgroup has a listed reply (one 16-byte LDS
 *          read tells), every group walks the listed replies in group
 *          order and takes every sixteenth job of them, counted across
 *          replies so that the rounds stay full where one plan ends and
 *          the next begins. A 64-member reply takes 9 rounds.
 *
 * There is no second barrier: a listed plan is complete at the first,
 * and the copies of different jobs never touch the same byte (groupCopy
 * writes whole dwords only inside its own destination range). Every
 * lane reaches the barrier; nothing returns above it.
 *
 * Trust is the opt-in pair's: qoff is checked per tile and per query,
 * the image is believed, and emit reads a query only where the lookup
 * served it and only below the end of the question the lookup found.
 */
#include "resolvelarge.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

extern "C" __global__ __launch_bounds__(kTile) void bamd_resolve_lookup_lim(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int64_t qbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena, uint32_t accept,
    uint32_t* __restrict__ bodyOff, int32_t* __restrict__ rlen,
    uint32_t* __restrict__ meta) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kTileBytes + 16) / 16];
    lookupTileExt<true>((uint8_t*)tile4, qbuf, qoff, qbytes, n, slots, cap,
                        arena, accept, bodyOff, rlen, meta);
}

__device__ __forceinline__ void runJob(ExtJob jb, uint8_t* dst,
                                       const uint8_t* body, const uint8_t* q,
                                       uint32_t lane) {
    const uint8_t* base = jb.source == kSrcBody    ? body
                          : jb.source == kSrcQuery ? q
                                                   : kOptSrc + 4;
    groupCopy(dst + jb.dst, base + jb.src, jb.len, lane);
}

extern "C" __global__ __launch_bounds__(kEmitBlock)
void bamd_resolve_emit_lim(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int32_t n, const uint8_t* __restrict__ arena,
    const uint32_t* __restrict__ bodyOff, const int32_t* __restrict__ rlen,
    const uint32_t* __restrict__ meta, const int64_t* __restrict__ roff,
    uint8_t* __restrict__ rbuf, uint64_t seed, uint32_t listAbove) {
    __shared__ uint8_t order[kGroupsPerBlock][64];
    __shared__ ExtJob jobs[kGroupsPerBlock][kMaxExtJobs];
    __shared__ uint32_t njobs[kGroupsPerBlock];
    /* of a listed reply: where its body, its query and its bytes lie */
    __shared__ uint32_t sBody[kGroupsPerBlock], sQ[kGroupsPerBlock];
    __shared__ int64_t sDst[kGroupsPerBlock];
    /* one byte per group, read back as one word: is its plan listed */
    __shared__ uint4 sListed4;
    static_assert(kGroupsPerBlock == sizeof(uint4));
    uint8_t* sListed = (uint8_t*)&sListed4;

    uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    int64_t i = (int64_t)blockIdx.x * kGroupsPerBlock + g;
    uint32_t total = i < n ? (uint32_t)rlen[i] : 0;
    const uint8_t *body = nullptr, *q = nullptr;
    uint8_t* dst = nullptr;
    if (total != 0) {
        uint32_t bo = bodyOff[i], m = meta[i];
        int32_t qo = qoff[i];
        int64_t ro = roff[i];
        body = arena + bo;
        q = qbuf + qo;
        dst = rbuf + ro;
        bool edns = (m & kMetaEdns) != 0, trunc = (m & kMetaTrunc) != 0;
        /* the reply's header: id and RD come from the query. In full,
         * an OPT behind the reply counts in ARCOUNT, bytes 10 and 11,
         * big-endian; truncated, TC is set and the counts are the
         * question's and the OPT's alone */
        const uint8_t* first =
            body[0] == 1 ? body + 6 + 8 * body[1] : body + 4;
        if (lane < 12) {
            uint32_t v = first[lane];
            if (lane < 2) v = q[lane];
            if (lane == 2) v |= (q[2] & 1u) | (trunc ? 2u : 0u);
            if (trunc) {
                if (lane >= 4) v = 0;
                if (lane == 5 || (edns && lane == 11)) v = 1;
            } else {
                if (edns && lane == 11) v += 1;
                if (edns && lane == 10) v += first[11] == 0xFF;
            }
            dst[lane] = (uint8_t)v;
        }
        if (lane == 0) {
            uint32_t nj =
                trunc ? planTruncated(m, jobs[g])
                      : planReply(body, total - (edns ? kOptLen : 0), m, seed,
                                  (uint64_t)i, order[g], jobs[g]);
            njobs[g] = nj;
            sListed[g] = nj > listAbove;
            if (nj > listAbove) {
                sBody[g] = bo;
                sQ[g] = (uint32_t)qo;
                sDst[g] = ro;
            }
        }
    } else if (lane == 0) {
        njobs[g] = 0;
        sListed[g] = 0;
    }
    __syncthreads();  /* the plans are in LDS; no barrier below */

    uint4 listed = sListed4;
    if (sListed[g] == 0) {
        uint32_t nj = njobs[g];
        for (uint32_t j = 0; j < nj; ++j)
            runJob(jobs[g][j], dst, body, q, lane);
    }
    if ((listed.x | listed.y | listed.z | listed.w) == 0) return;

    uint32_t dealt = 0;  /* jobs of listed replies handed out so far */
    for (uint32_t r = 0; r < (uint32_t)kGroupsPerBlock; ++r) {
        if (sListed[r] == 0) continue;
        uint32_t rj = njobs[r];
        const uint8_t* rbody = arena + sBody[r];
        const uint8_t* rq = qbuf + sQ[r];
        uint8_t* rdst = rbuf + sDst[r];
        for (uint32_t j = (g - dealt) % kGroupsPerBlock; j < rj;
             j += kGroupsPerBlock)
            runJob(jobs[r][j], rdst, rbody, rq, lane);
        dealt += rj;
    }
}

hipError_t launchLookupLim(const Batch& b, const Image& img,
                           uint32_t accept, uint32_t* bodyOff,
                           int32_t* rlen, uint32_t* meta,
                           hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if ((accept & ~kAcceptAll) != 0) return hipErrorInvalidValue;
    uint32_t blocks = ((uint32_t)b.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(bamd_resolve_lookup_lim, dim3(blocks), dim3(kTile), 0,
                       stream, b.qbuf, b.qoff, b.qbytes, b.n,
                       (const uint4*)img.slots, img.cap, img.arena, accept,
                       bodyOff, rlen, meta);
    return hipGetLastError();
}

hipError_t launchEmitLim(const Batch& b, const Image& img,
                         const uint32_t* bodyOff, const int32_t* rlen,
                         const uint32_t* meta, const int64_t* roff,
                         uint8_t* rbuf, uint64_t seed, uint32_t listAbove,
                         hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    uint32_t blocks =
        ((uint32_t)b.n + kGroupsPerBlock - 1) / kGroupsPerBlock;
    hipLaunchKernelGGL(bamd_resolve_emit_lim, dim3(blocks), dim3(kEmitBlock),
                       0, stream, b.qbuf, b.qoff, b.n, img.arena, bodyOff,
                       rlen, meta, roff, rbuf, seed, listAbove);
    return hipGetLastError();
}

}  // namespace bamd::gpu
