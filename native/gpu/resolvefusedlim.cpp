/*
 * binder-amd: GPU batch resolver - the fused gfx950 kernel for replies
 * above 512 bytes and for truncation (resolvefusedlim.hpp): a tile of
 * queries from wire bytes to reply bytes in one workgroup.
 *
 * Stage, look up and place are the fused kernel's (resolvefused.cpp),
 * with resolveOneExtT<true> for every accept: a hit is held against
 * what its query may take and served in full or truncated, and
 * kMetaTrunc rides in the meta word. A reply is up to 4096 bytes and a
 * tile's replies up to 256 KiB, so lengths and offsets inside the tile
 * are 32-bit words in LDS; only ExtJob::dst, which counts from the
 * reply's start, is 16 bits.
 *
 * Emit, in passes over one job pool in LDS as in the fused kernel:
 *
 *   plan   each group's first lane reserves room in the pool and lays
 *          its reply out there (planReply, or planTruncated: the echoed
 *          question comes from the staged tile like any echo). A copy
 *          of the reply's head (the echoed name, and the stored head
 *          of a service or the body of a wire reply) above `chunk`
 *          bytes keeps its first `chunk` bytes and the rest goes into
 *          further jobs behind the plan (splitJobs); the order of jobs
 *          means nothing, no two touch the same byte. The members'
 *          segments, 30 to 90 bytes each, are not looked at: a scan of
 *          all 131 jobs by the one planning lane cost more than it
 *          saved (profiles/GPURESOLVE.md). The reservation counts the
 *          cuts: a plan of j jobs over b bytes cuts into at most
 *          j + b / chunk. A plan that was cut, or has more
 *          than `listAbove` jobs, is listed: one bit per group in a
 *          64-bit LDS word. Meanwhile the lanes that own the 12 header
 *          bytes write them, TC and the counts in place.
 *   own    behind the barrier a group whose reply is not listed walks
 *          its plan, or makes the one copy of a short wire reply with
 *          no echo and no OPT, which has no plan.
 *   drain  every group reads the listed word; a tile with nothing
 *          listed is done with that one LDS read. Else every group
 *          walks the listed replies in group order and takes every
 *          kFusedGroups-th job of them, counted across replies so that
 *          the rounds stay full where one plan ends and the next
 *          begins. A 64-member service takes 3 rounds and a 4096-byte
 *          wire reply in chunks of 256 bytes one round of 16 groups.
 *
 * The barriers are the fused kernel's two a pass: the listed word and
 * the verdict "another pass" are one LDS word each per pass parity, so
 * every lane meets every barrier. The first reservation of a pass
 * always fits, so every pass writes a reply.
 *
 * Trust is the fused kernel's: qoff is checked per tile and per query,
 * the image is believed. Every write to rbuf lies in the tile's claim,
 * and a claim that ends past `capacity` is not written at all.
 * groupCopy may read 3 bytes in front of a source: a plan's jobs keep
 * that inside the blob, the query or kOptSrc as before, and a cut job
 * starts `chunk` bytes or more into its source.
 */
#include "resolvefusedlim.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

/* the first reservation of a pass must fit, the jobs cut off included */
static_assert(kFusedPool >= kMaxExtJobs + kLargeReply / kFusedMinChunk);
/* one bit per group in the listed word */
static_assert(kFusedGroups <= 64);

extern "C" __global__ __launch_bounds__(kFusedBlock)
void bamd_resolve_fused_lim(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int64_t qbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena, uint32_t accept,
    uint64_t seed, uint8_t* __restrict__ rbuf, uint64_t capacity,
    unsigned long long* __restrict__ cursor, int64_t* __restrict__ rstart,
    int32_t* __restrict__ rlen, uint32_t listAbove, uint32_t chunk) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kFusedTileBytes + 16) / 16];
    __shared__ uint32_t sBody[kFusedTile], sLen[kFusedTile],
        sMeta[kFusedTile], sQ[kFusedTile], sStart[kFusedTile];
    __shared__ uint32_t sWaveSum[kFusedWaves], sWaveHits[kFusedWaves];
    __shared__ unsigned long long sBase;
    __shared__ uint32_t sTotal, sFits;
    __shared__ uint8_t order[kFusedGroups][64];
    __shared__ ExtJob pool[kFusedPool];
    /* of a group's reply in this pass: where its jobs lie, how many, and
     * for a listed one which reply it is */
    __shared__ uint32_t sJobAt[kFusedGroups], njobs[kFusedGroups],
        sReply[kFusedGroups];
    __shared__ uint32_t sPoolUsed, sMore[2];
    __shared__ unsigned long long sListed[2];
    uint8_t* tile = (uint8_t*)tile4;

    uint32_t tid = threadIdx.x;
    int32_t t0 = (int32_t)blockIdx.x * kFusedTile;
    int32_t t1 = t0 + kFusedTile < n ? t0 + kFusedTile : n;
    uint32_t cnt = (uint32_t)(t1 - t0);
    int64_t b0 = qoff[t0], b1 = qoff[t1];
    bool spanOk = b0 >= 0 && b1 >= b0 && b1 <= qbytes;
    /* a span above kFusedTileBytes holds a query above kMaxQuery: leave
     * it in global memory, its lanes parse and echo from there */
    bool staged = spanOk && b1 - b0 <= kFusedTileBytes;
    uint32_t shift = 0;
    if (staged) {
        shift = (uint32_t)(uintptr_t)(qbuf + b0) & 15u;
        loadSpan<kFusedBlock>(tile + shift, qbuf + b0, (uint32_t)(b1 - b0));
    }
    __syncthreads();

    /* look up, and scan inside the wave; whole waves take this branch */
    int32_t i = t0 + (int32_t)tid;
    int32_t total = 0;
    uint32_t excl = 0;
    if (tid < (uint32_t)kFusedTile) {
        uint32_t off = kUnserved, m = 0;
        int64_t o0 = 0;
        if (i < t1) {
            o0 = qoff[i];
            int64_t o1 = qoff[i + 1];
            if (cap != 0 && spanOk && o0 >= b0 && o1 >= o0 && o1 <= b1 &&
                o1 - o0 <= kMaxQuery) {
                const uint8_t* q =
                    staged ? tile + shift + (uint32_t)(o0 - b0) : qbuf + o0;
                resolveOneExtT<true>(q, (uint32_t)(o1 - o0), accept, slots,
                                     cap, arena, &off, &total, &m);
            }
        }
        uint32_t lane64 = tid & 63u, wave = tid >> 6;
        uint32_t incl = (uint32_t)total;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            uint32_t up = __shfl_up(incl, d, 64);
            if (lane64 >= d) incl += up;
        }
        excl = incl - (uint32_t)total;
        uint32_t hits = (uint32_t)__popcll(__ballot(total != 0));
        if (lane64 == 63) sWaveSum[wave] = incl;
        if (lane64 == 0) sWaveHits[wave] = hits;
        sBody[tid] = off;
        sLen[tid] = (uint32_t)total;
        sMeta[tid] = m;
        sQ[tid] = (uint32_t)o0;  /* read only where the query is served */
    }
    __syncthreads();

    /* the waves' sums, then the claim: at most kFusedTile x kLargeReply
     * bytes, far inside 32 bits */
    if (tid < (uint32_t)kFusedTile) {
        for (uint32_t w = 0; w < (tid >> 6); ++w) excl += sWaveSum[w];
        sStart[tid] = excl;
    }
    if (tid == 0) {
        uint32_t sum = 0, hits = 0;
        for (uint32_t w = 0; w < (uint32_t)kFusedWaves; ++w) {
            sum += sWaveSum[w];
            hits += sWaveHits[w];
        }
        unsigned long long base = 0;
        if (sum != 0) base = atomicAdd(cursor, (unsigned long long)sum);
        bool fits = base + sum <= capacity;
        if (!fits) atomicAdd(cursor + 1, (unsigned long long)hits);
        sBase = base;
        sTotal = sum;
        sFits = fits;
        sMore[0] = sMore[1] = 0;
        sListed[0] = sListed[1] = 0;
    }
    __syncthreads();
    unsigned long long base = sBase;
    bool fits = sFits != 0;
    if (tid < (uint32_t)kFusedTile && i < t1) {
        rstart[i] = (int64_t)(base + excl);
        rlen[i] = fits ? total : 0;
    }
    if (!fits || sTotal == 0) return;  /* the whole workgroup */

    uint32_t g = tid / kGroup, lane = tid % kGroup;
    uint32_t r = g;  /* this group's next reply */
    for (uint32_t pass = 0;; ++pass) {
        while (r < cnt && sLen[r] == 0) r += kFusedGroups;
        if (tid == 0) sPoolUsed = 0;
        __syncthreads();  /* last pass's copies are done */
        if (tid == 0) {
            sMore[(pass + 1) & 1] = 0;
            sListed[(pass + 1) & 1] = 0;
        }
        uint32_t len = r < cnt ? sLen[r] : 0;
        const uint8_t* body = nullptr;
        bool edns = false, trunc = false, planned = false;
        if (len != 0) {
            body = arena + sBody[r];
            uint32_t m = sMeta[r];
            edns = (m & kMetaEdns) != 0;
            trunc = (m & kMetaTrunc) != 0;
            planned = body[0] == 1 || len - 12 > chunk ||
                      (m & (kMetaEdns | kMetaFolded | kMetaTrunc)) != 0;
            if (lane == 0) {
                uint32_t at = 0;
                if (planned) {
                    uint32_t need =
                        trunc ? 2u : 3 + (body[0] == 1 ? 2u * body[1] : 0u);
                    if (len > chunk) need += len / chunk;
                    at = atomicAdd(&sPoolUsed, need);
                    if (at + need > (uint32_t)kFusedPool) at = kNoRoom;
                }
                if (planned && at != kNoRoom) {
                    uint32_t nj =
                        trunc ? planTruncated(m, pool + at)
                              : planReply(body, len - (edns ? kOptLen : 0),
                                          m, seed,
                                          (uint64_t)(t0 + (int32_t)r),
                                          order[g], pool + at);
                    /* all but the members' segments and the OPT tail */
                    uint32_t cut = nj;
                    if (len > chunk)
                        cut = splitJobs(
                            pool + at, nj,
                            trunc ? nj
                                  : nj - (body[0] == 1 ? 2u * body[1] : 0u) -
                                        (edns ? 1u : 0u),
                            chunk);
                    njobs[g] = cut;
                    if (cut != nj || cut > listAbove) {
                        sReply[g] = r;
                        atomicOr(&sListed[pass & 1], 1ull << g);
                    }
                }
                sJobAt[g] = at;
                /* every writer stores the same 1 */
                if (at == kNoRoom || r + kFusedGroups < cnt)
                    sMore[pass & 1] = 1;
            }
        }
        __syncthreads();  /* the plans are in LDS */
        bool more = sMore[pass & 1] != 0;
        unsigned long long listed = sListed[pass & 1];
        uint32_t at = len != 0 ? sJobAt[g] : kNoRoom;
        if (at != kNoRoom) {
            uint8_t* dst = rbuf + base + sStart[r];
            const uint8_t* q = staged
                                   ? tile + shift + (sQ[r] - (uint32_t)b0)
                                   : qbuf + sQ[r];
            /* the reply's header: id and RD come from the query. In
             * full, an OPT behind the reply counts in ARCOUNT, bytes 10
             * and 11, big-endian; truncated, TC is set and the counts
             * are the question's and the OPT's alone */
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
            if (!planned) {
                groupCopy(dst + 12, first + 12, len - 12, lane);
            } else if (((listed >> g) & 1) == 0) {
                uint32_t nj = njobs[g];
                for (uint32_t j = 0; j < nj; ++j)
                    copyJob(pool[at + j], dst, body, q, lane);
            }
            r += kFusedGroups;
        }
        /* the listed replies' jobs, dealt out to every group */
        uint32_t dealt = 0;
        while (listed != 0) {
            uint32_t lg = (uint32_t)__ffsll((long long)listed) - 1;
            listed &= listed - 1;
            uint32_t lr = sReply[lg], lat = sJobAt[lg], lj = njobs[lg];
            const uint8_t* lbody = arena + sBody[lr];
            const uint8_t* lq = staged
                                    ? tile + shift + (sQ[lr] - (uint32_t)b0)
                                    : qbuf + sQ[lr];
            uint8_t* ldst = rbuf + base + sStart[lr];
            for (uint32_t j = (g - dealt) % kFusedGroups; j < lj;
                 j += kFusedGroups)
                copyJob(pool[lat + j], ldst, lbody, lq, lane);
            dealt += lj;
        }
        if (!more) break;
    }
}

hipError_t launchFusedLim(const Batch& b, const Image& img, uint32_t accept,
                          uint64_t seed, uint8_t* rbuf, uint64_t capacity,
                          uint64_t* cursor, int64_t* rstart, int32_t* rlen,
                          uint32_t listAbove, uint32_t chunk,
                          hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if ((accept & ~kAcceptAll) != 0 || capacity >= (1ull << 63) ||
        chunk < kFusedMinChunk)
        return hipErrorInvalidValue;
    uint32_t blocks = ((uint32_t)b.n + kFusedTile - 1) / kFusedTile;
    hipLaunchKernelGGL(bamd_resolve_fused_lim, dim3(blocks),
                       dim3(kFusedBlock), 0, stream, b.qbuf, b.qoff, b.qbytes,
                       b.n, (const uint4*)img.slots, img.cap, img.arena,
                       accept, seed, rbuf, capacity,
                       (unsigned long long*)cursor, rstart, rlen, listAbove,
                       chunk);
    return hipGetLastError();
}

}  // namespace bamd::gpu
