/*
 * binder-amd: GPU batch resolver - the fused gfx950 kernel
 * (resolvefused.hpp): a tile of queries from wire bytes to reply bytes
 * in one workgroup.
 *
 * Stage. The tile's span of qbuf comes into LDS once, as in the lookup
 * kernels, by all kFusedBlock lanes. It stays there to the end: the
 * emit takes id, RD and an echoed name from it, so a query is read from
 * global memory once.
 *
 * Look up. The first kFusedWaves waves take one query per lane, with
 * resolveOne (accept == 0) or resolveOneExt; `accept` is the same for
 * every lane. Body offset, reply length, meta word and the query's
 * offset go to LDS, five words per query with the scan's result; none
 * of them reaches global memory.
 *
 * Place. Each lookup wave scans its 64 lengths by cross-lane moves
 * (log2 64 = 6 steps of shuffle-up and add); the waves' sums meet in
 * LDS, where every lane adds those of the waves before its own. Lane 0
 * claims [base, base + total) with one atomicAdd on the cursor and
 * shares base and the verdict on capacity through LDS. A tile with no
 * hit claims nothing.
 *
 * Emit. kFusedGroups groups of kGroup lanes, one per query of the
 * tile, so a tile's replies are written side by side and not in rounds:
 * measured on one tile, rounds that wait for their slowest reply were
 * most of the kernel's time. A wire reply with no echo and no OPT is
 * the header lanes and one groupCopy. Anything else is laid out by the
 * group's first lane as planReply's jobs. A reply may take kMaxExtJobs
 * of them, which for every group at once would be 67 KiB, so the jobs
 * come from one pool of kFusedPool in LDS: the planning lane reserves
 * 2 x members + 3 with an LDS atomicAdd, and a group that finds the pool
 * spent waits for the next pass, when the pool is empty again. The
 * first reservation of a pass always fits, so every pass writes a reply;
 * the usual tile needs one. Two barriers a pass fence the plans from the
 * copies before and after them; the verdict "another pass" is one LDS
 * word per pass parity, so every lane meets every barrier.
 *
 * Trust is the pairs': qoff is checked per tile and per query, the
 * image is believed. Every write to rbuf lies in the tile's claim, and
 * a claim that ends past `capacity` is not written at all.
 */
#include "resolvefused.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

/* the first reservation of a pass must fit */
static_assert(kFusedPool >= kMaxExtJobs);

extern "C" __global__ __launch_bounds__(kFusedBlock) void bamd_resolve_fused(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int64_t qbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena, uint32_t accept,
    uint64_t seed, uint8_t* __restrict__ rbuf, uint64_t capacity,
    unsigned long long* __restrict__ cursor, int64_t* __restrict__ rstart,
    int32_t* __restrict__ rlen) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kFusedTileBytes + 16) / 16];
    __shared__ uint32_t sBody[kFusedTile], sLen[kFusedTile],
        sMeta[kFusedTile], sQ[kFusedTile], sStart[kFusedTile];
    __shared__ uint32_t sWaveSum[kFusedWaves], sWaveHits[kFusedWaves];
    __shared__ unsigned long long sBase;
    __shared__ uint32_t sTotal, sFits;
    __shared__ uint8_t order[kFusedGroups][64];
    __shared__ ExtJob pool[kFusedPool];
    __shared__ uint32_t sJobAt[kFusedGroups], njobs[kFusedGroups];
    __shared__ uint32_t sPoolUsed, sMore[2];
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
                uint32_t len = (uint32_t)(o1 - o0);
                const uint8_t* q =
                    staged ? tile + shift + (uint32_t)(o0 - b0) : qbuf + o0;
                if (accept == 0)
                    resolveOne(q, len, slots, cap, arena, &off, &total);
                else
                    resolveOneExt(q, len, accept, slots, cap, arena, &off,
                                  &total, &m);
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

    /* the waves' sums, then the claim */
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
        if (tid == 0) sMore[(pass + 1) & 1] = 0;
        uint32_t len = r < cnt ? sLen[r] : 0;
        const uint8_t* body = nullptr;
        bool edns = false, planned = false;
        if (len != 0) {
            body = arena + sBody[r];
            uint32_t m = sMeta[r];
            edns = (m & kMetaEdns) != 0;
            planned = body[0] == 1 || (m & (kMetaEdns | kMetaFolded)) != 0;
            if (lane == 0) {
                uint32_t at = 0;
                if (planned) {
                    uint32_t need = 3 + (body[0] == 1 ? 2u * body[1] : 0u);
                    at = atomicAdd(&sPoolUsed, need);
                    if (at + need > (uint32_t)kFusedPool) at = kNoRoom;
                }
                if (planned && at != kNoRoom)
                    njobs[g] = planReply(body, len - (edns ? kOptLen : 0), m,
                                         seed, (uint64_t)(t0 + (int32_t)r),
                                         order[g], pool + at);
                sJobAt[g] = at;
                /* every writer stores the same 1 */
                if (at == kNoRoom || r + kFusedGroups < cnt)
                    sMore[pass & 1] = 1;
            }
        }
        __syncthreads();  /* the plans are in LDS */
        bool more = sMore[pass & 1] != 0;
        uint32_t at = len != 0 ? sJobAt[g] : kNoRoom;
        if (at != kNoRoom) {
            uint8_t* dst = rbuf + base + sStart[r];
            const uint8_t* q = staged
                                   ? tile + shift + (sQ[r] - (uint32_t)b0)
                                   : qbuf + sQ[r];
            /* the reply's header: id and RD come from the query, and an
             * OPT behind the reply counts in ARCOUNT, bytes 10 and 11 */
            const uint8_t* first =
                body[0] == 1 ? body + 6 + 8 * body[1] : body + 4;
            if (lane < 12) {
                uint32_t v = first[lane];
                if (lane < 2) v = q[lane];
                if (lane == 2) v |= q[2] & 1u;
                if (edns && lane == 11) v += 1;
                if (edns && lane == 10) v += first[11] == 0xFF;
                dst[lane] = (uint8_t)v;
            }
            if (!planned) {
                groupCopy(dst + 12, first + 12, len - 12, lane);
            } else {
                uint32_t nj = njobs[g];
                for (uint32_t j = 0; j < nj; ++j) {
                    ExtJob jb = pool[at + j];
                    const uint8_t* src = jb.source == kSrcBody    ? body
                                         : jb.source == kSrcQuery ? q
                                                                  : kOptSrc + 4;
                    groupCopy(dst + jb.dst, src + jb.src, jb.len, lane);
                }
            }
            r += kFusedGroups;
        }
        if (!more) break;
    }
}

hipError_t launchFused(const Batch& b, const Image& img, uint32_t accept,
                       uint64_t seed, uint8_t* rbuf, uint64_t capacity,
                       uint64_t* cursor, int64_t* rstart, int32_t* rlen,
                       hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if ((accept & ~kAcceptAll) != 0 || capacity >= (1ull << 63))
        return hipErrorInvalidValue;
    uint32_t blocks = ((uint32_t)b.n + kFusedTile - 1) / kFusedTile;
    hipLaunchKernelGGL(bamd_resolve_fused, dim3(blocks), dim3(kFusedBlock),
                       0, stream, b.qbuf, b.qoff, b.qbytes, b.n,
                       (const uint4*)img.slots, img.cap, img.arena, accept,
                       seed, rbuf, capacity, (unsigned long long*)cursor,
                       rstart, rlen);
    return hipGetLastError();
}

}  // namespace bamd::gpu
