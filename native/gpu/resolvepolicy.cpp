/*
 * binder-amd: GPU batch resolver - the kernel pair that also writes the
 * server's NOTIMP and REFUSED replies (resolvepolicy.hpp).
 *
 * The lookup is the oversize lookup's tile (resolvedev.hpp,
 * lookupTileExt): one query per lane, the tile's span of qbuf staged in
 * LDS at its global address mod 16, qoff checked per tile and per
 * query. Two things are added. The zone's wire form, a few bytes every
 * in-zone test reads, is staged in LDS beside the tile by the lanes
 * that own its bytes, ahead of the same barrier. And no lane returns
 * above the end: each one classes its query (full, truncated, NOTIMP,
 * REFUSED, unserved), each wave counts a class with one ballot and a
 * popcount, the two waves' counts meet in LDS, and five lanes add the
 * workgroup's sums to the caller's counters, one 64-bit vector atomic
 * per class that occurred. Without a tally the kernel skips all of it on
 * a branch that is the same for every lane.
 *
 * The emit is the oversize emit (resolvelarge.cpp) with a third kind of
 * reply next to "in full" and "truncated". For a synthesized reply the
 * lanes that own the 12 header bytes build them in registers from the
 * query's id and RD and the metadata word's rcode, and the plan is the
 * truncated reply's two jobs: the question from the query, the OPT
 * tail from constant memory. Its body offset is kUnserved and is never
 * turned into a pointer. Two jobs are below kListAbove, so a policy
 * reply is never listed for the drain, and a batch without one takes
 * the oversize emit's path.
 *
 * Trust is the oversize pair's: qoff is checked per tile and per query,
 * the image is believed, the zone is what ZonePolicy validated, and
 * emit reads a query only where the lookup served it and only below the
 * end of the question the lookup found.
 */
#include "resolvepolicy.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

constexpr int kLookupWaves = kTile / 64;

extern "C" __global__ __launch_bounds__(kTile) void bamd_resolve_lookup_pol(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int64_t qbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena, uint32_t accept,
    const uint8_t* __restrict__ zone, uint32_t zlen,
    uint32_t* __restrict__ bodyOff, int32_t* __restrict__ rlen,
    uint32_t* __restrict__ meta, unsigned long long* __restrict__ tally) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kTileBytes + 16) / 16];
    __shared__ uint8_t sZone[kMaxZone + 1];
    __shared__ uint32_t sCount[kLookupWaves][kTallyWords];
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
    for (uint32_t k = threadIdx.x; k < zlen; k += kTile) sZone[k] = zone[k];
    __syncthreads();

    int32_t i = t0 + (int32_t)threadIdx.x;
    uint32_t cls = kTallyWords;  /* a lane behind the batch's end */
    if (i < t1) {
        int64_t o0 = qoff[i], o1 = qoff[i + 1];
        uint32_t off = kUnserved, m = 0;
        int32_t total = 0;
        if (spanOk && o0 >= b0 && o1 >= o0 && o1 <= b1 &&
            o1 - o0 <= kMaxQuery) {
            uint32_t len = (uint32_t)(o1 - o0);
            const uint8_t* q =
                staged ? tile + shift + (uint32_t)(o0 - b0) : qbuf + o0;
            resolveOnePol(q, len, accept, sZone, zlen, slots, cap, arena,
                          &off, &total, &m);
        }
        bodyOff[i] = off;
        rlen[i] = total;
        meta[i] = m;
        cls = total == 0 ? kTallyUnserved
              : (m & kMetaSynth) != 0
                  ? (((m >> kMetaRcodeShift) & kMetaRcodeMask) == kRcodeNotimp
                         ? kTallyNotimp
                         : kTallyRefused)
              : (m & kMetaTrunc) != 0 ? kTallyTruncated
                                      : kTallyFull;
    }
    if (tally == nullptr) return;  /* the same for every lane */

    uint32_t wave = threadIdx.x / 64;
    for (uint32_t c = 0; c < kTallyWords; ++c) {
        uint32_t count = (uint32_t)__popcll(__ballot(cls == c));
        if (threadIdx.x % 64 == 0) sCount[wave][c] = count;
    }
    __syncthreads();
    if (threadIdx.x < kTallyWords) {
        uint32_t sum = 0;
        for (int w = 0; w < kLookupWaves; ++w) sum += sCount[w][threadIdx.x];
        if (sum != 0) atomicAdd(tally + threadIdx.x, (unsigned long long)sum);
    }
}

extern "C" __global__ __launch_bounds__(kEmitBlock)
void bamd_resolve_emit_pol(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int32_t n, const uint8_t* __restrict__ arena,
    const uint32_t* __restrict__ bodyOff, const int32_t* __restrict__ rlen,
    const uint32_t* __restrict__ meta, const int64_t* __restrict__ roff,
    uint8_t* __restrict__ rbuf, uint64_t seed) {
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
        q = qbuf + qo;
        dst = rbuf + ro;
        bool edns = (m & kMetaEdns) != 0, trunc = (m & kMetaTrunc) != 0;
        bool synth = (m & kMetaSynth) != 0;
        if (synth) {
            /* Engine::handle's header as the encoder writes it: QR, AA,
             * RD echoed, RA clear, the rcode; one question, and the OPT
             * in ARCOUNT */
            if (lane < 12) {
                uint32_t v = 0;
                if (lane < 2) v = q[lane];
                if (lane == 2) v = 0x84u | (q[2] & 1u);
                if (lane == 3) v = (m >> kMetaRcodeShift) & kMetaRcodeMask;
                if (lane == 5 || (edns && lane == 11)) v = 1;
                dst[lane] = (uint8_t)v;
            }
        } else {
            /* the oversize emit's header, from the stored reply */
            body = arena + bo;
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
        }
        if (lane == 0) {
            /* question and OPT tail, or the stored reply's plan */
            uint32_t nj =
                synth || trunc
                    ? planTruncated(m, jobs[g])
                    : planReply(body, total - (edns ? kOptLen : 0), m, seed,
                                (uint64_t)i, order[g], jobs[g]);
            njobs[g] = nj;
            sListed[g] = nj > kListAbove;
            if (nj > kListAbove) {
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
            copyJob(jobs[g][j], dst, body, q, lane);
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
            copyJob(jobs[r][j], rdst, rbody, rq, lane);
        dealt += rj;
    }
}

hipError_t launchLookupPol(const Batch& b, const Image& img,
                           uint32_t accept, const uint8_t* zone,
                           uint32_t zlen, uint32_t* bodyOff, int32_t* rlen,
                           uint32_t* meta, unsigned long long* tally,
                           hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if ((accept & ~kAcceptAll) != 0 || zlen > kMaxZone ||
        (zlen != 0 && zone == nullptr))
        return hipErrorInvalidValue;
    uint32_t blocks = ((uint32_t)b.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(bamd_resolve_lookup_pol, dim3(blocks), dim3(kTile), 0,
                       stream, b.qbuf, b.qoff, b.qbytes, b.n,
                       (const uint4*)img.slots, img.cap, img.arena, accept,
                       zone, zlen, bodyOff, rlen, meta, tally);
    return hipGetLastError();
}

hipError_t launchEmitPol(const Batch& b, const Image& img,
                         const uint32_t* bodyOff, const int32_t* rlen,
                         const uint32_t* meta, const int64_t* roff,
                         uint8_t* rbuf, uint64_t seed, hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    uint32_t blocks =
        ((uint32_t)b.n + kGroupsPerBlock - 1) / kGroupsPerBlock;
    hipLaunchKernelGGL(bamd_resolve_emit_pol, dim3(blocks), dim3(kEmitBlock),
                       0, stream, b.qbuf, b.qoff, b.n, img.arena, bodyOff,
                       rlen, meta, roff, rbuf, seed);
    return hipGetLastError();
}

}  // namespace bamd::gpu
