/*
 * binder-amd: GPU batch resolver - the fused gfx950 kernel for a run of
 * bsock1 frames (resolveframes.hpp): a tile of frames from the bytes of
 * the ring to the bytes of REPLY frames in one workgroup.
 *
 *   stage   the tile's span of the run goes into LDS at its global
 *           address mod 16 (loadSpan); a span above kFramesTileBytes
 *           stays where it is and its lanes read global memory.
 *   check   one frame per lane of the first wave: the index ascends
 *           inside the run, the frame is a QUERY of the length the index
 *           says, its DNS message 30 bytes in has 17 to kMaxQuery bytes.
 *   look up resolveOneExtT<true> on that message, held against
 *           kTcpLimit when the frame's proto byte is not 0.
 *   place   a served frame takes kFrameReplyAt + its DNS reply's bytes:
 *           in-wave scan, wave sums in LDS, one 64-bit atomicAdd per
 *           tile; a claim that fits raises the stream's end (atomicMax).
 *   miss    the first wave ballots the frames it leaves unserved,
 *           reserves their room with one atomicAdd and writes their
 *           batch indices.
 *   emit    resolvefusedlim.cpp's passes over one job pool: plan, own,
 *           drain, the same two barriers a pass. Jobs count from the
 *           DNS reply's start, kFrameReplyAt bytes into the frame, so a
 *           16-bit dst holds the longest one. The lanes of a group own
 *           the frame's first 22 bytes instead of the reply's 12: lanes
 *           0..15 store the 10 bytes of frame header and the DNS
 *           header's first 6, lanes 0..5 its other 6; no byte is
 *           written twice.
 *
 * Trust: foff is checked per tile and per frame, the type and length
 * bytes of a frame are believed only where they agree with it, the
 * image is believed. Every write to rbuf lies in the tile's claim, and
 * a claim that ends past `capacity` is not written at all; miss[] takes
 * at most one entry per frame. groupCopy may read 3 bytes in front of a
 * source: inside the blob or kOptSrc as before, and 12 bytes into a
 * query that has 30 bytes of its own frame in front of it.
 */
#include "resolveframes.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

/* the first reservation of a pass must fit, the jobs cut off included */
static_assert(kFusedPool >=
              kMaxExtJobs + (kLargeReply + kOptLen) / kFusedMinChunk);
static_assert(kFusedGroups <= 64 && kGroup >= kFrameReplyAt + 6);
/* ExtJob::dst */
static_assert(kLargeReply + kOptLen <= 0xFFFF);

/* byte j of a reply's 12 header bytes: id and RD come from the query.
 * In full, an OPT behind the reply counts in ARCOUNT, bytes 10 and 11,
 * big-endian; truncated, TC is set and the counts are the question's
 * and the OPT's alone. `first` is the stored reply's header. */
static __device__ __forceinline__ uint32_t headerByte(
    uint32_t j, const uint8_t* first, const uint8_t* q, bool edns,
    bool trunc) {
    uint32_t v = first[j];
    if (j < 2) v = q[j];
    if (j == 2) v |= (q[2] & 1u) | (trunc ? 2u : 0u);
    if (trunc) {
        if (j >= 4) v = 0;
        if (j == 5 || (edns && j == 11)) v = 1;
    } else {
        if (edns && j == 11) v += 1;
        if (edns && j == 10) v += first[11] == 0xFF;
    }
    return v;
}

extern "C" __global__ __launch_bounds__(kFusedBlock)
void bamd_resolve_frames(
    const uint8_t* __restrict__ fbuf, const int32_t* __restrict__ foff,
    int64_t fbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena, uint32_t accept,
    uint64_t seed, uint8_t* __restrict__ rbuf, uint64_t capacity,
    unsigned long long* __restrict__ cursor, int64_t* __restrict__ rstart,
    int32_t* __restrict__ rlen, int32_t* __restrict__ miss,
    uint32_t listAbove, uint32_t chunk) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kFramesTileBytes + 16) / 16];
    /* of a frame: its answer body, its DNS reply's length, the meta
     * word, where its DNS message lies in fbuf, where its REPLY frame
     * starts in the tile's claim */
    __shared__ uint32_t sBody[kFusedTile], sLen[kFusedTile],
        sMeta[kFusedTile], sQ[kFusedTile], sStart[kFusedTile];
    __shared__ uint32_t sWaveSum[kFusedWaves], sWaveHits[kFusedWaves];
    __shared__ unsigned long long sBase;
    __shared__ uint32_t sTotal, sFits;
    __shared__ uint8_t order[kFusedGroups][64];
    __shared__ ExtJob pool[kFusedPool];
    __shared__ uint32_t sJobAt[kFusedGroups], njobs[kFusedGroups],
        sReply[kFusedGroups];
    __shared__ uint32_t sPoolUsed, sMore[2];
    __shared__ unsigned long long sListed[2];
    uint8_t* tile = (uint8_t*)tile4;

    uint32_t tid = threadIdx.x;
    int32_t t0 = (int32_t)blockIdx.x * kFusedTile;
    int32_t t1 = t0 + kFusedTile < n ? t0 + kFusedTile : n;
    uint32_t cnt = (uint32_t)(t1 - t0);
    int64_t b0 = foff[t0], b1 = foff[t1];
    bool spanOk = b0 >= 0 && b1 >= b0 && b1 <= fbytes;
    bool staged = spanOk && b1 - b0 <= kFramesTileBytes;
    uint32_t shift = 0;
    if (staged) {
        shift = (uint32_t)(uintptr_t)(fbuf + b0) & 15u;
        loadSpan<kFusedBlock>(tile + shift, fbuf + b0, (uint32_t)(b1 - b0));
    }
    __syncthreads();

    /* check, look up, and scan inside the wave; whole waves take this
     * branch */
    int32_t i = t0 + (int32_t)tid;
    int32_t total = 0;   /* the DNS reply's bytes */
    uint32_t flen = 0;   /* the REPLY frame's */
    uint32_t excl = 0;
    if (tid < (uint32_t)kFusedTile) {
        uint32_t off = kUnserved, m = 0;
        int64_t o0 = 0;
        if (i < t1) {
            o0 = foff[i];
            int64_t o1 = foff[i + 1];
            int64_t len = o1 - o0;
            if (cap != 0 && spanOk && o0 >= b0 && o1 >= o0 && o1 <= b1 &&
                len >= kFrameQueryAt + 17 &&
                len <= kFrameQueryAt + kMaxQuery) {
                const uint8_t* f =
                    staged ? tile + shift + (uint32_t)(o0 - b0) : fbuf + o0;
                uint32_t plen = f[2] | ((uint32_t)f[3] << 8) |
                                ((uint32_t)f[4] << 16) |
                                ((uint32_t)f[5] << 24);
                if (f[0] == 0xB5 && f[1] == 1 &&
                    plen == (uint32_t)len - kFrameHead)
                    resolveOneExtT<true>(
                        f + kFrameQueryAt, (uint32_t)len - kFrameQueryAt,
                        accept, slots, cap, arena, &off, &total, &m,
                        f[kFrameHead + 5] == 0 ? 0u : kTcpLimit);
            }
        }
        if (total != 0) flen = (uint32_t)total + kFrameReplyAt;
        uint32_t lane64 = tid & 63u, wave = tid >> 6;
        uint32_t incl = flen;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            uint32_t up = __shfl_up(incl, d, 64);
            if (lane64 >= d) incl += up;
        }
        excl = incl - flen;
        uint32_t hits = (uint32_t)__popcll(__ballot(flen != 0));
        if (lane64 == 63) sWaveSum[wave] = incl;
        if (lane64 == 0) sWaveHits[wave] = hits;
        sBody[tid] = off;
        sLen[tid] = (uint32_t)total;
        sMeta[tid] = m;
        /* read only where the frame is served */
        sQ[tid] = (uint32_t)o0 + kFrameQueryAt;
    }
    __syncthreads();

    /* the waves' sums, then the claim: at most kFusedTile x
     * kFramesReplyMax bytes, far inside 32 bits */
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
        if (fits && sum != 0) atomicMax(cursor + 2, base + sum);
        sBase = base;
        sTotal = sum;
        sFits = fits;
        sMore[0] = sMore[1] = 0;
        sListed[0] = sListed[1] = 0;
    }
    __syncthreads();
    unsigned long long base = sBase;
    bool fits = sFits != 0;
    if (tid < (uint32_t)kFusedTile) {
        bool left = i < t1 && (flen == 0 || !fits);
        if (i < t1) {
            rstart[i] = (int64_t)(base + excl);
            rlen[i] = left ? 0 : (int32_t)flen;
        }
        /* the miss list: a wave's entries lie together, in frame order */
        unsigned long long mask = __ballot(left);
        uint32_t lane64 = tid & 63u;
        uint32_t at = 0;
        if (lane64 == 0 && mask != 0)
            at = (uint32_t)atomicAdd(cursor + 3,
                                     (unsigned long long)__popcll(mask));
        at = __shfl(at, 0, 64);
        if (left)
            miss[at + (uint32_t)__popcll(mask & ((1ull << lane64) - 1))] = i;
    }
    if (!fits || sTotal == 0) return;  /* the whole workgroup */

    uint32_t g = tid / kGroup, lane = tid % kGroup;
    uint32_t r = g;  /* this group's next frame */
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
            uint8_t* frame = rbuf + base + sStart[r];
            uint8_t* dst = frame + kFrameReplyAt;  /* the DNS reply */
            const uint8_t* q = staged
                                   ? tile + shift + (sQ[r] - (uint32_t)b0)
                                   : fbuf + sQ[r];
            const uint8_t* first =
                body[0] == 1 ? body + 6 + 8 * body[1] : body + 4;
            /* the owned prefix: magic, REPLY, payload_len, the QUERY's
             * req_id, then the reply's header */
            uint32_t plen = len + kFrameReplyHead;
            uint32_t v;
            if (lane < 2)
                v = lane == 0 ? 0xB5u : 2u;
            else if (lane < (uint32_t)kFrameHead)
                v = plen >> (8 * (lane - 2));
            else if (lane < (uint32_t)kFrameReplyAt)
                v = q[(int32_t)lane - kFrameQueryAt];
            else
                v = headerByte(lane - kFrameReplyAt, first, q, edns, trunc);
            frame[lane] = (uint8_t)v;
            if (lane < kFrameReplyAt + 12 - kGroup)
                dst[lane + kGroup - kFrameReplyAt] = (uint8_t)headerByte(
                    lane + kGroup - kFrameReplyAt, first, q, edns, trunc);
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
                                    : fbuf + sQ[lr];
            uint8_t* ldst = rbuf + base + sStart[lr] + kFrameReplyAt;
            for (uint32_t j = (g - dealt) % kFusedGroups; j < lj;
                 j += kFusedGroups)
                copyJob(pool[lat + j], ldst, lbody, lq, lane);
            dealt += lj;
        }
        if (!more) break;
    }
}

hipError_t launchFrames(const Batch& b, const Image& img, uint32_t accept,
                        uint64_t seed, uint8_t* rbuf, uint64_t capacity,
                        uint64_t* cursor, int64_t* rstart, int32_t* rlen,
                        int32_t* miss, uint32_t listAbove, uint32_t chunk,
                        hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if ((accept & ~kAcceptAll) != 0 || capacity >= (1ull << 63) ||
        chunk < kFusedMinChunk)
        return hipErrorInvalidValue;
    uint32_t blocks = ((uint32_t)b.n + kFusedTile - 1) / kFusedTile;
    hipLaunchKernelGGL(bamd_resolve_frames, dim3(blocks), dim3(kFusedBlock),
                       0, stream, b.qbuf, b.qoff, b.qbytes, b.n,
                       (const uint4*)img.slots, img.cap, img.arena, accept,
                       seed, rbuf, capacity, (unsigned long long*)cursor,
                       rstart, rlen, miss, listAbove, chunk);
    return hipGetLastError();
}

}  // namespace bamd::gpu
