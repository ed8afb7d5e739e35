/*
 * binder-amd: GPU batch resolver - launcher interface.
 *
 * Two gfx950 kernels (resolve.cpp) resolve a run of wire queries
 * against a device copy of an answer image (answerimage.hpp):
 *
 *   bamd_resolve_lookup  parse, hash, probe, confirm the key; one
 *                        query per lane, kTile queries per workgroup
 *   bamd_resolve_emit    copy or assemble the replies into one packed
 *                        buffer; kGroup lanes per reply
 *
 * Between the two the caller turns rlen into offsets (an inclusive
 * prefix sum) and sizes the reply buffer. The launchers take raw device
 * pointers and a stream; they allocate nothing and do not synchronise.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace bamd::gpu {

/* queries per lookup workgroup, one per lane (2 waves). The tile's
 * bytes are staged in LDS: kTile x 300 = 37.5 KiB, so four workgroups
 * fit a CU's 160 KiB; 256 would give the same residency in half as
 * many, coarser pieces. */
constexpr int kTile = 128;
/* longest query the fast path looks at (fastparse.hpp) */
constexpr int kMaxQuery = 300;
constexpr int kTileBytes = kTile * kMaxQuery;

/* lanes that copy one reply: four replies per wave64. A typical reply
 * is 45-300 bytes, 3-19 dwords a lane-pass; wider groups idle on the
 * short ones. */
constexpr int kGroup = 16;
constexpr int kEmitBlock = 256;
constexpr int kGroupsPerBlock = kEmitBlock / kGroup;

constexpr uint32_t kUnserved = 0xFFFFFFFFu;

struct Batch {
    const uint8_t* qbuf;  /* query bytes end to end */
    const int32_t* qoff;  /* [n + 1] */
    int64_t qbytes;       /* size of qbuf, < 2^31 */
    int32_t n;
};

struct Image {
    const void* slots;    /* cap x { hash u64, off u32, len u32 } */
    uint32_t cap;         /* power of two, or 0 */
    const uint8_t* arena;
};

/* bodyOff[i] = arena offset of query i's answer body or kUnserved,
 * rlen[i] = its reply length or 0 */
hipError_t launchLookup(const Batch& b, const Image& img,
                        uint32_t* bodyOff, int32_t* rlen,
                        hipStream_t stream);

/* roff = [n + 1] prefix sums of rlen; rbuf has roff[n] bytes */
hipError_t launchEmit(const Batch& b, const Image& img,
                      const uint32_t* bodyOff, const int32_t* rlen,
                      const int64_t* roff, uint8_t* rbuf, uint64_t seed,
                      hipStream_t stream);

}  // namespace bamd::gpu
