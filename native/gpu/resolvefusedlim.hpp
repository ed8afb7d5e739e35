/*
 * binder-amd: GPU batch resolver - the fused kernel for bursts on an
 * image with a raised reply ceiling (answerrules.hpp: up to 4096
 * bytes), and for truncation.
 *
 *   bamd_resolve_fused_lim  bamd_resolve_fused (resolvefused.hpp) with
 *                           the server's size decision where that one
 *                           gives up, and with long replies written by
 *                           the whole workgroup instead of one group
 *
 * Queries are accepted, and hits served in full or truncated, exactly as
 * by the oversize pair (resolvelarge.hpp), for any accept in
 * 0..kAcceptAll. Placing, the cursor, `capacity` and the outputs are the
 * fused kernel's: a tile's replies lie end to end in query order, a
 * tile that finds no room writes nothing and counts its hits in
 * cursor[1]. A tile's claim is now up to kFusedTile x 4096 bytes.
 *
 * The fused kernel gives every reply of the tile one group of kGroup
 * lanes, which is right for replies of 30 to 500 bytes. Two kinds of
 * reply would keep one group busy while the other 63 wait at the pass
 * barrier, and are dealt out to all kFusedGroups groups instead:
 *
 *   long plans    a 64-member service is 131 copies of 30 to 90 bytes:
 *                 131 rounds for one group, 3 when dealt out
 *   long copies   a 4096-byte wire reply is one copy of 1021 dwords: 64
 *                 rounds for sixteen lanes. A copy of a reply's head
 *                 (echoed name, service head, wire body) above `chunk`
 *                 bytes is cut into jobs of `chunk` bytes, and those
 *                 are dealt out like any job
 *
 * LDS: the fused kernel's 40.5 KiB (the span 18.8 KiB, the pool 16 KiB,
 * member orders 4 KiB, five words per query) and one more word per
 * group and 16 bytes of listed-reply masks. Compiled for gfx950 the
 * kernel takes 68 VGPRs, 41800 bytes of LDS and no scratch (the fused
 * kernel, by the same compiler: 60 VGPRs, 41528 bytes): as there, one
 * workgroup of sixteen waves is resident per CU.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "resolvefused.hpp"

namespace bamd::gpu {

/* A reply whose plan has more jobs than this is listed: dealt out to
 * all groups. Its own group walks j jobs in j rounds; dealt out they
 * take ceil(j / kFusedGroups). The oversize emit's value
 * (resolvelarge.hpp): no reply of at most 512 bytes gets there, so a
 * tile of small replies lists nothing. */
constexpr uint32_t kFusedListAbove = 32;
/* A copy of a reply's head above this many bytes is cut into jobs of
 * this many, and its reply is listed. One round of a group moves kGroup
 * dwords, 64 bytes; of 64 to 1024 tried, 256 and 512 were the fastest
 * (profiles/GPURESOLVE.md). */
constexpr uint32_t kFusedChunk = 256;
/* the smallest chunk the launcher takes: one round of a group */
constexpr uint32_t kFusedMinChunk = 4 * kGroup;
/* the longest reply an image may hold (answerrules.hpp) */
constexpr uint32_t kLargeReply = 4096;

/* as launchFused, for any accept in 0..kAcceptAll. listAbove and chunk
 * are kFusedListAbove and kFusedChunk; values nothing exceeds (~0u)
 * leave every reply to its own group, the plain shape that the timing
 * script measures against. chunk is at least kFusedMinChunk. */
hipError_t launchFusedLim(const Batch& b, const Image& img, uint32_t accept,
                          uint64_t seed, uint8_t* rbuf, uint64_t capacity,
                          uint64_t* cursor, int64_t* rstart, int32_t* rlen,
                          uint32_t listAbove, uint32_t chunk,
                          hipStream_t stream);

}  // namespace bamd::gpu
