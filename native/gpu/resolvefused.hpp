/*
 * binder-amd: GPU batch resolver - the fused kernel for bursts.
 *
 *   bamd_resolve_fused  one launch from wire queries to reply bytes:
 *                       stage, look up, place, emit, per tile of
 *                       kFusedTile consecutive queries
 *
 * The two kernel pairs (resolve.hpp, resolveext.hpp) need the host
 * between them: a prefix sum over the whole batch and a read of its
 * total to size the reply buffer. That is right for a replay of a
 * million queries and wrong for a burst of 64. Here the caller owns the
 * reply buffer and a workgroup places its own tile: an exclusive scan
 * of the tile's reply lengths, then one 64-bit atomicAdd of the tile's
 * total on a device cursor. Replies of a tile lie end to end in query
 * order; tiles lie in the order their claims arrive. No workgroup waits
 * for another.
 *
 * A tile whose claim ends past `capacity` writes no reply byte, reports
 * all its queries unserved and adds its hits to cursor[1]. The cursor
 * has moved by then, so the tiles that claim after it overflow too.
 *
 * Accept/reject decisions, reply bytes and the member order
 * (drawOrder(n, seed, position in the batch)) are the two pairs'.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "resolveext.hpp"

namespace bamd::gpu {

/* queries per workgroup, one per lane of the first wave. A GSO burst is
 * at most 64 datagrams: it is one tile, so its replies are packed in
 * query order exactly as resolve() packs them, and the scan is a single
 * wave's. Half of kTile also halves the staged span (64 x 300 = 18.8
 * KiB), which pays for the job lists below. */
constexpr int kFusedTile = 64;
/* threads per workgroup: the lookup runs in kFusedTile / 64 waves, the
 * staging and the emit in all sixteen, so every query of the tile has
 * its own group of kGroup lanes and the replies are written at once. */
constexpr int kFusedBlock = 1024;
constexpr int kFusedGroups = kFusedBlock / kGroup;
constexpr int kFusedWaves = kFusedTile / 64;
constexpr int kFusedTileBytes = kFusedTile * kMaxQuery;
/* copy jobs for the whole tile, reserved reply by reply: a service of
 * 8 members takes 19, so the usual tile fits at once; a tile of 64
 * services of 64 members (131 each) takes 5 passes of 15. */
constexpr int kFusedPool = 2048;
constexpr uint32_t kNoRoom = 0xFFFFFFFFu;
/* LDS: the span 18.8 KiB, the pool 16 KiB, member orders 4 KiB, five
 * words per query 1.3 KiB: 40.5 KiB. The kernel takes 73 VGPRs, so one
 * workgroup of sixteen waves is resident per CU: built for the latency
 * of a burst, not for a replay's throughput, which resolve() keeps. */
static_assert(kFusedTile % 64 == 0 && kFusedBlock % 64 == 0 &&
              kFusedBlock >= kFusedTile);

/* cursor[0] = reply bytes claimed, cursor[1] = hits dropped for lack of
 * room; the caller zeroes both before the launch. rbuf has `capacity`
 * bytes, below 2^63. rstart[i] and rlen[i] are written once for every
 * query; rlen[i] == 0 means unserved, and rstart[i] is then unspecified.
 * Allocates nothing, does not synchronise. */
hipError_t launchFused(const Batch& b, const Image& img, uint32_t accept,
                       uint64_t seed, uint8_t* rbuf, uint64_t capacity,
                       uint64_t* cursor, int64_t* rstart, int32_t* rlen,
                       hipStream_t stream);

}  // namespace bamd::gpu
