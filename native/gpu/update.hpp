/*
 * binder-amd: GPU batch resolver - updating the device answer table in
 * place. Launcher interface of the gfx950 kernels in update.cpp.
 *
 * A delta (answerdelta.hpp) is applied in two phases on one stream:
 *
 *   bamd_update_invalidate  phase 1: every domain's A entry and its SRV
 *                           entries become tombstones
 *   bamd_update_insert      phase 2: every blob, already appended to
 *                           the arena, replaces its key's slot or
 *                           claims an empty one
 *
 * and the table is rebuilt without its dead space by
 *
 *   bamd_update_scan        blob length of every live slot, live count
 *                           and bytes
 *   bamd_update_move        copy the live blobs into a fresh arena and
 *                           place their slots in a fresh slot array
 *
 * with the caller's prefix sum over the lengths in between. Slot and
 * blob formats are those of the image (resolve.hpp); the resolve
 * kernels read an updated table as they read an uploaded one.
 *
 * Work split. Op batches are small next to query batches - one to a
 * few thousand ops between two bursts - so what counts is the latency
 * of one apply(), not throughput: the two phase kernels take one op
 * per lane in workgroups of one wave (kOpBlock = 64), which spreads
 * even a 1 000-op delta over 16 CUs and keeps a lone long probe chain
 * from holding more than 63 neighbours. An op is a dependent walk over
 * slots, 16 bytes a step, so wider groups per op would idle.
 * Invalidate stages its workgroup's domain bytes in LDS (64 x 255 =
 * 16 KiB at most) because each is compared with every same-hash blob
 * of a chain; insert compares its key about once, on a 64-bit hash
 * match, and reads it from the arena where the batch already lies.
 * Compaction is throughput work over the whole table: scan takes a
 * slot per lane, move takes kGroup lanes per slot, as emit does per
 * reply, since a blob is a reply-sized byte string at any alignment.
 *
 * The launchers take raw device pointers and a stream; they allocate
 * nothing and do not synchronise. Offsets in the op buffers are not
 * trusted: op i is applied only if off[i-1] <= off[i] < off[i+1] <=
 * the buffer's size (off[-1] = 0), so one bad entry leaves unapplied
 * the ops that read it, three at most, and no other. The table is
 * trusted.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "resolve.hpp"

namespace bamd::gpu {

/* ops per phase workgroup, one per lane: one wave */
constexpr int kOpBlock = 64;
constexpr int kMaxDomain = 255;
constexpr int kOpTileBytes = kOpBlock * kMaxDomain;
/* slots per scan workgroup */
constexpr int kScanBlock = 256;

/* a tombstone is { hash 0, off = tomb, len = kTombLen }: no blob is
 * that short, and the two bytes at `tomb` are zero */
constexpr uint32_t kTombLen = 2;

/* counter block, uint32 each */
enum Counter {
    kCntTombstones = 0, /* live slots turned into tombstones */
    kCntDeadBytes = 1,  /* blob bytes left behind by both phases */
    kCntClaims = 2,     /* empty slots claimed by inserts */
    kCntReplaced = 3,   /* slots replaced in place */
    kCounters = 4,
};

struct Table {
    void* slots;      /* cap x { hash u64, off u32, len u32 } */
    uint32_t cap;     /* power of two */
    uint8_t* arena;
    uint32_t tomb;    /* offset of the two zero bytes in arena */
    uint32_t* counters;
};

/* ibuf: domains end to end, ioff [n + 1], ihash [2 n] (A, SRV) */
hipError_t launchInvalidate(const Table& t, const uint8_t* ibuf,
                            const int32_t* ioff, int32_t ibytes,
                            const uint64_t* ihash, int32_t n,
                            hipStream_t stream);

/* the n blobs lie in the arena from `used` on, blob i at
 * used + uoff[i]; ubytes is their total size */
hipError_t launchInsert(const Table& t, uint32_t used, const int32_t* uoff,
                        int32_t ubytes, const uint64_t* uhash, int32_t n,
                        hipStream_t stream);

/* lens[i] = blob length of slot i or 0; totals[0] += live slots,
 * totals[1] += live bytes */
hipError_t launchScan(const Table& t, int32_t* lens,
                      unsigned long long* totals, hipStream_t stream);

/* incl = inclusive prefix sums of lens. `to` has zeroed slots, room
 * for incl[cap - 1] arena bytes below to.tomb and two bytes at it;
 * its counters are reset. */
hipError_t launchMove(const Table& from, const int32_t* lens,
                      const int64_t* incl, const Table& to,
                      hipStream_t stream);

}  // namespace bamd::gpu
