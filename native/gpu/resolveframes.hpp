/*
 * binder-amd: GPU batch resolver - the fused kernel for a burst as the
 * serving loop holds it: a run of bsock1 frames (balancer/protocol.hpp)
 * in, a run of REPLY frames out.
 *
 *   bamd_resolve_frames  bamd_resolve_fused_lim (resolvefusedlim.hpp)
 *                        with the 30 bytes in front of every query read
 *                        in place and the 10 bytes in front of every
 *                        reply written with it
 *
 * The caller supplies where the frames start (frameindex.hpp); the
 * kernel holds every frame against that index. A frame is a candidate
 * if it is a QUERY whose payload_len agrees with the index and whose
 * DNS message, 30 bytes in, has 17 to kMaxQuery bytes. PING, PONG,
 * SHM_*, unknown types and anything shorter, longer or inconsistent are
 * left to the CPU path, as is a query the table does not answer.
 *
 * A candidate is looked up as the oversize kernels look it up, for any
 * accept in 0..kAcceptAll, with one more input: the frame's proto byte.
 * Over UDP (proto 0) a hit is held against 512 bytes or the advertised
 * size and truncated when it passes it. Over anything else it is held
 * against 65535 as the server's slow path holds a TCP query, so a hit
 * comes back in full: the stored reply, and the OPT tail when the query
 * carried an accepted OPT, up to kFramesReplyMax bytes with the header.
 *
 * A served frame i gets `B5 02 len32le req_id dns` at rstart[i], rlen[i]
 * bytes in all, req_id copied from the QUERY. A tile's REPLY frames lie
 * end to end in frame order, tiles in the order their claims arrive.
 *
 * cursor, four 64-bit words, zero before the launch:
 *   [0] bytes claimed              [1] hits dropped for lack of room
 *   [2] end of the written stream  [3] entries of miss[]
 * Claims are contiguous and a claim behind one that did not fit does not
 * fit either, so rbuf[0..cursor[2]) is a gap-free run of whole REPLY
 * frames whatever `capacity` was. Every frame of the batch is answered
 * by exactly one REPLY frame in that run or listed once in
 * miss[0..cursor[3]), in no particular order: not a candidate, not
 * accepted, not in the table, or in a tile whose claim did not fit.
 *
 * LDS: the fused_lim kernel's, with a span of 64 x 330 bytes. Compiled
 * for gfx950 the kernel takes 72 VGPRs, 43720 bytes of LDS and no
 * scratch: one workgroup of sixteen waves per CU, as there.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "resolvefusedlim.hpp"

namespace bamd::gpu {

/* bsock1: magic, type, payload_len; then req_id, family, proto, port
 * and address in front of a QUERY's DNS message, req_id in front of a
 * REPLY's */
constexpr int kFrameHead = 6;
constexpr int kFrameQueryHead = 24;
constexpr int kFrameReplyHead = 4;
constexpr int kFrameQueryAt = kFrameHead + kFrameQueryHead;
constexpr int kFrameReplyAt = kFrameHead + kFrameReplyHead;
/* a tile's span that is staged in LDS; a longer one holds a frame no
 * candidate has and stays in global memory */
constexpr int kFramesTileBytes = kFusedTile * (kFrameQueryAt + kMaxQuery);
/* the longest REPLY frame: a TCP hit at the image's ceiling with the
 * OPT tail */
constexpr int kFramesReplyMax = kFrameReplyAt + (int)kLargeReply + kOptLen;
/* what a query over TCP may take (the server's slowPath) */
constexpr uint32_t kTcpLimit = 65535;

/* b.qbuf is the frame run and b.qoff its n + 1 frame starts. rbuf has
 * `capacity` bytes, below 2^63; cursor as above; rstart, rlen and miss
 * have n entries. rlen[i] == 0 means frame i is in miss[], and
 * rstart[i] is then unspecified. listAbove and chunk as in
 * launchFusedLim. Allocates nothing, does not synchronise. */
hipError_t launchFrames(const Batch& b, const Image& img, uint32_t accept,
                        uint64_t seed, uint8_t* rbuf, uint64_t capacity,
                        uint64_t* cursor, int64_t* rstart, int32_t* rlen,
                        int32_t* miss, uint32_t listAbove, uint32_t chunk,
                        hipStream_t stream);

}  // namespace bamd::gpu
