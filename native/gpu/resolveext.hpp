/*
 * binder-amd: GPU batch resolver - the opt-in kernel pair for queries
 * the base pair (resolve.hpp) leaves to the CPU path: an EDNS0 OPT
 * record behind the question, and uppercase in the question name.
 *
 *   bamd_resolve_lookup_ext  the base lookup with a folding key reader
 *                            and an OPT parse behind the question; adds
 *                            one metadata word per query
 *   bamd_resolve_emit_ext    the base emit with up to four sources per
 *                            reply: the query (id, RD, the name as it
 *                            was asked), the arena, the server's OPT
 *                            record and the patched ARCOUNT
 *
 * A query is accepted if parseFastQuery() accepts it once its name is
 * lowercased (kAcceptAnycase) and its OPT record dropped (kAcceptEdns).
 * The reply is the base pair's reply for that query, with the name put
 * back as asked when a byte was folded, and ARCOUNT + 1 and kOptTail
 * behind it when the query carried an OPT. Tiling, LDS staging, the
 * 300-byte cap and the span checks on qoff are the base pair's.
 *
 * Emit's copy plan has a source selector per job. A reply takes at
 * most kMaxJobs + 2 jobs: the base plan's head is split in two (the
 * name from the query, the rest from the arena) and the OPT tail
 * follows the last segment. That sizes the LDS arrays: kGroupsPerBlock
 * x (kMaxJobs + 2) x 8 bytes = 16.4 KiB, next to 1 KiB of member
 * orders.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "resolve.hpp"

namespace bamd::gpu {

/* bits of `accept` */
constexpr uint32_t kAcceptEdns = 1;     /* ARCOUNT 1, a well-formed OPT */
constexpr uint32_t kAcceptAnycase = 2;  /* 'A'-'Z' in labels */
constexpr uint32_t kAcceptAll = kAcceptEdns | kAcceptAnycase;

/* Record::OPT(1400) on the wire: root, type 41, class 1400, no TTL
 * bits, no options */
constexpr int kOptLen = 11;

/* the metadata word: the wire length of the question name (length
 * bytes and root byte included, at most 258), then two flags */
constexpr uint32_t kMetaNameMask = 0x1FF;
constexpr uint32_t kMetaEdns = 1u << 9;    /* the query carried an OPT */
constexpr uint32_t kMetaFolded = 1u << 10; /* a name byte was folded */
/* the reply is header, question and OPT tail (resolvelarge.hpp only) */
constexpr uint32_t kMetaTrunc = 1u << 11;

/* the longest reply this pair and the base pair serve: what a query
 * without an OPT record may take over UDP. An image with a raised
 * ceiling may hold longer ones, which these kernels leave unserved. */
constexpr int kSmallReply = 512;

/* as launchLookup; rlen counts the OPT tail, meta[i] is written for
 * every query */
hipError_t launchLookupExt(const Batch& b, const Image& img,
                           uint32_t accept, uint32_t* bodyOff,
                           int32_t* rlen, uint32_t* meta,
                           hipStream_t stream);

/* as launchEmit, with the lookup's metadata words */
hipError_t launchEmitExt(const Batch& b, const Image& img,
                         const uint32_t* bodyOff, const int32_t* rlen,
                         const uint32_t* meta, const int64_t* roff,
                         uint8_t* rbuf, uint64_t seed, hipStream_t stream);

}  // namespace bamd::gpu
