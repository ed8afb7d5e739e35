/*
 * binder-amd: GPU batch resolver - the kernel pair for an image with a
 * raised reply ceiling (answerrules.hpp: up to 4096 bytes), and for
 * truncation.
 *
 *   bamd_resolve_lookup_lim  the opt-in lookup (resolveext.hpp) with the
 *                            server's size decision where that one gives
 *                            up: a hit is served in full or truncated
 *   bamd_resolve_emit_lim    the opt-in emit with a truncated plan, and
 *                            with long plans written by the whole
 *                            workgroup instead of one group
 *
 * A query is accepted exactly as `accept` says for the opt-in pair; 0
 * accepts what the base pair does. For a hit whose stored reply has t
 * bytes, with e = kOptLen when the query carried an accepted OPT record
 * and 0 otherwise, and L = 512 without an OPT record, else the
 * advertised size clamped to [512, 4096]:
 *
 *   t + e <= L  the opt-in pair's reply at any t up to the ceiling
 *   otherwise   DnsServer's truncated reply, 12 + w + 4 + e bytes for
 *               a question name of w wire bytes: id and RD from the
 *               query, the stored flags with TC set, QDCOUNT 1, no
 *               answers, the question as it was asked, and ARCOUNT 1
 *               with kOptTail behind it when e != 0
 *
 * LDS of the emit: the opt-in emit's plans, kGroupsPerBlock x
 * kMaxExtJobs x 8 bytes = 16.4 KiB, 1 KiB of member orders, and four
 * words per group for the shared drain.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "resolveext.hpp"

namespace bamd::gpu {

/* A reply whose plan has more jobs than this is drained by the whole
 * workgroup. One group walks a plan of j jobs in j rounds on one wave;
 * the workgroup's four waves drain it in ceil(j / 16) rounds each. At 33
 * jobs that is 33 wave-rounds against 12, enough to pay for the drain
 * loop every group then runs. No SRV reply of at most 512 bytes gets
 * there (a member costs 40 bytes and two jobs, so 12 members and 27
 * jobs at the most): a batch with no large reply takes the opt-in
 * emit's path through this kernel. */
constexpr uint32_t kListAbove = 32;

/* as launchLookupExt, for any accept in 0..kAcceptAll; rlen is the full
 * or the truncated length and meta carries kMetaTrunc */
hipError_t launchLookupLim(const Batch& b, const Image& img,
                           uint32_t accept, uint32_t* bodyOff,
                           int32_t* rlen, uint32_t* meta,
                           hipStream_t stream);

/* as launchEmitExt, with this lookup's metadata words. listAbove is
 * kListAbove; a value no plan exceeds (~0u) lists nothing, which is the
 * plain shape of one group per reply that the timing script measures
 * against. */
hipError_t launchEmitLim(const Batch& b, const Image& img,
                         const uint32_t* bodyOff, const int32_t* rlen,
                         const uint32_t* meta, const int64_t* roff,
                         uint8_t* rbuf, uint64_t seed, uint32_t listAbove,
                         hipStream_t stream);

}  // namespace bamd::gpu
