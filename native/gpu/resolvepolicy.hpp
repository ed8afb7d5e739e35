/*
 * binder-amd: GPU batch resolver - the kernel pair that also answers
 * what the server answers from the query alone: NOTIMP for a query type
 * it does not implement, REFUSED for an SRV name of the wrong shape and
 * for a name outside the configured zone.
 *
 *   bamd_resolve_lookup_pol  the oversize lookup (resolvelarge.hpp) with
 *                            the type test replaced by Engine::handle's
 *                            decisions, and an optional tally of what
 *                            became of the batch
 *   bamd_resolve_emit_pol    the oversize emit with a third kind of
 *                            reply: header from registers, the question
 *                            from the query, the OPT tail
 *
 * A query is a candidate exactly as for the oversize pair, except for
 * its type: both type bytes are read, and the decisions run in the
 * engine's order (resolveOnePol below).
 *
 *   qtype not 1, 12, 33   NOTIMP; the zone is not looked at
 *   qtype 12              unserved: the device has no reverse index
 *   qtype 33, not         REFUSED (Engine::resolve: !match ||
 *   _svc._proto.domain    rest.empty())
 *   outside the zone      REFUSED, with a non-empty zone only. D is the
 *                         whole name for A and the name behind the first
 *                         two labels for SRV; D must be one label or more
 *                         followed by the zone, so the zone itself is
 *                         outside
 *   otherwise             the table, as resolveOneExtT<true> walks it
 *
 * A policy reply is 12 + w + 4 + e bytes for a question name of w wire
 * bytes: the query's id, 0x84 | RD, the rcode, QDCOUNT 1, ARCOUNT 1 when
 * e != 0, the question as it was asked, and kOptTail. The server drops a
 * query whose name is above 255 wire bytes, so such a query gets no
 * policy reply; that bounds the reply at 282 bytes, and none is ever
 * truncated.
 *
 * What the engine decides on the name as it was asked (its suffix test
 * is case-sensitive), its doubled-suffix rule and PTR outside
 * in-addr.arpa stay with the CPU path: here the zone test runs on the
 * folded name, and a name it finds inside goes to the table.
 *
 * LDS of the lookup: the tile, kMaxZone + 1 bytes of zone, ten words of
 * tally. LDS of the emit: resolvelarge.hpp's.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "resolvedev.hpp"
#include "resolvelarge.hpp"

namespace bamd::gpu {

/* the zone in wire form, "\3foo\3com\0": at most a name's 255 bytes; a
 * length of 0 is no zone rule */
constexpr uint32_t kMaxZone = 255;

/* the metadata word above kMetaTrunc: the reply is synthesized from the
 * query, with this rcode */
constexpr uint32_t kMetaSynth = 1u << 12;
constexpr uint32_t kMetaRcodeShift = 13;
constexpr uint32_t kMetaRcodeMask = 0xF;

constexpr uint32_t kRcodeNotimp = 4;
constexpr uint32_t kRcodeRefused = 5;

/* words of `tally`, what became of each query */
enum Tally : uint32_t {
    kTallyFull = 0,  /* served in full from the table */
    kTallyTruncated = 1,
    kTallyNotimp = 2,
    kTallyRefused = 3,
    kTallyUnserved = 4,
    kTallyWords = 5,
};

/* as launchLookupLim. `zone` is zlen <= kMaxZone bytes of device memory
 * that ZonePolicy validated: lowercase labels, the root byte last.
 * `tally` is null or kTallyWords 64-bit counters, which are added to and
 * never cleared. */
hipError_t launchLookupPol(const Batch& b, const Image& img,
                           uint32_t accept, const uint8_t* zone,
                           uint32_t zlen, uint32_t* bodyOff, int32_t* rlen,
                           uint32_t* meta, unsigned long long* tally,
                           hipStream_t stream);

/* as launchEmitLim at kListAbove, with this lookup's metadata words */
hipError_t launchEmitPol(const Batch& b, const Image& img,
                         const uint32_t* bodyOff, const int32_t* rlen,
                         const uint32_t* meta, const int64_t* roff,
                         uint8_t* rbuf, uint64_t seed, hipStream_t stream);

/* Is the wire name q[dstart, end), root byte included, one label or
 * more followed by the zone? The compare is on the folded bytes and
 * takes the zone's first length byte along. That byte may equal a label
 * byte ('-' is 45, '0' is 48), so the match must also begin where a
 * label begins: hop from dstart. The caller has walked the labels, so
 * the hops stay inside the name. (Skipping the hops for a first label
 * below 45 bytes was tried and measured no gain.) */
__device__ __forceinline__ bool underZone(const uint8_t* q, uint32_t dstart,
                                          uint32_t end, const uint8_t* zone,
                                          uint32_t zlen, bool anycase) {
    if (end - dstart <= zlen) return false;
    uint32_t at = end - zlen;
    for (uint32_t k = 0; k < zlen; ++k) {
        uint32_t c = q[at + k];
        if (anycase && c - 'A' < 26u) c |= 0x20;
        if (c != zone[k]) return false;
    }
    uint32_t p = dstart;
    while (p < at) p += 1u + q[p];
    return p == at;
}

/* One query, shaped like resolveOneExtT: the outputs are left alone
 * when it is not served. A policy reply leaves *bodyOff alone too and
 * sets kMetaSynth and the rcode in *meta.
 *
 * The first walk only hops over the labels: it finds the type, and with
 * it the decision. A query bound for the table goes to
 * resolveOneExtT<true>, which checks all of it; only a policy query is
 * checked here, against the same rules (label bytes, class, the OPT
 * record), and does no hash, no probe and no arena read. */
__device__ __forceinline__ void resolveOnePol(
    const uint8_t* q, uint32_t len, uint32_t accept, const uint8_t* zone,
    uint32_t zlen, const uint4* slots, uint32_t cap, const uint8_t* arena,
    uint32_t* bodyOff, int32_t* total, uint32_t* meta) {
    if (len < 17 || len > (uint32_t)kMaxQuery) return;
    if (((q[2] & 0xFE) | q[3]) != 0) return;
    if ((q[4] | (q[5] ^ 1) | q[6] | q[7] | q[8] | q[9] | q[10]) != 0)
        return;
    uint32_t ar = q[11];
    if (ar > (accept & kAcceptEdns)) return;
    bool anycase = (accept & kAcceptAnycase) != 0;

    /* hop: nlab labels, the third one's length byte at p3, the root
     * byte at pos */
    uint32_t pos = 12, nlab = 0, p3 = 0;
    while (true) {
        if (pos >= len) return;
        uint32_t l = q[pos];
        if (l == 0) break;
        if ((l & 0xC0) != 0 || pos + 1 + l > len) return;
        if (nlab == 2) p3 = pos;
        pos += 1 + l;
        ++nlab;
    }
    uint32_t end = pos + 1;  /* the question's type bytes */
    if (end + 4 > len) return;
    uint32_t qtype = ((uint32_t)q[end] << 8) | q[end + 1];
    if (q[end + 2] != 0 || q[end + 3] != 1) return;  /* class IN */

    uint32_t rcode = 0;
    if (qtype != 1 && qtype != 33) {
        if (qtype == 12) return;
        rcode = kRcodeNotimp;
    } else {
        uint32_t dstart = 12;
        if (qtype == 33) {
            /* the first two labels: '_', then no further '_' */
            bool srvOk = nlab >= 3;
            for (uint32_t p = 12; srvOk && p < p3; p += 1u + q[p])
                for (uint32_t k = 0; k < q[p]; ++k)
                    srvOk &= (q[p + 1 + k] == '_') == (k == 0);
            if (!srvOk) rcode = kRcodeRefused;
            dstart = p3;
        }
        if (rcode == 0 && zlen != 0 &&
            !underZone(q, dstart, end, zone, zlen, anycase))
            rcode = kRcodeRefused;
    }
    if (rcode == 0) {
        if (cap != 0)
            resolveOneExtT<true>(q, len, accept, slots, cap, arena, bodyOff,
                                 total, meta);
        return;
    }

    /* a policy reply: the rest of the opt-in lookup's acceptance */
    uint32_t nameWire = end - 12;
    if (nameWire > 255) return;  /* the server drops it */
    for (uint32_t p = 12; q[p] != 0; p += 1u + q[p]) {
        for (uint32_t k = 0; k < q[p]; ++k) {
            uint32_t c = q[p + 1 + k];
            if (anycase && c - 'A' < 26u) c |= 0x20;
            bool ok = (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') ||
                      c == '_' || c == '-';
            if (!ok) return;
        }
    }
    uint32_t m = nameWire | kMetaSynth | (rcode << kMetaRcodeShift);
    uint32_t t = 12 + nameWire + 4;
    if (ar != 0) {
        uint32_t at = end + 4;
        if (at + kOptLen > len) return;
        const uint8_t* o = q + at;
        if ((o[0] | o[1] | (o[2] ^ 41) | o[5] | o[6]) != 0) return;
        uint32_t rdlen = ((uint32_t)o[9] << 8) | o[10];
        if (at + kOptLen + rdlen > len) return;
        m |= kMetaEdns;
        t += kOptLen;
    }
    *total = (int32_t)t;
    *meta = m;
}

}  // namespace bamd::gpu
