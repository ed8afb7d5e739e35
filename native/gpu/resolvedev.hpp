/*
 * binder-amd: device helpers shared by the four resolve kernel pairs
 * (resolve.cpp, resolveext.cpp, resolvelarge.cpp, resolvepolicy.cpp)
 * and the fused kernels (resolvefused.cpp, resolvefusedlim.cpp,
 * resolveframes.cpp): the streamed key and its hash, the member-order
 * generator, the per-query lookups and the copy plans of a reply.
 * Device code only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "devcopy.hpp"
#include "resolveext.hpp"

namespace bamd::gpu {

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kLenMul = 0xD6E8FEB86659FD93ull;
constexpr uint64_t kStepMul = 0xBF58476D1CE4E5B9ull;
constexpr uint64_t kSmMul2 = 0x94D049BB133111EBull;

/* Streams the dotted key out of the wire name. `pos` is the wire
 * position of the next key byte, `nextLen` the position of the next
 * length byte; that byte reads as '.', and its value says where the
 * one after it lies. With kFold a label byte 'A'-'Z' reads as its
 * lowercase. */
template <bool kFold>
struct KeyReaderT {
    const uint8_t* q;
    uint32_t pos;
    uint32_t nextLen;

    __device__ __forceinline__ uint32_t next() {
        uint32_t c = q[pos];
        if (pos == nextLen) {
            nextLen += c + 1;
            c = '.';
        } else if constexpr (kFold) {
            if (c - 'A' < 26u) c |= 0x20;
        }
        ++pos;
        return c;
    }
    __device__ __forceinline__ uint64_t word(uint32_t nbytes) {
        uint32_t lo = 0, hi = 0;
        for (uint32_t b = 0; b < nbytes && b < 4; ++b)
            lo |= next() << (8 * b);
        for (uint32_t b = 4; b < nbytes; ++b)
            hi |= next() << (8 * (b - 4));
        return ((uint64_t)hi << 32) | lo;
    }
};
using KeyReader = KeyReaderT<false>;
using FoldReader = KeyReaderT<true>;

/* AnswerTable::hashKey, bit for bit, over the streamed key */
template <class Reader>
__device__ __forceinline__ uint64_t hashKey(Reader r, uint32_t klen,
                                            uint32_t qtype) {
    uint64_t h = kGold ^ ((uint64_t)klen * kLenMul) ^
                 ((uint64_t)qtype << 56);
    uint32_t n = klen;
    while (n >= 8) {
        h = (h ^ r.word(8)) * kStepMul;
        h ^= h >> 32;
        n -= 8;
    }
    if (n != 0) {
        h = (h ^ r.word(n)) * kStepMul;
        h ^= h >> 32;
    }
    h ^= h >> 32;
    h *= kGold;
    h ^= h >> 29;
    h *= kStepMul;
    h ^= h >> 32;
    return h;
}

__device__ __forceinline__ uint32_t get16(const uint8_t* p) {
    return p[0] | ((uint32_t)p[1] << 8);
}

__device__ __forceinline__ uint64_t splitmix(uint64_t x) {
    x += kGold;
    uint64_t z = (x ^ (x >> 30)) * kStepMul;
    z = (z ^ (z >> 27)) * kSmMul2;
    return z ^ (z >> 31);
}

/* The member order of reply `index`: Fisher-Yates from the
 * counter-based generator. */
__device__ __forceinline__ void drawOrder(uint32_t n, uint64_t seed,
                                          uint64_t index, uint8_t* order) {
    for (uint32_t i = 0; i < n; ++i) order[i] = (uint8_t)i;
    uint64_t s0 = seed ^ (index * kLenMul);
    uint64_t k = 0;
    for (uint32_t i = n; i > 1;) {
        --i;
        uint64_t draw = splitmix(s0 + k * kGold);
        uint32_t j = (uint32_t)(draw >> 32) % (i + 1);
        uint8_t t = order[i];
        order[i] = order[j];
        order[j] = t;
        ++k;
    }
}

/* head + 64 first segments + 64 second segments */
constexpr int kMaxJobs = 129;

/* One copy of a service reply: `src` counts from the body's start,
 * `dst` from the reply's. */
struct Job {
    uint16_t src, dst, len;
};

/* Lane 0 of a group: draw the member order and lay out
 * answerbody::serviceAssemble's copies - head, first segments in order,
 * second segments in order. The head's first 12 bytes are left to the
 * header patch. */
__device__ inline void planService(const uint8_t* body, uint64_t seed,
                                   uint64_t index, uint8_t* order,
                                   Job* jobs) {
    uint32_t n = body[1];
    uint32_t headLen = get16(body + 4);
    const uint8_t* tab = body + 6;
    uint32_t headOff = 6 + 8 * n;
    uint32_t segOff = headOff + headLen;
    drawOrder(n, seed, index, order);
    jobs[0] = Job{(uint16_t)(headOff + 12), 12, (uint16_t)(headLen - 12)};
    uint32_t w = headLen;
    for (uint32_t pass = 0; pass < 2; ++pass) {
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t* e = tab + 8 * order[i] + 4 * pass;
            uint32_t len = get16(e + 2);
            jobs[1 + pass * n + i] = Job{(uint16_t)(segOff + get16(e)),
                                         (uint16_t)w, (uint16_t)len};
            w += len;
        }
    }
}

/* One query: parseFastQuery()'s accept/reject decisions, then the
 * table walk of AnswerTable::find(). Leaves *bodyOff / *total alone
 * when the query is not served. */
__device__ __forceinline__ void resolveOne(
    const uint8_t* q, uint32_t len, const uint4* slots, uint32_t cap,
    const uint8_t* arena, uint32_t* bodyOff, int32_t* total) {
    if (len < 17 || len > (uint32_t)kMaxQuery) return;
    /* flags: QR/opcode/AA/TC clear, RD free; byte 3 must be zero */
    if (((q[2] & 0xFE) | q[3]) != 0) return;
    /* counts: qd=1, an=ns=ar=0 */
    if ((q[4] | (q[5] ^ 1) | q[6] | q[7] | q[8] | q[9] | q[10] |
         q[11]) != 0)
        return;

    /* pass 1: walk the labels. nlen is the dotted name's length, p3
     * the position of the third label's length byte, srvOk whether the
     * first two labels are '_' followed by no further '_'. */
    uint32_t pos = 12, nlen = 0, nlab = 0, p3 = 0;
    bool srvOk = true;
    while (true) {
        if (pos >= len) return;
        uint32_t l = q[pos++];
        if (l == 0) break;
        if ((l & 0xC0) != 0 || pos + l > len) return;
        if (nlen + l + 1 > 256) return;
        if (nlen > 0) ++nlen;
        if (nlab == 2) p3 = pos - 1;
        for (uint32_t k = 0; k < l; ++k) {
            uint32_t c = q[pos + k];
            bool ok = (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') ||
                      c == '_' || c == '-';
            if (!ok) return;
            if (nlab < 2) srvOk &= (c == '_') == (k == 0);
        }
        nlen += l;
        pos += l;
        ++nlab;
    }
    if (pos + 4 > len) return;
    uint32_t qtype = q[pos + 1];
    if (q[pos] != 0 || (qtype != 1 && qtype != 33)) return;
    if (q[pos + 2] != 0 || q[pos + 3] != 1) return;  /* class IN */

    /* pass 2: hash. A: the whole name. SRV: from the third label on. */
    KeyReader whole{q, 13, 13u + q[12]};
    KeyReader hashed = whole;
    uint32_t klen = nlen;
    if (qtype == 33) {
        if (nlab < 3 || !srvOk) return;
        hashed = KeyReader{q, p3 + 1, p3 + 1 + q[p3]};
        klen = nlen - (p3 - 12);
    }
    uint64_t h = hashKey(hashed, klen, qtype);
    uint32_t hlo = (uint32_t)h, hhi = (uint32_t)(h >> 32);

    /* probe: at most cap steps whatever the slots hold */
    uint32_t mask = cap - 1;
    uint32_t idx = hlo & mask;
    for (uint32_t step = 0; step < cap; ++step, idx = (idx + 1) & mask) {
        uint4 s = slots[idx];  /* hash lo, hash hi, off, len */
        if (s.w == 0) return;
        if (s.x != hlo || s.y != hhi) continue;
        /* same hash: confirm klen, qtype and the whole name. nlen may
         * be 256, which no blob's one-byte klen equals. */
        const uint8_t* b = arena + s.z;
        if (b[0] != nlen || b[1] != qtype) continue;
        KeyReader r = whole;
        bool same = true;
        for (uint32_t k = 0; k < nlen; ++k) {
            if (b[2 + k] != r.next()) {
                same = false;
                break;
            }
        }
        if (!same) continue;
        const uint8_t* body = b + 2 + nlen;
        uint32_t t = get16(body + 2);
        /* only an image with a raised ceiling holds such an entry */
        if (t > (uint32_t)kSmallReply) return;
        *bodyOff = s.z + 2 + nlen;
        *total = (int32_t)t;
        return;
    }
}

/* One query: parseFastQuery()'s decisions on the folded name and the
 * question alone, the OPT record's on what follows, then the table
 * walk. Leaves the outputs alone when the query is not served.
 *
 * kLim picks what a hit is held against. Without it a reply above
 * kSmallReply, or one that passes the advertised size with the OPT
 * tail, is left unserved. With it (resolvelarge.cpp) the query is
 * served either way: in full when the reply and the tail fit the size
 * the query may take, 512 without an OPT record, else truncated to
 * header, question and tail, which *total then counts, with
 * kMetaTrunc set. A non-zero `fixedLimit` is that size whatever the
 * query says: 65535 for a query that came over TCP (resolveframes.cpp). */
template <bool kLim>
__device__ __forceinline__ void resolveOneExtT(
    const uint8_t* q, uint32_t len, uint32_t accept, const uint4* slots,
    uint32_t cap, const uint8_t* arena, uint32_t* bodyOff, int32_t* total,
    uint32_t* meta, uint32_t fixedLimit = 0) {
    if (len < 17 || len > (uint32_t)kMaxQuery) return;
    /* flags: QR/opcode/AA/TC clear, RD free; byte 3 must be zero */
    if (((q[2] & 0xFE) | q[3]) != 0) return;
    /* counts: qd=1, an=ns=0; ar=0, or 1 where an OPT is accepted */
    if ((q[4] | (q[5] ^ 1) | q[6] | q[7] | q[8] | q[9] | q[10]) != 0)
        return;
    uint32_t ar = q[11];
    if (ar > (accept & kAcceptEdns)) return;
    bool anycase = (accept & kAcceptAnycase) != 0;

    /* pass 1: walk the labels, as the base lookup does, on the folded
     * bytes */
    uint32_t pos = 12, nlen = 0, nlab = 0, p3 = 0;
    bool srvOk = true, folded = false;
    while (true) {
        if (pos >= len) return;
        uint32_t l = q[pos++];
        if (l == 0) break;
        if ((l & 0xC0) != 0 || pos + l > len) return;
        if (nlen + l + 1 > 256) return;
        if (nlen > 0) ++nlen;
        if (nlab == 2) p3 = pos - 1;
        for (uint32_t k = 0; k < l; ++k) {
            uint32_t c = q[pos + k];
            if (anycase && c - 'A' < 26u) {
                c |= 0x20;
                folded = true;
            }
            bool ok = (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') ||
                      c == '_' || c == '-';
            if (!ok) return;
            if (nlab < 2) srvOk &= (c == '_') == (k == 0);
        }
        nlen += l;
        pos += l;
        ++nlab;
    }
    if (pos + 4 > len) return;
    uint32_t qtype = q[pos + 1];
    if (q[pos] != 0 || (qtype != 1 && qtype != 33)) return;
    if (q[pos + 2] != 0 || q[pos + 3] != 1) return;  /* class IN */
    uint32_t nameWire = pos - 12;  /* at most 258 */

    /* the OPT record: root name, type 41, class = advertised size, TTL
     * = extended rcode, version, flags; rdata inside the query. Flags
     * and options are not looked at. */
    uint32_t limit = 0;
    if (ar != 0) {
        uint32_t at = pos + 4;
        if (at + kOptLen > len) return;
        const uint8_t* o = q + at;
        if ((o[0] | o[1] | (o[2] ^ 41) | o[5] | o[6]) != 0) return;
        uint32_t rdlen = ((uint32_t)o[9] << 8) | o[10];
        if (at + kOptLen + rdlen > len) return;
        uint32_t adv = ((uint32_t)o[3] << 8) | o[4];
        limit = adv < 512 ? 512 : (adv > 4096 ? 4096 : adv);
    }

    /* pass 2: hash. A: the whole name. SRV: from the third label on. */
    FoldReader whole{q, 13, 13u + q[12]};
    FoldReader hashed = whole;
    uint32_t klen = nlen;
    if (qtype == 33) {
        if (nlab < 3 || !srvOk) return;
        hashed = FoldReader{q, p3 + 1, p3 + 1 + q[p3]};
        klen = nlen - (p3 - 12);
    }
    uint64_t h = hashKey(hashed, klen, qtype);
    uint32_t hlo = (uint32_t)h, hhi = (uint32_t)(h >> 32);

    /* probe: at most cap steps whatever the slots hold */
    uint32_t mask = cap - 1;
    uint32_t idx = hlo & mask;
    for (uint32_t step = 0; step < cap; ++step, idx = (idx + 1) & mask) {
        uint4 s = slots[idx];  /* hash lo, hash hi, off, len */
        if (s.w == 0) return;
        if (s.x != hlo || s.y != hhi) continue;
        const uint8_t* b = arena + s.z;
        if (b[0] != nlen || b[1] != qtype) continue;
        FoldReader r = whole;
        bool same = true;
        for (uint32_t k = 0; k < nlen; ++k) {
            if (b[2 + k] != r.next()) {
                same = false;
                break;
            }
        }
        if (!same) continue;
        const uint8_t* body = b + 2 + nlen;
        uint32_t t = get16(body + 2);
        uint32_t m = nameWire;
        uint32_t e = ar != 0 ? (uint32_t)kOptLen : 0;
        if constexpr (kLim) {
            uint32_t lim = ar != 0 ? limit : (uint32_t)kSmallReply;
            if (fixedLimit != 0) lim = fixedLimit;
            if (t + e > lim) {
                t = 12 + nameWire + 4;
                m |= kMetaTrunc;
            }
        } else {
            /* the CPU path owns truncation */
            if (t > (uint32_t)kSmallReply) return;
            if (ar != 0 && t + e > limit) return;
        }
        t += e;
        if (ar != 0) m |= kMetaEdns;
        if (folded) m |= kMetaFolded;
        *bodyOff = s.z + 2 + nlen;
        *total = (int32_t)t;
        *meta = m;
        return;
    }
}

__device__ __forceinline__ void resolveOneExt(
    const uint8_t* q, uint32_t len, uint32_t accept, const uint4* slots,
    uint32_t cap, const uint8_t* arena, uint32_t* bodyOff, int32_t* total,
    uint32_t* meta) {
    resolveOneExtT<false>(q, len, accept, slots, cap, arena, bodyOff, total,
                          meta);
}

/* The lookup kernel of the opt-in pairs, one query per lane: stage the
 * tile's span of qbuf in `tile` (LDS, kTileBytes + 16) at its global
 * address mod 16, check qoff per tile and per query, resolve. */
template <bool kLim>
__device__ __forceinline__ void lookupTileExt(
    uint8_t* tile, const uint8_t* qbuf, const int32_t* qoff, int64_t qbytes,
    int32_t n, const uint4* slots, uint32_t cap, const uint8_t* arena,
    uint32_t accept, uint32_t* bodyOff, int32_t* rlen, uint32_t* meta) {
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
    __syncthreads();

    int32_t i = t0 + (int32_t)threadIdx.x;
    if (i >= t1) return;
    int64_t o0 = qoff[i], o1 = qoff[i + 1];
    uint32_t off = kUnserved, m = 0;
    int32_t total = 0;
    if (cap != 0 && spanOk && o0 >= b0 && o1 >= o0 && o1 <= b1 &&
        o1 - o0 <= kMaxQuery) {
        uint32_t len = (uint32_t)(o1 - o0);
        const uint8_t* q =
            staged ? tile + shift + (uint32_t)(o0 - b0) : qbuf + o0;
        resolveOneExtT<kLim>(q, len, accept, slots, cap, arena, &off, &total,
                             &m);
    }
    bodyOff[i] = off;
    rlen[i] = total;
    meta[i] = m;
}

/* the server's OPT record behind 4 bytes that groupCopy may read in
 * front of a source */
static __constant__ __attribute__((aligned(16))) uint8_t kOptSrc[16] = {
    0, 0, 0, 0, 0x00, 0x00, 0x29, 0x05, 0x78, 0, 0, 0, 0, 0, 0, 0};

constexpr int kMaxExtJobs = kMaxJobs + 2;

enum Source : uint16_t {
    kSrcBody = 0,   /* src counts from the answer body's start */
    kSrcQuery = 1,  /* ... from the query's */
    kSrcOpt = 2,    /* ... from the OPT record's */
};

struct ExtJob {
    uint16_t source, src, dst, len;
};

/* A group's first lane: lay out reply `index` behind its 12 header
 * bytes. `len0` is the reply's length without the OPT tail. Returns
 * the number of jobs. */
__device__ inline uint32_t planReply(const uint8_t* body, uint32_t len0,
                                     uint32_t meta, uint64_t seed,
                                     uint64_t index, uint8_t* order,
                                     ExtJob* jobs) {
    bool service = body[0] == 1;
    uint32_t n = service ? body[1] : 0;
    uint32_t headLen = service ? get16(body + 4) : len0;
    uint32_t headOff = service ? 6 + 8 * n : 4;
    /* the name as asked, clipped to the head */
    uint32_t echo = 0;
    if ((meta & kMetaFolded) != 0) {
        uint32_t end = 12 + (meta & kMetaNameMask);
        echo = (end < headLen ? end : headLen) - 12;
    }
    uint32_t nj = 0;
    if (echo != 0) jobs[nj++] = ExtJob{kSrcQuery, 12, 12, (uint16_t)echo};
    uint32_t w = 12 + echo;
    if (w != headLen)
        jobs[nj++] = ExtJob{kSrcBody, (uint16_t)(headOff + w), (uint16_t)w,
                            (uint16_t)(headLen - w)};
    w = headLen;
    if (service) {
        const uint8_t* tab = body + 6;
        uint32_t segOff = headOff + headLen;
        drawOrder(n, seed, index, order);
        for (uint32_t pass = 0; pass < 2; ++pass) {
            for (uint32_t i = 0; i < n; ++i) {
                const uint8_t* e = tab + 8 * order[i] + 4 * pass;
                uint32_t len = get16(e + 2);
                jobs[nj++] = ExtJob{kSrcBody, (uint16_t)(segOff + get16(e)),
                                    (uint16_t)w, (uint16_t)len};
                w += len;
            }
        }
    }
    if ((meta & kMetaEdns) != 0)
        jobs[nj++] = ExtJob{kSrcOpt, 0, (uint16_t)w, (uint16_t)kOptLen};
    return nj;
}

/* A group's first lane: lay out a truncated reply behind its 12 header
 * bytes - the question as it was asked, and the OPT tail when the
 * query carried one. Returns the number of jobs. */
__device__ inline uint32_t planTruncated(uint32_t meta, ExtJob* jobs) {
    uint32_t qlen = (meta & kMetaNameMask) + 4;
    jobs[0] = ExtJob{kSrcQuery, 12, 12, (uint16_t)qlen};
    if ((meta & kMetaEdns) == 0) return 1;
    jobs[1] = ExtJob{kSrcOpt, 0, (uint16_t)(12 + qlen), (uint16_t)kOptLen};
    return 2;
}

/* A group's first lane: cut each of the plan's first `heads` jobs that
 * is above `chunk` bytes down to its first `chunk` and append the rest
 * behind the plan's nj jobs as jobs of at most `chunk`. Returns the
 * number of jobs. */
__device__ inline uint32_t splitJobs(ExtJob* jobs, uint32_t nj,
                                     uint32_t heads, uint32_t chunk) {
    uint32_t end = nj;
    for (uint32_t j = 0; j < heads; ++j) {
        ExtJob jb = jobs[j];
        if (jb.len <= chunk) continue;
        jobs[j].len = (uint16_t)chunk;
        for (uint32_t o = chunk; o < jb.len; o += chunk) {
            uint32_t rest = jb.len - o;
            jobs[end++] = ExtJob{jb.source, (uint16_t)(jb.src + o),
                                 (uint16_t)(jb.dst + o),
                                 (uint16_t)(rest < chunk ? rest : chunk)};
        }
    }
    return end;
}

/* kGroup lanes make one copy of a plan into the reply at `dst` */
static __device__ __forceinline__ void copyJob(ExtJob jb, uint8_t* dst,
                                               const uint8_t* body,
                                               const uint8_t* q,
                                               uint32_t lane) {
    const uint8_t* base = jb.source == kSrcBody    ? body
                          : jb.source == kSrcQuery ? q
                                                   : kOptSrc + 4;
    groupCopy(dst + jb.dst, base + jb.src, jb.len, lane);
}

}  // namespace bamd::gpu
