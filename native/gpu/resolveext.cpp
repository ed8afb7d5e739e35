/*
 * binder-amd: GPU batch resolver - the opt-in kernel pair for EDNS0
 * and mixed-case queries (resolveext.hpp).
 *
 * The lookup is the base lookup (resolve.cpp) with three changes. The
 * label walk folds 'A'-'Z' when kAcceptAnycase is set and remembers
 * that it did; hash and key compare read the name through FoldReader,
 * so no lowercase copy of the name is made in LDS or registers. With
 * kAcceptEdns an ARCOUNT of 1 is let through, and the 11 fixed bytes
 * of an OPT record are checked right behind the question, from the
 * same staged bytes; every read is below the query's own length, so
 * the staged and the unstaged tile need no separate care. A hit is
 * then held against the advertised size, and its length grows by the
 * server's OPT. `accept` is a kernel argument: the branches on it are
 * the same for every lane.
 *
 * The emit keeps one 16-lane group per reply and the base copy
 * routine. What changes is the plan: the group's first lane lays out
 * every reply, wire or service, as jobs { source, src, dst, len } in
 * LDS, where source says which base `src` counts from - the answer
 * body in the arena, the query, or the constant OPT record. The 12
 * header bytes are still written by the lanes that own them, with
 * ARCOUNT's carry worked out from the stored bytes 10 and 11.
 *
 * Trust is the base pair's: qoff is checked per tile and per query,
 * the image is believed, and emit reads a query only where the lookup
 * served it and only below the name length the lookup found in it.
 */
#include "resolveext.hpp"

#include <hip/hip_runtime.h>

#include "devcopy.hpp"
#include "resolvedev.hpp"

namespace bamd::gpu {

namespace {

/* One query: parseFastQuery()'s decisions on the folded name and the
 * question alone, the OPT record's on what follows, then the table
 * walk. Leaves the outputs alone when the query is not served. */
__device__ __forceinline__ void resolveOneExt(
    const uint8_t* q, uint32_t len, uint32_t accept, const uint4* slots,
    uint32_t cap, const uint8_t* arena, uint32_t* bodyOff, int32_t* total,
    uint32_t* meta) {
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
        if (ar != 0) {
            /* the CPU path owns truncation */
            if (t + kOptLen > limit) return;
            t += kOptLen;
            m |= kMetaEdns;
        }
        if (folded) m |= kMetaFolded;
        *bodyOff = s.z + 2 + nlen;
        *total = (int32_t)t;
        *meta = m;
        return;
    }
}

/* the server's OPT record behind 4 bytes that groupCopy may read in
 * front of a source */
__constant__ __attribute__((aligned(16))) uint8_t kOptSrc[16] = {
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
__device__ uint32_t planReply(const uint8_t* body, uint32_t len0,
                              uint32_t meta, uint64_t seed, uint64_t index,
                              uint8_t* order, ExtJob* jobs) {
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

}  // namespace

extern "C" __global__ __launch_bounds__(kTile) void bamd_resolve_lookup_ext(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int64_t qbytes, int32_t n, const uint4* __restrict__ slots,
    uint32_t cap, const uint8_t* __restrict__ arena, uint32_t accept,
    uint32_t* __restrict__ bodyOff, int32_t* __restrict__ rlen,
    uint32_t* __restrict__ meta) {
    /* + 16: the span sits in LDS at its global address mod 16 */
    __shared__ uint4 tile4[(kTileBytes + 16) / 16];
    uint8_t* tile = (uint8_t*)tile4;

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
        resolveOneExt(q, len, accept, slots, cap, arena, &off, &total, &m);
    }
    bodyOff[i] = off;
    rlen[i] = total;
    meta[i] = m;
}

extern "C" __global__ __launch_bounds__(kEmitBlock)
void bamd_resolve_emit_ext(
    const uint8_t* __restrict__ qbuf, const int32_t* __restrict__ qoff,
    int32_t n, const uint8_t* __restrict__ arena,
    const uint32_t* __restrict__ bodyOff, const int32_t* __restrict__ rlen,
    const uint32_t* __restrict__ meta, const int64_t* __restrict__ roff,
    uint8_t* __restrict__ rbuf, uint64_t seed) {
    __shared__ uint8_t order[kGroupsPerBlock][64];
    __shared__ ExtJob jobs[kGroupsPerBlock][kMaxExtJobs];
    __shared__ uint32_t njobs[kGroupsPerBlock];

    uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    int64_t i = (int64_t)blockIdx.x * kGroupsPerBlock + g;
    uint32_t total = i < n ? (uint32_t)rlen[i] : 0;
    const uint8_t* body = nullptr;
    bool edns = false;
    if (total != 0) {
        body = arena + bodyOff[i];
        uint32_t m = meta[i];
        edns = (m & kMetaEdns) != 0;
        if (lane == 0)
            njobs[g] = planReply(body, total - (edns ? kOptLen : 0), m, seed,
                                 (uint64_t)i, order[g], jobs[g]);
    }
    __syncthreads();  /* the plans are in LDS; no barrier below */
    if (total == 0) return;

    uint8_t* dst = rbuf + roff[i];
    const uint8_t* q = qbuf + qoff[i];
    /* the reply's header: id and RD come from the query, and an OPT
     * behind the reply counts in ARCOUNT, bytes 10 and 11, big-endian */
    const uint8_t* first = body[0] == 1 ? body + 6 + 8 * body[1] : body + 4;
    if (lane < 12) {
        uint32_t v = first[lane];
        if (lane < 2) v = q[lane];
        if (lane == 2) v |= q[2] & 1u;
        if (edns && lane == 11) v += 1;
        if (edns && lane == 10) v += first[11] == 0xFF;
        dst[lane] = (uint8_t)v;
    }
    uint32_t nj = njobs[g];
    for (uint32_t j = 0; j < nj; ++j) {
        ExtJob jb = jobs[g][j];
        const uint8_t* base = jb.source == kSrcBody    ? body
                              : jb.source == kSrcQuery ? q
                                                       : kOptSrc + 4;
        groupCopy(dst + jb.dst, base + jb.src, jb.len, lane);
    }
}

hipError_t launchLookupExt(const Batch& b, const Image& img,
                           uint32_t accept, uint32_t* bodyOff,
                           int32_t* rlen, uint32_t* meta,
                           hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    if ((accept & ~kAcceptAll) != 0) return hipErrorInvalidValue;
    uint32_t blocks = ((uint32_t)b.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(bamd_resolve_lookup_ext, dim3(blocks), dim3(kTile), 0,
                       stream, b.qbuf, b.qoff, b.qbytes, b.n,
                       (const uint4*)img.slots, img.cap, img.arena, accept,
                       bodyOff, rlen, meta);
    return hipGetLastError();
}

hipError_t launchEmitExt(const Batch& b, const Image& img,
                         const uint32_t* bodyOff, const int32_t* rlen,
                         const uint32_t* meta, const int64_t* roff,
                         uint8_t* rbuf, uint64_t seed, hipStream_t stream) {
    if (b.n <= 0) return hipSuccess;
    uint32_t blocks =
        ((uint32_t)b.n + kGroupsPerBlock - 1) / kGroupsPerBlock;
    hipLaunchKernelGGL(bamd_resolve_emit_ext, dim3(blocks), dim3(kEmitBlock),
                       0, stream, b.qbuf, b.qoff, b.n, img.arena, bodyOff,
                       rlen, meta, roff, rbuf, seed);
    return hipGetLastError();
}

}  // namespace bamd::gpu
