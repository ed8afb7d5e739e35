/*
 * binder-amd: dense answer table - a memo of the fast path's finished
 * replies, keyed by (lowercase qname, qtype).
 *
 * The store walk behind a fast-path answer touches ~5 dependent cache
 * lines for a host and ~20 for an SRV (hash bucket, key node, mirror
 * node, CompiledRecord, wire block, service cache, member vectors,
 * three segment vectors per member). Here a hit touches one 16-byte
 * slot and one contiguous blob:
 *
 *   slot  := hash(u64) off(u32) len(u32)          len == 0: empty
 *   blob  := klen(u8) qtype(u8) key[klen] body
 *
 * Slots form an open-addressing, power-of-two table with linear
 * probing and backward-shift deletion (no tombstones). Blobs live end
 * to end in one byte arena; a hit is confirmed by comparing the key
 * bytes in the blob, never by the hash alone. The caller supplies the
 * hash, so related entries can share one: the server hashes a
 * service's SRV entry on the service's domain, and removeSuffix()
 * then finds it given only that domain.
 *
 * Arena bound: a removed or replaced blob's bytes stay behind as dead
 * space. When dead bytes exceed both kCompactMinDead and the live
 * bytes, the arena is rebuilt from the live blobs (slots keep their
 * place, offsets change). An insert that would take the arena past
 * maxArena even after a rebuild clears the whole table instead: the
 * table is a memo, so dropping it only costs misses. Steady-state
 * arena size is therefore <= 2 x live + kCompactMinDead, and never
 * above maxArena (default 256 MiB; 100 k records take ~25 MiB).
 *
 * Pointers and offsets returned by find()/probe()/insert() hold until
 * the next mutating call; generation() changes on every mutation so a
 * caller can tell whether a remembered offset is still good.
 *
 * Body helpers below define the two body layouts the server stores:
 * a finished wire reply, and a service reply kept as head + per-member
 * segments that are permuted per query.
 *
 * No dependency on the server, the stores or sockets (stand-alone
 * check: `make check-answertab`).
 */
#pragma once

#include <cstdint>
#include <cstring>
#include <memory>

namespace bamd {

#ifdef BAMD_ANSWERTAB_TEST_HASH_MASK
/* test builds force collisions by masking every key hash */
inline uint64_t answertabTestHashMask = ~0ull;
#endif

class AnswerTable {
  public:
    static constexpr size_t kMaxKey = 255;
    static constexpr uint32_t kNone = 0xFFFFFFFFu;
    static constexpr size_t kMinSlots = 1024;
    static constexpr size_t kCompactMinDead = 1u << 20;
    static constexpr size_t kDefaultMaxArena = 256u << 20;

    explicit AnswerTable(size_t maxArena = kDefaultMaxArena,
                         size_t compactMinDead = kCompactMinDead)
        : maxArena_(maxArena), compactMinDead_(compactMinDead) {}

    /* the hash callers are expected to use */
    static uint64_t hashKey(const void* key, size_t klen, uint8_t qtype) {
        const uint8_t* p = (const uint8_t*)key;
        uint64_t h = 0x9E3779B97F4A7C15ull ^
                     ((uint64_t)klen * 0xD6E8FEB86659FD93ull) ^
                     ((uint64_t)qtype << 56);
        size_t n = klen;
        /* one multiply per 8 bytes; the closing mix() spreads every
         * input bit over the low (slot index) bits */
        while (n >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
            h ^= h >> 32;
            p += 8;
            n -= 8;
        }
        if (n != 0) {
            uint64_t w = 0;
            memcpy(&w, p, n);
            h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
            h ^= h >> 32;
        }
        h = mix(h);
#ifdef BAMD_ANSWERTAB_TEST_HASH_MASK
        h &= answertabTestHashMask;
#endif
        return h;
    }

    size_t size() const { return count_; }
    size_t slots() const { return cap_; }
    size_t arenaBytes() const { return used_; }
    size_t deadBytes() const { return dead_; }
    uint64_t generation() const { return gen_; }
    uint64_t rebuilds() const { return rebuilds_; }
    uint64_t clears() const { return clears_; }

    void prefetchSlot(uint64_t h) const {
        if (cap_ != 0) __builtin_prefetch(&slots_[h & (cap_ - 1)]);
    }

    /* Offset of the first blob whose slot carries exactly this hash,
     * or kNone. Reads slot lines only; the blob is not touched, so the
     * caller can prefetch it and confirm the key later with at(). */
    uint32_t probe(uint64_t h, uint32_t* blobLen = nullptr) const {
        if (cap_ == 0) return kNone;
        size_t mask = cap_ - 1;
        for (size_t i = h & mask;; i = (i + 1) & mask) {
            const Slot& s = slots_[i];
            if (s.len == 0) return kNone;
            if (s.hash == h) {
                if (blobLen != nullptr) *blobLen = s.len;
                return s.off;
            }
        }
    }
    void prefetchBlob(uint32_t off, uint32_t len) const {
        const uint8_t* p = arena_.get() + off;
        for (uint32_t o = 0; o < len; o += 64) __builtin_prefetch(p + o);
        __builtin_prefetch(p + len - 1);
    }
    /* Body of the blob at `off` when its key is (key, qtype), else
     * nullptr. `off` must come from probe() in this generation. */
    const uint8_t* at(uint32_t off, uint8_t qtype, const void* key,
                      size_t klen) const {
        const uint8_t* b = arena_.get() + off;
        if (b[0] != klen || b[1] != qtype ||
            memcmp(b + 2, key, klen) != 0)
            return nullptr;
        return b + 2 + klen;
    }

    /* body of the entry, or nullptr; *bodyLen set on a hit */
    const uint8_t* find(uint64_t h, uint8_t qtype, const void* key,
                        size_t klen, uint32_t* bodyLen = nullptr) const {
        size_t i = locate(h, qtype, key, klen);
        if (i == kNoSlot) return nullptr;
        const Slot& s = slots_[i];
        if (bodyLen != nullptr) *bodyLen = s.len - 2 - (uint32_t)klen;
        return arena_.get() + s.off + 2 + klen;
    }

    /* Add or replace an entry and return its zero-filled body of
     * bodyLen bytes for the caller to fill in, or nullptr when the
     * entry cannot be stored (key too long, blob above maxArena). */
    uint8_t* insert(uint64_t h, uint8_t qtype, const void* key,
                    size_t klen, size_t bodyLen) {
        if (klen > kMaxKey) return nullptr;
        size_t blen = 2 + klen + bodyLen;
        if (blen > maxArena_ || blen >= kNone) return nullptr;
        ++gen_;
        size_t i = locate(h, qtype, key, klen);
        if (i != kNoSlot) {  /* replace: old blob becomes dead space */
            dead_ += slots_[i].len;
            slots_[i].len = 0;  /* keeps reserve()'s rebuild off it */
            if (!reserve(blen)) return nullptr;  /* table cleared */
            slots_[i].hash = h;
        } else {
            if (!reserve(blen)) return nullptr;
            if ((count_ + 1) * 2 > cap_) growSlots();
            size_t mask = cap_ - 1;
            i = h & mask;
            while (slots_[i].len != 0) i = (i + 1) & mask;
            slots_[i].hash = h;
            ++count_;
        }
        slots_[i].off = (uint32_t)used_;
        slots_[i].len = (uint32_t)blen;
        uint8_t* b = arena_.get() + used_;
        used_ += blen;
        b[0] = (uint8_t)klen;
        b[1] = qtype;
        if (klen != 0) memcpy(b + 2, key, klen);
        memset(b + 2 + klen, 0, bodyLen);
        return b + 2 + klen;
    }

    bool remove(uint64_t h, uint8_t qtype, const void* key, size_t klen) {
        size_t i = locate(h, qtype, key, klen);
        if (i == kNoSlot) return false;
        ++gen_;
        eraseSlot(i);
        return true;
    }

    /* Remove every entry stored under hash h with this qtype whose key
     * is `suffix` or ends in "." + suffix. Returns how many went. */
    size_t removeSuffix(uint64_t h, uint8_t qtype, const void* suffix,
                        size_t slen) {
        if (cap_ == 0) return 0;
        size_t mask = cap_ - 1, removed = 0;
        size_t i = h & mask;
        while (slots_[i].len != 0) {
            const Slot& s = slots_[i];
            const uint8_t* b = arena_.get() + s.off;
            size_t klen = b[0];
            bool match =
                s.hash == h && b[1] == qtype && klen >= slen &&
                memcmp(b + 2 + klen - slen, suffix, slen) == 0 &&
                (klen == slen || b[2 + klen - slen - 1] == '.');
            if (match) {
                ++gen_;
                eraseSlot(i);  /* shifts a successor into i: look again */
                ++removed;
            } else {
                i = (i + 1) & mask;
            }
        }
        return removed;
    }

    void clear() {
        ++gen_;
        ++clears_;
        if (cap_ != 0) memset(slots_.get(), 0, cap_ * sizeof(Slot));
        count_ = 0;
        used_ = 0;
        dead_ = 0;
    }

  private:
    struct Slot {
        uint64_t hash;
        uint32_t off;
        uint32_t len;  /* whole blob; 0 = empty slot */
    };
    static constexpr size_t kNoSlot = ~(size_t)0;

    static uint64_t mix(uint64_t h) {
        h ^= h >> 32;
        h *= 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 32;
        return h;
    }

    size_t locate(uint64_t h, uint8_t qtype, const void* key,
                  size_t klen) const {
        if (cap_ == 0) return kNoSlot;
        size_t mask = cap_ - 1;
        for (size_t i = h & mask;; i = (i + 1) & mask) {
            const Slot& s = slots_[i];
            if (s.len == 0) return kNoSlot;
            if (s.hash != h) continue;
            const uint8_t* b = arena_.get() + s.off;
            if (b[0] == klen && b[1] == qtype &&
                memcmp(b + 2, key, klen) == 0)
                return i;
        }
    }

    /* backward-shift deletion: close the gap so probe chains stay
     * unbroken without tombstones */
    void eraseSlot(size_t i) {
        size_t mask = cap_ - 1;
        dead_ += slots_[i].len;
        --count_;
        size_t j = i;
        while (true) {
            j = (j + 1) & mask;
            if (slots_[j].len == 0) break;
            size_t home = slots_[j].hash & mask;
            /* move j back to i unless its home lies in (i, j] */
            bool stays = i <= j ? (home > i && home <= j)
                                : (home > i || home <= j);
            if (stays) continue;
            slots_[i] = slots_[j];
            i = j;
        }
        slots_[i].len = 0;
    }

    void growSlots() {
        size_t ncap = cap_ == 0 ? kMinSlots : cap_ * 2;
        std::unique_ptr<Slot[]> ns(new Slot[ncap]());
        size_t mask = ncap - 1;
        for (size_t k = 0; k < cap_; ++k) {
            if (slots_[k].len == 0) continue;
            size_t i = slots_[k].hash & mask;
            while (ns[i].len != 0) i = (i + 1) & mask;
            ns[i] = slots_[k];
        }
        slots_ = std::move(ns);
        cap_ = ncap;
    }

    /* Make room for blen more arena bytes. False = the bound was hit
     * and the whole table has been cleared (nothing was stored). */
    bool reserve(size_t blen) {
        if (dead_ > compactMinDead_ && dead_ > used_ - dead_) rebuild();
        if (used_ + blen > maxArena_) {
            if (dead_ != 0) rebuild();
            if (used_ + blen > maxArena_) {
                clear();
                return false;
            }
        }
        if (used_ + blen > arenaCap_) {
            size_t ncap = arenaCap_ == 0 ? (64u << 10) : arenaCap_ * 2;
            while (ncap < used_ + blen) ncap *= 2;
            if (ncap > maxArena_) ncap = maxArena_;
            std::unique_ptr<uint8_t[]> na(new uint8_t[ncap]);
            if (used_ != 0) memcpy(na.get(), arena_.get(), used_);
            arena_ = std::move(na);
            arenaCap_ = ncap;
        }
        return true;
    }

    /* copy the live blobs into a fresh arena, dropping dead space */
    void rebuild() {
        ++rebuilds_;
        size_t live = used_ - dead_;
        size_t ncap = 64u << 10;
        while (ncap < live * 2) ncap *= 2;
        if (ncap > maxArena_) ncap = maxArena_;
        std::unique_ptr<uint8_t[]> na(new uint8_t[ncap]);
        size_t w = 0;
        for (size_t k = 0; k < cap_; ++k) {
            Slot& s = slots_[k];
            if (s.len == 0) continue;
            memcpy(na.get() + w, arena_.get() + s.off, s.len);
            s.off = (uint32_t)w;
            w += s.len;
        }
        arena_ = std::move(na);
        arenaCap_ = ncap;
        used_ = w;
        dead_ = 0;
    }

    std::unique_ptr<Slot[]> slots_;
    size_t cap_ = 0;
    size_t count_ = 0;
    std::unique_ptr<uint8_t[]> arena_;
    size_t arenaCap_ = 0;
    size_t used_ = 0;
    size_t dead_ = 0;
    size_t maxArena_;
    size_t compactMinDead_;
    uint64_t gen_ = 0;
    uint64_t rebuilds_ = 0;
    uint64_t clears_ = 0;
};

/*
 * Body layouts. All integers little-endian u16, read bytewise (bodies
 * are not aligned).
 *
 *   wire     := kind(0) 0 total(u16) reply[total]
 *   service  := kind(1) n(u8) total(u16) headLen(u16)
 *               n x { off1 len1 off2 len2 }(u16 each)
 *               head[headLen] segments
 *
 * A service reply is head, then every member's first segment, then
 * every member's second segment, members in the caller's order: the
 * plain-A answer uses first segments only (len2 = 0), the SRV answer
 * has SRV records first and the additional A records second. Segment
 * offsets count from the start of `segments`.
 */
namespace answerbody {

constexpr uint8_t kWire = 0;
constexpr uint8_t kService = 1;
constexpr size_t kMaxMembers = 64;

inline void put16(uint8_t* p, size_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
inline size_t get16(const uint8_t* p) {
    return (size_t)p[0] | ((size_t)p[1] << 8);
}

inline uint8_t kind(const uint8_t* body) { return body[0]; }
inline size_t total(const uint8_t* body) { return get16(body + 2); }

inline size_t wireBodyLen(size_t total) { return 4 + total; }
inline void wireFill(uint8_t* body, const uint8_t* reply, size_t total) {
    body[0] = kWire;
    body[1] = 0;
    put16(body + 2, total);
    memcpy(body + 4, reply, total);
}
inline const uint8_t* wireReply(const uint8_t* body) { return body + 4; }

struct Seg {
    const uint8_t* p;
    size_t n;
};

inline size_t serviceBodyLen(size_t n, size_t headLen, size_t segBytes) {
    return 6 + 8 * n + headLen + segBytes;
}
/* seg1[i]/seg2[i] are member i's segments */
inline void serviceFill(uint8_t* body, size_t n, const uint8_t* head,
                        size_t headLen, const Seg* seg1,
                        const Seg* seg2) {
    body[0] = kService;
    body[1] = (uint8_t)n;
    put16(body + 4, headLen);
    uint8_t* tab = body + 6;
    uint8_t* segs = tab + 8 * n + headLen;
    memcpy(tab + 8 * n, head, headLen);
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {
        put16(tab + 8 * i, off);
        put16(tab + 8 * i + 2, seg1[i].n);
        if (seg1[i].n != 0) memcpy(segs + off, seg1[i].p, seg1[i].n);
        off += seg1[i].n;
        put16(tab + 8 * i + 4, off);
        put16(tab + 8 * i + 6, seg2[i].n);
        if (seg2[i].n != 0) memcpy(segs + off, seg2[i].p, seg2[i].n);
        off += seg2[i].n;
    }
    put16(body + 2, headLen + off);
}
inline size_t serviceMembers(const uint8_t* body) { return body[1]; }
/* Write the reply with members in the order order[0..n) into dst,
 * which has room for total(body) bytes. Returns the bytes written. */
inline size_t serviceAssemble(const uint8_t* body, const uint8_t* order,
                              uint8_t* dst) {
    size_t n = body[1];
    size_t headLen = get16(body + 4);
    const uint8_t* tab = body + 6;
    const uint8_t* head = tab + 8 * n;
    const uint8_t* segs = head + headLen;
    uint8_t* w = dst;
    memcpy(w, head, headLen);
    w += headLen;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* e = tab + 8 * order[i];
        size_t len = get16(e + 2);
        memcpy(w, segs + get16(e), len);
        w += len;
    }
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* e = tab + 8 * order[i];
        size_t len = get16(e + 6);
        if (len != 0) memcpy(w, segs + get16(e + 4), len);
        w += len;
    }
    return (size_t)(w - dst);
}

}  // namespace answerbody

}  // namespace bamd
