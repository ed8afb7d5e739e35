/*
 * binder-amd: one-pass grouping of UDP replies into UDP_SEGMENT runs.
 *
 * A backend read event carries hundreds of replies for a handful of
 * client sockets. Sent one by one, each costs a full loopback/NIC
 * traversal; sent as one UDP_SEGMENT super-packet per destination, the
 * kernel cost is per run. The balancer used to collect 128 replies,
 * sort them by (address, length) and rediscover the runs; here each
 * reply is filed under its (destination, length) key as it is parsed,
 * in a small fixed table found by hash and confirmed by full compare,
 * and the runs are sent when they fill up or when the event ends.
 *
 * Rules of a run: one destination; every segment the same length,
 * except that one shorter reply for the same destination may close it
 * (UDP_SEGMENT's trailing segment); at most kMaxSegs segments and
 * kMaxBytes bytes (one UDP datagram caps near 64 KB). A run of one
 * leaves through the singles batch (sendmmsg). When the table has no
 * room for a new key an entry is replaced, its open run flushed first;
 * nothing is allocated after construction.
 *
 * The iovecs handed to add() are kept, not copied: whatever they point
 * into must stay where it is until finish() returns.
 *
 * No dependency on sockets or the event loop. The Sink provides
 *   int  sendRun(const sockaddr*, socklen_t, iovec*, size_t n,
 *                uint16_t seg)          0, or the errno of the failure
 *   void sendOne(const sockaddr*, socklen_t, iovec*)
 *   void sendBatch(mmsghdr*, unsigned n)
 * Any sendRun failure re-sends that run's replies one by one;
 * EINVAL/EIO/ENOTSUP (no UDP_SEGMENT here) also turns runs off for
 * good, after which every reply takes the singles batch.
 */
#pragma once

#include <netinet/in.h>
#include <sys/socket.h>

#include <cerrno>
#include <cstdint>
#include <cstring>

namespace bamd {

template <class Sink>
class ReplyRuns {
  public:
    static constexpr size_t kMaxSegs = 48;
    static constexpr size_t kMaxBytes = 60000;
    /* table entries. A worker serves a few client flows times a few
     * reply sizes; 64 keys cover that without replacement. */
    static constexpr size_t kRuns = 64;
    static constexpr size_t kIndex = 256;  /* hash slots, 1/4 full */
    static constexpr unsigned kSingleBatch = 128;

    explicit ReplyRuns(Sink& sink) : sink_(sink) {
        memset(heads_, 0, sizeof(heads_));
        memset(index_, 0, sizeof(index_));
        memset(singleHdrs_, 0, sizeof(singleHdrs_));
    }

    bool gso() const { return gso_; }
    void setGso(bool on) { gso_ = on; }

    /* replies accepted and not yet handed to the sink */
    size_t pending() const { return held_ + nSingle_; }

    uint64_t runs() const { return runs_; }
    uint64_t runSegments() const { return runSegments_; }
    uint64_t singles() const { return singles_; }

    /* family 4 or 6; addr holds 4 or 16 bytes (network order); port in
     * host order */
    void add(uint8_t family, const uint8_t* addr, uint16_t port,
             const struct iovec& iov) {
        size_t len = iov.iov_len;
        uint64_t a0 = 0, a1 = 0;
        if (family == 4) {
            uint32_t v4;
            memcpy(&v4, addr, 4);
            a0 = v4;
        } else {
            memcpy(&a0, addr, 8);
            memcpy(&a1, addr + 8, 8);
        }
        /* no run possible: GSO off, an empty payload (a zero segment
         * size is not a valid UDP_SEGMENT), or two of these would
         * already pass the byte cap */
        if (!gso_ || len == 0 || len * 2 > kMaxBytes) {
            single(family, a0, a1, port, iov);
            return;
        }
        uint64_t meta = ((uint64_t)len << 32) | ((uint64_t)port << 8) |
                        family;
        uint64_t h = (a0 ^ (a1 * 0x9e3779b97f4a7c15ull) ^
                      (meta * 0xff51afd7ed558ccdull));
        h ^= h >> 29;
        h *= 0xc4ceb9fe1a85ec53ull;
        h ^= h >> 32;
        /* hash first, then the whole key. A key stays in the table
         * after its run has left: the same client asks again. */
        size_t i = (size_t)h & (kIndex - 1);
        for (; index_[i] != 0; i = (i + 1) & (kIndex - 1)) {
            Head* e = &heads_[index_[i] - 1];
            if (e->hash == h && e->meta == meta && e->a0 == a0 &&
                e->a1 == a1) {
                append(e, iov);
                return;
            }
        }
        Head* e;
        if (used_ < kRuns) {
            e = &heads_[used_++];
        } else {
            /* table full: the entry under the clock hand makes room,
             * its open run (if any) leaves now */
            e = &heads_[hand_];
            hand_ = (hand_ + 1) % kRuns;
            if (e->count != 0) flushRun(e);
            unindex(e);
            for (i = (size_t)h & (kIndex - 1); index_[i] != 0;
                 i = (i + 1) & (kIndex - 1)) {
            }
        }
        index_[i] = (uint8_t)(e - heads_ + 1);
        e->hash = h;
        e->meta = meta;
        e->a0 = a0;
        e->a1 = a1;
        append(e, iov);
    }

    /* End of the event: every reply accepted so far is handed to the
     * sink before this returns. */
    void finish() {
        if (held_ != 0) {
            /* a lone reply may still close a longer-segment run for
             * the same destination (the trailing-segment rule) */
            for (unsigned k = 0; k < nActive_; ++k) {
                Head* e = &heads_[active_[k]];
                if (e->count == 1) adoptAsTail(e);
            }
        }
        for (unsigned k = 0; k < nActive_; ++k) {
            Head* e = &heads_[active_[k]];
            e->listed = 0;
            if (e->count != 0) flushRun(e);
        }
        nActive_ = 0;
        flushSingles();
    }

  private:
    struct Head {
        uint64_t hash;
        uint64_t meta;  /* len << 32 | port << 8 | family */
        uint64_t a0, a1;
        uint32_t bytes;
        uint16_t count;  /* replies in the open run; 0 = none */
        uint16_t listed; /* on active_ for this event */
    };
    union Addr {
        struct sockaddr_in v4;
        struct sockaddr_in6 v6;
    };

    static uint8_t familyOf(uint64_t meta) { return (uint8_t)meta; }
    static uint16_t portOf(uint64_t meta) {
        return (uint16_t)(meta >> 8);
    }
    static size_t segOf(uint64_t meta) { return (size_t)(meta >> 32); }

    static socklen_t fill(Addr* out, uint8_t family, uint64_t a0,
                          uint64_t a1, uint16_t port) {
        if (family == 4) {
            out->v4 = {};
            out->v4.sin_family = AF_INET;
            out->v4.sin_port = htons(port);
            uint32_t v4 = (uint32_t)a0;
            memcpy(&out->v4.sin_addr, &v4, 4);
            return sizeof(out->v4);
        }
        out->v6 = {};
        out->v6.sin6_family = AF_INET6;
        out->v6.sin6_port = htons(port);
        memcpy(&out->v6.sin6_addr, &a0, 8);
        memcpy((uint8_t*)&out->v6.sin6_addr + 8, &a1, 8);
        return sizeof(out->v6);
    }

    struct iovec* iovsOf(Head* e) {
        return iovs_[(size_t)(e - heads_)];
    }

    void append(Head* e, const struct iovec& iov) {
        if (e->count == 0) {
            e->bytes = 0;
            if (!e->listed) {
                e->listed = 1;
                active_[nActive_++] = (uint8_t)(e - heads_);
            }
        }
        iovsOf(e)[e->count++] = iov;
        e->bytes += (uint32_t)iov.iov_len;
        held_++;
        size_t seg = segOf(e->meta);
        if (e->count == kMaxSegs || e->bytes + seg > kMaxBytes)
            flushRun(e);
    }

    /* take e's key out of the hash index (linear probing, backward
     * shift: no tombstones) */
    void unindex(Head* e) {
        constexpr size_t mask = kIndex - 1;
        uint8_t id = (uint8_t)(e - heads_ + 1);
        size_t i = (size_t)e->hash & mask;
        while (index_[i] != id) i = (i + 1) & mask;
        for (size_t j = i;;) {
            j = (j + 1) & mask;
            if (index_[j] == 0) break;
            size_t home = (size_t)heads_[index_[j] - 1].hash & mask;
            /* an entry whose home lies cyclically in (i, j] stays */
            bool stays = i <= j ? (i < home && home <= j)
                                : (i < home || home <= j);
            if (stays) continue;
            index_[i] = index_[j];
            i = j;
        }
        index_[i] = 0;
    }

    void adoptAsTail(Head* lone) {
        size_t len = segOf(lone->meta);
        uint64_t dest = lone->meta & 0xffffffffull;
        for (unsigned k = 0; k < nActive_; ++k) {
            Head* e = &heads_[active_[k]];
            if (e->count == 0 || e == lone) continue;
            if ((e->meta & 0xffffffffull) != dest || e->a0 != lone->a0 ||
                e->a1 != lone->a1)
                continue;
            /* open runs hold equal segments only, so a shorter reply
             * is a valid last segment of any of them; append() left
             * room for one more under both caps */
            if (segOf(e->meta) <= len) continue;
            iovsOf(e)[e->count++] = iovsOf(lone)[0];
            e->bytes += (uint32_t)len;
            lone->count = 0;
            flushRun(e);
            return;
        }
    }

    /* hand one open run to the sink and free its entry */
    void flushRun(Head* e) {
        struct iovec* iov = iovsOf(e);
        size_t n = e->count;
        uint8_t family = familyOf(e->meta);
        uint16_t port = portOf(e->meta);
        e->count = 0;
        held_ -= n;
        if (n == 1 || !gso_) {
            for (size_t k = 0; k < n; ++k)
                single(family, e->a0, e->a1, port, iov[k]);
            return;
        }
        Addr dst;
        socklen_t dlen = fill(&dst, family, e->a0, e->a1, port);
        int err = sink_.sendRun((const struct sockaddr*)&dst, dlen, iov,
                                n, (uint16_t)segOf(e->meta));
        if (err == 0) {
            runs_++;
            runSegments_ += n;
            return;
        }
        if (err == EINVAL || err == EIO || err == ENOTSUP)
            gso_ = false;  /* disable permanently */
        /* ANY failure: the whole run would be lost - resend its
         * replies individually */
        for (size_t k = 0; k < n; ++k)
            sink_.sendOne((const struct sockaddr*)&dst, dlen, &iov[k]);
        singles_ += n;
    }

    void single(uint8_t family, uint64_t a0, uint64_t a1, uint16_t port,
                const struct iovec& iov) {
        if (nSingle_ == kSingleBatch) flushSingles();
        unsigned i = nSingle_++;
        singleIovs_[i] = iov;
        struct msghdr* mh = &singleHdrs_[i].msg_hdr;
        mh->msg_namelen = fill(&singleAddrs_[i], family, a0, a1, port);
        mh->msg_name = &singleAddrs_[i];
        mh->msg_iov = &singleIovs_[i];
        mh->msg_iovlen = 1;
    }

    void flushSingles() {
        if (nSingle_ == 0) return;
        sink_.sendBatch(singleHdrs_, nSingle_);
        singles_ += nSingle_;
        nSingle_ = 0;
    }

    Sink& sink_;
    bool gso_ = true;
    size_t held_ = 0;  /* replies sitting in open runs */
    unsigned nSingle_ = 0;
    uint64_t runs_ = 0, runSegments_ = 0, singles_ = 0;
    unsigned used_ = 0;    /* entries that hold a key */
    unsigned hand_ = 0;    /* replacement clock */
    unsigned nActive_ = 0; /* entries touched in this event */
    Head heads_[kRuns];
    uint8_t index_[kIndex];  /* 0 = empty, else entry number + 1 */
    uint8_t active_[kRuns];
    struct iovec iovs_[kRuns][kMaxSegs];
    struct mmsghdr singleHdrs_[kSingleBatch];
    struct iovec singleIovs_[kSingleBatch];
    Addr singleAddrs_[kSingleBatch];
};

}  // namespace bamd
