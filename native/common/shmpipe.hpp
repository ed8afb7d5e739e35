/*
 * binder-amd: a pair of single-producer/single-consumer byte rings in one
 * shared-memory region, with eventfd doorbells.
 *
 * The balancer <-> binderd hop carries bsock1 frames. Over the UNIX
 * stream socket every batch costs a write(), an epoll wakeup and a
 * read() in each direction; here a batch is a memcpy into a ring, and a
 * syscall is made only when the other side is asleep.
 *
 * Layout of the region (one memfd, mapped by both processes):
 *
 *   [0, kDataOff)                  two control blocks (RingCtl), the
 *                                  query ring's first
 *   [kDataOff, +cap)               query ring data   (balancer -> binderd)
 *   [kDataOff + cap, +cap)         reply ring data   (binderd -> balancer)
 *
 * cap is a power of two. Every field of a control block sits on a cache
 * line of its own: `tail` is written by the producer only, `head` by the
 * consumer only, and the two flags are what the doorbells hang on.
 *
 * It is a byte pipe, not a frame queue: write() takes what fits (a
 * partial accept is normal, like a short write on a socket), read()
 * copies out what is there. The consumer copies into a buffer of its
 * own and parses that; no parser ever looks at memory the peer can
 * still change.
 *
 * Hostile peer. The peer owns one index of each ring and can store
 * anything there. Each side therefore keeps its own index in private
 * memory (it never reads it back from the region), loads the peer's
 * index exactly once per call into a local, and checks it before use:
 * head <= tail, tail - head <= cap, and no step backwards against the
 * value seen last time (the indices are free-running 64-bit byte counts;
 * they do not wrap in the life of a connection). A violation marks the
 * ring bad(); read() and write() then return 0 for good and the owner
 * closes the connection as it does for a bad frame magic. The two
 * indices are the only lengths taken from shared memory, and after the
 * check every offset is masked with cap - 1, so no access leaves the
 * data area. The memfd is sealed against resizing by its maker and the
 * accepting side refuses one that is not, so the mapping cannot be
 * truncated under either of them.
 *
 * Doorbells. One eventfd per direction of wakeup (not per ring): a
 * process waits on one, registered edge-triggered so it never needs
 * reading, and writes the other. Two flags per ring say who is asleep:
 *
 *   consumerParked   set by the consumer before it sleeps
 *   producerWaiting  set by the producer after a short write
 *
 * Consumer, going to sleep:            Producer, after a write:
 *   parked = 1                           tail = new (release)
 *   fence(seq_cst)                       fence(seq_cst)
 *   if (tail != head) don't sleep        if (parked) { if (xchg(parked,0))
 *                                                         ring doorbell }
 *
 * No wakeup is lost: both sides store, fence, then load the other's
 * variable. In the single total order of seq_cst fences one fence comes
 * first. If the consumer's does, the producer's load of `parked` comes
 * after the consumer's store and sees 1: it rings. If the producer's
 * does, the consumer's load of `tail` sees the new value: it does not
 * sleep. (Both may happen; then the doorbell is merely spurious.) The
 * doorbell is an eventfd counter, so a ring that arrives before the
 * consumer reaches epoll_wait is still there when it does. The same
 * argument, with head for tail, holds for producerWaiting: the producer
 * sets it, fences and re-checks the space; the consumer publishes head,
 * fences and looks at the flag.
 *
 * The argument needs the flag to be stored on *every* way into sleep,
 * not only the first. The other side clears it with exchange(0) when it
 * rings, and it may ring late: the producer publishes D1, is descheduled
 * before it looks at the flag, the consumer (awake for another reason)
 * takes D1 and parks again, and only then does the producer see the
 * flag, clear it and ring. The consumer wakes to an empty ring with the
 * shared flag at 0. If it now went back to sleep remembering "I have
 * set it already", the next write would see 0, ring nothing, and the
 * data would sit there until some unrelated event. So park() and
 * waitForSpace() store the flag unconditionally each time; the private
 * parked_ only tells read() that there may be a flag to take down. A
 * flag left set by a side that did not go to sleep after all, or a
 * doorbell rung late, costs one spurious wakeup; with the flag
 * re-stored on every park it cannot cost a lost one.
 *
 * No dependency on sockets or on the event loop.
 */
#pragma once

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>

namespace bamd::shm {

constexpr uint32_t kVersion = 1;
constexpr size_t kMinRing = 4096;
constexpr size_t kMaxRing = 64u << 20;
/* per direction. A ring's cursor walks its whole data area, so all of
 * it is touched sooner or later: the size is resident memory and cache
 * footprint per connection, not just address space. 256 KiB holds some
 * twenty batches of the size the chain runs at; what does not fit waits
 * in the producer's own queue, as it does behind a full socket. */
constexpr size_t kDefaultRing = 256u << 10;
constexpr size_t kDataOff = 4096;

struct RingCtl {
    alignas(64) std::atomic<uint64_t> tail;  /* producer */
    alignas(64) std::atomic<uint64_t> head;  /* consumer */
    alignas(64) std::atomic<uint32_t> consumerParked;
    alignas(64) std::atomic<uint32_t> producerWaiting;
};
static_assert(std::atomic<uint64_t>::is_always_lock_free &&
                  std::atomic<uint32_t>::is_always_lock_free,
              "ring indices live in memory shared between processes");
static_assert(sizeof(RingCtl) == 256 && 2 * sizeof(RingCtl) <= kDataOff);

inline bool validRingBytes(uint64_t cap) {
    return cap >= kMinRing && cap <= kMaxRing && (cap & (cap - 1)) == 0;
}
inline size_t regionBytes(size_t cap) { return kDataOff + 2 * cap; }

/* write the doorbell's eventfd; a full counter (never, in practice) or
 * a closed fd is not an error worth acting on */
inline void ringDoorbell(int efd) {
    uint64_t one = 1;
    ssize_t rv = ::write(efd, &one, sizeof(one));
    (void)rv;
}

/* The producing end of one ring. */
class Producer {
  public:
    void attach(RingCtl* ctl, uint8_t* data, size_t cap) {
        ctl_ = ctl;
        data_ = data;
        cap_ = cap;
        tail_ = 0;
        lastHead_ = 0;
        bad_ = false;
    }
    bool bad() const { return bad_; }

    /* bytes accepted, 0..len */
    size_t write(const void* src, size_t len) {
        size_t room = space();
        if (len > room) len = room;
        if (len == 0) return 0;
        size_t off = (size_t)(tail_ & (cap_ - 1));
        size_t first = cap_ - off;
        if (first > len) first = len;
        memcpy(data_ + off, src, first);
        if (len > first)
            memcpy(data_, (const uint8_t*)src + first, len - first);
        tail_ += len;
        ctl_->tail.store(tail_, std::memory_order_release);
        return len;
    }

    /* After publishing: must the consumer be woken? True at most once
     * per parking; the caller then rings the doorbell. */
    bool consumerNeedsWake() {
        std::atomic_thread_fence(std::memory_order_seq_cst);
        if (ctl_->consumerParked.load(std::memory_order_relaxed) == 0)
            return false;
        return ctl_->consumerParked.exchange(
                   0, std::memory_order_acq_rel) != 0;
    }

    /* After a short write: announce that this side waits for space.
     * False = space has appeared meanwhile, write again. True = the
     * consumer will ring the doorbell when it has advanced. */
    bool waitForSpace() {
        ctl_->producerWaiting.store(1, std::memory_order_relaxed);
        std::atomic_thread_fence(std::memory_order_seq_cst);
        if (space() == 0 && !bad_) return true;
        ctl_->producerWaiting.store(0, std::memory_order_relaxed);
        return false;
    }

  private:
    size_t space() {
        if (bad_) return 0;
        uint64_t head = ctl_->head.load(std::memory_order_acquire);
        if (head > tail_ || tail_ - head > cap_ || head < lastHead_) {
            bad_ = true;
            return 0;
        }
        lastHead_ = head;
        return cap_ - (size_t)(tail_ - head);
    }

    RingCtl* ctl_ = nullptr;
    uint8_t* data_ = nullptr;
    size_t cap_ = 0;
    uint64_t tail_ = 0;      /* ours; never read back from the region */
    uint64_t lastHead_ = 0;  /* the peer's, as last accepted */
    bool bad_ = false;
};

/* The consuming end of one ring. */
class Consumer {
  public:
    void attach(RingCtl* ctl, const uint8_t* data, size_t cap) {
        ctl_ = ctl;
        data_ = data;
        cap_ = cap;
        head_ = 0;
        lastTail_ = 0;
        parked_ = false;
        bad_ = false;
    }
    bool bad() const { return bad_; }

    /* bytes waiting; 0 on a bad ring (look at bad()) */
    size_t readable() {
        if (bad_) return 0;
        uint64_t tail = ctl_->tail.load(std::memory_order_acquire);
        if (tail < head_ || tail - head_ > cap_ || tail < lastTail_) {
            bad_ = true;
            return 0;
        }
        lastTail_ = tail;
        return (size_t)(tail - head_);
    }

    /* bytes copied out, 0..len */
    size_t read(void* dst, size_t len) {
        size_t have = readable();
        if (len > have) len = have;
        if (len == 0) return 0;
        if (parked_) {
            parked_ = false;
            ctl_->consumerParked.store(0, std::memory_order_relaxed);
        }
        size_t off = (size_t)(head_ & (cap_ - 1));
        size_t first = cap_ - off;
        if (first > len) first = len;
        memcpy(dst, data_ + off, first);
        if (len > first) memcpy((uint8_t*)dst + first, data_, len - first);
        head_ += len;
        ctl_->head.store(head_, std::memory_order_release);
        return len;
    }

    /* After read() advanced the head: must a waiting producer be
     * woken? The caller then rings the doorbell. */
    bool producerNeedsWake() {
        std::atomic_thread_fence(std::memory_order_seq_cst);
        if (ctl_->producerWaiting.load(std::memory_order_relaxed) == 0)
            return false;
        return ctl_->producerWaiting.exchange(
                   0, std::memory_order_acq_rel) != 0;
    }

    /* Before sleeping. True = parked, go to sleep; false = there is
     * something to read (or the ring is bad), do not sleep. */
    bool park() {
        /* stored every time: the producer's exchange(0) clears the flag
         * behind our back (a doorbell rung late finds the ring already
         * empty), so what we set last time says nothing about now */
        parked_ = true;
        ctl_->consumerParked.store(1, std::memory_order_relaxed);
        std::atomic_thread_fence(std::memory_order_seq_cst);
        return readable() == 0 && !bad_;
    }

  private:
    RingCtl* ctl_ = nullptr;
    const uint8_t* data_ = nullptr;
    size_t cap_ = 0;
    uint64_t head_ = 0;      /* ours; never read back from the region */
    uint64_t lastTail_ = 0;  /* the peer's, as last accepted */
    bool parked_ = false;    /* we left consumerParked set */
    bool bad_ = false;
};

/* The mapped region. The offering side create()s it, the accepting
 * side attach()es to the fd it was sent. */
class Region {
  public:
    Region() = default;
    Region(const Region&) = delete;
    Region& operator=(const Region&) = delete;
    ~Region() { reset(); }

    /* new memfd of the right size, mapped and zeroed; -1 on failure,
     * else the fd (owned by the caller) */
    int create(size_t cap) {
        reset();
        if (!validRingBytes(cap)) return -1;
        int fd = memfd_create("bsock1-rings",
                              MFD_CLOEXEC | MFD_ALLOW_SEALING);
        if (fd < 0) return -1;
        /* sealed against resizing: the accepting side will not map a
         * file that its peer could truncate under it (SIGBUS) */
        if (ftruncate(fd, (off_t)regionBytes(cap)) != 0 ||
            fcntl(fd, F_ADD_SEALS, F_SEAL_SHRINK | F_SEAL_GROW) != 0 ||
            !map(fd, cap)) {
            ::close(fd);
            return -1;
        }
        for (int i = 0; i < 2; ++i) {
            RingCtl* c = new (base_ + i * sizeof(RingCtl)) RingCtl;
            c->tail.store(0, std::memory_order_relaxed);
            c->head.store(0, std::memory_order_relaxed);
            c->consumerParked.store(0, std::memory_order_relaxed);
            c->producerWaiting.store(0, std::memory_order_relaxed);
        }
        return fd;
    }

    /* map a region made by the peer; the geometry it claims must be
     * what the fd really holds */
    bool attach(int fd, uint64_t cap) {
        reset();
        if (!validRingBytes(cap)) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) ||
            (uint64_t)st.st_size != regionBytes((size_t)cap))
            return false;
        int seals = fcntl(fd, F_GET_SEALS);
        if (seals < 0 || (seals & F_SEAL_SHRINK) == 0) return false;
        return map(fd, (size_t)cap);
    }

    void reset() {
        if (base_ != nullptr) munmap(base_, regionBytes(cap_));
        base_ = nullptr;
        cap_ = 0;
    }

    bool mapped() const { return base_ != nullptr; }
    size_t cap() const { return cap_; }
    /* ring 0 = queries, ring 1 = replies */
    RingCtl* ctl(int ring) const {
        return reinterpret_cast<RingCtl*>(base_ + ring * sizeof(RingCtl));
    }
    uint8_t* data(int ring) const {
        return base_ + kDataOff + (size_t)ring * cap_;
    }

  private:
    bool map(int fd, size_t cap) {
        void* p = mmap(nullptr, regionBytes(cap), PROT_READ | PROT_WRITE,
                       MAP_SHARED, fd, 0);
        if (p == MAP_FAILED) return false;
        base_ = (uint8_t*)p;
        cap_ = cap;
        return true;
    }

    uint8_t* base_ = nullptr;
    size_t cap_ = 0;
};

/* One connection's end of the pair: the mapping, the ring ends this
 * side uses, and the two doorbells. The memfd itself is closed as soon
 * as it is mapped (and, on the offering side, sent). */
struct Link {
    Region region;
    Producer tx;
    Consumer rx;
    int wakeMe = -1;    /* eventfd this side waits on (EPOLLET) */
    int wakePeer = -1;  /* eventfd this side writes */

    Link() = default;
    Link(const Link&) = delete;
    Link& operator=(const Link&) = delete;
    ~Link() { close(); }

    /* balancer: writes ring 0, reads ring 1; backend: the reverse */
    void attachEnds(bool balancer) {
        int t = balancer ? 0 : 1, r = balancer ? 1 : 0;
        tx.attach(region.ctl(t), region.data(t), region.cap());
        rx.attach(region.ctl(r), region.data(r), region.cap());
    }
    void close() {
        region.reset();
        if (wakeMe >= 0) ::close(wakeMe);
        if (wakePeer >= 0) ::close(wakePeer);
        wakeMe = wakePeer = -1;
    }
};

}  // namespace bamd::shm
