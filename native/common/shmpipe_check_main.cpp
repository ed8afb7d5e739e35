/*
 * Stand-alone check of shmpipe.hpp, meant to be built with
 * -fsanitize=address,undefined and again with -fsanitize=thread
 * (`make check-shmpipe`). Producer and consumer are two threads of this
 * program, over a real memfd region where the case is about the region
 * and over heap blocks of exactly the ring's size where the point is
 * that nothing is touched outside them.
 *
 *   shmpipe_check [seed] [handoffs]
 *
 * Every wait has a timeout: a lost wakeup fails the program instead of
 * hanging it.
 */
#include <poll.h>
#include <sys/eventfd.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "shmpipe.hpp"

using namespace bamd;

namespace {

std::atomic<int> g_failures{0};

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,    \
                    #cond);                                            \
            g_failures++;                                              \
        }                                                              \
    } while (0)

constexpr int kWaitMs = 10000;

/* the byte at position i of the test stream */
inline uint8_t streamByte(uint64_t i) {
    return (uint8_t)((i * 2654435761u) >> 13);
}

/* Sleep on a doorbell (level-triggered here: the counter is read to
 * clear it). False = timed out. */
bool waitBell(int efd) {
    struct pollfd p = {efd, POLLIN, 0};
    int rv = poll(&p, 1, kWaitMs);
    if (rv <= 0) return false;
    uint64_t v;
    ssize_t n = read(efd, &v, sizeof(v));
    (void)n;
    return true;
}

/* a region plus a second mapping of it, as two processes would have */
struct Pair {
    shm::Region a, b;
    int bellToB = -1, bellToA = -1;
    bool make(size_t cap) {
        int fd = a.create(cap);
        if (fd < 0) return false;
        bool ok = b.attach(fd, cap);
        close(fd);
        bellToB = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        bellToA = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        return ok && bellToA >= 0 && bellToB >= 0;
    }
    ~Pair() {
        if (bellToA >= 0) close(bellToA);
        if (bellToB >= 0) close(bellToB);
    }
};

/* 1. random chunk sizes through a 4 KiB ring, byte for byte */
void caseStream(unsigned seed) {
    Pair pr;
    CHECK(pr.make(4096));
    if (g_failures) return;
    constexpr uint64_t kTotal = 6u << 20;  /* 1536 wraps */
    std::atomic<bool> lost{false};

    std::thread producer([&]() {
        shm::Producer tx;
        tx.attach(pr.a.ctl(0), pr.a.data(0), pr.a.cap());
        std::mt19937 rng(seed);
        std::vector<uint8_t> chunk(9000);
        uint64_t sent = 0;
        while (sent < kTotal && !lost) {
            /* up to twice the ring, so partial accepts are common */
            size_t want = 1 + rng() % 9000;
            if (want > kTotal - sent) want = (size_t)(kTotal - sent);
            for (size_t i = 0; i < want; ++i)
                chunk[i] = streamByte(sent + i);
            size_t off = 0;
            while (off < want && !lost) {
                size_t n = tx.write(chunk.data() + off, want - off);
                off += n;
                if (n != 0 && tx.consumerNeedsWake())
                    shm::ringDoorbell(pr.bellToB);
                if (off < want && tx.waitForSpace() &&
                    !waitBell(pr.bellToA))
                    lost = true;
            }
            sent += want;
        }
        CHECK(!tx.bad());
    });
    std::thread consumer([&]() {
        shm::Consumer rx;
        rx.attach(pr.b.ctl(0), pr.b.data(0), pr.b.cap());
        std::mt19937 rng(seed + 1);
        std::vector<uint8_t> buf(9000);
        uint64_t seen = 0, wrong = 0;
        while (seen < kTotal && !lost) {
            size_t n = rx.read(buf.data(), 1 + rng() % 9000);
            if (n == 0) {
                if (rx.park() && !waitBell(pr.bellToB)) lost = true;
                continue;
            }
            for (size_t i = 0; i < n; ++i)
                if (buf[i] != streamByte(seen + i)) wrong++;
            seen += n;
            if (rx.producerNeedsWake()) shm::ringDoorbell(pr.bellToA);
        }
        CHECK(wrong == 0);
        CHECK(seen == kTotal);
        CHECK(!rx.bad());
    });
    producer.join();
    consumer.join();
    CHECK(!lost);
}

/* 2. ring full, partial accept, resume (one thread, heap-backed) */
void caseFull() {
    constexpr size_t kCap = 4096;
    auto ctl = std::make_unique<shm::RingCtl>();
    ctl->tail = 0;
    ctl->head = 0;
    ctl->consumerParked = 0;
    ctl->producerWaiting = 0;
    std::vector<uint8_t> data(kCap);
    shm::Producer tx;
    shm::Consumer rx;
    tx.attach(ctl.get(), data.data(), kCap);
    rx.attach(ctl.get(), data.data(), kCap);

    std::vector<uint8_t> src(6000), dst(6000);
    for (size_t i = 0; i < src.size(); ++i) src[i] = streamByte(i);
    CHECK(rx.park());                  /* empty: may sleep */
    CHECK(tx.write(src.data(), 100) == 100);
    CHECK(tx.consumerNeedsWake());     /* it was parked: ring */
    CHECK(!tx.consumerNeedsWake());    /* and only once */
    CHECK(tx.write(src.data() + 100, 5900) == kCap - 100);
    CHECK(tx.write(src.data(), 1) == 0);
    CHECK(tx.waitForSpace());          /* full: wait */
    CHECK(!rx.park());                 /* data: must not sleep */
    CHECK(rx.read(dst.data(), 1000) == 1000);
    CHECK(rx.producerNeedsWake());
    CHECK(!rx.producerNeedsWake());
    CHECK(tx.write(src.data() + kCap, 1904) == 1000);  /* wraps */
    CHECK(rx.read(dst.data() + 1000, 6000) == kCap);
    CHECK(memcmp(dst.data(), src.data(), kCap + 1000) == 0);
    CHECK(rx.readable() == 0);
    CHECK(!tx.bad() && !rx.bad());
}

/* 3. the park/doorbell handshake over many handoffs: a token goes back
 * and forth through the two rings, each side sleeping whenever it finds
 * nothing */
void caseHandoffs(int handoffs) {
    Pair pr;
    CHECK(pr.make(4096));
    if (g_failures) return;
    std::atomic<bool> lost{false};
    const int rounds = handoffs / 2;

    auto side = [&](bool first) {
        shm::Region& r = first ? pr.a : pr.b;
        int mine = first ? pr.bellToA : pr.bellToB;
        int theirs = first ? pr.bellToB : pr.bellToA;
        shm::Producer tx;
        shm::Consumer rx;
        tx.attach(r.ctl(first ? 0 : 1), r.data(first ? 0 : 1), r.cap());
        rx.attach(r.ctl(first ? 1 : 0), r.data(first ? 1 : 0), r.cap());
        uint64_t token = 0;
        for (int i = 0; i < rounds && !lost; ++i) {
            if (first) {
                token = (uint64_t)i;
                CHECK(tx.write(&token, sizeof(token)) == sizeof(token));
                if (tx.consumerNeedsWake()) shm::ringDoorbell(theirs);
            }
            uint64_t got = 0;
            size_t have = 0;
            while (have < sizeof(got) && !lost) {
                size_t n = rx.read((uint8_t*)&got + have,
                                   sizeof(got) - have);
                have += n;
                if (n == 0 && rx.park() && !waitBell(mine)) lost = true;
            }
            if (lost) break;
            CHECK(got == (uint64_t)i);
            if (!first) {
                CHECK(tx.write(&got, sizeof(got)) == sizeof(got));
                if (tx.consumerNeedsWake()) shm::ringDoorbell(theirs);
            }
        }
        CHECK(!tx.bad() && !rx.bad());
    };
    std::thread a(side, true), b(side, false);
    a.join();
    b.join();
    CHECK(!lost);
}

/* 3b. a doorbell rung late (shmpipe.hpp, "every way into sleep"): the
 * producer publishes, is held up before it looks at the parked flag,
 * and the consumer - awake for another reason - takes the data and
 * parks again in between. The late ring clears the shared flag behind
 * the consumer's back; the park that follows must set it again, or the
 * next write rings nobody. One thread, the interleaving spelled out. */
void caseLateDoorbell() {
    constexpr size_t kCap = 4096;
    auto ctl = std::make_unique<shm::RingCtl>();
    ctl->tail = 0;
    ctl->head = 0;
    ctl->consumerParked = 0;
    ctl->producerWaiting = 0;
    std::vector<uint8_t> data(kCap);
    shm::Producer tx;
    shm::Consumer rx;
    tx.attach(ctl.get(), data.data(), kCap);
    rx.attach(ctl.get(), data.data(), kCap);
    uint8_t d[64] = {1}, got[64];

    CHECK(rx.park());                           /* 1. consumer sleeps */
    CHECK(tx.write(d, sizeof(d)) == sizeof(d)); /* 2. D1 published... */
    /*    ...and the producer is descheduled before consumerNeedsWake() */
    CHECK(rx.read(got, sizeof(got)) == sizeof(got)); /* 3. polled, taken */
    CHECK(rx.park());                           /* 4. idle: parks again */
    CHECK(ctl->consumerParked.load() == 1);
    CHECK(tx.consumerNeedsWake());              /* 5. late: rings, clears */
    CHECK(ctl->consumerParked.load() == 0);
    CHECK(rx.read(got, sizeof(got)) == 0);      /* 6. woken for nothing */
    CHECK(rx.park());                           /*    back to sleep */
    CHECK(ctl->consumerParked.load() == 1);     /*    and says so again */
    CHECK(tx.write(d, sizeof(d)) == sizeof(d)); /* 7. D2 */
    CHECK(tx.consumerNeedsWake());              /*    must ring */
    CHECK(rx.read(got, sizeof(got)) == sizeof(got));

    /* the same the other way round: room announced late */
    std::vector<uint8_t> fill(kCap);
    CHECK(tx.write(fill.data(), kCap) == kCap);
    CHECK(tx.write(d, 1) == 0 && tx.waitForSpace());   /* producer waits */
    CHECK(rx.read(fill.data(), 100) == 100);           /* room, no look yet */
    CHECK(tx.write(fill.data(), 100) == 100);          /* producer polled */
    CHECK(tx.write(d, 1) == 0 && tx.waitForSpace());   /* full, waits again */
    CHECK(rx.producerNeedsWake());                     /* late: clears */
    CHECK(ctl->producerWaiting.load() == 0);
    CHECK(tx.write(d, 1) == 0 && tx.waitForSpace());   /* woken for nothing */
    CHECK(ctl->producerWaiting.load() == 1);           /* says so again */
    CHECK(rx.read(fill.data(), 100) == 100);
    CHECK(rx.producerNeedsWake());                     /* must ring */
    CHECK(!tx.bad() && !rx.bad());
}

/* 4. a peer that scribbles on the control block: reported as bad, and
 * (heap blocks of exactly the ring's size, under ASan) nothing outside
 * the data area is read or written */
void caseCorrupt(unsigned seed) {
    constexpr size_t kCap = 4096;
    std::mt19937_64 rng(seed);
    std::vector<uint8_t> buf(3 * kCap);
    struct Wild {
        uint64_t head, tail;
    };
    std::vector<Wild> wild = {
        {100, 50},                     /* tail behind head */
        {0, kCap + 1},                 /* more than the ring holds */
        {0, ~0ull},
        {~0ull, 0},
        {1ull << 63, (1ull << 63) - 1},
    };
    for (int i = 0; i < 200; ++i) wild.push_back({rng(), rng()});

    for (const Wild& w : wild) {
        /* consumer against a hostile producer index */
        {
            auto ctl = std::make_unique<shm::RingCtl>();
            ctl->tail = 0;
            ctl->head = 0;
            ctl->consumerParked = 0;
            ctl->producerWaiting = 0;
            std::vector<uint8_t> data(kCap);
            shm::Consumer rx;
            rx.attach(ctl.get(), data.data(), kCap);
            ctl->tail.store(w.tail);
            size_t n = rx.read(buf.data(), buf.size());
            if (w.tail <= kCap) {
                CHECK(n == w.tail && !rx.bad());
                /* then a step backwards */
                if (w.tail > 0) {
                    ctl->tail.store(w.tail - 1);
                    CHECK(rx.read(buf.data(), buf.size()) == 0);
                    CHECK(rx.bad());
                }
            } else {
                CHECK(n == 0 && rx.bad());
                CHECK(!rx.park());  /* a bad ring never sleeps on it */
            }
            /* bad is for good */
            if (rx.bad()) {
                ctl->tail.store(0);
                CHECK(rx.read(buf.data(), buf.size()) == 0 && rx.bad());
            }
        }
        /* producer against a hostile consumer index */
        {
            auto ctl = std::make_unique<shm::RingCtl>();
            ctl->tail = 0;
            ctl->head = 0;
            ctl->consumerParked = 0;
            ctl->producerWaiting = 0;
            std::vector<uint8_t> data(kCap);
            shm::Producer tx;
            tx.attach(ctl.get(), data.data(), kCap);
            CHECK(tx.write(buf.data(), 1000) == 1000);  /* tail = 1000 */
            ctl->head.store(w.head);
            size_t n = tx.write(buf.data(), buf.size());
            if (w.head <= 1000) {
                CHECK(n == kCap - (1000 - w.head) && !tx.bad());
            } else {
                CHECK(n == 0 && tx.bad());
                CHECK(!tx.waitForSpace());
            }
        }
    }

    /* geometry the accepting side must refuse */
    shm::Region good, r;
    int fd = good.create(8192);
    CHECK(fd >= 0);
    CHECK(r.attach(fd, 8192));
    CHECK(!r.attach(fd, 4096));    /* not what the fd holds */
    CHECK(!r.attach(fd, 16384));
    CHECK(!r.attach(fd, 5000));    /* not a power of two */
    CHECK(!r.attach(fd, 0));
    CHECK(ftruncate(fd, 4096) != 0);  /* sealed against shrinking */
    close(fd);
    int plain = memfd_create("unsealed", MFD_CLOEXEC);
    CHECK(plain >= 0);
    CHECK(ftruncate(plain, (off_t)shm::regionBytes(4096)) == 0);
    CHECK(!r.attach(plain, 4096));  /* could be truncated under us */
    close(plain);
    CHECK(good.create(100) < 0);
}

}  // namespace

int main(int argc, char** argv) {
    unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    int handoffs = argc > 2 ? atoi(argv[2]) : 100000;
    caseFull();
    caseLateDoorbell();
    caseCorrupt(seed);
    caseStream(seed);
    caseHandoffs(handoffs);
    if (g_failures != 0) {
        fprintf(stderr, "shmpipe_check: %d failure(s)\n",
                g_failures.load());
        return 1;
    }
    printf("shmpipe_check OK (seed %u, %d handoffs)\n", seed, handoffs);
    return 0;
}
