/*
 * Stand-alone check of bsocklink.hpp, meant to be built with
 * -fsanitize=address,undefined (`make check-bsocklink`). Two endpoints
 * of this program face each other over a socketpair and a real memfd
 * region with the smallest rings (4 KiB: they wrap and fill within a
 * few frames), with recording sinks. One thread: the cases step the
 * sender and the receiver in turn, so every state in between can be
 * looked at, and a bounded number of steps stands in for every wait.
 *
 *   bsocklink_check [seed]
 */
#include <sys/eventfd.h>
#include <sys/ioctl.h>
#include <sys/socket.h>

#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "bsocklink.hpp"

using namespace bamd;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,    \
                    #cond);                                            \
            g_failures++;                                              \
        }                                                              \
    } while (0)

using Flush = BsockLink::Flush;
enum class Park { NoRings, Idle, Work };
constexpr size_t kCap = shm::kMinRing;

struct RecSink {
    int armed = 0, disarmed = 0, bells = 0, drains = 0;
    void armWrite() { armed++; }
    void disarmWrite() { disarmed++; }
    void doorbell() { bells++; }
    void drained() { drains++; }
};

/* the balancer's end (a) and binderd's (b) of one connection */
struct Wire {
    BsockLink a, b;
    RecSink sa, sb;
    explicit Wire(bool rings = true) {
        int sv[2] = {-1, -1};
        CHECK(socketpair(AF_UNIX, SOCK_STREAM | SOCK_NONBLOCK | SOCK_CLOEXEC,
                         0, sv) == 0);
        a.fd = sv[0];
        b.fd = sv[1];
        if (!rings) return;
        int fd = a.shm.region.create(kCap);
        CHECK(fd >= 0 && b.shm.region.attach(fd, kCap));
        close(fd);
        a.shm.wakeMe = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        b.shm.wakeMe = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
        a.shm.wakePeer = dup(b.shm.wakeMe);
        b.shm.wakePeer = dup(a.shm.wakeMe);
        CHECK(a.shm.wakePeer >= 0 && b.shm.wakePeer >= 0);
        a.shm.attachEnds(true);
        b.shm.attachEnds(false);
        a.shmReady = b.shmReady = true;
    }
    ~Wire() {
        close(a.fd);
        close(b.fd);
    }
};

/* take the count off a doorbell; false = it had not been rung */
bool takeBell(int efd) {
    uint64_t v = 0;
    return read(efd, &v, sizeof(v)) == (ssize_t)sizeof(v) && v != 0;
}

/* One direction of a connection. queue() puts numbered frames of random
 * sizes into the sender's `out` and keeps a copy of every byte; step()
 * is one flush and one receive, the receiver parsing frames the way the
 * daemons do: from the stream until it sees `ctl`, from the ring after
 * that. */
struct Pump {
    BsockLink& tx;
    RecSink& txRec;
    BsockLink& rx;
    RecSink& rxRec;
    uint8_t ctl;
    size_t quota, chunk;  /* the receiver's, per step */
    std::mt19937 rng;

    std::string queued, seen;
    uint32_t nextNo = 0;
    size_t ctlEnd = 0;     /* of the control frame, in `queued` */
    size_t sockBytes = 0;  /* the receiver read from the socket */
    size_t ringBytes = 0;
    bool compacted = false;  /* ...with the control frame still queued */
    Flush last = Flush::Ok;

    Pump(BsockLink& t, RecSink& tr, BsockLink& r, RecSink& rr, uint8_t c,
         size_t q, size_t ch, unsigned seed)
        : tx(t), txRec(tr), rx(r), rxRec(rr), ctl(c), quota(q), chunk(ch),
          rng(seed) {}

    void queue(size_t bytes, size_t maxPayload = 3000) {
        size_t until = queued.size() + bytes;
        while (queued.size() < until) {
            std::string p(4 + rng() % maxPayload, (char)nextNo);
            memcpy(p.data(), &nextNo, 4);
            nextNo++;
            size_t at = tx.out.size();
            bsock::appendFrame(tx.out, bsock::FRAME_QUERY, p);
            queued.append(tx.out, at);
        }
    }
    void queueSwitch() {
        tx.queueSwitch(ctl);
        queued.append(tx.out, tx.out.size() - bsock::kHeaderLen);
        ctlEnd = queued.size();
    }

    void flush() {
        bool wasShm = tx.txShm;
        size_t outSize = tx.out.size();
        last = tx.flush(txRec);
        CHECK(last == Flush::Ok || last == Flush::Blocked);
        CHECK((last == Flush::Blocked) == tx.writeBlocked);
        /* EPOLLOUT is armed exactly while the stream is what blocks */
        CHECK(txRec.armed - txRec.disarmed ==
              (tx.writeBlocked && !tx.txShm ? 1 : 0));
        if (tx.streamEnd != 0 && tx.out.size() < outSize) compacted = true;
        if (tx.txShm && !wasShm) {
            /* the switch: every stream byte has left, the control frame
             * the last of them, and no byte more */
            int inFlight = 0;
            CHECK(ioctl(rx.fd, FIONREAD, &inFlight) == 0);
            CHECK(ctlEnd != 0 && sockBytes + (size_t)inFlight == ctlEnd);
            CHECK(tx.streamEnd == 0);
        }
        if (last == Flush::Ok) CHECK(tx.out.empty() && tx.outOff == 0);
    }

    void receive() {
        if (!rx.rxShm) {
            ssize_t nr = read(rx.fd, rx.in.tail(quota), quota);
            if (nr > 0) {
                rx.in.commit((size_t)nr);
                sockBytes += (size_t)nr;
            } else {
                CHECK(nr < 0 && errno == EAGAIN);
            }
        } else {
            /* nothing may follow the control frame on the socket */
            CHECK(rx.streamStillOpen());
            int bells = rxRec.bells;
            bool waiting = tx.bellWantsFlush();
            size_t n = rx.drainRing(quota, chunk, rxRec);
            CHECK(n != BsockLink::kRingBad && n < quota + chunk);
            if (n == BsockLink::kRingBad) return;
            ringBytes += n;
            if (rxRec.bells != bells) {
                /* the sender had said it waits, and now finds the bell */
                CHECK(rxRec.bells == bells + 1 && n != 0 && waiting);
                CHECK(takeBell(tx.shm.wakeMe));
            }
        }
        bsock::FrameView f;
        bsock::FrameStatus st;
        while ((st = bsock::nextFrame(rx.in, f)) == bsock::FrameStatus::Ok) {
            seen.append((const char*)f.payload - bsock::kHeaderLen,
                        bsock::kHeaderLen + f.plen);
            if (f.type != ctl) continue;
            CHECK(!rx.rxShm);
            rx.rxShm = true;
            /* no partial frame behind it */
            CHECK(rx.in.size() == 0);
        }
        CHECK(st == bsock::FrameStatus::NeedMore);
        rx.in.compact();
    }

    /* until every queued byte has been seen */
    void run() {
        for (int i = 0; i < 200000 && seen.size() < queued.size(); ++i) {
            flush();
            receive();
        }
        flush();  /* the sender learns that all of it has left */
        CHECK(seen == queued);
        CHECK(last == Flush::Ok && txRec.armed == txRec.disarmed);
        if (ctlEnd == 0) return;
        CHECK(tx.txShm && rx.rxShm && sockBytes == ctlEnd);
        CHECK(sockBytes + ringBytes == queued.size());
        CHECK(rx.streamStillOpen());
    }
};

/* 1. order across the switch, both directions; the balancer takes its
 * ring in small chunks, binderd in one piece */
void caseOrder(unsigned seed) {
    Wire w;
    Pump go(w.a, w.sa, w.b, w.sb, bsock::FRAME_SHM_GO, 128 << 10, 128 << 10,
            seed);
    Pump ok(w.b, w.sb, w.a, w.sa, bsock::FRAME_SHM_OK, 3000, 1000,
            seed + 1);
    for (Pump* p : {&ok, &go}) {
        p->queue(20000);
        p->queueSwitch();
        p->queue(10 * kCap);  /* wraps the ring ten times */
        p->run();
        CHECK(p->rxRec.drains > 10);
        /* and more of it once both sides are on the ring */
        p->queue(3 * kCap);
        p->run();
    }
    CHECK(w.a.parkState<Park>(false) == Park::Idle);
}

/* 2. a slow reader behind a small send buffer, more than the
 * compaction threshold queued ahead of the control frame */
void caseStreamPressure(unsigned seed) {
    Wire w;
    int sz = 4096;
    CHECK(setsockopt(w.a.fd, SOL_SOCKET, SO_SNDBUF, &sz, sizeof(sz)) == 0);
    Pump p(w.a, w.sa, w.b, w.sb, bsock::FRAME_SHM_GO, 16000, 16000, seed);
    p.queue(BsockLink::kCompactAt + (256 << 10), 60000);
    p.queueSwitch();
    p.queue(4 * kCap);
    p.flush();
    CHECK(p.last == Flush::Blocked && !w.a.txShm && w.sa.armed == 1);
    p.run();
    CHECK(p.compacted);
    CHECK(w.sa.armed >= 1 && w.sa.armed == w.sa.disarmed);
}

/* 3. a full ring: blocked, one doorbell from the consumer, resumed; and
 * the doorbell the other way, for a consumer that said it sleeps */
void caseRingPressure(unsigned seed) {
    Wire w;
    Pump p(w.a, w.sa, w.b, w.sb, bsock::FRAME_SHM_GO, 128 << 10, 128 << 10,
           seed);
    CHECK(w.b.parkState<Park>(false) == Park::NoRings);
    p.queue(100);
    p.queueSwitch();
    p.run();
    CHECK(w.b.parkState<Park>(false) == Park::Idle);

    p.queue(5 * kCap);
    p.flush();
    CHECK(p.last == Flush::Blocked && w.a.writeBlocked);
    CHECK(w.a.bellWantsFlush() && w.sa.armed == 0);
    CHECK(w.a.outOff == kCap);  /* the ring is full */
    CHECK(w.b.parkState<Park>(false) == Park::Work);
    CHECK(w.b.parkState<Park>(true) == Park::Work);  /* must not sleep */
    int bells = w.sb.bells;
    p.receive();
    CHECK(w.sb.bells == bells + 1);
    p.flush();
    CHECK(w.a.outOff == 2 * kCap);  /* it went on */
    p.run();
    CHECK(w.sb.bells > bells + 1);

    /* an idle consumer parks; the next flush rings it, once */
    CHECK(w.b.parkState<Park>(true) == Park::Idle);
    bells = w.sa.bells;
    p.queue(100);
    p.flush();
    CHECK(w.sa.bells == bells + 1 && takeBell(w.b.shm.wakeMe));
    p.queue(100);
    p.flush();
    CHECK(w.sa.bells == bells + 1 && !takeBell(w.b.shm.wakeMe));
    p.run();
}

/* 4. impossible indices written by "the peer" (the cases of
 * shmpipe_check): reported, nothing copied */
void caseHostile(unsigned seed) {
    std::mt19937_64 rng(seed);
    struct Wild {
        uint64_t head, tail;
    };
    std::vector<Wild> wild = {
        {100, 50},
        {0, kCap + 1},
        {0, ~0ull},
        {~0ull, 0},
        {1ull << 63, (1ull << 63) - 1},
    };
    for (int i = 0; i < 20; ++i)
        wild.push_back({rng() | (1ull << 40), rng() | (1ull << 40)});
    for (const Wild& x : wild) {
        Wire w;
        Pump p(w.a, w.sa, w.b, w.sb, bsock::FRAME_SHM_GO, 128 << 10,
               128 << 10, seed);
        p.queue(100);
        p.queueSwitch();
        /* both indices of the query ring end up past 2 * kCap + 100, so
         * every value above is out of the question for either side */
        p.queue(2 * kCap + 100, 500);
        p.run();
        shm::RingCtl* ring = w.a.shm.region.ctl(0);

        /* binderd's view: the balancer stores a wild tail */
        uint64_t tail = ring->tail.load();
        ring->tail.store(x.tail);
        size_t had = w.b.in.size();
        CHECK(w.b.parkState<Park>(false) == Park::Work);
        CHECK(w.b.drainRing(128 << 10, 128 << 10, w.sb) ==
              BsockLink::kRingBad);
        CHECK(w.b.in.size() == had);
        CHECK(w.b.parkState<Park>(true) == Park::Work);
        ring->tail.store(tail);
        CHECK(w.b.drainRing(128 << 10, 128 << 10, w.sb) ==
              BsockLink::kRingBad);  /* bad is for good */

        /* the balancer's view: binderd stores a wild head */
        ring->head.store(x.head);
        p.queue(100);
        size_t left = w.a.out.size() - w.a.outOff;
        int bells = w.sa.bells;
        CHECK(w.a.flush(w.sa) == Flush::RingBad);
        CHECK(w.a.out.size() - w.a.outOff == left && w.sa.bells == bells);
        CHECK(ring->tail.load() == tail);
    }
}

/* 5. after the switch the socket may only show its end */
void caseStreamAfterSwitch() {
    for (bool closes : {false, true}) {
        Wire w;
        w.b.rxShm = true;
        CHECK(w.b.streamStillOpen());
        CHECK(w.b.streamStillOpen());
        if (closes) {
            CHECK(shutdown(w.a.fd, SHUT_WR) == 0);
        } else {
            CHECK(write(w.a.fd, "x", 1) == 1);
        }
        CHECK(!w.b.streamStillOpen());
    }
}

/* 6. an offer that is never answered: a plain stream, blocked and
 * resumed, `out` given back when all of it is written */
void caseNoSwitch(unsigned seed) {
    for (bool rings : {false, true}) {
        Wire w(rings);
        int sz = 4096;
        CHECK(setsockopt(w.a.fd, SOL_SOCKET, SO_SNDBUF, &sz, sizeof(sz)) ==
              0);
        Pump p(w.a, w.sa, w.b, w.sb, bsock::FRAME_SHM_GO, 16000, 16000,
               seed);
        CHECK(w.a.flush(w.sa) == Flush::Ok);  /* nothing to do */
        p.queue(300000);
        p.run();
        CHECK(!w.a.txShm && !w.b.rxShm && w.sa.armed >= 1);
        CHECK(w.a.out.empty() && w.a.outOff == 0 && w.a.streamEnd == 0);
        CHECK(p.sockBytes == p.queued.size() && w.sa.bells == 0);
        CHECK(w.a.parkState<Park>(false) == Park::NoRings);
        /* a peer that went away is an error of the stream */
        close(w.b.fd);
        w.b.fd = -1;
        p.queue(100);
        CHECK(w.a.flush(w.sa) == Flush::StreamError);
    }
}

}  // namespace

int main(int argc, char** argv) {
    unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    signal(SIGPIPE, SIG_IGN);
    caseOrder(seed);
    caseStreamPressure(seed);
    caseRingPressure(seed);
    caseHostile(seed);
    caseStreamAfterSwitch();
    caseNoSwitch(seed);
    if (g_failures != 0) {
        fprintf(stderr, "bsocklink_check: %d failure(s)\n", g_failures);
        return 1;
    }
    printf("bsocklink_check OK (seed %u)\n", seed);
    return 0;
}
