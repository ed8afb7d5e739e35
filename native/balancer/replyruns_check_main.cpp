/*
 * replyruns_check: stand-alone exerciser for balancer/replyruns.hpp,
 * meant to be built with -fsanitize=address,undefined and run on the
 * CPU (`make check-replyruns`). No sockets: the sink records.
 *
 * Seeded reply sequences are fed through ReplyRuns; the sink checks
 * every run as it arrives (one destination, equal lengths except an
 * optional shorter last segment, at most 48 segments and 60000 bytes)
 * and every reply's bytes and destination, and counts emissions. After
 * finish() every reply must have left exactly once and nothing may be
 * pending. Fixed cases: one destination and size; 8 destinations x 4
 * sizes interleaved; more keys than table entries; v4 and v6 mixed;
 * 1300-byte replies (byte cap); zero-length payloads. Each also runs
 * with a sink that fails some runs (resend one by one) and with one
 * that reports EINVAL (no run may follow). Then random rounds.
 *
 * usage: replyruns_check [seed] [random-rounds]
 */
#include <arpa/inet.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "replyruns.hpp"

using namespace bamd;

namespace {

unsigned gSeed = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "replyruns_check: %s:%d: %s failed "        \
                    "(seed %u)\n", __FILE__, __LINE__, #cond, gSeed);   \
            exit(1);                                                    \
        }                                                               \
    } while (0)

struct Dest {
    uint8_t family;  /* 4 or 6 */
    uint8_t addr[16];
    uint16_t port;
};

struct Reply {
    Dest dst;
    size_t off;  /* into the arena */
    size_t len;
    int emitted = 0;
};

enum class Fail { None, Some, Einval };

struct Recorder {
    std::vector<Reply>* replies = nullptr;
    const std::vector<uint8_t>* arena = nullptr;    /* what add() saw */
    const std::vector<uint8_t>* pristine = nullptr; /* untouched copy */
    const std::vector<int>* byOff = nullptr;  /* arena offset -> reply */
    Fail fail = Fail::None;
    unsigned runCalls = 0, runsOk = 0, runSegs = 0, singles = 0;
    bool sawEinval = false;
    size_t longestRun = 0;

    Reply& lookup(const struct iovec& iov) {
        const uint8_t* p = (const uint8_t*)iov.iov_base;
        CHECK(p >= arena->data() && p < arena->data() + arena->size());
        size_t off = (size_t)(p - arena->data());
        /* every reply owns at least one arena byte, so its offset
         * names it even when it is empty */
        CHECK((*byOff)[off] >= 0);
        Reply& r = (*replies)[(size_t)(*byOff)[off]];
        CHECK(r.len == iov.iov_len);
        CHECK(memcmp(p, pristine->data() + off, r.len) == 0);
        return r;
    }

    static void checkDest(const Reply& r, const struct sockaddr* sa,
                          socklen_t len) {
        if (r.dst.family == 4) {
            CHECK(len == sizeof(struct sockaddr_in));
            auto* s4 = (const struct sockaddr_in*)sa;
            CHECK(s4->sin_family == AF_INET);
            CHECK(ntohs(s4->sin_port) == r.dst.port);
            CHECK(memcmp(&s4->sin_addr, r.dst.addr, 4) == 0);
        } else {
            CHECK(len == sizeof(struct sockaddr_in6));
            auto* s6 = (const struct sockaddr_in6*)sa;
            CHECK(s6->sin6_family == AF_INET6);
            CHECK(ntohs(s6->sin6_port) == r.dst.port);
            CHECK(memcmp(&s6->sin6_addr, r.dst.addr, 16) == 0);
            CHECK(s6->sin6_scope_id == 0 && s6->sin6_flowinfo == 0);
        }
    }

    int sendRun(const struct sockaddr* sa, socklen_t salen,
                struct iovec* iov, size_t n, uint16_t seg) {
        CHECK(!sawEinval);  /* runs are off for good after EINVAL */
        runCalls++;
        CHECK(n >= 2 && n <= 48);
        CHECK(seg > 0);
        size_t bytes = 0;
        for (size_t k = 0; k < n; ++k) {
            Reply& r = lookup(iov[k]);
            checkDest(r, sa, salen);
            if (k + 1 < n)
                CHECK(iov[k].iov_len == seg);
            else
                CHECK(iov[k].iov_len <= seg && iov[k].iov_len > 0);
            bytes += iov[k].iov_len;
        }
        CHECK(bytes <= 60000);
        if (fail == Fail::Einval && runCalls == 3) {
            sawEinval = true;
            return EINVAL;
        }
        if (fail == Fail::Some && runCalls % 3 == 0) return EMSGSIZE;
        for (size_t k = 0; k < n; ++k) lookup(iov[k]).emitted++;
        runsOk++;
        runSegs += (unsigned)n;
        if (n > longestRun) longestRun = n;
        return 0;
    }

    void sendOne(const struct sockaddr* sa, socklen_t salen,
                 struct iovec* iov) {
        Reply& r = lookup(*iov);
        checkDest(r, sa, salen);
        r.emitted++;
        singles++;
    }

    void sendBatch(struct mmsghdr* hdrs, unsigned n) {
        CHECK(n >= 1 && n <= 128);
        for (unsigned i = 0; i < n; ++i) {
            const struct msghdr& mh = hdrs[i].msg_hdr;
            CHECK(mh.msg_iovlen == 1);
            CHECK(mh.msg_control == nullptr && mh.msg_controllen == 0);
            Reply& r = lookup(mh.msg_iov[0]);
            checkDest(r, (const struct sockaddr*)mh.msg_name,
                      mh.msg_namelen);
            r.emitted++;
            singles++;
        }
    }
};

Dest makeDest(unsigned i, bool v6) {
    Dest d{};
    d.port = (uint16_t)(20000 + i * 7);
    if (v6) {
        d.family = 6;
        d.addr[0] = 0xfd;
        d.addr[15] = (uint8_t)(1 + i);
        d.addr[7] = (uint8_t)(i >> 3);
    } else {
        d.family = 4;
        d.addr[0] = 127;
        d.addr[2] = (uint8_t)(i >> 6);
        d.addr[3] = (uint8_t)(1 + i % 64);
        /* the balancer's pending slots leave bytes 4..15 of a v4
         * address stale: they must not take part in the key */
        for (int k = 4; k < 16; ++k) d.addr[k] = (uint8_t)rand();
    }
    return d;
}

struct Outcome {
    unsigned runsOk, runSegs, singles;
    size_t longestRun;
};

/* feed `seq` (destination, length) in order, in events of eventLen
 * replies (0 = one event), and check the books */
Outcome play(const std::vector<std::pair<Dest, size_t>>& seq, Fail fail,
             size_t eventLen = 0) {
    std::vector<Reply> replies;
    size_t total = 0;
    for (auto& [d, len] : seq) {
        Reply r;
        r.dst = d;
        r.off = total;
        r.len = len;
        total += len > 0 ? len : 1;
        replies.push_back(r);
    }
    std::vector<uint8_t> arena(total + 1);
    std::mt19937 rng(gSeed ^ (unsigned)seq.size());
    for (auto& b : arena) b = (uint8_t)rng();
    std::vector<uint8_t> pristine = arena;
    std::vector<int> byOff(arena.size(), -1);
    for (size_t k = 0; k < replies.size(); ++k)
        byOff[replies[k].off] = (int)k;

    Recorder rec;
    rec.replies = &replies;
    rec.arena = &arena;
    rec.pristine = &pristine;
    rec.byOff = &byOff;
    rec.fail = fail;
    auto runs = std::make_unique<ReplyRuns<Recorder>>(rec);
    size_t inEvent = 0;
    for (Reply& r : replies) {
        struct iovec iov = {arena.data() + r.off, r.len};
        /* a v4 caller passes 4 meaningful bytes */
        runs->add(r.dst.family, r.dst.addr, r.dst.port, iov);
        if (eventLen != 0 && ++inEvent == eventLen) {
            runs->finish();
            CHECK(runs->pending() == 0);
            inEvent = 0;
        }
    }
    runs->finish();
    CHECK(runs->pending() == 0);
    for (const Reply& r : replies) CHECK(r.emitted == 1);
    CHECK(rec.runSegs + rec.singles == replies.size());
    CHECK(runs->runs() == rec.runsOk);
    CHECK(runs->runSegments() == rec.runSegs);
    CHECK(runs->singles() == rec.singles);
    if (fail == Fail::Einval && rec.sawEinval) CHECK(!runs->gso());
    /* a second finish has nothing left to send */
    unsigned before = rec.runCalls + rec.singles;
    runs->finish();
    CHECK(rec.runCalls + rec.singles == before);
    return {rec.runsOk, rec.runSegs, rec.singles, rec.longestRun};
}

void fixedCases() {
    using Seq = std::vector<std::pair<Dest, size_t>>;
    const Fail modes[] = {Fail::None, Fail::Some, Fail::Einval};

    /* 1 destination x 1 size x 200 replies: 4 runs of 48 and one of 8 */
    {
        Seq s;
        Dest d = makeDest(0, false);
        for (int i = 0; i < 200; ++i) s.push_back({d, 90});
        for (Fail f : modes) {
            Outcome o = play(s, f);
            if (f == Fail::None) {
                CHECK(o.runsOk == 5 && o.runSegs == 200);
                CHECK(o.singles == 0 && o.longestRun == 48);
            }
        }
    }
    /* 8 destinations x 4 sizes interleaved: 32 keys, all fit */
    {
        Seq s;
        const size_t sizes[4] = {60, 61, 75, 140};
        for (int i = 0; i < 640; ++i)
            s.push_back({makeDest((unsigned)i % 8, false),
                         sizes[(i / 8) % 4]});
        for (Fail f : modes) {
            Outcome o = play(s, f);
            if (f == Fail::None) CHECK(o.singles == 0);
            play(s, f, 37);  /* events that cut runs short */
        }
    }
    /* more distinct keys than table entries: 40 destinations x 5 sizes */
    {
        Seq s;
        for (int round = 0; round < 6; ++round)
            for (unsigned d = 0; d < 40; ++d)
                for (size_t k = 0; k < 5; ++k)
                    s.push_back({makeDest(d, false), 50 + 11 * k});
        CHECK(200 > ReplyRuns<Recorder>::kRuns);
        for (Fail f : modes) play(s, f);
    }
    /* v4 and v6 mixed, same ports, same sizes */
    {
        Seq s;
        for (int i = 0; i < 300; ++i)
            s.push_back({makeDest((unsigned)i % 3, i % 2 == 0),
                         (size_t)(70 + (i % 5 == 0 ? 9 : 0))});
        for (Fail f : modes) {
            play(s, f);
            play(s, f, 50);
        }
    }
    /* 1300 bytes: the byte cap closes a run at 46 segments */
    {
        Seq s;
        Dest d = makeDest(5, true);
        for (int i = 0; i < 100; ++i) s.push_back({d, 1300});
        for (Fail f : modes) {
            Outcome o = play(s, f);
            if (f == Fail::None) {
                CHECK(o.longestRun == 46);
                CHECK(o.runsOk == 3 && o.singles == 0);
            }
        }
    }
    /* zero-length payloads never join a run, and do not disturb one */
    {
        Seq s;
        Dest d = makeDest(1, false);
        for (int i = 0; i < 40; ++i)
            s.push_back({d, i % 4 == 0 ? (size_t)0 : (size_t)33});
        for (Fail f : modes) {
            Outcome o = play(s, f);
            if (f == Fail::None)
                CHECK(o.singles == 10 && o.runSegs == 30);
        }
    }
    /* the trailing-segment rule: a lone shorter reply closes the run */
    {
        Seq s;
        Dest d = makeDest(2, false);
        for (int i = 0; i < 10; ++i) s.push_back({d, 80});
        s.push_back({d, 64});
        Outcome o = play(s, Fail::None);
        CHECK(o.runsOk == 1 && o.runSegs == 11 && o.singles == 0);
    }
    /* sizes past half the byte cap travel alone */
    {
        Seq s;
        Dest d = makeDest(3, false);
        for (int i = 0; i < 5; ++i) s.push_back({d, 30001});
        Outcome o = play(s, Fail::None);
        CHECK(o.runsOk == 0 && o.singles == 5);
    }
}

void randomRounds(unsigned rounds) {
    std::mt19937 rng(gSeed);
    for (unsigned r = 0; r < rounds; ++r) {
        unsigned nDest = 1 + rng() % 90;
        unsigned nSize = 1 + rng() % 9;
        std::vector<size_t> sizes;
        for (unsigned k = 0; k < nSize; ++k) {
            unsigned pick = rng() % 10;
            sizes.push_back(pick == 0 ? 0
                            : pick == 1 ? 1200 + rng() % 400
                            : pick == 2 ? 29990 + rng() % 20
                                        : 1 + rng() % 300);
        }
        size_t n = 1 + rng() % 1500;
        std::vector<std::pair<Dest, size_t>> s;
        for (size_t i = 0; i < n; ++i) {
            unsigned d = rng() % nDest;
            s.push_back({makeDest(d, d % 3 == 0),
                         sizes[rng() % nSize]});
        }
        Fail f = (Fail)(rng() % 3);
        size_t ev = rng() % 2 ? 0 : 1 + rng() % 400;
        play(s, f, ev);
    }
}

}  // namespace

int main(int argc, char** argv) {
    gSeed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    unsigned rounds = argc > 2 ? (unsigned)atoi(argv[2]) : 200;
    srand(gSeed);
    fixedCases();
    randomRounds(rounds);
    printf("replyruns_check OK (seed %u, %u random rounds)\n", gSeed,
           rounds);
    return 0;
}
