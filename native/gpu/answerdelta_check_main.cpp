/*
 * answerdelta_check: stand-alone exerciser for gpu/answerdelta.hpp,
 * meant to be built with -fsanitize=address,undefined and run on the
 * CPU (`make check-answerdelta`).
 *
 * Each round fills a std::map model of a table, then feeds one seeded
 * random sequence of upserts (wire and service bodies) and
 * invalidations both to an AnswerDelta and, call by call, to a copy of
 * the model. The delta's packed normal form is then applied the way
 * the device does - every invalidation first, every upsert after, each
 * phase in reverse order to show that order inside a phase is free -
 * and must leave the same map. Every packed blob is verified again,
 * every hash recomputed, every offset list checked to ascend. Names
 * come from a small pool so that keys repeat, domains repeat, services
 * share a domain, and one domain is a dotted or a mere string suffix
 * of another.
 */
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "answerdelta.hpp"

using namespace bamd;
using namespace bamd::gpu;

namespace {

unsigned gSeed = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "answerdelta_check: %s:%d: %s failed "      \
                    "(seed %u)\n", __FILE__, __LINE__, #cond, gSeed);   \
            exit(1);                                                    \
        }                                                               \
    } while (0)

/* model: qtype byte + qname -> blob */
using Model = std::map<std::string, std::string>;

std::string randomBytes(std::mt19937& rng, size_t n) {
    std::string b(n, '\0');
    for (char& ch : b) ch = (char)rng();
    return b;
}

std::vector<std::string> makeDomains(std::mt19937& rng) {
    std::vector<std::string> d = {"foo.com", "b.foo.com", "ab.foo.com",
                                  "a.b.foo.com", "com", "x"};
    for (int i = 0; i < 12; ++i)
        d.push_back("h" + std::to_string(rng() % 8) + "." + d[rng() % 4]);
    d.push_back(std::string(247, 'k'));
    d.push_back(std::string(255, 'k'));
    return d;
}

/* applyInvalidate on the model */
void invalidateModel(Model& m, const std::string& dom) {
    m.erase(std::string(1, (char)1) + dom);
    uint64_t h33 = AnswerTable::hashKey(dom.data(), dom.size(), 33);
    for (auto it = m.begin(); it != m.end();) {
        std::string_view key = std::string_view(it->first).substr(1);
        if (it->first[0] == 33 && hashOf(key, 33) == h33 &&
            AnswerDelta::covers(dom, key))
            it = m.erase(it);
        else
            ++it;
    }
}

/* the blob AnswerTable would hold for a wire reply */
std::string wireBlob(const std::string& name, int qtype,
                     const std::string& reply) {
    std::string b(2 + name.size() + answerbody::wireBodyLen(reply.size()),
                  '\0');
    b[0] = (char)name.size();
    b[1] = (char)qtype;
    b.replace(2, name.size(), name);
    answerbody::wireFill((uint8_t*)b.data() + 2 + name.size(),
                         (const uint8_t*)reply.data(), reply.size());
    return b;
}

void oneUpsert(std::mt19937& rng, const std::vector<std::string>& doms,
               AnswerDelta& delta, Model& serial) {
    std::string name = doms[rng() % doms.size()];
    int qtype = 1;
    if (rng() % 2 == 0 && name.size() <= 247) {
        static const char* const svc[] = {"_a._tcp.", "_b._udp."};
        name = svc[rng() % 2] + name;
        qtype = 33;
    }
    std::string mk = std::string(1, (char)qtype) + name;
    if (rng() % 3 != 0) {
        std::string reply = randomBytes(rng, 12 + rng() % 501);
        delta.upsertReply(name, qtype, reply);
        serial[mk] = wireBlob(name, qtype, reply);
        return;
    }
    size_t n = rng() % 65;
    std::string head = randomBytes(rng, 12 + rng() % 20);
    std::vector<std::string> a(n), b(n);
    std::vector<Member> mem;
    for (size_t i = 0; i < n; ++i) {
        a[i] = randomBytes(rng, rng() % 5);
        b[i] = randomBytes(rng, rng() % 3);
        mem.emplace_back(a[i], b[i]);
    }
    delta.upsertService(name, qtype, head, mem);
    /* the body is answerbody's own; the check is on key, length and
     * verifyBlob below */
    serial[mk] = std::string();
}

void round(std::mt19937& rng, size_t ops) {
    std::vector<std::string> doms = makeDomains(rng);
    Model start;
    AnswerDelta fill;
    for (size_t i = 0; i < 40; ++i) oneUpsert(rng, doms, fill, start);
    Model serial = start;
    AnswerDelta delta;
    for (size_t i = 0; i < ops; ++i) {
        if (rng() % 3 == 0) {
            const std::string& d = doms[rng() % doms.size()];
            delta.invalidate(d);
            invalidateModel(serial, d);
        } else {
            oneUpsert(rng, doms, delta, serial);
        }
        if (rng() % 97 == 0) {  /* clear() forgets, the table does not */
            delta.clear();
            CHECK(delta.size() == 0);
            start = serial;
        }
    }

    AnswerDelta::Packed p = delta.pack();
    size_t ni = p.ioff.size() - 1, nu = p.uoff.size() - 1;
    CHECK(ni == delta.invalidations() && nu == delta.upserts());
    CHECK(ni + nu == delta.size());
    CHECK(p.ihash.size() == 2 * ni && p.uhash.size() == nu);
    CHECK(p.ioff[0] == 0 && (size_t)p.ioff[ni] == p.ibuf.size());
    CHECK(p.uoff[0] == 0 && (size_t)p.uoff[nu] == p.ubuf.size());

    Model phased = start;
    for (size_t i = ni; i-- > 0;) {
        CHECK(p.ioff[i] < p.ioff[i + 1]);
        std::string d = p.ibuf.substr(p.ioff[i], p.ioff[i + 1] - p.ioff[i]);
        CHECK(p.ihash[2 * i] == AnswerTable::hashKey(d.data(), d.size(), 1));
        CHECK(p.ihash[2 * i + 1] ==
              AnswerTable::hashKey(d.data(), d.size(), 33));
        invalidateModel(phased, d);
    }
    for (size_t i = nu; i-- > 0;) {
        CHECK(p.uoff[i] < p.uoff[i + 1]);
        std::string blob =
            p.ubuf.substr(p.uoff[i], p.uoff[i + 1] - p.uoff[i]);
        /* an exact-size heap copy: a read past the blob is a report */
        std::vector<uint8_t> exact(blob.begin(), blob.end());
        verifyBlob(exact.data(), exact.size(), kMaxReply);
        size_t klen = exact[0];
        std::string name = blob.substr(2, klen);
        CHECK(p.uhash[i] == hashOf(name, exact[1]));
        std::string mk = std::string(1, (char)exact[1]) + name;
        phased[mk] = answerbody::kind(exact.data() + 2 + klen) ==
                             answerbody::kWire
                         ? blob
                         : std::string();
        CHECK(serial.count(mk) == 1);
        if (!phased[mk].empty()) CHECK(phased[mk] == serial[mk]);
    }
    CHECK(phased == serial);
}

template <typename F>
void refused(F call) {
    AnswerDelta d;
    bool threw = false;
    try {
        call(d);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw && d.size() == 0);
}

void checkRefusals() {
    std::string ok(12, 'x');
    refused([&](AnswerDelta& d) { d.upsertReply("a", 1, ok.substr(1)); });
    refused([&](AnswerDelta& d) {
        d.upsertReply("a", 1, std::string(513, 'x'));
    });
    refused([&](AnswerDelta& d) {
        d.upsertReply(std::string(256, 'a'), 1, ok);
    });
    refused([&](AnswerDelta& d) { d.upsertReply("a", 28, ok); });
    refused([&](AnswerDelta& d) { d.upsertReply("_s.d", 33, ok); });
    refused([&](AnswerDelta& d) {
        d.upsertService("a", 1, ok, std::vector<Member>(65, {"s", ""}));
    });
    refused([&](AnswerDelta& d) { d.upsertService("a", 1, "short", {}); });
    refused([&](AnswerDelta& d) { d.invalidate(""); });
    refused([&](AnswerDelta& d) { d.invalidate(std::string(256, 'a')); });

    /* a ceiling of the producer's own: the same rules one size up */
    AnswerDelta large(4096);
    large.upsertReply("a", 1, std::string(4096, 'x'));
    std::string seg(60, 's');  /* 12 + 64 x 61 = 3916 bytes */
    large.upsertService("s", 1, ok, std::vector<Member>(64, {seg, "t"}));
    bool threw = false;
    try {
        large.upsertReply("b", 1, std::string(4097, 'x'));
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw && large.size() == 2 && large.maxReply() == 4096);
    AnswerDelta::Packed p = large.pack();
    for (size_t i = 0; i < 2; ++i)
        verifyBlob((const uint8_t*)p.ubuf.data() + p.uoff[i],
                   (size_t)(p.uoff[i + 1] - p.uoff[i]), 4096);
    for (size_t bad : {511, 4097}) {
        threw = false;
        try {
            AnswerDelta d(bad);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        CHECK(threw);
    }
}

}  // namespace

int main(int argc, char** argv) {
    gSeed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    size_t rounds = argc > 2 ? (size_t)atol(argv[2]) : 300;
    std::mt19937 rng(gSeed);
    printf("answerdelta_check: seed %u, %zu rounds\n", gSeed, rounds);
    checkRefusals();
    for (size_t r = 0; r < rounds; ++r) round(rng, 1 + rng() % 200);
    printf("answerdelta_check OK\n");
    return 0;
}
