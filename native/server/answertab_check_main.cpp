/*
 * answertab_check: stand-alone exerciser for server/answertab.hpp,
 * meant to be built with -fsanitize=address,undefined and run on the
 * CPU (`make check-answertab`).
 *
 * A seeded random sequence of inserts, replacements, lookups, removes
 * and suffix removes runs against a std::unordered_map model; after
 * every operation the touched key, and at intervals every key, must
 * read back exactly what the model holds. Phases: real hashes; hashes
 * masked down to 4 and to 0 bits (every key collides, so every absent
 * lookup walks a whole probe chain); a small arena bound that forces
 * rebuilds and whole-table clears. Keys run from zero to 255 bytes,
 * the pool is large enough to grow the slot array several times. The
 * service body helpers are checked against a plain concatenation.
 */
#define BAMD_ANSWERTAB_TEST_HASH_MASK 1
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "answertab.hpp"

using namespace bamd;

namespace {

unsigned gSeed = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "answertab_check: %s:%d: %s failed "        \
                    "(seed %u)\n", __FILE__, __LINE__, #cond, gSeed);   \
            exit(1);                                                    \
        }                                                               \
    } while (0)

struct Key {
    std::string name;
    uint8_t qtype;
};

/* model key: qtype byte + name */
std::string modelKey(const Key& k) {
    return std::string(1, (char)k.qtype) + k.name;
}

/* SRV entries are stored under the hash of the name behind the first
 * two labels, the way the server files a service's SRV answer */
std::string domainOf(const std::string& name) {
    size_t d1 = name.find('.');
    if (d1 == std::string::npos) return name;
    size_t d2 = name.find('.', d1 + 1);
    if (d2 == std::string::npos) return name;
    return name.substr(d2 + 1);
}

uint64_t hashOf(const Key& k) {
    if (k.qtype == 33) {
        std::string d = domainOf(k.name);
        return AnswerTable::hashKey(d.data(), d.size(), 33);
    }
    return AnswerTable::hashKey(k.name.data(), k.name.size(), k.qtype);
}

std::vector<Key> makePool(std::mt19937& rng, size_t n) {
    std::vector<Key> pool;
    pool.push_back({"", 1});                       /* zero-length key */
    pool.push_back({std::string(255, 'k'), 1});    /* longest key */
    pool.push_back({std::string(255, 'k'), 33});
    for (size_t i = 0; pool.size() < n; ++i) {
        std::string dom = "s" + std::to_string(i) + ".foo.com";
        if (rng() % 8 == 0) dom += std::string(rng() % 200, 'x');
        pool.push_back({dom, 1});
        pool.push_back({"_x._tcp." + dom, 33});
        /* a second SRV name under the same domain hash */
        if (rng() % 4 == 0) pool.push_back({"_y._udp." + dom, 33});
    }
    return pool;
}

std::string randomBody(std::mt19937& rng) {
    size_t len = rng() % 16 == 0 ? rng() % 3000 : 1 + rng() % 300;
    std::string b(len, '\0');
    for (char& ch : b) ch = (char)rng();
    return b;
}

void verifyKey(const AnswerTable& t,
               const std::unordered_map<std::string, std::string>& model,
               const Key& k) {
    uint64_t h = hashOf(k);
    uint32_t blen = 0;
    const uint8_t* body =
        t.find(h, k.qtype, k.name.data(), k.name.size(), &blen);
    auto it = model.find(modelKey(k));
    if (it == model.end()) {
        CHECK(body == nullptr);
        return;
    }
    CHECK(body != nullptr);
    CHECK(blen == it->second.size());
    CHECK(memcmp(body, it->second.data(), blen) == 0);
    /* the two-step lookup the server's pipeline uses */
    uint32_t wholeLen = 0;
    uint32_t off = t.probe(h, &wholeLen);
    CHECK(off != AnswerTable::kNone);
    const uint8_t* viaAt =
        t.at(off, k.qtype, k.name.data(), k.name.size());
    /* with colliding hashes probe() may land on a neighbour */
    CHECK(viaAt == nullptr || viaAt == body);
}

void runPhase(std::mt19937& rng, uint64_t mask, size_t poolSize,
              size_t ops, size_t maxArena, size_t compactMinDead) {
    answertabTestHashMask = mask;
    AnswerTable t(maxArena, compactMinDead);
    std::unordered_map<std::string, std::string> model;
    std::vector<Key> pool = makePool(rng, poolSize);
    uint64_t clearsSeen = 0;

    for (size_t op = 0; op < ops; ++op) {
        const Key& k = pool[rng() % pool.size()];
        uint64_t h = hashOf(k);
        unsigned what = rng() % 100;
        if (what < 45) {            /* insert or replace */
            std::string body = randomBody(rng);
            uint64_t gen = t.generation();
            uint8_t* w = t.insert(h, k.qtype, k.name.data(),
                                  k.name.size(), body.size());
            CHECK(t.generation() != gen);
            if (t.clears() != clearsSeen) {  /* bound hit: memo dropped */
                clearsSeen = t.clears();
                model.clear();
                CHECK(w == nullptr);
                CHECK(t.size() == 0);
            } else {
                CHECK(w != nullptr);
                for (size_t i = 0; i < body.size(); ++i) CHECK(w[i] == 0);
                memcpy(w, body.data(), body.size());
                model[modelKey(k)] = body;
            }
        } else if (what < 75) {     /* lookup, present or absent */
            verifyKey(t, model, k);
        } else if (what < 92) {     /* remove */
            bool had = model.erase(modelKey(k)) != 0;
            CHECK(t.remove(h, k.qtype, k.name.data(), k.name.size()) ==
                  had);
        } else {                    /* drop a domain's SRV entries */
            std::string dom = k.qtype == 33 ? domainOf(k.name) : k.name;
            size_t want = 0;
            for (auto it = model.begin(); it != model.end();) {
                const std::string& mk = it->first;
                bool hit =
                    (uint8_t)mk[0] == 33 && mk.size() - 1 >= dom.size() &&
                    mk.compare(mk.size() - dom.size(), dom.size(), dom) ==
                        0 &&
                    (mk.size() - 1 == dom.size() ||
                     mk[mk.size() - dom.size() - 1] == '.') &&
                    AnswerTable::hashKey(dom.data(), dom.size(), 33) ==
                        hashOf({mk.substr(1), 33});
                if (hit) {
                    it = model.erase(it);
                    ++want;
                } else {
                    ++it;
                }
            }
            CHECK(t.removeSuffix(
                      AnswerTable::hashKey(dom.data(), dom.size(), 33),
                      33, dom.data(), dom.size()) == want);
        }
        CHECK(t.size() == model.size());
        CHECK(t.arenaBytes() <= maxArena);
        CHECK(t.size() * 2 <= t.slots() || t.size() == 0);
        verifyKey(t, model, k);
        if (op % 5000 == 4999)
            for (const Key& each : pool) verifyKey(t, model, each);
    }
    for (const Key& each : pool) verifyKey(t, model, each);
    t.clear();
    CHECK(t.size() == 0 && t.arenaBytes() == 0);
    for (const Key& each : pool)
        CHECK(t.find(hashOf(each), each.qtype, each.name.data(),
                     each.name.size()) == nullptr);
    printf("  mask %016llx pool %zu: %zu ops, %llu rebuilds, "
           "%llu clears, %zu slots\n",
           (unsigned long long)mask, pool.size(), ops,
           (unsigned long long)t.rebuilds(),
           (unsigned long long)t.clears(), t.slots());
}

void checkBodies(std::mt19937& rng) {
    using namespace answerbody;
    for (int round = 0; round < 200; ++round) {
        size_t n = rng() % (kMaxMembers + 1);
        std::string head = randomBody(rng).substr(0, 40);
        std::vector<std::string> a(n), b(n);
        std::vector<Seg> s1(n), s2(n);
        size_t segBytes = 0;
        for (size_t i = 0; i < n; ++i) {
            a[i] = randomBody(rng).substr(0, 1 + rng() % 60);
            if (round % 2 == 0) b[i] = randomBody(rng).substr(0, 30);
            s1[i] = {(const uint8_t*)a[i].data(), a[i].size()};
            s2[i] = {(const uint8_t*)b[i].data(), b[i].size()};
            segBytes += a[i].size() + b[i].size();
        }
        std::vector<uint8_t> body(
            serviceBodyLen(n, head.size(), segBytes));
        serviceFill(body.data(), n, (const uint8_t*)head.data(),
                    head.size(), s1.data(), s2.data());
        CHECK(kind(body.data()) == kService);
        CHECK(serviceMembers(body.data()) == n);
        CHECK(total(body.data()) == head.size() + segBytes);
        std::vector<uint8_t> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = (uint8_t)i;
        for (size_t i = n; i > 1;) {
            --i;
            std::swap(order[i], order[rng() % (i + 1)]);
        }
        std::string want = head;
        for (size_t i = 0; i < n; ++i) want += a[order[i]];
        for (size_t i = 0; i < n; ++i) want += b[order[i]];
        std::vector<uint8_t> got(total(body.data()));
        CHECK(serviceAssemble(body.data(), order.data(), got.data()) ==
              want.size());
        CHECK(memcmp(got.data(), want.data(), want.size()) == 0);

        std::vector<uint8_t> wb(wireBodyLen(want.size()));
        wireFill(wb.data(), (const uint8_t*)want.data(), want.size());
        CHECK(kind(wb.data()) == kWire);
        CHECK(total(wb.data()) == want.size());
        CHECK(memcmp(wireReply(wb.data()), want.data(), want.size()) ==
              0);
    }
}

}  // namespace

int main(int argc, char** argv) {
    gSeed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    size_t ops = argc > 2 ? (size_t)atol(argv[2]) : 100000;
    std::mt19937 rng(gSeed);
    const size_t big = AnswerTable::kDefaultMaxArena;
    printf("answertab_check: seed %u, %zu ops per phase\n", gSeed, ops);
    /* real hashes, enough keys to grow the slot array 3 times */
    runPhase(rng, ~0ull, 6000, ops, big, AnswerTable::kCompactMinDead);
    /* 16 distinct hashes, then a single one: long shared chains */
    runPhase(rng, 0xFull, 300, ops / 4, big, 1u << 16);
    runPhase(rng, 0, 120, ops / 4, big, 1u << 14);
    /* arena bound below the working set: rebuilds and clears */
    runPhase(rng, ~0ull, 400, ops, 48u << 10, 4u << 10);
    runPhase(rng, 0xFFull, 400, ops / 2, 24u << 10, 1u << 10);
    checkBodies(rng);
    printf("answertab_check OK\n");
    return 0;
}
