/*
 * hostlist_check: stand-alone exerciser for zk/hostlist.hpp, meant to be
 * built with -fsanitize=address,undefined and run on the CPU
 * (`make check-zkhosts`).
 *
 * A fixed table of connect strings that must parse, with the list each
 * must give, and of strings that must be refused, with an error that
 * names the offending entry; then seeded random strings over the
 * alphabet [a-z0-9.,:/\[\] -]. Every input is parsed from a heap block
 * of exactly its length, so a read past either end is a sanitizer
 * report. Whatever is accepted is printed with formatHostList() and
 * parsed again, and must come back as the same list.
 *
 * usage: hostlist_check [seed] [random-strings]
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "hostlist.hpp"

using namespace bamd::zk;

namespace {

unsigned gSeed = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "hostlist_check: %s:%d: %s failed "         \
                    "(seed %u)\n", __FILE__, __LINE__, #cond, gSeed);   \
            exit(1);                                                    \
        }                                                               \
    } while (0)

/* Parses `text` from a heap block of exactly its length. */
bool parseExact(const std::string& text, uint16_t defaultPort,
                std::vector<ZkServer>& out, std::string& err) {
    std::unique_ptr<char[]> block(new char[text.size()]);
    if (!text.empty()) memcpy(block.get(), text.data(), text.size());
    return parseHostList(std::string_view(block.get(), text.size()),
                         defaultPort, out, err);
}

/* accepted => prints and parses back to the same list */
void roundTrip(const std::vector<ZkServer>& servers) {
    CHECK(!servers.empty());
    for (size_t i = 0; i < servers.size(); i++)
        for (size_t j = i + 1; j < servers.size(); j++)
            CHECK(!(servers[i] == servers[j]));
    std::vector<ZkServer> again;
    std::string err;
    /* a default port no entry can depend on: every entry is printed
     * with its own */
    CHECK(parseExact(formatHostList(servers), 1, again, err));
    CHECK(err.empty());
    CHECK(again == servers);
}

struct Accept {
    const char* text;
    std::vector<ZkServer> want;
};

struct Reject {
    const char* text;
    const char* entry;  /* what the error must name */
};

void fixedTable() {
    const Accept accepts[] = {
        {"a", {{"a", 2181}}},
        {"a:1", {{"a", 1}}},
        {"a:65535", {{"a", 65535}}},
        {"10.0.0.1:2181, b ,c:3",
         {{"10.0.0.1", 2181}, {"b", 2181}, {"c", 3}}},
        {"a,a:2181,a", {{"a", 2181}}},
        {" \ta:00080\r\n", {{"a", 80}}},
        {"Zk-1.example_net.,b:2", {{"Zk-1.example_net.", 2181}, {"b", 2}}},
        {"b:2,a:1,b:2,a:2", {{"b", 2}, {"a", 1}, {"a", 2}}},
    };
    for (const Accept& a : accepts) {
        std::vector<ZkServer> got;
        std::string err;
        CHECK(parseExact(a.text, 2181, got, err));
        CHECK(err.empty());
        CHECK(got == a.want);
        roundTrip(got);
    }
    const Reject rejects[] = {
        {"", "\"\""},
        {",", "\"\""},
        {"a,,b", "\"\""},
        {"a, ,b", "\"\""},
        {"a:", "\"a:\""},
        {"a:0", "\"a:0\""},
        {"a:65536", "\"a:65536\""},
        {"a:99999999999999999999", "\"a:99999999999999999999\""},
        {"a:x", "\"a:x\""},
        {"a:-1", "\"a:-1\""},
        {"a:1:2", "\"a:1:2\""},
        {":2181", "\":2181\""},
        {"[::1]:2181", "\"[::1]:2181\""},
        {"a:2181/chroot", "\"a:2181/chroot\""},
        {"b,a:2181/chroot", "\"a:2181/chroot\""},
        {"a b", "\"a b\""},
        {"a,b!", "\"b!\""},
    };
    for (const Reject& r : rejects) {
        std::vector<ZkServer> got{{"stale", 1}};
        std::string err;
        CHECK(!parseExact(r.text, 2181, got, err));
        CHECK(got.empty());
        CHECK(err.find(r.entry) != std::string::npos);
    }
    std::vector<ZkServer> got;
    std::string err;
    CHECK(!parseExact("[::1]:2181", 2181, got, err));
    CHECK(err.find("IPv6") != std::string::npos);
    CHECK(!parseExact("a:2181/chroot", 2181, got, err));
    CHECK(err.find("chroot") != std::string::npos);
    CHECK(parseExact(std::string(255, 'h'), 2181, got, err));
    CHECK(!parseExact(std::string(256, 'h'), 2181, got, err));
}

void randomStrings(unsigned seed, unsigned rounds) {
    static const char kAlphabet[] =
        "abcdefghijklmnopqrstuvwxyz0123456789.,:/[] -";
    std::mt19937 rng(seed);
    unsigned accepted = 0;
    for (unsigned i = 0; i < rounds; i++) {
        /* mostly hostname characters, so that a fair share parses */
        size_t len = rng() % 24;
        std::string text;
        for (size_t k = 0; k < len; k++) {
            unsigned r = rng() % 100;
            if (r < 60) text += kAlphabet[rng() % 36];
            else if (r < 75) text += ',';
            else if (r < 85) text += ':';
            else text += kAlphabet[rng() % (sizeof(kAlphabet) - 1)];
        }
        std::vector<ZkServer> got;
        std::string err;
        bool ok = parseExact(text, (uint16_t)(1 + rng() % 65535), got, err);
        if (ok) {
            CHECK(err.empty());
            roundTrip(got);
            accepted++;
        } else {
            CHECK(got.empty());
            CHECK(!err.empty());
        }
    }
    /* both outcomes must have been seen, or the mix above is off */
    CHECK(accepted > rounds / 50);
    CHECK(accepted < rounds);
    printf("hostlist_check: %u random strings, %u accepted\n", rounds,
           accepted);
}

}  // namespace

int main(int argc, char** argv) {
    gSeed = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10) : 1;
    unsigned rounds =
        argc > 2 ? (unsigned)strtoul(argv[2], nullptr, 10) : 20000;
    fixedTable();
    randomStrings(gSeed, rounds);
    printf("hostlist_check OK (seed %u)\n", gSeed);
    return 0;
}
