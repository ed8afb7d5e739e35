/*
 * codec_check: stand-alone exerciser for dns/codec.cpp, meant to be
 * built with -fsanitize=address,undefined and run on the CPU
 * (`make check-codec`).
 *
 * The decoder faces the network. Every input here is copied into a heap
 * block of exactly its own length before Message::decode sees it, so a
 * read of even one octet past the end is an AddressSanitizer report
 * (the Python fuzzers hand over bytes objects with slack behind them).
 * The corpus is made in the program from a seed: a few messages of
 * every record type, every prefix of each, copies with 1-5 octets
 * changed, and random buffers. Whatever decodes is encoded again and
 * decoded again, and the two decoded messages must be equal: the
 * encoder writes nothing its own decoder reads differently, and refuses
 * nothing the decoder let in.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "codec.hpp"

using namespace bamd::dns;

namespace {

unsigned gSeed = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "codec_check: %s:%d: %s failed "            \
                    "(seed %u)\n", __FILE__, __LINE__, #cond, gSeed);   \
            exit(1);                                                    \
        }                                                               \
    } while (0)

bool same(const Record& a, const Record& b) {
    return a.name == b.name && a.type == b.type && a.rclass == b.rclass &&
           a.ttl == b.ttl && a.a == b.a && a.aaaa == b.aaaa &&
           a.target == b.target && a.priority == b.priority &&
           a.weight == b.weight && a.port == b.port &&
           a.soa.mname == b.soa.mname && a.soa.rname == b.soa.rname &&
           a.soa.serial == b.soa.serial &&
           a.soa.refresh == b.soa.refresh && a.soa.retry == b.soa.retry &&
           a.soa.expire == b.soa.expire &&
           a.soa.minimum == b.soa.minimum && a.rdataRaw == b.rdataRaw;
}

bool same(const std::vector<Record>& a, const std::vector<Record>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!same(a[i], b[i])) return false;
    return true;
}

bool same(const Message& a, const Message& b) {
    const Header &x = a.header, &y = b.header;
    if (x.id != y.id || x.qr != y.qr || x.opcode != y.opcode ||
        x.aa != y.aa || x.tc != y.tc || x.rd != y.rd || x.ra != y.ra ||
        x.rcode != y.rcode)
        return false;
    if (a.questions.size() != b.questions.size()) return false;
    for (size_t i = 0; i < a.questions.size(); ++i) {
        const Question &p = a.questions[i], &q = b.questions[i];
        if (p.name != q.name || p.qtype != q.qtype || p.qclass != q.qclass)
            return false;
    }
    return same(a.answers, b.answers) &&
           same(a.authorities, b.authorities) &&
           same(a.additionals, b.additionals);
}

size_t gDecoded = 0, gRefused = 0;

/* decode from a block of exactly len octets; what decodes must survive
 * encode + decode unchanged */
void feed(const uint8_t* data, size_t len) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);
    if (len != 0) memcpy(exact.get(), data, len);
    auto m = Message::decode(exact.get(), len);
    if (!m) {
        ++gRefused;
        return;
    }
    ++gDecoded;
    std::vector<uint8_t> again = m->encode(0);
    std::unique_ptr<uint8_t[]> exact2(new uint8_t[again.size()]);
    memcpy(exact2.get(), again.data(), again.size());
    auto m2 = Message::decode(exact2.get(), again.size());
    CHECK(m2.has_value());
    CHECK(same(*m, *m2));
}

std::string label(std::mt19937& rng, size_t most) {
    static const char kChars[] =
        "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-";
    size_t n = 1 + rng() % (rng() % 8 == 0 ? 63 : 10);
    if (n > most) n = most;
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back(kChars[rng() % 64]);
    return s;
}

/* a name under one of a few shared suffixes, so that the encoder has
 * something to compress; now and then as long as a name may be */
std::string name(std::mt19937& rng) {
    static const char* kTails[] = {"foo.com", "svc.foo.com", "example",
                                   ""};
    std::string s = kTails[rng() % 4];
    if (s.empty() && rng() % 4 == 0) return s;  /* root */
    size_t labels = rng() % 16 == 0 ? 127 : rng() % 4;
    for (size_t i = 0; i < labels; ++i) {
        /* presentation size + 2 = octets on the wire (RFC 1035 2.3.4) */
        size_t room = 253 - s.size();
        if (room < 2) break;
        std::string l = label(rng, room - 1 < 63 ? room - 1 : 63);
        s = s.empty() ? l : l + "." + s;
    }
    return s.empty() ? "x" : s;
}

Record record(std::mt19937& rng, uint16_t type) {
    Record r;
    switch (type) {
    case TYPE_A:
        r = Record::A(name(rng), "10.1.2.3", rng());
        break;
    case TYPE_AAAA:
        r = Record::AAAA(name(rng), "2001:db8::1", rng());
        break;
    case TYPE_NS:
        r = Record::CNAME(name(rng), name(rng), rng());
        r.type = TYPE_NS;
        break;
    case TYPE_CNAME:
        r = Record::CNAME(name(rng), name(rng), rng());
        break;
    case TYPE_PTR:
        r = Record::PTR(name(rng), name(rng), rng());
        break;
    case TYPE_TXT: {
        static const size_t kSizes[] = {0, 1, 20, 255, 256, 600};
        r = Record::TXT(name(rng), std::string(kSizes[rng() % 6], 't'),
                        rng());
        break;
    }
    case TYPE_SRV:
        r = Record::SRV(name(rng), name(rng), (uint16_t)rng(), rng(),
                        (uint16_t)rng(), (uint16_t)rng());
        break;
    case TYPE_SOA: {
        SoaData soa;
        soa.mname = name(rng);
        soa.rname = name(rng);
        soa.serial = rng();
        soa.refresh = rng();
        soa.retry = rng();
        soa.expire = rng();
        soa.minimum = rng();
        r = Record::SOA(name(rng), std::move(soa), rng());
        break;
    }
    case TYPE_OPT:
        r = Record::OPT((uint16_t)rng());
        r.ttl = rng();
        r.rdataRaw.assign(rng() % 12, (uint8_t)rng());
        break;
    default:  /* a type the codec carries as raw rdata */
        r.name = name(rng);
        r.type = type;
        r.ttl = rng();
        r.rdataRaw.assign(rng() % 40, (uint8_t)rng());
        break;
    }
    if (type != TYPE_OPT && rng() % 4 == 0) r.rclass = (uint16_t)rng();
    return r;
}

const uint16_t kTypes[] = {TYPE_A,   TYPE_AAAA, TYPE_NS,  TYPE_CNAME,
                           TYPE_PTR, TYPE_TXT,  TYPE_SRV, TYPE_SOA,
                           TYPE_OPT, TYPE_MX,   99};

Message message(std::mt19937& rng, uint16_t mainType) {
    Message m;
    m.header.id = (uint16_t)rng();
    m.header.qr = rng() % 2;
    m.header.opcode = (uint8_t)(rng() % 16);
    m.header.aa = rng() % 2;
    m.header.tc = rng() % 2;
    m.header.rd = rng() % 2;
    m.header.ra = rng() % 2;
    m.header.rcode = (uint8_t)(rng() % 16);
    for (size_t i = rng() % 3; i > 0; --i) {
        Question q;
        q.name = name(rng);
        q.qtype = mainType;
        q.qclass = (uint16_t)(rng() % 4 == 0 ? rng() : 1);
        m.questions.push_back(std::move(q));
    }
    std::vector<Record>* secs[] = {&m.answers, &m.authorities,
                                   &m.additionals};
    secs[rng() % 3]->push_back(record(rng, mainType));
    for (auto* sec : secs)
        for (size_t i = rng() % 4; i > 0; --i)
            sec->push_back(record(rng, kTypes[rng() % 11]));
    return m;
}

}  // namespace

int main(int argc, char** argv) {
    gSeed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    size_t rounds = argc > 2 ? (size_t)atoi(argv[2]) : 20;
    std::mt19937 rng(gSeed);

    size_t inputs = 0;
    for (size_t round = 0; round < rounds; ++round) {
        for (uint16_t type : kTypes) {
            Message m = message(rng, type);
            std::vector<uint8_t> wire = m.encode(0);
            /* what the encoder wrote, its own decoder reads back */
            {
                auto back = Message::decode(wire.data(), wire.size());
                CHECK(back.has_value());
                CHECK(same(m, *back));
            }
            feed(wire.data(), wire.size());
            ++inputs;
            for (size_t cut = 0; cut < wire.size(); ++cut, ++inputs)
                feed(wire.data(), cut);
            for (size_t k = 0; k < 200; ++k, ++inputs) {
                std::vector<uint8_t> mut = wire;
                for (size_t c = 1 + rng() % 5; c > 0; --c) {
                    size_t at = rng() % mut.size();
                    /* pointers, lengths and counts more often than not */
                    static const uint8_t kLikely[] = {0x00, 0x01, 0x0C,
                                                      0x2E, 0x3F, 0x40,
                                                      0xC0, 0xFF};
                    mut[at] = rng() % 2 ? kLikely[rng() % 8]
                                        : (uint8_t)rng();
                }
                feed(mut.data(), mut.size());
            }
        }
        for (size_t k = 0; k < 500; ++k, ++inputs) {
            std::vector<uint8_t> junk(rng() % 160);
            for (auto& b : junk) b = (uint8_t)rng();
            /* a plausible header in front of half of them */
            if (junk.size() >= 12 && rng() % 2) {
                for (size_t i = 2; i < 12; ++i) junk[i] = 0;
                junk[5] = 1;
                junk[7] = (uint8_t)(rng() % 3);
            }
            feed(junk.data(), junk.size());
        }
    }
    CHECK(gDecoded > inputs / 100);  /* the corpus is not all refusals */
    CHECK(gRefused > inputs / 100);
    printf("codec_check OK: %zu inputs, %zu decoded, %zu refused "
           "(seed %u)\n", inputs, gDecoded, gRefused, gSeed);
    return 0;
}
