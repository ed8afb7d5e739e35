/*
 * framebuf_check: stand-alone exerciser for server/framebuf.hpp, meant
 * to be built with -fsanitize=address,undefined and run on the CPU
 * (`make check-framebuf`).
 *
 * Random bsock1 frame streams - mixed types, payloads from empty up to
 * one maximum-size frame - are fed through FrameBuf in random read
 * sizes (the server's per-event quota among them) and must come out as
 * exactly the frames that went in, byte for byte; after every "event"
 * the buffer must hold less than one frame, and it must be back at its
 * resting capacity once a large frame has passed. Bad magic and an
 * oversize length must be reported as such.
 */
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "framebuf.hpp"

using namespace bamd;

namespace {

struct Frame {
    uint8_t type;
    std::string payload;
};

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "framebuf_check: %s:%d: %s failed "         \
                    "(seed %u)\n", __FILE__, __LINE__, #cond, gSeed);   \
            exit(1);                                                    \
        }                                                               \
    } while (0)

unsigned gSeed = 0;

void runStream(std::mt19937& rng, bool withMaxFrame) {
    /* build the stream */
    std::vector<Frame> frames;
    size_t n = 50 + rng() % 400;
    size_t maxAt = withMaxFrame ? rng() % n : n;
    for (size_t i = 0; i < n; ++i) {
        Frame f;
        f.type = (uint8_t)(1 + rng() % 4);
        size_t len;
        if (i == maxAt)
            len = bsock::kMaxPayload;
        else if (rng() % 16 == 0)
            len = rng() % 70000;       /* larger than one read quota/2 */
        else if (rng() % 8 == 0)
            len = 0;                   /* PING-like */
        else
            len = 24 + rng() % 80;     /* the common QUERY size */
        f.payload.resize(len);
        for (size_t k = 0; k < len; k += 1 + rng() % 97)
            f.payload[k] = (char)rng();
        frames.push_back(std::move(f));
    }
    std::string stream;
    for (const auto& f : frames)
        bsock::appendFrame(stream, f.type, f.payload);

    /* feed it the way the server does: per event, up to a quota of
     * new bytes in one or more reads into the tail, then parse, then
     * compact once */
    static const size_t kQuotas[] = {1, 5, 6, 7, 29, 30, 31, 4096,
                                     16384, 128 * 1024};
    FrameBuf in;
    size_t off = 0, next = 0;
    while (off < stream.size()) {
        size_t quota = kQuotas[rng() % (sizeof(kQuotas) /
                                        sizeof(kQuotas[0]))];
        size_t got = 0;
        while (got < quota && off < stream.size()) {
            size_t want = quota - got;
            uint8_t* t = in.tail(want);
            /* a read() may return anything from 1 to want bytes */
            size_t nr = 1 + rng() % want;
            if (rng() % 2) nr = want;
            if (nr > stream.size() - off) nr = stream.size() - off;
            memcpy(t, stream.data() + off, nr);
            in.commit(nr);
            off += nr;
            got += nr;
            if (nr < want) break;
        }
        bsock::FrameView fv;
        bsock::FrameStatus st;
        while ((st = bsock::nextFrame(in, fv)) ==
               bsock::FrameStatus::Ok) {
            CHECK(next < frames.size());
            const Frame& f = frames[next++];
            CHECK(fv.type == f.type);
            CHECK(fv.plen == f.payload.size());
            CHECK(memcmp(fv.payload, f.payload.data(), fv.plen) == 0);
        }
        CHECK(st == bsock::FrameStatus::NeedMore);
        in.compact();
        /* what is left is a partial frame */
        CHECK(in.size() < bsock::kHeaderLen + bsock::kMaxPayload);
        if (in.size() <= FrameBuf::kRestCap / 4)
            CHECK(in.capacity() <= FrameBuf::kRestCap);
    }
    CHECK(next == frames.size());
    CHECK(in.size() == 0);
    CHECK(in.capacity() <= FrameBuf::kRestCap);
}

void runBad() {
    FrameBuf in;
    std::string s;
    bsock::appendFrame(s, bsock::FRAME_PING, "");
    s[0] = (char)0xB4;
    memcpy(in.tail(s.size()), s.data(), s.size());
    in.commit(s.size());
    bsock::FrameView fv;
    CHECK(bsock::nextFrame(in, fv) == bsock::FrameStatus::Bad);

    FrameBuf in2;
    uint8_t h[6] = {bsock::kMagic, bsock::FRAME_QUERY, 0, 0, 0, 0};
    uint32_t plen = bsock::kMaxPayload + 1;
    h[2] = (uint8_t)plen;
    h[3] = (uint8_t)(plen >> 8);
    h[4] = (uint8_t)(plen >> 16);
    h[5] = (uint8_t)(plen >> 24);
    memcpy(in2.tail(5), h, 5);
    in2.commit(5);
    CHECK(bsock::nextFrame(in2, fv) == bsock::FrameStatus::NeedMore);
    memcpy(in2.tail(1), h + 5, 1);
    in2.commit(1);
    CHECK(bsock::nextFrame(in2, fv) == bsock::FrameStatus::Bad);
}

}  // namespace

int main(int argc, char** argv) {
    unsigned seed0 = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10)
                              : 1;
    int rounds = argc > 2 ? atoi(argv[2]) : 40;
    runBad();
    for (int r = 0; r < rounds; ++r) {
        gSeed = seed0 + (unsigned)r;
        std::mt19937 rng(gSeed);
        runStream(rng, r % 4 == 0);
    }
    printf("framebuf_check OK: %d streams from seed %u\n", rounds, seed0);
    return 0;
}
