/*
 * frameindex_check: stand-alone exerciser for gpu/frameindex.hpp, meant
 * to be built with -fsanitize=address,undefined and run on the CPU
 * (`make check-frameindex`).
 *
 * A run of frames of every type is indexed from a heap block of exactly
 * its length, so a read past the run is a report: whole, cut at every
 * byte (inside a header, inside a payload), with a bad magic and an
 * oversized payload_len in the middle, and with maxFrames below the
 * run's count.
 */
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "frameindex.hpp"

using namespace bamd;
using namespace bamd::gpu;

namespace {

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "frameindex_check: %s:%d: %s failed\n",     \
                    __FILE__, __LINE__, #cond);                         \
            exit(1);                                                    \
        }                                                               \
    } while (0)

FrameIndex indexExact(const std::string& run, size_t len, size_t max) {
    std::vector<uint8_t> exact(run.begin(), run.begin() + len);
    return frameIndex(exact.data(), exact.size(), max);
}

}  // namespace

int main() {
    std::string run;
    std::vector<size_t> starts;
    const size_t plens[] = {0, 41, 0, 12, 300, 5, 0, 1};
    for (size_t i = 0; i < 8; ++i) {
        starts.push_back(run.size());
        bsock::appendFrame(run, (uint8_t)(i == 3 ? 9 : 1 + i % 7),
                           std::string(plens[i], (char)(0xB5 - i)));
    }
    starts.push_back(run.size());

    /* cut at every byte: the whole frames in front of the cut */
    for (size_t len = 0; len <= run.size(); ++len) {
        FrameIndex ix = indexExact(run, len, 100);
        size_t whole = 0;
        while (whole + 1 < starts.size() && starts[whole + 1] <= len) ++whole;
        CHECK(ix.status == IndexStatus::NeedMore);
        CHECK(ix.foff.size() == whole + 1 && ix.consumed == starts[whole]);
        for (size_t i = 0; i <= whole; ++i)
            CHECK((size_t)ix.foff[i] == starts[i]);
    }

    /* maxFrames reached, also exactly at the run's end and at zero */
    for (size_t max : {0, 1, 5, 8}) {
        FrameIndex ix = indexExact(run, run.size(), max);
        CHECK(ix.status == IndexStatus::Full);
        CHECK(ix.foff.size() == max + 1 && ix.consumed == starts[max]);
    }

    /* a bad magic and a payload_len above the limit at frames 0, 3, 7 */
    for (size_t f : {0, 3, 7}) {
        std::string bad = run;
        bad[starts[f]] = (char)0xB4;
        FrameIndex ix = indexExact(bad, bad.size(), 100);
        CHECK(ix.status == IndexStatus::Bad && ix.consumed == starts[f]);
        CHECK(ix.foff.size() == f + 1);
        /* the header is judged as soon as it is whole, not before */
        CHECK(indexExact(bad, starts[f] + 6, 100).status == IndexStatus::Bad);
        CHECK(indexExact(bad, starts[f] + 5, 100).status ==
              IndexStatus::NeedMore);

        std::string big = run.substr(0, starts[f]);
        bsock::appendFrame(big, 1, "");
        uint32_t over = bsock::kMaxPayload + 1;
        for (int b = 0; b < 4; ++b)
            big[starts[f] + 2 + b] = (char)(over >> (8 * b));
        CHECK(indexExact(big, big.size(), 100).status == IndexStatus::Bad);
        big[starts[f] + 2] = 0;  /* kMaxPayload itself only needs more */
        ix = indexExact(big, big.size(), 100);
        CHECK(ix.status == IndexStatus::NeedMore && ix.consumed == starts[f]);
    }
    printf("frameindex_check OK\n");
    return 0;
}
