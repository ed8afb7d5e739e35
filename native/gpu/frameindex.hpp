/*
 * binder-amd: GPU batch resolver - the host side of a frame burst
 * (resolveframes.hpp): where the bsock1 frames of a byte run start.
 *
 * Frame boundaries are a serial chain through payload_len, a few
 * nanoseconds per frame for the host, which walks the run anyway. The
 * walk makes bsock::nextFrame's decisions (server/framebuf.hpp) and
 * looks at no payload; the kernel holds every frame against the index
 * again. Host code only, no HIP.
 */
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../balancer/protocol.hpp"

namespace bamd::gpu {

enum class IndexStatus : int {
    Full = 0,      /* stopped at maxFrames, or at the 2^31 bytes below */
    NeedMore = 1,  /* an incomplete header or payload, or no byte, is left */
    Bad = 2,       /* wrong magic, or payload_len above kMaxPayload */
};

struct FrameIndex {
    std::vector<int32_t> foff;  /* [frames + 1], foff[frames] == consumed */
    size_t consumed = 0;
    IndexStatus status = IndexStatus::NeedMore;
};

/* Index the whole frames of data[0..len), of every type, at most
 * maxFrames of them. Offsets are the kernel's 32-bit ones, so the walk
 * also stops in front of a frame that ends past 2^31 - 1. */
inline FrameIndex frameIndex(const uint8_t* data, size_t len,
                             size_t maxFrames) {
    FrameIndex out;
    out.foff.push_back(0);
    size_t at = 0;
    while (true) {
        if (out.foff.size() - 1 == maxFrames) {
            out.status = IndexStatus::Full;
            break;
        }
        size_t left = len - at;
        if (left < bsock::kHeaderLen) break;
        const uint8_t* h = data + at;
        uint32_t plen = bsock::getU32(h + 2);
        if (h[0] != bsock::kMagic || plen > bsock::kMaxPayload) {
            out.status = IndexStatus::Bad;
            break;
        }
        if (left < bsock::kHeaderLen + (size_t)plen) break;
        size_t next = at + bsock::kHeaderLen + plen;
        if (next > 0x7FFFFFFFu) {
            out.status = IndexStatus::Full;
            break;
        }
        at = next;
        out.foff.push_back((int32_t)at);
    }
    out.consumed = at;
    return out;
}

}  // namespace bamd::gpu
