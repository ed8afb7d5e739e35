/*
 * binder-amd: receive buffer with a read cursor for the bsock1 stream.
 *
 * The balancer socket delivers hundreds of small frames per epoll
 * event. Erasing each parsed frame from the front of a std::string
 * moves the whole remainder every time (quadratic in the bytes
 * buffered); here parsing only advances a cursor, and compact() moves
 * the trailing partial frame (less than one frame) to the front once
 * per event. read() targets the tail directly, so there is no bounce
 * buffer either.
 *
 * No dependency on the event loop or on sockets: the owner asks for
 * tail space, fills it (read(), memcpy, ...) and commits the count.
 */
#pragma once

#include <cstdint>
#include <cstring>
#include <memory>

#include "../balancer/protocol.hpp"

namespace bamd {

class FrameBuf {
  public:
    /* resting capacity: one per-event read quota plus a small partial
     * frame; larger frames grow the buffer, compact() shrinks it back.
     * An owner that reads more per event passes its own. */
    static constexpr size_t kRestCap = 160 * 1024;

    explicit FrameBuf(size_t restCap = kRestCap) : restCap_(restCap) {}

    /* unparsed bytes */
    const uint8_t* data() const { return buf_.get() + rd_; }
    size_t size() const { return wr_ - rd_; }
    size_t capacity() const { return cap_; }

    /* Writable tail with room for at least `want` bytes. Invalidates
     * pointers previously obtained from data(). */
    uint8_t* tail(size_t want) {
        if (cap_ - wr_ < want) grow(want);
        return buf_.get() + wr_;
    }
    void commit(size_t n) { wr_ += n; }

    /* drop n parsed bytes from the front (cursor move only) */
    void consume(size_t n) { rd_ += n; }

    /* forget everything received (the connection is gone) */
    void clear() { rd_ = wr_ = 0; }

    /* Once per event, after the parse loop: bring the unparsed rest to
     * the front and give back memory a large frame made us take. */
    void compact() {
        size_t left = wr_ - rd_;
        if (cap_ > restCap_ && left <= restCap_ / 4) {
            move(restCap_);
            return;
        }
        if (rd_ != 0) {
            if (left != 0) memmove(buf_.get(), buf_.get() + rd_, left);
            rd_ = 0;
            wr_ = left;
        }
    }

  private:
    void grow(size_t want) {
        /* reuse the consumed prefix before asking for more memory */
        size_t left = wr_ - rd_;
        if (rd_ != 0 && cap_ - left >= want) {
            if (left != 0) memmove(buf_.get(), buf_.get() + rd_, left);
            rd_ = 0;
            wr_ = left;
            return;
        }
        size_t need = left + want;
        size_t ncap = cap_ == 0 ? restCap_ : cap_ * 2;
        if (ncap < need) ncap = need;
        move(ncap);
    }

    /* new block of ncap bytes (left uninitialised), unparsed bytes at
     * its front */
    void move(size_t ncap) {
        size_t left = wr_ - rd_;
        std::unique_ptr<uint8_t[]> nb(new uint8_t[ncap]);
        if (left != 0) memcpy(nb.get(), buf_.get() + rd_, left);
        buf_ = std::move(nb);
        cap_ = ncap;
        rd_ = 0;
        wr_ = left;
    }

    std::unique_ptr<uint8_t[]> buf_;
    size_t restCap_;
    size_t cap_ = 0;
    size_t rd_ = 0;  /* parse cursor */
    size_t wr_ = 0;  /* end of received bytes */
};

namespace bsock {

struct FrameView {
    uint8_t type;
    uint32_t plen;
    const uint8_t* payload;  /* valid until the next tail()/compact() */
};

enum class FrameStatus { Ok, NeedMore, Bad };

/* Take the next complete frame off the buffer. Bad = wrong magic or
 * payload length above kMaxPayload (the stream cannot be resynced). */
inline FrameStatus nextFrame(FrameBuf& in, FrameView& f) {
    if (in.size() < kHeaderLen) return FrameStatus::NeedMore;
    const uint8_t* h = in.data();
    if (h[0] != kMagic) return FrameStatus::Bad;
    uint32_t plen = getU32(h + 2);
    if (plen > kMaxPayload) return FrameStatus::Bad;
    if (in.size() < kHeaderLen + (size_t)plen) return FrameStatus::NeedMore;
    f.type = h[1];
    f.plen = plen;
    f.payload = h + kHeaderLen;
    in.consume(kHeaderLen + plen);
    return FrameStatus::Ok;
}

}  // namespace bsock

}  // namespace bamd
