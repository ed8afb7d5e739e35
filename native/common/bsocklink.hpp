/*
 * binder-amd: one end of a bsock1 connection (balancer/protocol.hpp) -
 * the transport state machine that the balancer and binderd share.
 *
 * A connection starts on the UNIX stream socket. When the rings are
 * agreed on (types 5-7), each side queues one control frame - SHM_OK
 * from binderd, SHM_GO from the balancer - as its last word on the
 * stream, and queueSwitch() remembers where that frame ends in `out`.
 * flush() sends the bytes before that mark to the socket and, once the
 * last of them is written, everything after it to the ring
 * (shmpipe.hpp): never interleaved, and the mark moves with the bytes
 * when the flushed prefix is dropped. The other direction switches when
 * the owner sees the peer's control frame and sets rxShm: from then on
 * drainRing() fills `in`, and the socket may only show its end.
 *
 * What the endpoint cannot own it is handed with each call, the way
 * replyruns.hpp takes its sink. The Sink provides
 *   void armWrite()      wait for EPOLLOUT on fd as well
 *   void disarmWrite()   back to EPOLLIN alone
 *   void doorbell()      the peer's doorbell was rung (a counter)
 *   void drained()       a take from the ring returned data (a counter)
 * Errors are reported, not acted on: closing the connection, and saying
 * why, is the owner's, and it makes no further call on a closed one.
 * Reading the socket into `in` is the owner's too (binderd needs
 * recvmsg for the offer's descriptors, the balancer a plain read).
 *
 * Depends on shmpipe.hpp, framebuf.hpp and POSIX only.
 */
#pragma once

#include <unistd.h>

#include <cerrno>
#include <string>

#include "../server/framebuf.hpp"
#include "shmpipe.hpp"

namespace bamd {

struct BsockLink {
    enum class Flush { Ok, Blocked, StreamError, RingBad };
    static constexpr size_t kRingBad = (size_t)-1;
    /* a flushed prefix of `out` longer than this is dropped, so a peer
     * that stays blocked does not keep it resident (amortized O(1)
     * against the memmove-per-write of erase(0, nw)) */
    static constexpr size_t kCompactAt = 1u << 20;

    int fd = -1;
    FrameBuf in;
    std::string out;
    size_t outOff = 0;  /* flushed prefix of `out` (write cursor) */
    /* stream: EPOLLOUT is armed; ring: the peer rings when it made room */
    bool writeBlocked = false;

    /* shmReady: the region is mapped and our doorbell registered (the
     * offer went out, or was accepted). rxShm: the peer's control frame
     * was seen, its bytes are taken from the ring. txShm: ours has left
     * on the stream, our bytes go to the ring. streamEnd: end of our
     * queued control frame in `out`, 0 when there is none. */
    shm::Link shm;
    bool shmReady = false, rxShm = false, txShm = false;
    size_t streamEnd = 0;

    explicit BsockLink(size_t inRestCap = FrameBuf::kRestCap)
        : in(inRestCap) {}

    /* SHM_OK or SHM_GO: the last bytes this side puts on the stream */
    void queueSwitch(uint8_t frameType) {
        bsock::appendFrame(out, frameType, "");
        streamEnd = out.size();
    }

    /* back to the stream alone (the owner unregisters the doorbell) */
    void dropRings() {
        shm.close();
        shmReady = rxShm = txShm = false;
        streamEnd = 0;
    }

    /* Write what `out` holds past outOff, to the socket or to the ring. */
    template <class Sink>
    Flush flush(Sink&& sink) {
        /* with a control frame queued, the stream gets the bytes up to
         * its end */
        while (!txShm) {
            size_t end = streamEnd != 0 ? streamEnd : out.size();
            if (outOff >= end) break;
            ssize_t nw = ::write(fd, out.data() + outOff, end - outOff);
            if (nw > 0) {
                outOff += (size_t)nw;
                continue;
            }
            if (nw == 0 || (errno != EAGAIN && errno != EWOULDBLOCK))
                return Flush::StreamError;
            if (outOff > kCompactAt) {
                out.erase(0, outOff);
                if (streamEnd != 0) streamEnd -= outOff;
                outOff = 0;
            }
            if (!writeBlocked) {
                writeBlocked = true;
                sink.armWrite();
            }
            return Flush::Blocked;
        }
        if (!txShm && writeBlocked) sink.disarmWrite();
        if (streamEnd != 0) {
            /* the control frame is on the wire: the ring from here on */
            streamEnd = 0;
            txShm = true;
        }
        /* the ring takes what fits now; the rest stays in `out` and the
         * peer rings our doorbell when it has made room */
        bool wrote = false;
        writeBlocked = false;
        while (txShm && outOff < out.size()) {
            size_t n = shm.tx.write(out.data() + outOff, out.size() - outOff);
            outOff += n;
            if (n != 0) wrote = true;
            if (outOff >= out.size()) break;
            if (shm.tx.bad()) return Flush::RingBad;
            writeBlocked = shm.tx.waitForSpace();
            if (writeBlocked) break;
        }
        if (wrote && shm.tx.consumerNeedsWake()) {
            shm::ringDoorbell(shm.wakePeer);
            sink.doorbell();
        }
        if (outOff >= out.size()) {
            out.clear();
            outOff = 0;
        } else if (outOff > kCompactAt) {
            out.erase(0, outOff);
            outOff = 0;
        }
        return writeBlocked ? Flush::Blocked : Flush::Ok;
    }

    /* Take up to `quota` bytes (the last take may pass it by less than
     * a chunk) from the ring into in.tail(), `chunk` at a time; a take
     * that comes back short has emptied the ring. Returns the bytes
     * taken, or kRingBad. */
    template <class Sink>
    size_t drainRing(size_t quota, size_t chunk, Sink&& sink) {
        size_t got = 0;
        while (got < quota) {
            size_t n = shm.rx.read(in.tail(chunk), chunk);
            if (n == 0) break;
            in.commit(n);
            got += n;
            sink.drained();
            if (n < chunk) break;
        }
        if (shm.rx.bad()) return kRingBad;
        if (got != 0 && shm.rx.producerNeedsWake()) {
            shm::ringDoorbell(shm.wakePeer);
            sink.doorbell();
        }
        return got;
    }

    /* The socket became readable after rxShm. The control frame was the
     * peer's last word on the stream: all that can show up now is its
     * end, or a peer gone wrong. False = close the connection. */
    bool streamStillOpen() {
        char junk[64];
        ssize_t nr = ::read(fd, junk, sizeof(junk));
        return nr < 0 && (errno == EAGAIN || errno == EWOULDBLOCK);
    }

    /* Our doorbell rang (edge-triggered; the eventfd is not read): room
     * in the ring we were waiting for - then flush() first - or bytes
     * for us, which the owner drains when rxShm. */
    bool bellWantsFlush() const { return txShm && writeBlocked; }

    /* For the loop's before-park hook (loop.hpp); P is EventLoop::Park,
     * whose values fold with max: NoRings < Idle < Work. park = false,
     * every round: Work when the ring holds bytes or has gone bad, and
     * the owner then drains it. park = true, before a real sleep: says
     * so to the producer; Work when something slipped in. */
    template <class P>
    P parkState(bool park) {
        if (!rxShm) return P::NoRings;
        if (park) return shm.rx.park() ? P::Idle : P::Work;
        return shm.rx.readable() != 0 || shm.rx.bad() ? P::Work : P::Idle;
    }
};

}  // namespace bamd
