/*
 * binder-amd: single-threaded epoll event loop.
 *
 * The reference is a single-threaded event-driven server (Node's event loop;
 * SURVEY.md §3.1 "no worker threads"). We keep the same concurrency model —
 * one loop per process, N processes behind the balancer for scale-out — but
 * on raw epoll with edge-level callbacks and a timer heap.
 *
 * Threads. A loop belongs to the thread that calls run()/runUntil():
 *  - postFromThread() and stop() are legal from any thread, always;
 *  - everything else (addFd, modFd, delFd, addTimer, cancelTimer, defer)
 *    is legal from the loop thread, from its callbacks;
 *  - on a loop with a dispatch lock (setDispatchLock), the same calls are
 *    also legal from another thread *while that thread holds the lock*.
 *    The loop holds the lock whenever it runs callbacks, timers or
 *    deferred tasks and drops it only around epoll_wait, so the lock
 *    holder has the loop's tables to itself. addFd, addTimer and defer
 *    made that way wake the loop, so a new timer deadline or deferred
 *    task is seen at once instead of after the current wait.
 */
#pragma once

#include <atomic>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <thread>
#include <vector>

namespace bamd {

class EventLoop {
  public:
    using FdCallback = std::function<void(uint32_t events)>;
    using TimerCallback = std::function<void()>;

    EventLoop();
    ~EventLoop();
    EventLoop(const EventLoop&) = delete;
    EventLoop& operator=(const EventLoop&) = delete;

    /* events: EPOLLIN / EPOLLOUT bitmask. Callback owns the fd lifecycle. */
    void addFd(int fd, uint32_t events, FdCallback cb);
    void modFd(int fd, uint32_t events);
    void delFd(int fd);

    /* One-shot timer; returns an id usable with cancelTimer. */
    uint64_t addTimer(int64_t delayMs, TimerCallback cb);
    void cancelTimer(uint64_t id);

    /* Run cb on the next loop iteration (loop thread only). */
    void defer(TimerCallback cb);

    /* Thread-safe: queue cb for execution on the loop thread and wake
     * it. Used by helper threads (e.g. the blocking LDAP refresh). */
    void postFromThread(TimerCallback cb);

    void run();
    void stop() { running_ = false; }
    bool running() const { return running_; }

    /* Run until pred() is true or timeout; for tests/clients. */
    bool runUntil(const std::function<bool()>& pred, int64_t timeoutMs);

    /* Optional dispatch lock, see "Threads" above. Set before run();
     * the mutex outlives the loop's last iteration. */
    void setDispatchLock(std::mutex* m) { dispatchLock_ = m; }

    /* For what has no fd to become ready - shared-memory rings. Called
     * on the loop thread (under the dispatch lock, where there is one):
     *
     *  - hook(false) once per round, after deferred tasks and before
     *    epoll_wait: look at the rings and do the work found there.
     *    Returns Work if there was any, Idle if there was none, and
     *    NoRings if the hook has no ring to look at right now: the
     *    round then runs exactly as on a loop without a hook.
     *  - hook(true) only when the loop is about to sleep for real, that
     *    is after a whole round in which neither the hook nor any fd had
     *    anything: announce that this thread is going to sleep (so that
     *    the peers know to wake it) and look once more. Returns Work if
     *    something has arrived meanwhile: the loop then does not sleep.
     *
     * While there are rings, a round that follows one with work or
     * events only polls the fds (epoll_wait with a zero timeout), so a
     * loop under load never announces sleep and nobody spends a syscall
     * on waking it; going idle costs one empty round. One hook per
     * loop; set before run(). */
    enum class Park { NoRings, Idle, Work };
    using ParkHook = std::function<Park(bool park)>;
    void setBeforePark(ParkHook h) { beforePark_ = std::move(h); }

    /* True on the thread that is running this loop. */
    bool inLoopThread() const {
        return loopThread_.load(std::memory_order_relaxed) ==
               std::this_thread::get_id();
    }

  private:
    void runOnce(int64_t maxWaitMs);
    void wake();
    /* a registration made under the dispatch lock by another thread */
    void wakeIfForeign() {
        if (dispatchLock_ != nullptr && !inLoopThread()) wake();
    }
    int64_t nextTimerDelay() const;
    void fireTimers();

    struct Timer {
        int64_t deadline;
        uint64_t id;
        bool operator>(const Timer& o) const {
            return deadline > o.deadline ||
                   (deadline == o.deadline && id > o.id);
        }
    };

    /* Each registration carries a generation; epoll events are tagged
     * with it (data.u64 = gen<<32 | fd) so a stale queued event for a
     * closed-and-reused fd within one epoll_wait batch is dropped
     * instead of being delivered to the new registration (fd-reuse ABA). */
    /* The callback lives on the heap at a stable address and dispatch
     * calls it by reference: nothing is copied or counted per event. A
     * delFd (or a re-registration) made while callbacks are being
     * dispatched - typically by the callback about itself - moves the
     * function into retired_, which is emptied after the round, so the
     * reference stays good for as long as the callback runs. */
    struct FdReg {
        uint32_t gen;
        std::unique_ptr<FdCallback> cb;
    };
    void retire(FdReg& r) {
        if (dispatching_ && r.cb) retired_.push_back(std::move(r.cb));
    }

    int epfd_;
    std::atomic<bool> running_{false};
    std::map<int, FdReg> fds_;
    std::vector<std::unique_ptr<FdCallback>> retired_;
    bool dispatching_ = false;  /* inside the fd callback loop */
    uint32_t nextFdGen_ = 1;
    std::priority_queue<Timer, std::vector<Timer>, std::greater<Timer>> heap_;
    std::map<uint64_t, TimerCallback> timers_;  // id -> cb (absent=cancelled)
    uint64_t nextTimerId_ = 1;
    std::vector<TimerCallback> deferred_;
    ParkHook beforePark_;
    bool hadWork_ = false;  /* the previous round found some */

    int wakeFd_ = -1;
    std::mutex* dispatchLock_ = nullptr;
    std::atomic<std::thread::id> loopThread_{};
    std::mutex postMutex_;
    std::vector<TimerCallback> posted_;
};

/* fcntl O_NONBLOCK helper; returns false on error. */
bool setNonBlocking(int fd);

}  // namespace bamd
