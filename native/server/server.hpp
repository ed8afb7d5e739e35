/*
 * binder-amd: the DNS serving core (lib/server.js equivalent) — UDP, TCP
 * and balancer-socket listeners feeding the resolution engine, with the
 * reference's after-hook metrics and per-query log lines
 * (/root/reference/lib/server.js:435-660).
 *
 * Native design notes (not a translation):
 *  - UDP RX/TX uses recvmmsg/sendmmsg batches (up to 64 datagrams per
 *    syscall) — the dominant cost at high QPS is syscalls, not lookups;
 *  - responses are encoded straight into a flat TX arena;
 *  - the balancer hop is a framed protocol over a UNIX stream socket
 *    ("bsock1", see balancer/protocol.hpp) carrying the original client
 *    address, like mname's listenBalancer (server.js:621-631);
 *  - balancer connections can be served by a pool of threads, each with
 *    an event loop and an answer table of its own (ServeCtx below;
 *    ownership and locking rules in docs/ARCHITECTURE.md).
 */
#pragma once

#include <netinet/in.h>
#include <sys/socket.h>
#include <sys/un.h>

#include <atomic>
#include <functional>
#include <random>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../common/bsocklink.hpp"
#include "../common/log.hpp"
#include "../common/loop.hpp"
#include "../engine/engine.hpp"
#include "answertab.hpp"
#include "metrics.hpp"

namespace bamd {

struct ServerOptions {
    std::string name = "binder";
    std::string host;  // bind address; empty = all interfaces
    uint16_t port = 53;
    std::string balancerSocket;  // unix socket path; empty = none
    /* threads serving balancer connections; 1 = none besides the main
     * thread. See defaultServeThreads(). */
    int serveThreads = 1;
    /* accept a balancer's offer of shared-memory rings for its
     * connection (config balancerShm, environment BINDER_BAL_SHM) */
    bool balancerShm = true;
};

/* clamp(cpus / 4, 1, 4), cpus being what this process may actually use:
 * the cgroup CPU quota (v2 cpu.max, then v1 cfs), else the affinity
 * mask - never the machine's hardware thread count. */
int defaultServeThreads();

struct QueryTimers {
    int64_t parseUs = 0;
    int64_t resolveUs = 0;
    int64_t encodeUs = 0;
};

/* Who asked. The address stays in raw form: only the per-query log line
 * wants the presentation string, and formatting it for every query was
 * ~100 ns of inet_ntop that nothing read at warn level. */
struct ClientInfo {
    uint8_t addr[16] = {};   // network order; first 4 bytes when ipFamily=4
    uint8_t ipFamily = 0;    // 4, 6, or 0 = unknown (formats as "")
    uint16_t port = 0;
    const char* family = "udp";  // matches query.src.family usage in logs

    /* presentation form, written into buf; call where a log line is
     * actually emitted */
    const char* address(char (&buf)[48]) const;
};

/*
 * Where a synchronous reply is written. Vector mode (UDP tx arena slot,
 * TCP scratch): the DNS message replaces the vector's content. Frame
 * mode (balancer socket): a bsock1 REPLY frame is appended to the
 * connection's out buffer - header first, then the message bytes - so
 * the answer is copied exactly once, from the cache to the socket
 * buffer.
 */
class ReplySink {
  public:
    explicit ReplySink(std::vector<uint8_t>* v) : vec_(v) {}
    ReplySink(std::string* frames, uint32_t reqId)
        : frames_(frames), reqId_(reqId) {}

    /* start a reply of exactly dnsLen bytes (append() supplies them) */
    void open(size_t dnsLen);
    /* start a reply of exactly dnsLen bytes and return where to write
     * them: the caller fills the message in place, no append() */
    uint8_t* openWrite(size_t dnsLen);
    void append(const uint8_t* p, size_t n) {
        if (vec_ != nullptr)
            vec_->insert(vec_->end(), p, p + n);
        else
            frames_->append((const char*)p, n);
    }
    /* the message written so far, for in-place id/RD patching */
    uint8_t* dns() {
        return vec_ != nullptr ? vec_->data()
                               : (uint8_t*)frames_->data() + start_;
    }
    size_t dnsLen() const {
        return vec_ != nullptr ? vec_->size() : frames_->size() - start_;
    }
    /* the vector to encode into directly, or nullptr in frame mode */
    std::vector<uint8_t>* vec() { return vec_; }

  private:
    std::vector<uint8_t>* vec_ = nullptr;
    std::string* frames_ = nullptr;
    uint32_t reqId_ = 0;
    size_t start_ = 0;  /* offset of the DNS message in *frames_ */
};

class RecursionIface {
  public:
    virtual ~RecursionIface() = default;
    /* Fill resp (REFUSED if nothing found) and invoke done. May complete
     * synchronously or later from the event loop. */
    virtual void resolve(const dns::Message& query, dns::Message& resp,
                         std::function<void()> done) = 0;
};

class DnsServer {
  public:
    DnsServer(EventLoop* loop, Logger log, ServerOptions opts,
              Engine* engine, Collector* collector);
    ~DnsServer();

    void setRecursion(RecursionIface* r) { recursion_ = r; }

    bool start();  // listen UDP + TCP (+ balancer socket if configured)
    void stop();

    uint16_t boundPort() const { return boundPort_; }

    uint64_t queriesServed() const;

  private:
    /* whether start() runs a pool: serveThreads >= 2, a balancer
     * socket, and the answer table in use (fixed at start) */
    bool pooled() const;

    struct TcpConn : std::enable_shared_from_this<TcpConn> {
        int fd;
        std::string in;
        std::string out;
        bool writeBlocked = false;
        ClientInfo ci;
        uint32_t pendingAsync = 0;
        bool closed = false;
        int64_t lastActivityMs = 0;
    };
    struct ServeCtx;
    struct LinkSink;
    struct BalConn: std::enable_shared_from_this<BalConn> {
        ServeCtx* ctx = nullptr;  /* owner; only its thread touches us */
        /* socket, buffers and, once an offer is accepted, the rings */
        BsockLink link;
        bool closed = false;
        /* the descriptors that arrived with the stream bytes, until
         * the SHM_OFFER frame they belong to is parsed */
        int rxFds[bsock::kShmOfferFds] = {-1, -1, -1};
        int nRxFds = 0;
        ~BalConn();
    };

    /* Where an asynchronous (recursion) reply goes. Non-owning and
     * trivially copyable: callers fill it on the stack per query, and
     * process() turns it into an owning closure only when the engine
     * actually hands the query to recursion. */
    struct ReplyTarget {
        enum class Kind : uint8_t { Udp, Tcp, Bal } kind;
        const struct sockaddr_storage* src = nullptr;  /* Udp */
        socklen_t srcLen = 0;
        TcpConn* tcp = nullptr;
        BalConn* bal = nullptr;
        uint32_t reqId = 0;  /* Bal */
    };
    std::function<void(std::vector<uint8_t>)> makeAsyncReply(
        const ReplyTarget& t);

    bool openUdp();
    bool openTcp();
    bool openBalancer();

    void onUdpReadable();
    void onTcpAccept();
    void onTcpConn(TcpConn* c, uint32_t events);
    void onBalAccept();
    void adoptBal(ServeCtx& ctx, int fd);
    void onBalConn(ServeCtx& ctx, BalConn* c, uint32_t events);
    void onBalBell(ServeCtx& ctx, BalConn* c);
    void serveBal(ServeCtx& ctx, BalConn* c, bool fromRing);
    void acceptShm(ServeCtx& ctx, BalConn* c, const uint8_t* p, size_t len);
    void dropRxFds(BalConn* c);
    EventLoop::Park balBeforePark(ServeCtx& ctx, bool park);

    /*
     * Decode + resolve + encode. Returns true when the answer is
     * synchronous: it has been written to `out`, or nothing has when
     * the packet is dropped. Returns false when handed to recursion;
     * delivery then goes through a closure built from `target`.
     */
    bool process(ServeCtx& ctx, const uint8_t* data, size_t len, bool udp,
                 const ClientInfo& ci, ReplySink& out,
                 const ReplyTarget& target);
    bool fastPath(ServeCtx& ctx, const uint8_t* data, size_t len, bool udp,
                  const ClientInfo& ci, ReplySink& out);
    /* The rest of process() once fastPath() has declined. */
    bool slowPath(const uint8_t* data, size_t len, bool udp,
                  const ClientInfo& ci, ReplySink& out,
                  const ReplyTarget& target);

    /* A query the fast path may serve: header and question checked,
     * name lowercase [a-z0-9_-] labels in dotted form. For SRV the
     * store key is the name behind the _svc._proto labels. */
    struct FastQuery {
        char name[256];
        uint16_t nlen = 0;
        uint16_t keyOff = 0;  /* SRV: where the service's domain starts */
        uint16_t svcLen = 0;  /* SRV: length of the _svc label */
        bool isSrv = false;
        uint64_t hash = 0;    /* answer-table hash, see answerHash() */

        std::string_view qname() const { return {name, nlen}; }
        std::string_view key() const {
            return {name + keyOff, (size_t)(nlen - keyOff)};
        }
        std::string_view svc() const { return {name, svcLen}; }
        std::string_view proto() const {
            return {name + svcLen + 1, (size_t)(keyOff - svcLen - 2)};
        }
    };
    static bool parseFast(const uint8_t* data, size_t len, FastQuery& q);
    /* policy checks + store lookup + cached-record serve (the fast
     * path proper); memoises what it served when `memo` is set */
    bool fastResolve(ServeCtx& ctx, const FastQuery& q,
                     const uint8_t* data, bool udp, const ClientInfo& ci,
                     ReplySink& out, bool memo);
    /* serve a memoised answer body (answerbody:: layouts) */
    void serveHit(ServeCtx& ctx, const uint8_t* body, bool isSrv,
                  const uint8_t* data, ReplySink& out);
    /* info and debug levels bypass the answer table: their per-query
     * log lines are built from the records, not from the memo */
    bool answersOn() const { return !log_.enabled(LogLevel::Info); }
    void onStoreInvalidate(std::string_view domain);
    static void applyInvalidate(AnswerTable& t, std::string_view domain);

    /* the hit path's metric shards (metrics.hpp), per context */
    struct HitShards {
        CounterShard cntA, cntSrv;
        Histogram::Shard latA, latSrv, sizeA, sizeSrv;
    };
    struct HitFolds {
        CounterFold cntA, cntSrv;
        Histogram::Fold latA, latSrv, sizeA, sizeSrv;
    };
    void countFast(ServeCtx& ctx, bool isSrv, size_t bytes);
    void foldShards();  /* under the serving lock, before a scrape */

    /*
     * Serving context: all that the hit path touches, owned by one
     * thread. The main thread has one (UDP, TCP, and the balancer
     * connections when no pool runs); each pool thread has one.
     *
     * answers - the answer table: memo of fastResolve()'s replies,
     * (qname, qtype) -> finished bytes. Inserted only by fastResolve()
     * run by the owning thread; dropped per name through the store's
     * invalidate hook, wholesale when the store's readiness changes.
     * An SRV entry is hashed on the service's domain (the A entry on
     * the whole name) so both can be found from the domain alone.
     *
     * inbox - invalidations for a pool thread's table, appended by
     * the store hook (main thread, serving lock held), applied by the
     * owner in drainInbox(): after every read() and after every take
     * of the serving lock. An empty string means clear all.
     *
     * Aligned so that two threads' contexts never share a cache line.
     */
    struct alignas(64) ServeCtx {
        AnswerTable answers;
        std::mt19937 rng{std::random_device{}()};
        HitShards hits;
        EventLoop* loop = nullptr;
        std::map<int, std::shared_ptr<BalConn>> balConns;
        /* those of balConns that have rings, polled before the thread
         * sleeps; and what the thread did with them (owner writes) */
        std::vector<BalConn*> shmConns;
        CounterShard shmDoorbells, shmDrains;
        CounterFold shmDoorbellsFold, shmDrainsFold;
        bool pooled = false;

        std::atomic<uint64_t> inboxSeq{0};
        uint64_t inboxSeen = 0;  /* owner only */
        std::mutex inboxMu;
        std::vector<std::string> inbox;

        HitFolds folds;  /* scraping side */

        /* pool threads only */
        std::unique_ptr<EventLoop> ownLoop;
        std::thread thread;
    };
    void postInvalidate(ServeCtx& ctx, std::string_view domain);
    void drainInbox(ServeCtx& ctx) {
        if (ctx.inboxSeq.load(std::memory_order_acquire) != ctx.inboxSeen)
            drainInboxSlow(ctx);
    }
    void drainInboxSlow(ServeCtx& ctx);
    /* a pooled inbox longer than this collapses into one clear-all */
    static constexpr size_t kInboxMax = 4096;

    /* Takes the serving lock for a pool thread (and drains its inbox
     * once it has it); nothing for the main context, whose loop holds
     * the lock already. */
    class ServeLock {
      public:
        ServeLock(DnsServer* s, ServeCtx& ctx);
        ~ServeLock();
        ServeLock(const ServeLock&) = delete;
        ServeLock& operator=(const ServeLock&) = delete;

      private:
        std::mutex* mu_ = nullptr;
    };

    ServeCtx main_;
    std::vector<std::unique_ptr<ServeCtx>> pool_;
    size_t nextPool_ = 0;  /* round-robin cursor of onBalAccept() */
    /* The serving lock: guards everything that is not a ServeCtx's
     * own - store, engine, recursion, logger, the collector's maps,
     * the scratch buffers below, the main loop's tables. With a pool
     * the main loop holds it whenever it dispatches. */
    std::mutex serveMu_;
    void stopPool();

    static uint64_t answerHash(const FastQuery& q) {
        return q.isSrv ? AnswerTable::hashKey(q.name + q.keyOff,
                                              q.nlen - q.keyOff, 33)
                       : AnswerTable::hashKey(q.name, q.nlen, 1);
    }
    /* onBalConn software pipeline: a frame is parsed, hashed and its
     * table slot prefetched kPipeDepth frames before it is served,
     * and its blob prefetched kPipeBlobLead frames before. Measured
     * with bsockblast on the bench tree (profiles/SCALING.md). */
    static constexpr size_t kPipeDepth = 8;
    static constexpr size_t kPipeBlobLead = 4;
    /* "." + dnsDomain and dnsDomain + "." + datacenterName; the engine
     * config is immutable after start, so built once */
    std::string dotDomain_, dcSuffix_;
    std::vector<uint8_t> encScratch_;  /* slow-path encode, frame mode */
    std::vector<uint8_t> tcpOut_;      /* TCP sync reply scratch */
    std::vector<uint32_t> shuffleIdx_;
    std::string logFields_, logScratch_;   /* afterQuery log buffers */

  public:
    /* the store behind the engine (fast-path lookups); set by main */
    void setStore(Store* s);

  private:
    Store* engineStore_ = nullptr;

    void afterQuery(const dns::Message& query, const dns::Message& resp,
                    const QueryResult& qr, const ClientInfo& ci,
                    size_t bytesSent, int64_t startUs,
                    const QueryTimers& tm);

    void tcpFlush(TcpConn* c);
    void sweepIdleTcp();
    /* the sweep's timer callback, which re-arms itself; owned here (a
     * shared_ptr captured by its own closure would never be freed) */
    std::function<void()> sweepTimer_;
    void balFlush(ServeCtx& ctx, BalConn* c);
    void closeTcp(TcpConn* c);
    void closeBal(ServeCtx& ctx, BalConn* c);

    EventLoop* loop_;
    Logger log_;
    ServerOptions opts_;
    Engine* engine_;
    Collector* collector_;
    RecursionIface* recursion_ = nullptr;

    Counter* reqCounter_ = nullptr;
    Counter* shmDoorbellCounter_ = nullptr;
    Counter* shmDrainCounter_ = nullptr;
    Histogram* latHist_ = nullptr;
    Histogram* sizeHist_ = nullptr;

    int udpFd_ = -1;
    int tcpFd_ = -1;
    int balFd_ = -1;
    uint16_t boundPort_ = 0;
    uint64_t servedSlow_ = 0;  /* afterQuery()'s, under the serving lock */

    /* shared_ptr: async recursion replies may outlive the connection
     * (fds get reused; a closed conn object must stay valid until the
     * last in-flight reply fires and observes `closed`). */
    std::map<int, std::shared_ptr<TcpConn>> tcpConns_;

    /* UDP batched I/O arenas. */
    static constexpr int kBatch = 64;
    static constexpr size_t kInBuf = 4096;
    std::vector<uint8_t> rxArena_;
    std::vector<struct mmsghdr> rxHdrs_;
    std::vector<struct iovec> rxIovs_;
    std::vector<struct sockaddr_storage> rxAddrs_;
    std::vector<std::vector<uint8_t>> txBufs_;
    std::vector<struct mmsghdr> txHdrs_;
    std::vector<struct iovec> txIovs_;
    std::vector<struct sockaddr_storage> txAddrs_;
};

void fillClientInfo(ClientInfo& ci, const struct sockaddr_storage& ss,
                    const char* family);

}  // namespace bamd
