#include "server.hpp"

#include <arpa/inet.h>
#include <sched.h>
#include <sys/epoll.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "../balancer/protocol.hpp"
#include "../common/probes.hpp"

namespace bamd {

using namespace dns;

void fillClientInfo(ClientInfo& ci, const struct sockaddr_storage& ss,
                    const char* family) {
    ci.family = family;
    if (ss.ss_family == AF_INET) {
        const auto* sa = (const struct sockaddr_in*)&ss;
        memcpy(ci.addr, &sa->sin_addr, 4);
        ci.ipFamily = 4;
        ci.port = ntohs(sa->sin_port);
    } else if (ss.ss_family == AF_INET6) {
        const auto* sa = (const struct sockaddr_in6*)&ss;
        memcpy(ci.addr, &sa->sin6_addr, 16);
        ci.ipFamily = 6;
        ci.port = ntohs(sa->sin6_port);
    }
}

const char* ClientInfo::address(char (&buf)[48]) const {
    buf[0] = '\0';
    if (ipFamily == 4)
        inet_ntop(AF_INET, addr, buf, sizeof(buf));
    else if (ipFamily == 6)
        inet_ntop(AF_INET6, addr, buf, sizeof(buf));
    return buf;
}

void ReplySink::open(size_t dnsLen) {
    if (vec_ != nullptr) {
        vec_->clear();
        vec_->reserve(dnsLen);
        return;
    }
    uint32_t plen = (uint32_t)(4 + dnsLen);
    uint8_t head[bsock::kHeaderLen + 4];
    head[0] = bsock::kMagic;
    head[1] = bsock::FRAME_REPLY;
    head[2] = (uint8_t)plen;
    head[3] = (uint8_t)(plen >> 8);
    head[4] = (uint8_t)(plen >> 16);
    head[5] = (uint8_t)(plen >> 24);
    head[6] = (uint8_t)reqId_;
    head[7] = (uint8_t)(reqId_ >> 8);
    head[8] = (uint8_t)(reqId_ >> 16);
    head[9] = (uint8_t)(reqId_ >> 24);
    frames_->append((const char*)head, sizeof(head));
    start_ = frames_->size();
}

uint8_t* ReplySink::openWrite(size_t dnsLen) {
    if (vec_ != nullptr) {
        vec_->resize(dnsLen);
        return vec_->data();
    }
    constexpr size_t kHead = bsock::kHeaderLen + 4;
    size_t at = frames_->size();
    frames_->resize(at + kHead + dnsLen);
    uint8_t* h = (uint8_t*)frames_->data() + at;
    uint32_t plen = (uint32_t)(4 + dnsLen);
    h[0] = bsock::kMagic;
    h[1] = bsock::FRAME_REPLY;
    h[2] = (uint8_t)plen;
    h[3] = (uint8_t)(plen >> 8);
    h[4] = (uint8_t)(plen >> 16);
    h[5] = (uint8_t)(plen >> 24);
    h[6] = (uint8_t)reqId_;
    h[7] = (uint8_t)(reqId_ >> 8);
    h[8] = (uint8_t)(reqId_ >> 16);
    h[9] = (uint8_t)(reqId_ >> 24);
    start_ = at + kHead;
    return h + kHead;
}

DnsServer::DnsServer(EventLoop* loop, Logger log, ServerOptions opts,
                     Engine* engine, Collector* collector)
    : loop_(loop), log_(std::move(log)), opts_(std::move(opts)),
      engine_(engine), collector_(collector) {
    main_.loop = loop_;
    collector_->setBeforeExpose([this]() { foldShards(); });
    /* Metric names/help strings match the reference
     * (lib/server.js:31-34, 456-469). */
    reqCounter_ = collector->counter("binder_requests_completed",
                                     "count of Binder requests completed");
    latHist_ = collector->histogram(
        "binder_request_latency_seconds",
        "total time to process Binder requests");
    sizeHist_ = collector->histogram("binder_response_size_bytes",
                                     "size in bytes of Binder responses");
    shmDoorbellCounter_ = collector->counter(
        "binder_balancer_shm_doorbells",
        "doorbells rung to wake a balancer across shared-memory rings");
    shmDrainCounter_ = collector->counter(
        "binder_balancer_shm_drains",
        "takes from a shared-memory query ring that returned data");

    const EngineConfig& cfg = engine_->config();
    if (!cfg.dnsDomain.empty()) dotDomain_ = "." + cfg.dnsDomain;
    dcSuffix_ = cfg.dnsDomain + "." + cfg.datacenterName;

    rxArena_.resize(kBatch * kInBuf);
    rxHdrs_.resize(kBatch);
    rxIovs_.resize(kBatch);
    rxAddrs_.resize(kBatch);
    txBufs_.resize(kBatch);
    txHdrs_.resize(kBatch);
    txIovs_.resize(kBatch);
    txAddrs_.resize(kBatch);
}

DnsServer::~DnsServer() {
    stop();
    collector_->setBeforeExpose(nullptr);
    if (engineStore_ != nullptr) engineStore_->setInvalidateHook(nullptr);
}

/* Bind a socket of the given type to opts_.host:port; v6 when the host
 * looks v6 or is empty (dual-stack any). */
static int bindSocket(const std::string& host, uint16_t port, int type,
                      uint16_t* boundPort) {
    bool v6 = host.empty() || host.find(':') != std::string::npos;
    int fd = socket(v6 ? AF_INET6 : AF_INET,
                    type | SOCK_NONBLOCK | SOCK_CLOEXEC, 0);
    if (fd < 0) return -1;
    int one = 1;
    /* SO_REUSEADDR only for TCP (TIME_WAIT rebinds). On UDP it would
     * allow two processes to bind the same port with packets landing
     * on the older socket — a silent split brain during restarts. */
    if (type == SOCK_STREAM)
        setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    if (type == SOCK_DGRAM) {
        int sz = 4 << 20;
        setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &sz, sizeof(sz));
        setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &sz, sizeof(sz));
    }
    int rv;
    if (v6) {
        int zero = 0;
        setsockopt(fd, IPPROTO_IPV6, IPV6_V6ONLY,
                   host.empty() ? &zero : &one, sizeof(int));
        struct sockaddr_in6 sa {};
        sa.sin6_family = AF_INET6;
        sa.sin6_port = htons(port);
        if (host.empty())
            sa.sin6_addr = in6addr_any;
        else if (inet_pton(AF_INET6, host.c_str(), &sa.sin6_addr) != 1) {
            close(fd);
            return -1;
        }
        rv = bind(fd, (struct sockaddr*)&sa, sizeof(sa));
        if (rv == 0 && boundPort) {
            socklen_t sl = sizeof(sa);
            getsockname(fd, (struct sockaddr*)&sa, &sl);
            *boundPort = ntohs(sa.sin6_port);
        }
    } else {
        struct sockaddr_in sa {};
        sa.sin_family = AF_INET;
        sa.sin_port = htons(port);
        if (inet_pton(AF_INET, host.c_str(), &sa.sin_addr) != 1) {
            close(fd);
            return -1;
        }
        rv = bind(fd, (struct sockaddr*)&sa, sizeof(sa));
        if (rv == 0 && boundPort) {
            socklen_t sl = sizeof(sa);
            getsockname(fd, (struct sockaddr*)&sa, &sl);
            *boundPort = ntohs(sa.sin_port);
        }
    }
    if (rv != 0) {
        close(fd);
        return -1;
    }
    return fd;
}

bool DnsServer::openUdp() {
    udpFd_ = bindSocket(opts_.host, opts_.port, SOCK_DGRAM, &boundPort_);
    if (udpFd_ < 0) {
        log_.error({{"port", Json((int)opts_.port)},
                    {"host", Json(opts_.host)}},
                   "failed to bind UDP socket");
        return false;
    }
    loop_->addFd(udpFd_, EPOLLIN, [this](uint32_t) { onUdpReadable(); });
    log_.info({{"host", Json(opts_.host)}, {"port", Json((int)boundPort_)}},
              "UDP DNS service started");
    return true;
}

bool DnsServer::openTcp() {
    tcpFd_ = bindSocket(opts_.host, boundPort_ ? boundPort_ : opts_.port,
                        SOCK_STREAM, nullptr);
    if (tcpFd_ < 0) {
        log_.error("failed to bind TCP socket");
        return false;
    }
    if (listen(tcpFd_, 512) != 0) {
        log_.error("failed to listen on TCP socket");
        return false;
    }
    loop_->addFd(tcpFd_, EPOLLIN, [this](uint32_t) { onTcpAccept(); });
    log_.info({{"host", Json(opts_.host)}, {"port", Json((int)boundPort_)}},
              "TCP DNS service started");
    return true;
}

bool DnsServer::openBalancer() {
    balFd_ = socket(AF_UNIX, SOCK_STREAM | SOCK_NONBLOCK | SOCK_CLOEXEC, 0);
    if (balFd_ < 0) return false;
    struct sockaddr_un sa {};
    sa.sun_family = AF_UNIX;
    snprintf(sa.sun_path, sizeof(sa.sun_path), "%s",
             opts_.balancerSocket.c_str());
    /* Pre-unlink stale socket (main.js:196-199). */
    unlink(sa.sun_path);
    if (bind(balFd_, (struct sockaddr*)&sa, sizeof(sa)) != 0 ||
        listen(balFd_, 64) != 0) {
        log_.error({{"path", Json(opts_.balancerSocket)}},
                   "failed to bind balancer socket");
        close(balFd_);
        balFd_ = -1;
        return false;
    }
    loop_->addFd(balFd_, EPOLLIN, [this](uint32_t) { onBalAccept(); });
    log_.info({{"path", Json(opts_.balancerSocket)}},
              "Balancer service started");
    return true;
}

/* whole CPUs this process may use: cgroup quota (v2, then v1), capped
 * by the affinity mask; the affinity mask alone when there is no quota */
static int usableCpus() {
    int cpus = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0)
        cpus = CPU_COUNT(&set);
    if (cpus < 1) cpus = 1;
    long long quota = -1, period = 0;
    {
        std::ifstream f("/sys/fs/cgroup/cpu.max");
        std::string q;
        if (f >> q >> period && q != "max") quota = atoll(q.c_str());
    }
    if (quota <= 0) {
        std::ifstream fq("/sys/fs/cgroup/cpu/cpu.cfs_quota_us");
        std::ifstream fp("/sys/fs/cgroup/cpu/cpu.cfs_period_us");
        if (!(fq >> quota) || !(fp >> period)) quota = -1;
    }
    if (quota > 0 && period > 0) {
        long long q = quota / period;
        if (q < 1) q = 1;
        if (q < cpus) cpus = (int)q;
    }
    return cpus;
}

int defaultServeThreads() {
    int t = usableCpus() / 4;
    return t < 1 ? 1 : (t > 4 ? 4 : t);
}

bool DnsServer::pooled() const {
    return opts_.serveThreads >= 2 && !opts_.balancerSocket.empty() &&
           answersOn();
}

bool DnsServer::start() {
    if (!openUdp() || !openTcp()) return false;
    if (!opts_.balancerSocket.empty() && !openBalancer()) return false;
    if (!opts_.balancerSocket.empty() && opts_.balancerShm)
        loop_->setBeforePark(
            [this](bool park) { return balBeforePark(main_, park); });
    if (pooled()) {
        /* from here on the main loop dispatches under the serving lock */
        loop_->setDispatchLock(&serveMu_);
        for (int i = 0; i < opts_.serveThreads; ++i) {
            auto ctx = std::make_unique<ServeCtx>();
            ctx->pooled = true;
            ctx->ownLoop = std::make_unique<EventLoop>();
            ctx->loop = ctx->ownLoop.get();
            EventLoop* l = ctx->loop;
            if (opts_.balancerShm) {
                ServeCtx* cp = ctx.get();
                l->setBeforePark([this, cp](bool park) {
                    return balBeforePark(*cp, park);
                });
            }
            ctx->thread = std::thread([l]() { l->run(); });
            pool_.push_back(std::move(ctx));
        }
        log_.info({{"threads", Json((int64_t)opts_.serveThreads)}},
                  "balancer connections served by a thread pool");
    }
    /* idle TCP sweep: DNS-over-TCP clients that neither query nor
     * close get reaped after 60s (resource protection; the balancer
     * socket is exempt — it is a long-lived peer) */
    sweepTimer_ = [this]() {
        sweepIdleTcp();
        loop_->addTimer(10000, sweepTimer_);
    };
    loop_->addTimer(10000, sweepTimer_);
    return true;
}

void DnsServer::sweepIdleTcp() {
    int64_t cutoff = monotonicMillis() - 60000;
    std::vector<TcpConn*> idle;
    for (auto& [fd, c] : tcpConns_)
        if (c->lastActivityMs < cutoff && c->pendingAsync == 0)
            idle.push_back(c.get());
    for (TcpConn* c : idle) closeTcp(c);
}

/* Stop and join the pool. Not to be called with the serving lock held:
 * a pool thread may be waiting for it. */
void DnsServer::stopPool() {
    for (auto& ctx : pool_) {
        EventLoop* l = ctx->loop;
        /* stopped from inside, so a thread that has not reached run()
         * yet still sees it */
        l->postFromThread([l]() { l->stop(); });
    }
    for (auto& ctx : pool_)
        if (ctx->thread.joinable()) ctx->thread.join();
    /* the threads are gone: their connections are ours to close */
    for (auto& ctx : pool_) {
        for (auto& [fd, c] : ctx->balConns) {
            c->closed = true;
            close(fd);
        }
        ctx->balConns.clear();
    }
}

void DnsServer::stop() {
    stopPool();
    auto closeFd = [this](int& fd) {
        if (fd >= 0) {
            loop_->delFd(fd);
            close(fd);
            fd = -1;
        }
    };
    closeFd(udpFd_);
    closeFd(tcpFd_);
    closeFd(balFd_);
    if (!opts_.balancerSocket.empty()) unlink(opts_.balancerSocket.c_str());
    for (auto& [fd, c] : tcpConns_) {
        loop_->delFd(fd);
        close(fd);
    }
    tcpConns_.clear();
    for (auto& [fd, c] : main_.balConns) {
        loop_->delFd(fd);
        close(fd);
    }
    main_.balConns.clear();
}

uint64_t DnsServer::queriesServed() const {
    uint64_t n = servedSlow_;
    auto add = [&n](const ServeCtx& c) {
        n += c.hits.cntA.read() + c.hits.cntSrv.read();
    };
    add(main_);
    for (const auto& c : pool_) add(*c);
    return n;
}

/* ---------------- query pipeline ---------------- */

static inline int64_t nowUs() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (int64_t)ts.tv_sec * 1000000 + ts.tv_nsec / 1000;
}

/*
 * Fast path: all-lowercase A/IN query with no EDNS for a host-like or
 * database node => serve a prebuilt wire response (header id/rd
 * patched). Falls back to the full path for anything else, including
 * whenever info-level logging is on (the per-query log line needs the
 * decoded message). Policy checks mirror Engine::resolve exactly for
 * the subset they cover; anything non-trivial bails to slow.
 */
/* append one big-endian u16 */
static inline void putU16be(std::vector<uint8_t>& v, uint16_t x) {
    v.push_back((uint8_t)(x >> 8));
    v.push_back((uint8_t)x);
}
static inline void putU32be(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back((uint8_t)(x >> 24));
    v.push_back((uint8_t)(x >> 16));
    v.push_back((uint8_t)(x >> 8));
    v.push_back((uint8_t)x);
}
static void putName(std::vector<uint8_t>& v, std::string_view name) {
    size_t start = 0;
    while (start <= name.size() && !name.empty()) {
        size_t dot = name.find('.', start);
        size_t end = dot == std::string_view::npos ? name.size() : dot;
        v.push_back((uint8_t)(end - start));
        v.insert(v.end(), name.begin() + start, name.begin() + end);
        if (dot == std::string_view::npos) break;
        start = dot + 1;
    }
    v.push_back(0);
}

/* Build the permutable service-response cache (see store.hpp). Returns
 * a cache marked unusable when any member needs slow-path handling
 * (invalid member record => SERVFAIL-partial semantics). */
static void buildServiceCache(const StoreNode* node,
                              std::string_view key,
                              const std::string& dotdd) {
    const CompiledRecord& rec = node->rec();
    /* log-name compaction, afterQuery parity (stripSuffix + "...") */
    auto strippedTarget = [&dotdd](const std::string& t) {
        if (!dotdd.empty() && t.size() > dotdd.size() &&
            t.compare(t.size() - dotdd.size(), dotdd.size(), dotdd) == 0)
            return t.substr(0, t.size() - dotdd.size()) + "...";
        return t;
    };
    /* the only SRV qname this cache can serve is the registered one
     * (mismatches fall back to the slow path before cache use) */
    std::string srvQname =
        rec.srvce + "." + rec.proto + "." + std::string(key);
    auto cache = std::make_unique<CompiledRecord::ServiceCache>();
    cache->usable = true;
    uint32_t svcTtl = rec.ttl;

    for (const StoreNode* kid : node->children()) {
        const CompiledRecord& kr = kid->rec();
        if (!kr.hasData || !recTypeServesUnderService(kr.type)) continue;
        if (!kr.valid) {
            cache->usable = false;  /* slow path owns SERVFAIL-partial */
            break;
        }
        if (kr.address.empty()) continue;
        CompiledRecord::ServiceCache::Member m;
        uint32_t rttl = kr.memberTtlOverride.value_or(svcTtl);
        uint32_t aTtl = rttl < svcTtl ? rttl : svcTtl;
        std::string target = kid->name() + "." + std::string(key);
        uint8_t a4[4];
        if (inet_pton(AF_INET, kr.address.c_str(), a4) != 1) {
            cache->usable = false;
            break;
        }
        /* plain-A segment: name=ptr(12), A IN, min-ttl, addr */
        m.aSeg.push_back(0xC0);
        m.aSeg.push_back(0x0C);
        putU16be(m.aSeg, 1);
        putU16be(m.aSeg, 1);
        putU32be(m.aSeg, aTtl);
        putU16be(m.aSeg, 4);
        m.aSeg.insert(m.aSeg.end(), a4, a4 + 4);
        jsonEscape("A " + kr.address, m.aLog);
        /* SRV segment(s): one per port */
        std::vector<uint16_t> ports = kr.ports;
        if (ports.empty())
            ports.push_back(rec.hasDefaultPort ? rec.defaultPort : 0);
        std::string logTarget = strippedTarget(target);
        for (uint16_t p : ports) {
            m.srvSeg.push_back(0xC0);
            m.srvSeg.push_back(0x0C);
            putU16be(m.srvSeg, 33);
            putU16be(m.srvSeg, 1);
            putU32be(m.srvSeg, svcTtl);
            putU16be(m.srvSeg, (uint16_t)(6 + target.size() + 2));
            putU16be(m.srvSeg, 0);   /* priority */
            putU16be(m.srvSeg, 10);  /* weight (Record::SRV default) */
            putU16be(m.srvSeg, p);
            putName(m.srvSeg, target);
            cache->srvAnCount++;
            if (!m.srvLog.empty()) m.srvLog += ',';
            jsonEscape("SRV " + logTarget + ":" + std::to_string(p),
                       m.srvLog);
        }
        /* additional A: full (uncompressed) target name */
        putName(m.addSeg, target);
        putU16be(m.addSeg, 1);
        putU16be(m.addSeg, 1);
        putU32be(m.addSeg, rttl);
        putU16be(m.addSeg, 4);
        m.addSeg.insert(m.addSeg.end(), a4, a4 + 4);
        jsonEscape(logTarget + " A " + kr.address, m.addLog);
        cache->members.push_back(std::move(m));
    }

    auto buildHead = [&](std::vector<uint8_t>& head,
                         std::string_view qname, uint16_t qtype,
                         uint16_t an, uint16_t ar) {
        head.reserve(16 + qname.size() + 6);
        putU16be(head, 0);        /* id patched per query */
        head.push_back(0x84);     /* QR|AA */
        head.push_back(0x00);
        putU16be(head, 1);
        putU16be(head, an);
        putU16be(head, 0);
        putU16be(head, ar);
        putName(head, qname);
        putU16be(head, qtype);
        putU16be(head, 1);
    };
    buildHead(cache->headA, key, 1, (uint16_t)cache->members.size(), 0);
    buildHead(cache->headSrv, srvQname, 33, cache->srvAnCount,
              (uint16_t)cache->members.size());
    cache->totalA = cache->headA.size();
    cache->totalSrv = cache->headSrv.size();
    for (const auto& m : cache->members) {
        cache->totalA += m.aSeg.size();
        cache->totalSrv += m.srvSeg.size() + m.addSeg.size();
    }
    rec.svc = std::move(cache);
}

void DnsServer::setStore(Store* s) {
    if (engineStore_ != nullptr) engineStore_->setInvalidateHook(nullptr);
    engineStore_ = s;
    main_.answers.clear();
    if (s != nullptr)
        s->setInvalidateHook(
            [this](std::string_view d) { onStoreInvalidate(d); });
}

/* The store's hook: main thread, serving lock held when a pool runs.
 * Returns only once every pool thread's inbox holds the invalidation,
 * which is what makes a mutation visible everywhere before any fresh
 * answer can be built from it (docs/ARCHITECTURE.md). */
void DnsServer::onStoreInvalidate(std::string_view domain) {
    applyInvalidate(main_.answers, domain);
    for (auto& ctx : pool_) postInvalidate(*ctx, domain);
}

void DnsServer::applyInvalidate(AnswerTable& answers,
                                std::string_view domain) {
    if (domain.empty()) {  /* readiness changed: forget everything */
        if (answers.size() != 0) answers.clear();
        return;
    }
    if (answers.size() == 0 || domain.size() > AnswerTable::kMaxKey)
        return;
    answers.remove(AnswerTable::hashKey(domain.data(), domain.size(), 1),
                   1, domain.data(), domain.size());
    /* the service's SRV entry, _svc._proto.<domain>, hashed on domain */
    answers.removeSuffix(
        AnswerTable::hashKey(domain.data(), domain.size(), 33), 33,
        domain.data(), domain.size());
}

void DnsServer::postInvalidate(ServeCtx& ctx, std::string_view domain) {
    std::lock_guard<std::mutex> g(ctx.inboxMu);
    bool clearPending = ctx.inbox.size() == 1 && ctx.inbox[0].empty();
    if (domain.empty() || ctx.inbox.size() >= kInboxMax) {
        /* an idle thread never drains: bound what it is owed */
        ctx.inbox.clear();
        ctx.inbox.emplace_back();
    } else if (!clearPending) {
        ctx.inbox.emplace_back(domain);
    }
    ctx.inboxSeq.store(
        ctx.inboxSeq.load(std::memory_order_relaxed) + 1,
        std::memory_order_release);
}

void DnsServer::drainInboxSlow(ServeCtx& ctx) {
    std::vector<std::string> todo;
    {
        std::lock_guard<std::mutex> g(ctx.inboxMu);
        todo.swap(ctx.inbox);
        ctx.inboxSeen = ctx.inboxSeq.load(std::memory_order_relaxed);
    }
    for (const std::string& d : todo) applyInvalidate(ctx.answers, d);
}

DnsServer::ServeLock::ServeLock(DnsServer* s, ServeCtx& ctx) {
    if (!ctx.pooled) return;
    mu_ = &s->serveMu_;
    mu_->lock();
    s->drainInbox(ctx);
}

DnsServer::ServeLock::~ServeLock() {
    if (mu_ != nullptr) mu_->unlock();
}

void DnsServer::countFast(ServeCtx& ctx, bool isSrv, size_t bytes) {
    HitShards& h = ctx.hits;
    (isSrv ? h.cntSrv : h.cntA).bump();
    latHist_->observeShard(isSrv ? h.latSrv : h.latA, 1e-6);  /* sub-us */
    sizeHist_->observeShard(isSrv ? h.sizeSrv : h.sizeA, (double)bytes);
}

void DnsServer::foldShards() {
    static const std::string kA = "type=\"A\"";
    static const std::string kSrv = "type=\"SRV\"";
    auto fold = [this](ServeCtx& c) {
        reqCounter_->fold(kA, c.hits.cntA, c.folds.cntA);
        reqCounter_->fold(kSrv, c.hits.cntSrv, c.folds.cntSrv);
        latHist_->fold(kA, c.hits.latA, c.folds.latA);
        latHist_->fold(kSrv, c.hits.latSrv, c.folds.latSrv);
        sizeHist_->fold(kA, c.hits.sizeA, c.folds.sizeA);
        sizeHist_->fold(kSrv, c.hits.sizeSrv, c.folds.sizeSrv);
    };
    fold(main_);
    for (auto& c : pool_) fold(*c);
    auto foldShm = [this](ServeCtx& c) {
        shmDoorbellCounter_->fold("", c.shmDoorbells, c.shmDoorbellsFold);
        shmDrainCounter_->fold("", c.shmDrains, c.shmDrainsFold);
    };
    foldShm(main_);
    for (auto& c : pool_) foldShm(*c);
    /* the first fast-path reply of either type brings both series */
    if (queriesServed() != servedSlow_) {
        reqCounter_->slot(kA);
        reqCounter_->slot(kSrv);
        latHist_->seriesRef(kA);
        latHist_->seriesRef(kSrv);
        sizeHist_->seriesRef(kA);
        sizeHist_->seriesRef(kSrv);
    }
}

/* Write a memoised answer: copy (or permute) straight into the out
 * buffer, patch id and RD, count it exactly as fastResolve() does. */
void DnsServer::serveHit(ServeCtx& ctx, const uint8_t* body, bool isSrv,
                         const uint8_t* data, ReplySink& out) {
    const size_t total = answerbody::total(body);
    uint8_t* w = out.openWrite(total);
    if (answerbody::kind(body) == answerbody::kWire) {
        memcpy(w, answerbody::wireReply(body), total);
    } else {
        /* Fisher-Yates member order (server.js:40-53, 361): the same
         * draws from ctx.rng, in the same order, as fastResolve() */
        size_t n = answerbody::serviceMembers(body);
        uint8_t order[answerbody::kMaxMembers];
        for (size_t i = 0; i < n; ++i) order[i] = (uint8_t)i;
        for (size_t i = n; i > 1;) {
            --i;
            size_t j = ctx.rng() % (i + 1);
            std::swap(order[i], order[j]);
        }
        answerbody::serviceAssemble(body, order, w);
    }
    w[0] = data[0];
    w[1] = data[1];
    w[2] = (uint8_t)(w[2] | (data[2] & 0x01));

    countFast(ctx, isSrv, total);
    BAMD_PROBE2("op-req-done", total, 0);
}

bool DnsServer::fastPath(ServeCtx& ctx, const uint8_t* data, size_t len,
                         bool udp, const ClientInfo& ci, ReplySink& out) {
    /* debug/trace want the slow path's extra detail; info-level
     * per-query lines are emitted from cached fragments */
    if (log_.enabled(LogLevel::Debug)) return false;
    FastQuery q;
    if (!parseFast(data, len, q)) return false;
    bool memo = answersOn();
    if (memo) {
        q.hash = answerHash(q);
        const uint8_t* body = ctx.answers.find(q.hash, q.isSrv ? 33 : 1,
                                               q.name, q.nlen);
        if (body != nullptr) {
            serveHit(ctx, body, q.isSrv, data, out);
            return true;
        }
    }
    return fastResolve(ctx, q, data, udp, ci, out, memo);
}

bool DnsServer::parseFast(const uint8_t* data, size_t len, FastQuery& q) {
    if (len < 17 || len > 300) return false;
    /* flags: QR/opcode/AA/TC clear, RD free; byte 3 must be zero */
    if ((data[2] & 0xFE) != 0 || data[3] != 0) return false;
    /* counts: qd=1, an=ns=ar=0 */
    if (data[4] != 0 || data[5] != 1 || data[6] | data[7] ||
        data[8] | data[9] || data[10] | data[11])
        return false;

    char* name = q.name;
    size_t nlen = 0;
    size_t pos = 12;
    while (true) {
        if (pos >= len) return false;
        uint8_t l = data[pos++];
        if (l == 0) break;
        if ((l & 0xC0) != 0 || pos + l > len) return false;
        if (nlen + l + 1 > sizeof(q.name)) return false;
        if (nlen > 0) name[nlen++] = '.';
        for (uint8_t i = 0; i < l; ++i) {
            char c = (char)data[pos + i];
            bool ok = (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') ||
                      c == '_' || c == '-';
            if (!ok) return false;  // uppercase/odd chars: slow path
            name[nlen++] = c;
        }
        pos += l;
    }
    if (pos + 4 > len) return false;
    bool isSrv;
    if (data[pos] == 0 && data[pos + 1] == 1)
        isSrv = false;
    else if (data[pos] == 0 && data[pos + 1] == 33)
        isSrv = true;
    else
        return false;
    if (data[pos + 2] != 0 || data[pos + 3] != 1)  /* class IN */
        return false;

    q.nlen = (uint16_t)nlen;
    q.isSrv = isSrv;
    q.keyOff = 0;
    q.svcLen = 0;
    std::string_view key(name, nlen);
    if (isSrv) {
        /* strip _svc._proto (engine srvShape rules); mismatches fall
         * back to the slow path */
        size_t d1 = key.find('.');
        if (d1 == std::string_view::npos || d1 == 0 || key[0] != '_')
            return false;
        size_t d2 = key.find('.', d1 + 1);
        if (d2 == std::string_view::npos || key[d1 + 1] != '_')
            return false;
        std::string_view l1 = key.substr(0, d1);
        std::string_view l2 = key.substr(d1 + 1, d2 - d1 - 1);
        if (l1.find('_', 1) != std::string_view::npos ||
            l2.find('_', 1) != std::string_view::npos)
            return false;
        q.svcLen = (uint16_t)d1;
        q.keyOff = (uint16_t)(d2 + 1);
        if (q.keyOff >= nlen) return false;
    }
    return true;
}

bool DnsServer::fastResolve(ServeCtx& ctx, const FastQuery& q,
                            const uint8_t* data, bool udp,
                            const ClientInfo& ci, ReplySink& out,
                            bool memo) {
    const bool isSrv = q.isSrv;
    const char* name = q.name;
    const size_t nlen = q.nlen;
    const std::string_view key = q.key();
    std::string_view srvSvc, srvProto;
    if (isSrv) {
        srvSvc = q.svc();
        srvProto = q.proto();
    }
    const EngineConfig& cfg = engine_->config();
    if (!cfg.dnsDomain.empty()) {
        /* must be a strict subdomain of dnsDomain, not doubled */
        size_t dl = cfg.dnsDomain.size();
        if (key.size() <= dl + 1) return false;
        if (key[key.size() - dl - 1] != '.' ||
            key.substr(key.size() - dl) != cfg.dnsDomain)
            return false;
        std::string_view stripped = key.substr(0, key.size() - dl - 1);
        auto endsWith = [](std::string_view s, std::string_view suf) {
            return s.size() >= suf.size() &&
                   s.substr(s.size() - suf.size()) == suf;
        };
        if (endsWith(stripped, cfg.dnsDomain)) return false;
        if (endsWith(stripped, dcSuffix_)) return false;
    }

    const Store* store = engineStore_;
    if (store == nullptr || !store->ready()) return false;
    const StoreNode* node = store->lookupView(key);
    if (node == nullptr) return false;
    const CompiledRecord& rec = node->rec();
    if (!rec.valid) return false;

    /* shared prefix of the fast-path info log line */
    auto logOpen = [&](const char* qtype) -> std::string& {
        std::string& f = logFields_;
        f.clear();
        char nb[96], ab[48];
        uint16_t qid = (uint16_t)(((uint16_t)data[0] << 8) | data[1]);
        snprintf(nb, sizeof(nb),
                 ",\"req_id\":%u,\"client\":\"%s\",\"port\":\"%u/%s\"",
                 (unsigned)qid, ci.address(ab), (unsigned)ci.port,
                 ci.family);
        f += nb;
        f += ",\"query\":{\"name\":\"";
        f.append(name, nlen);  /* fast path admits [a-z0-9_.-] only */
        f += "\",\"type\":\"";
        f += qtype;
        f += "\"},\"edns\":false,\"rcode\":\"NOERROR\",\"answers\":[";
        return f;
    };
    static const char kLogClose[] =
        "],\"latency\":0,\"timers\":{\"parse_us\":0,\"resolve_us\":0,"
        "\"encode_us\":0}";

    if (rec.type == RecType::Service) {
        if (isSrv &&
            (srvSvc != rec.srvce || srvProto != rec.proto))
            return false;  /* slow path: NXDOMAIN */
        if (!rec.svc) buildServiceCache(node, key, dotDomain_);
        const CompiledRecord::ServiceCache& c = *rec.svc;
        if (!c.usable) return false;

        /* size check against the UDP limit; oversize => slow path
         * (which truncates with TC exactly as before) */
        size_t total = isSrv ? c.totalSrv : c.totalA;
        if (udp && total > 512) return false;

        /* Fisher-Yates member order (server.js:40-53, 361) */
        size_t n = c.members.size();
        if (n > shuffleIdx_.size()) shuffleIdx_.resize(n);
        for (size_t i = 0; i < n; ++i) shuffleIdx_[i] = (uint32_t)i;
        for (size_t i = n; i > 1;) {
            --i;
            size_t j = ctx.rng() % (i + 1);
            std::swap(shuffleIdx_[i], shuffleIdx_[j]);
        }

        out.open(total);
        const auto& head = isSrv ? c.headSrv : c.headA;
        out.append(head.data(), head.size());
        if (isSrv) {
            for (size_t i = 0; i < n; ++i) {
                const auto& m = c.members[shuffleIdx_[i]];
                out.append(m.srvSeg.data(), m.srvSeg.size());
            }
            for (size_t i = 0; i < n; ++i) {
                const auto& m = c.members[shuffleIdx_[i]];
                out.append(m.addSeg.data(), m.addSeg.size());
            }
        } else {
            for (size_t i = 0; i < n; ++i) {
                const auto& m = c.members[shuffleIdx_[i]];
                out.append(m.aSeg.data(), m.aSeg.size());
            }
        }
        uint8_t* w = out.dns();
        w[0] = data[0];
        w[1] = data[1];
        w[2] = (uint8_t)(w[2] | (data[2] & 0x01));

        /* per-context shards, no string-keyed lookup: those were 12%
         * of binderd user CPU at saturation (gprof, profiles/) */
        countFast(ctx, isSrv, total);
        if (log_.enabled(LogLevel::Info)) {
            std::string& f = logOpen(isSrv ? "SRV" : "A");
            bool lfirst = true;
            for (size_t i = 0; i < n; ++i) {
                const auto& m = c.members[shuffleIdx_[i]];
                const std::string& frag = isSrv ? m.srvLog : m.aLog;
                if (frag.empty()) continue;
                if (!lfirst) f += ',';
                lfirst = false;
                f += frag;
            }
            f += "],\"additional\":[";
            if (isSrv) {
                lfirst = true;
                for (size_t i = 0; i < n; ++i) {
                    const auto& m = c.members[shuffleIdx_[i]];
                    if (m.addLog.empty()) continue;
                    if (!lfirst) f += ',';
                    lfirst = false;
                    f += m.addLog;
                }
            }
            f += kLogClose;
            log_.logRaw(LogLevel::Info, "DNS query", f);
        }
        BAMD_PROBE2("op-req-done", total, 0);
        /* memoise: head + segments laid end to end in one blob.
         * Replies past 512 bytes are left out, so a hit never has to
         * ask which transport the query came over. */
        if (memo && total <= 512 && n <= answerbody::kMaxMembers) {
            answerbody::Seg s1[answerbody::kMaxMembers];
            answerbody::Seg s2[answerbody::kMaxMembers];
            size_t segBytes = 0;
            for (size_t i = 0; i < n; ++i) {
                const auto& m = c.members[i];
                if (isSrv) {
                    s1[i] = {m.srvSeg.data(), m.srvSeg.size()};
                    s2[i] = {m.addSeg.data(), m.addSeg.size()};
                } else {
                    s1[i] = {m.aSeg.data(), m.aSeg.size()};
                    s2[i] = {nullptr, 0};
                }
                segBytes += s1[i].n + s2[i].n;
            }
            uint8_t* body = ctx.answers.insert(
                q.hash, (uint8_t)(isSrv ? 33 : 1), name, nlen,
                answerbody::serviceBodyLen(n, head.size(), segBytes));
            if (body != nullptr)
                answerbody::serviceFill(body, n, head.data(), head.size(),
                                        s1, s2);
        }
        return true;
    }

    if (isSrv) return false;  /* SRV on non-service: slow (NODATA+SOA) */
    if (rec.address.empty()) return false;
    bool hostish = recTypeIsHostLike(rec.type) ||
                   rec.type == RecType::Database;
    if (!hostish) return false;

    if (rec.wireA.empty()) {
        /* build: header + question + answer (name = ptr to offset 12) */
        dns::Message m;
        m.header.qr = true;
        m.header.aa = true;
        dns::Question q;
        q.name = std::string(key);
        m.questions.push_back(std::move(q));
        m.answers.push_back(
            dns::Record::A(std::string(key), rec.address, rec.ttl));
        rec.wireA = m.encode(0);
        rec.logA.clear();
        jsonEscape("A " + m.answers[0].addrString(), rec.logA);
    }
    const size_t wlen = rec.wireA.size();
    out.open(wlen);
    out.append(rec.wireA.data(), wlen);
    uint8_t* w = out.dns();
    w[0] = data[0];  /* id */
    w[1] = data[1];
    w[2] = (uint8_t)(w[2] | (data[2] & 0x01));  /* echo RD */

    countFast(ctx, false, wlen);
    if (log_.enabled(LogLevel::Info)) {
        std::string& f = logOpen("A");
        f += rec.logA;
        f += "],\"additional\":[";
        f += kLogClose;
        log_.logRaw(LogLevel::Info, "DNS query", f);
    }
    BAMD_PROBE2("op-req-done", wlen, 0);
    if (memo && wlen <= 512) {
        uint8_t* body = ctx.answers.insert(q.hash, 1, name, nlen,
                                           answerbody::wireBodyLen(wlen));
        if (body != nullptr)
            answerbody::wireFill(body, rec.wireA.data(), wlen);
    }
    return true;
}

/* REPLY frame assembled in one header append + one payload append
 * (the string-builder form did ~6 appends + a double copy per reply
 * — gprof showed _M_append at 7.5% of binderd user CPU). */
static void appendReplyFrame(std::string& out, uint32_t reqId,
                             const uint8_t* dns, size_t dnsLen) {
    uint32_t plen = (uint32_t)(4 + dnsLen);
    uint8_t head[bsock::kHeaderLen + 4];
    head[0] = bsock::kMagic;
    head[1] = bsock::FRAME_REPLY;
    head[2] = (uint8_t)plen;
    head[3] = (uint8_t)(plen >> 8);
    head[4] = (uint8_t)(plen >> 16);
    head[5] = (uint8_t)(plen >> 24);
    head[6] = (uint8_t)reqId;
    head[7] = (uint8_t)(reqId >> 8);
    head[8] = (uint8_t)(reqId >> 16);
    head[9] = (uint8_t)(reqId >> 24);
    out.append((const char*)head, sizeof(head));
    out.append((const char*)dns, dnsLen);
}

std::function<void(std::vector<uint8_t>)> DnsServer::makeAsyncReply(
    const ReplyTarget& t) {
    switch (t.kind) {
    case ReplyTarget::Kind::Udp: {
        struct sockaddr_storage srcCopy = *t.src;
        socklen_t srcLen = t.srcLen;
        return [this, srcCopy, srcLen](std::vector<uint8_t> wire) {
            sendto(udpFd_, wire.data(), wire.size(), 0,
                   (const struct sockaddr*)&srcCopy, srcLen);
        };
    }
    case ReplyTarget::Kind::Tcp: {
        /* shared_ptr: the reply may outlive the connection */
        std::shared_ptr<TcpConn> self = t.tcp->shared_from_this();
        return [this, self](std::vector<uint8_t> wire) {
            if (self->closed) return;
            self->out.push_back((char)(wire.size() >> 8));
            self->out.push_back((char)wire.size());
            self->out.append((const char*)wire.data(), wire.size());
            tcpFlush(self.get());
        };
    }
    case ReplyTarget::Kind::Bal:
        break;
    }
    /* Only the connection's owning thread touches its buffers. The
     * reply is written here when that is the thread we are on (no
     * pool, or recursion answered synchronously); otherwise it is
     * posted to the owner's loop. The shared_ptr keeps the connection
     * object alive either way and `closed` is checked over there. */
    std::shared_ptr<BalConn> self = t.bal->shared_from_this();
    uint32_t reqId = t.reqId;
    return [this, self, reqId](std::vector<uint8_t> wire) {
        ServeCtx* ctx = self->ctx;
        auto deliver = [this, self, ctx, reqId](
                           const std::vector<uint8_t>& w) {
            if (self->closed) return;
            appendReplyFrame(self->link.out, reqId, w.data(), w.size());
            balFlush(*ctx, self.get());
        };
        if (ctx->loop->inLoopThread()) {
            deliver(wire);
            return;
        }
        ctx->loop->postFromThread(
            [deliver, wire = std::move(wire)]() { deliver(wire); });
    };
}

bool DnsServer::process(ServeCtx& ctx, const uint8_t* data, size_t len,
                        bool udp, const ClientInfo& ci, ReplySink& out,
                        const ReplyTarget& target) {
    BAMD_PROBE2("op-req-start", len, (int)udp);
    if (fastPath(ctx, data, len, udp, ci, out)) return true;
    return slowPath(data, len, udp, ci, out, target);
}

bool DnsServer::slowPath(const uint8_t* data, size_t len, bool udp,
                         const ClientInfo& ci, ReplySink& out,
                         const ReplyTarget& target) {
    int64_t start = nowUs();
    auto parsed = Message::decode(data, len);
    if (!parsed) return true;  // drop malformed (out empty)
    if (parsed->header.qr) return true;  // ignore responses
    int64_t tParse = nowUs();

    Message& query = *parsed;
    /* TCP responses must fit the u16 length prefix; oversize answers
     * degrade to TC like UDP rather than corrupting the stream */
    size_t limit = 65535;
    bool hasEdns = query.edns() != nullptr;
    if (udp) {
        limit = 512;
        if (hasEdns) {
            uint16_t adv = query.edns()->rclass;
            limit = adv < 512 ? 512 : (adv > 4096 ? 4096 : adv);
        }
    }

    Message resp;
    QueryResult qr = engine_->handle(query, resp);
    int64_t tResolve = nowUs();

    if (qr.action == QueryResult::Action::Recurse &&
        recursion_ != nullptr) {
        /* Hand off: recursion fills resp then we encode+deliver. */
        auto respHeap = std::make_shared<Message>(std::move(resp));
        auto queryHeap = std::make_shared<Message>(std::move(query));
        ClientInfo ciCopy = ci;
        size_t lim = limit;
        bool edns = hasEdns;
        auto asyncReply = makeAsyncReply(target);
        recursion_->resolve(
            *queryHeap, *respHeap,
            [this, respHeap, queryHeap, ciCopy, lim, edns, start,
             asyncReply = std::move(asyncReply), qr]() {
                if (edns)
                    respHeap->additionals.push_back(Record::OPT(1400));
                auto wire = respHeap->encode(lim);
                size_t n = wire.size();
                asyncReply(std::move(wire));
                afterQuery(*queryHeap, *respHeap, qr, ciCopy, n, start,
                           QueryTimers{});
            });
        return false;
    }

    if (hasEdns) resp.additionals.push_back(Record::OPT(1400));
    size_t sent;
    if (std::vector<uint8_t>* v = out.vec()) {
        resp.encodeInto(*v, limit);
        sent = v->size();
    } else {
        resp.encodeInto(encScratch_, limit);
        sent = encScratch_.size();
        if (sent != 0) {
            out.open(sent);
            out.append(encScratch_.data(), sent);
        }
    }
    QueryTimers tm;
    tm.parseUs = tParse - start;
    tm.resolveUs = tResolve - tParse;
    tm.encodeUs = nowUs() - tResolve;
    afterQuery(query, resp, qr, ci, sent, start, tm);
    return true;
}

void DnsServer::afterQuery(const Message& query, const Message& resp,
                           const QueryResult& qr, const ClientInfo& ci,
                           size_t bytesSent, int64_t startUs,
                           const QueryTimers& tm) {
    ++servedSlow_;
    int64_t latUs = nowUs() - startUs;
    int64_t lat = latUs / 1000;
    BAMD_PROBE2("op-req-done", bytesSent, (int)resp.header.rcode);

    const char* qtype = query.questions.empty()
                            ? nullptr
                            : typeName(query.questions[0].qtype);
    if (qtype != nullptr) {
        std::string label = std::string("type=\"") + qtype + "\"";
        reqCounter_->increment(label);
        latHist_->observe(label, (double)latUs / 1e6);
        sizeHist_->observe(label, (double)bytesSent);
    }

    /* Per-query log line (server.js:537-590); warn when >1s.
     * Built through Logger::logRaw with direct appends into reused
     * buffers: the JsonObject DOM version of this block was ~35% of
     * binderd CPU at info level (25 jsonEscape calls + a std::map
     * build/teardown per query, measured with gprof). */
    LogLevel lv = lat > 1000 ? LogLevel::Warn : LogLevel::Info;
    if (!log_.enabled(lv)) return;

    const std::string& dd = engine_->config().dnsDomain;
    const std::string& dotdd = dotDomain_;
    std::string& f = logFields_;
    std::string& s = logScratch_;
    f.clear();
    char nbuf[96], abuf[48];
    snprintf(nbuf, sizeof(nbuf),
             ",\"req_id\":%u,\"client\":\"%s\",\"port\":\"%u/%s\"",
             (unsigned)query.header.id, ci.address(abuf), (unsigned)ci.port,
             ci.family);
    f += nbuf;
    f += ",\"query\":{";
    if (!query.questions.empty()) {
        f += "\"name\":";
        jsonEscape(query.questions[0].name, f);
        f += ",\"type\":\"";
        f += typeName(query.questions[0].qtype);
        f += "\"";
    }
    f += query.edns() != nullptr ? "},\"edns\":true,\"rcode\":\""
                                 : "},\"edns\":false,\"rcode\":\"";
    f += rcodeName(resp.header.rcode);
    f += "\",\"answers\":[";
    bool first = true;
    for (const auto& r : resp.answers) {
        s.clear();
        s += typeName(r.type);
        if (r.type == TYPE_SRV) {
            s += ' ';
            s += dd.empty() ? r.target : stripSuffix(dotdd, r.target);
            s += ':';
            s += std::to_string(r.port);
        } else if (r.type == TYPE_A || r.type == TYPE_AAAA) {
            s += ' ';
            s += r.addrString();
        } else if (r.type == TYPE_PTR) {
            s += ' ';
            s += r.target;
        }
        if (!first) f += ',';
        first = false;
        jsonEscape(s, f);
    }
    f += "],\"additional\":[";
    first = true;
    for (const auto& r : resp.additionals) {
        if (r.type == TYPE_OPT) continue;  // OPT filtered from logs
        s.clear();
        s += dd.empty() ? r.name : stripSuffix(dotdd, r.name);
        s += ' ';
        s += typeName(r.type);
        s += ' ';
        s += r.addrString();
        if (!first) f += ',';
        first = false;
        jsonEscape(s, f);
    }
    /* phase timers, the query._times equivalent (server.js:476-483) */
    snprintf(nbuf, sizeof(nbuf),
             "],\"latency\":%lld,\"timers\":{\"parse_us\":%lld,"
             "\"resolve_us\":%lld,\"encode_us\":%lld}",
             (long long)lat, (long long)tm.parseUs,
             (long long)tm.resolveUs, (long long)tm.encodeUs);
    f += nbuf;
    log_.logRaw(lv, "DNS query", f);
}

/* ---------------- UDP ---------------- */

void DnsServer::onUdpReadable() {
    while (true) {
        for (int i = 0; i < kBatch; ++i) {
            rxIovs_[i].iov_base = rxArena_.data() + (size_t)i * kInBuf;
            rxIovs_[i].iov_len = kInBuf;
            memset(&rxHdrs_[i], 0, sizeof(rxHdrs_[i]));
            rxHdrs_[i].msg_hdr.msg_iov = &rxIovs_[i];
            rxHdrs_[i].msg_hdr.msg_iovlen = 1;
            rxHdrs_[i].msg_hdr.msg_name = &rxAddrs_[i];
            rxHdrs_[i].msg_hdr.msg_namelen = sizeof(rxAddrs_[i]);
        }
        int n = recvmmsg(udpFd_, rxHdrs_.data(), kBatch, 0, nullptr);
        if (n <= 0) return;  // EAGAIN or error: wait for next wakeup

        int nOut = 0;
        for (int i = 0; i < n; ++i) {
            ClientInfo ci;
            fillClientInfo(ci, rxAddrs_[i], "udp");
            std::vector<uint8_t>& out = txBufs_[nOut];
            out.clear();
            socklen_t srcLen = rxHdrs_[i].msg_hdr.msg_namelen;
            ReplySink sink(&out);
            ReplyTarget target{ReplyTarget::Kind::Udp};
            target.src = &rxAddrs_[i];  /* copied if it goes async */
            target.srcLen = srcLen;
            bool sync = process(
                main_, rxArena_.data() + (size_t)i * kInBuf, rxHdrs_[i].msg_len,
                true, ci, sink, target);
            if (sync && !out.empty()) {
                txAddrs_[nOut] = rxAddrs_[i];
                txIovs_[nOut].iov_base = out.data();
                txIovs_[nOut].iov_len = out.size();
                memset(&txHdrs_[nOut], 0, sizeof(txHdrs_[nOut]));
                txHdrs_[nOut].msg_hdr.msg_iov = &txIovs_[nOut];
                txHdrs_[nOut].msg_hdr.msg_iovlen = 1;
                txHdrs_[nOut].msg_hdr.msg_name = &txAddrs_[nOut];
                txHdrs_[nOut].msg_hdr.msg_namelen = srcLen;
                ++nOut;
            }
        }
        int sent = 0;
        while (sent < nOut) {
            int rv = sendmmsg(udpFd_, txHdrs_.data() + sent, nOut - sent, 0);
            if (rv <= 0) break;  // EAGAIN: drop the rest (UDP best-effort)
            sent += rv;
        }
        if (n < kBatch) return;  // drained
    }
}

/* ---------------- TCP ---------------- */

void DnsServer::onTcpAccept() {
    while (true) {
        struct sockaddr_storage ss;
        socklen_t sl = sizeof(ss);
        int fd = accept4(tcpFd_, (struct sockaddr*)&ss, &sl,
                         SOCK_NONBLOCK | SOCK_CLOEXEC);
        if (fd < 0) return;
        if (tcpConns_.size() >= 4096) {  /* fd-exhaustion guard */
            close(fd);
            continue;
        }
        auto conn = std::make_shared<TcpConn>();
        conn->fd = fd;
        conn->lastActivityMs = monotonicMillis();
        fillClientInfo(conn->ci, ss, "tcp");
        TcpConn* raw = conn.get();
        tcpConns_[fd] = std::move(conn);
        loop_->addFd(fd, EPOLLIN,
                     [this, raw](uint32_t ev) { onTcpConn(raw, ev); });
    }
}

void DnsServer::closeTcp(TcpConn* c) {
    if (c->closed) return;
    c->closed = true;
    loop_->delFd(c->fd);
    close(c->fd);
    /* shared_ptr keeps the object alive for in-flight async replies */
    tcpConns_.erase(c->fd);
}

void DnsServer::tcpFlush(TcpConn* c) {
    while (!c->out.empty()) {
        ssize_t nw = write(c->fd, c->out.data(), c->out.size());
        if (nw > 0) {
            c->out.erase(0, (size_t)nw);
            continue;
        }
        if (nw < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) {
            if (!c->writeBlocked) {
                c->writeBlocked = true;
                loop_->modFd(c->fd, EPOLLIN | EPOLLOUT);
            }
            return;
        }
        closeTcp(c);
        return;
    }
    if (c->writeBlocked) {
        c->writeBlocked = false;
        loop_->modFd(c->fd, EPOLLIN);
    }
}

void DnsServer::onTcpConn(TcpConn* c, uint32_t events) {
    /* keep-alive: flush paths may close+erase the connection */
    std::shared_ptr<TcpConn> keep = tcpConns_[c->fd];
    if (events & (EPOLLHUP | EPOLLERR)) {
        closeTcp(c);
        return;
    }
    if (events & EPOLLOUT) tcpFlush(c);
    if (c->closed || !(events & EPOLLIN)) return;

    c->lastActivityMs = monotonicMillis();
    char buf[8192];
    while (true) {
        ssize_t nr = read(c->fd, buf, sizeof(buf));
        if (nr > 0) {
            c->in.append(buf, (size_t)nr);
            if (c->in.size() > (1 << 20)) {  // runaway client
                closeTcp(c);
                return;
            }
            continue;
        }
        if (nr < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) break;
        closeTcp(c);
        return;
    }

    /* DNS-over-TCP framing: u16be length prefix per message. */
    while (c->in.size() >= 2) {
        size_t mlen = ((size_t)(uint8_t)c->in[0] << 8) |
                      (uint8_t)c->in[1];
        if (c->in.size() < 2 + mlen) break;
        std::vector<uint8_t>& out = tcpOut_;
        out.clear();
        ReplySink sink(&out);
        ReplyTarget target{ReplyTarget::Kind::Tcp};
        target.tcp = c;
        bool sync = process(
            main_, (const uint8_t*)c->in.data() + 2, mlen, false, c->ci, sink,
            target);
        if (sync) {
            if (!out.empty()) {
                c->out.push_back((char)(out.size() >> 8));
                c->out.push_back((char)out.size());
                c->out.append((const char*)out.data(), out.size());
            }
        }
        c->in.erase(0, 2 + mlen);
    }
    tcpFlush(c);
}

/* ---------------- balancer socket ---------------- */

void DnsServer::onBalAccept() {
    while (true) {
        int fd = accept4(balFd_, nullptr, nullptr,
                         SOCK_NONBLOCK | SOCK_CLOEXEC);
        if (fd < 0) return;
        int sz = 4 << 20;
        setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &sz, sizeof(sz));
        setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &sz, sizeof(sz));
        if (pool_.empty()) {
            adoptBal(main_, fd);
            continue;
        }
        /* round-robin over the pool; the connection object is made by
         * the thread that will own it */
        ServeCtx* ctx = pool_[nextPool_++ % pool_.size()].get();
        ctx->loop->postFromThread([this, ctx, fd]() { adoptBal(*ctx, fd); });
    }
}

/* on ctx's thread */
void DnsServer::adoptBal(ServeCtx& ctx, int fd) {
    auto conn = std::make_shared<BalConn>();
    conn->ctx = &ctx;
    conn->link.fd = fd;
    BalConn* raw = conn.get();
    ctx.balConns[fd] = std::move(conn);
    ServeCtx* cp = &ctx;
    ctx.loop->addFd(fd, EPOLLIN, [this, cp, raw](uint32_t ev) {
        onBalConn(*cp, raw, ev);
    });
}

DnsServer::BalConn::~BalConn() {
    for (int i = 0; i < nRxFds; ++i) close(rxFds[i]);
}

void DnsServer::dropRxFds(BalConn* c) {
    for (int i = 0; i < c->nRxFds; ++i) close(c->rxFds[i]);
    c->nRxFds = 0;
}

void DnsServer::closeBal(ServeCtx& ctx, BalConn* c) {
    if (c->closed) return;
    c->closed = true;
    ctx.loop->delFd(c->link.fd);
    close(c->link.fd);
    if (c->link.shmReady) {
        ctx.loop->delFd(c->link.shm.wakeMe);
        auto& v = ctx.shmConns;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
    }
    c->link.dropRings();
    dropRxFds(c);
    ctx.balConns.erase(c->link.fd);
}

/* SHM_OFFER, at its place in the batch. Accepting means: map the region
 * the balancer made, check that it is what the offer says, register our
 * doorbell, and queue SHM_OK as the last reply bytes of the stream.
 * Declining is silent: the descriptors are closed and the balancer,
 * never hearing SHM_OK, stays on the stream. */
void DnsServer::acceptShm(ServeCtx& ctx, BalConn* c, const uint8_t* p,
                          size_t len) {
    shm::Link& rings = c->link.shm;
    bool ok = opts_.balancerShm && !c->link.shmReady &&
              c->nRxFds == bsock::kShmOfferFds &&
              len >= bsock::kShmOfferLen &&
              bsock::getU32(p) == shm::kVersion &&
              bsock::getU32(p + 8) == shm::kDataOff &&
              rings.region.attach(c->rxFds[0], bsock::getU32(p + 4)) &&
              setNonBlocking(c->rxFds[1]) && setNonBlocking(c->rxFds[2]);
    if (ok) {
        BalConn* raw = c;
        ServeCtx* cp = &ctx;
        try {
            ctx.loop->addFd(c->rxFds[1], EPOLLIN | EPOLLET,
                            [this, cp, raw](uint32_t) {
                                onBalBell(*cp, raw);
                            });
        } catch (const std::runtime_error&) {
            ok = false;  /* not something epoll can wait on */
        }
    }
    if (!ok) {
        log_.debug("shared-memory offer declined");
        rings.region.reset();
        dropRxFds(c);
        return;
    }
    close(c->rxFds[0]);  /* mapped */
    rings.wakeMe = c->rxFds[1];
    rings.wakePeer = c->rxFds[2];
    c->nRxFds = 0;
    rings.attachEnds(false);
    c->link.shmReady = true;
    ctx.shmConns.push_back(c);
    c->link.queueSwitch(bsock::FRAME_SHM_OK);
}

/* what a connection's link leaves to its owner (bsocklink.hpp) */
struct DnsServer::LinkSink {
    ServeCtx& ctx;
    int fd;
    void armWrite() { ctx.loop->modFd(fd, EPOLLIN | EPOLLOUT); }
    void disarmWrite() { ctx.loop->modFd(fd, EPOLLIN); }
    void doorbell() { ctx.shmDoorbells.bump(); }
    void drained() { ctx.shmDrains.bump(); }
};

void DnsServer::balFlush(ServeCtx& ctx, BalConn* c) {
    if (c->closed) return;
    BsockLink::Flush r = c->link.flush(LinkSink{ctx, c->link.fd});
    if (r == BsockLink::Flush::StreamError || r == BsockLink::Flush::RingBad)
        closeBal(ctx, c);
}

/* the balancer's doorbell: queries in the ring, or room in the reply
 * ring we were waiting for */
void DnsServer::onBalBell(ServeCtx& ctx, BalConn* c) {
    std::shared_ptr<BalConn> keep = c->shared_from_this();
    if (c->closed) return;
    if (c->link.bellWantsFlush()) balFlush(ctx, c);
    if (!c->closed && c->link.rxShm) serveBal(ctx, c, true);
}

/* The hook of ctx's loop (loop.hpp). Every round: serve what the query
 * rings hold - under load there is something, and nobody had to wake us
 * for it. Before a real sleep: tell the balancers, and look once more. */
EventLoop::Park DnsServer::balBeforePark(ServeCtx& ctx, bool park) {
    auto& v = ctx.shmConns;
    EventLoop::Park out = EventLoop::Park::NoRings;
    for (size_t i = 0; i < v.size();) {
        BalConn* c = v[i];
        EventLoop::Park s = c->link.parkState<EventLoop::Park>(park);
        if (s == EventLoop::Park::Work && !park) {
            std::shared_ptr<BalConn> keep = c->shared_from_this();
            serveBal(ctx, c, true);
        }
        if (s > out) out = s;
        if (i < v.size() && v[i] == c) ++i;  /* else it was closed */
    }
    return out;
}

void DnsServer::onBalConn(ServeCtx& ctx, BalConn* c, uint32_t events) {
    std::shared_ptr<BalConn> keep = ctx.balConns[c->link.fd];
    if (events & (EPOLLHUP | EPOLLERR)) {
        closeBal(ctx, c);
        return;
    }
    if (events & EPOLLOUT) balFlush(ctx, c);
    if (c->closed || !(events & EPOLLIN)) return;
    if (c->link.rxShm) {
        if (!c->link.streamStillOpen()) closeBal(ctx, c);
        return;
    }
    serveBal(ctx, c, false);
}

/* Take a batch of bytes off the socket, or off the query ring once the
 * connection has moved there, and serve the frames in it. The caller
 * holds a reference to c. */
void DnsServer::serveBal(ServeCtx& ctx, BalConn* c, bool fromRing) {
    /* Bounded batch per epoll event: the GSO-era balancer can queue
     * megabytes behind one connection, and draining it all here would
     * process tens of thousands of queries (10+ ms) while the other
     * workers' connections wait - measured as bimodal multi-ms p99 at
     * N=1. Level-triggered epoll re-fires for the remainder, so
     * capping the read keeps per-event latency bounded and service
     * across connections fair.
     *
     * read() lands in the tail of the receive buffer (no bounce
     * buffer). A short read means the socket is drained for now, so
     * the EAGAIN round trip is skipped too; EOF shows on the next
     * event. */
    constexpr size_t kMaxReadPerEvent = 128 * 1024;
    size_t got = 0;
    if (fromRing) {
        /* the same quota, copied to the same place; a ring drained
         * short of it is empty, and whatever is left is found by the
         * poll before this thread sleeps */
        got = c->link.drainRing(kMaxReadPerEvent, kMaxReadPerEvent,
                                LinkSink{ctx, c->link.fd});
        if (got == BsockLink::kRingBad) {
            closeBal(ctx, c);
            return;
        }
        if (got == 0) return;
    }
    while (!fromRing && got < kMaxReadPerEvent) {
        size_t want = kMaxReadPerEvent - got;
        /* recvmsg, not read: a SHM_OFFER brings descriptors, and they
         * arrive with the read that returns its first byte */
        struct iovec iov = {c->link.in.tail(want), want};
        alignas(struct cmsghdr) char
            cbuf[CMSG_SPACE(sizeof(int) * bsock::kShmOfferFds)];
        struct msghdr mh {};
        mh.msg_iov = &iov;
        mh.msg_iovlen = 1;
        mh.msg_control = cbuf;
        mh.msg_controllen = sizeof(cbuf);
        const bool mayOffer = opts_.balancerShm && !c->link.shmReady;
        ssize_t nr = mayOffer ? recvmsg(c->link.fd, &mh, MSG_CMSG_CLOEXEC)
                              : read(c->link.fd, iov.iov_base, want);
        if (mayOffer && nr >= 0 && mh.msg_controllen != 0) {
            for (struct cmsghdr* cm = CMSG_FIRSTHDR(&mh); cm != nullptr;
                 cm = CMSG_NXTHDR(&mh, cm)) {
                if (cm->cmsg_level != SOL_SOCKET ||
                    cm->cmsg_type != SCM_RIGHTS)
                    continue;
                /* only the latest set is kept (what did not fit in
                 * cbuf the kernel has closed already) */
                dropRxFds(c);
                size_t n = (cm->cmsg_len - CMSG_LEN(0)) / sizeof(int);
                for (size_t i = 0; i < n; ++i) {
                    int fd;
                    memcpy(&fd, CMSG_DATA(cm) + i * sizeof(int),
                           sizeof(int));
                    if (c->nRxFds < bsock::kShmOfferFds)
                        c->rxFds[c->nRxFds++] = fd;
                    else
                        close(fd);
                }
            }
        }
        if (nr > 0) {
            c->link.in.commit((size_t)nr);
            got += (size_t)nr;
            if ((size_t)nr < want) break;
            continue;
        }
        if (nr < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) break;
        closeBal(ctx, c);
        return;
    }
    /* invalidations posted before these bytes were read apply before
     * any of them is answered */
    drainInbox(ctx);
    AnswerTable& answers = ctx.answers;

    /* Frames are parsed by advancing the buffer's cursor; the partial
     * frame left at the end moves to the front once, below. */
    /*
     * The frames of this read are served through a short software
     * pipeline: the per-query cost at saturation is cache misses on
     * the answer table, and the addresses are known as soon as a
     * frame's name has been parsed. Frame i+kPipeDepth is parsed,
     * hashed and its slot prefetched; frame i+kPipeBlobLead has its
     * slot read and its blob prefetched; frame i is then served from
     * lines already on their way. Frames are served strictly in
     * arrival order, so replies leave in the order they do without
     * the pipeline; PINGs, queries the fast path does not take and
     * table misses go through the usual code at their place in that
     * order. With the table bypassed (info/debug logging) nothing is
     * parsed ahead.
     */
    enum : uint8_t { kSkip, kPing, kQuery, kFastQuery, kShmOffer, kShmGo };
    struct PipeFrame {
        uint8_t kind;
        const uint8_t* raw;  /* kShmOffer: payload, in c->link.in */
        uint32_t rawLen;
        bsock::QueryFrame qf;
        FastQuery q;
        uint32_t off;   /* probe() result, good while gen matches */
        uint64_t gen;
    };
    static_assert((kPipeDepth & (kPipeDepth - 1)) == 0 &&
                  kPipeBlobLead >= 1 && kPipeBlobLead <= kPipeDepth);
    PipeFrame ring[kPipeDepth];
    const bool memo = answersOn() && engineStore_ != nullptr;
    bsock::FrameStatus st = bsock::FrameStatus::Ok;
    size_t fetched = 0, probed = 0, served = 0;
    bool sawGo = false;
    while (true) {
        /* stage 1: take frames off the buffer, up to the lookahead */
        while (st == bsock::FrameStatus::Ok &&
               fetched - served < kPipeDepth) {
            bsock::FrameView fr;
            st = bsock::nextFrame(c->link.in, fr);
            if (st != bsock::FrameStatus::Ok) break;
            PipeFrame& p = ring[fetched++ & (kPipeDepth - 1)];
            p.off = AnswerTable::kNone;
            if (fr.type == bsock::FRAME_PING) {
                p.kind = kPing;
            } else if (fr.type == bsock::FRAME_QUERY &&
                       bsock::parseQuery(fr.payload, fr.plen, p.qf)) {
                p.kind = kQuery;
                if (memo && parseFast(p.qf.dns, p.qf.dnsLen, p.q)) {
                    p.kind = kFastQuery;
                    p.q.hash = answerHash(p.q);
                    answers.prefetchSlot(p.q.hash);
                }
            } else if (fr.type == bsock::FRAME_SHM_OFFER) {
                p.kind = kShmOffer;
                p.raw = fr.payload;
                p.rawLen = fr.plen;
            } else if (fr.type == bsock::FRAME_SHM_GO) {
                p.kind = kShmGo;
            } else {
                p.kind = kSkip;
            }
        }
        if (served == fetched) break;
        /* stage 2: slot -> blob address, blob lines requested */
        while (probed < fetched && probed - served < kPipeBlobLead) {
            PipeFrame& p = ring[probed++ & (kPipeDepth - 1)];
            if (p.kind != kFastQuery) continue;
            uint32_t blen = 0;
            p.off = answers.probe(p.q.hash, &blen);
            p.gen = answers.generation();
            if (p.off != AnswerTable::kNone)
                answers.prefetchBlob(p.off, blen);
        }
        /* stage 3: serve the oldest frame */
        PipeFrame& p = ring[served++ & (kPipeDepth - 1)];
        if (p.kind == kPing) {
            bsock::appendFrame(c->link.out, bsock::FRAME_PONG, "");
            continue;
        }
        if (p.kind == kSkip) continue;
        if (p.kind == kShmOffer) {
            acceptShm(ctx, c, p.raw, p.rawLen);
            continue;
        }
        if (p.kind == kShmGo) {
            /* the balancer's queries continue in the ring (looked at
             * before this thread sleeps, at the latest) */
            if (c->link.shmReady && !c->link.rxShm)
                c->link.rxShm = sawGo = true;
            continue;
        }
        const bsock::QueryFrame& qf = p.qf;
        ReplySink sink(&c->link.out, qf.reqId);
        const bool udp = qf.proto == 0;
        if (p.kind == kFastQuery) {
            const uint8_t qt = p.q.isSrv ? 33 : 1;
            const uint8_t* body = nullptr;
            if (p.off != AnswerTable::kNone &&
                p.gen == answers.generation())
                body = answers.at(p.off, qt, p.q.name, p.q.nlen);
            if (body == nullptr)  /* not probed, stale, or a collision */
                body = answers.find(p.q.hash, qt, p.q.name, p.q.nlen);
            if (body != nullptr) {
                BAMD_PROBE2("op-req-start", qf.dnsLen, (int)udp);
                serveHit(ctx, body, p.q.isSrv, qf.dns, sink);
                continue;
            }
        }
        ClientInfo ci;
        ci.family = qf.proto == 1 ? "tcp" : "udp";
        ci.port = qf.srcPort;
        ci.ipFamily = qf.family == 4 ? 4 : 6;
        memcpy(ci.addr, qf.srcAddr, sizeof(ci.addr));
        ReplyTarget target{ReplyTarget::Kind::Bal};
        target.bal = c;
        target.reqId = qf.reqId;
        /* not a hit: the shared code, under the serving lock when this
         * is a pool thread (which drains its inbox first, so what it
         * memoises is no older than what it has been told to drop) */
        ServeLock lock(this, ctx);
        if (p.kind == kFastQuery) {
            /* table miss: the fast path proper, from the parse at hand */
            BAMD_PROBE2("op-req-start", qf.dnsLen, (int)udp);
            if (!fastResolve(ctx, p.q, qf.dns, udp, ci, sink, true))
                slowPath(qf.dns, qf.dnsLen, udp, ci, sink, target);
        } else {
            process(ctx, qf.dns, qf.dnsLen, udp, ci, sink, target);
        }
    }
    /* SHM_GO ends the stream: a partial frame behind it can never be
     * completed */
    if (st == bsock::FrameStatus::Bad ||
        (sawGo && c->link.in.size() != 0)) {
        closeBal(ctx, c);
        return;
    }
    /* a synchronous recursion reply may have hit a write error */
    if (c->closed) return;
    c->link.in.compact();
    balFlush(ctx, c);
}

}  // namespace bamd
