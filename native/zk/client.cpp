#include "client.hpp"

#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/epoll.h>
#include <sys/random.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cstring>
#include <utility>

namespace bamd::zk {

ZkClient::ZkClient(EventLoop* loop, Logger log, ZkConfig cfg)
    : loop_(loop),
      log_(log.child({{"component", Json("ZkClient")}})),
      cfg_(std::move(cfg)) {
    servers_ = cfg_.servers;
    if (servers_.empty()) servers_.push_back({cfg_.host, cfg_.port});
    if (cfg_.shuffle && servers_.size() > 1) {
        /* Fisher-Yates, drawn once per process from getrandom(2) so that
         * every client of one process sees one order */
        static const uint64_t kSeed = []() {
            uint64_t s = 0;
            if (getrandom(&s, sizeof(s), 0) != (ssize_t)sizeof(s))
                s = (uint64_t)wallMillis() ^ ((uint64_t)getpid() << 32);
            return s;
        }();
        uint64_t x = kSeed | 1;
        for (size_t i = servers_.size() - 1; i > 0; i--) {
            x ^= x << 13;  /* xorshift64 */
            x ^= x >> 7;
            x ^= x << 17;
            std::swap(servers_[i], servers_[x % (i + 1)]);
        }
    }
    for (const ZkServer& s : servers_) names_.push_back(serverName(s));
}

ZkClient::~ZkClient() { close(); }

JsonObject ZkClient::serverField() const {
    return {{"server", Json(names_[cur_])}};
}

int ZkClient::connectDeadlineMs() const {
    if (cfg_.connectTimeoutMs > 0) return cfg_.connectTimeoutMs;
    int t = cfg_.sessionTimeoutMs / (int)servers_.size();
    return t > 0 ? t : 1;
}

void ZkClient::start() {
    closing_ = false;
    if (state_ == State::Closed) connectStart();
}

void ZkClient::close() {
    closing_ = true;
    if (reconnectTimer_) {
        loop_->cancelTimer(reconnectTimer_);
        reconnectTimer_ = 0;
    }
    if (state_ == State::Connected) {
        /* best-effort CloseSession */
        Writer w;
        w.i32(nextXid());
        w.i32(OP_CLOSE);
        sendPacket(w.buf);
        flush();
    }
    teardown();
    state_ = State::Closed;
}

void ZkClient::teardown() {
    if (pingTimer_) {
        loop_->cancelTimer(pingTimer_);
        pingTimer_ = 0;
    }
    if (connectTimer_) {
        loop_->cancelTimer(connectTimer_);
        connectTimer_ = 0;
    }
    if (fd_ >= 0) {
        loop_->delFd(fd_);
        ::close(fd_);
        fd_ = -1;
    }
    inBuf_.clear();
    outBuf_.clear();
    writeBlocked_ = false;
    failAllPending();
}

void ZkClient::failAllPending() {
    auto pend = std::move(pending_);
    pending_.clear();
    static const Stat kStat;
    for (auto& [xid, p] : pend) {
        if (p.dataCb) p.dataCb(ZCONNECTIONLOSS, "", kStat);
        if (p.childrenCb) p.childrenCb(ZCONNECTIONLOSS, {});
        if (p.statCb) p.statCb(ZCONNECTIONLOSS, kStat);
        if (p.stringCb) p.stringCb(ZCONNECTIONLOSS, "");
        if (p.voidCb) p.voidCb(ZCONNECTIONLOSS);
    }
}

void ZkClient::scheduleReconnect(int delayMs) {
    if (closing_ || reconnectTimer_) return;
    state_ = State::Closed;
    reconnects_++;
    reconnectTimer_ = loop_->addTimer(delayMs, [this]() {
        reconnectTimer_ = 0;
        if (!closing_) connectStart();
    });
}

/* The current server failed us: move to the next and try it at once, or,
 * when a whole pass over the list has failed, after reconnectDelayMs.
 * The session credentials stay as they are. The next attempt starts from
 * a zero-delay timer, not from here, so that no caller finds a new
 * connection under its feet. */
void ZkClient::serverFailed() {
    teardown();
    if (closing_ || reconnectTimer_) return;
    if (failureCb_) failureCb_(names_[cur_]);
    cur_ = (cur_ + 1) % servers_.size();
    int delay = 0;
    if (++failures_ >= servers_.size()) {
        failures_ = 0;
        delay = cfg_.reconnectDelayMs;
    }
    scheduleReconnect(delay);
}

void ZkClient::connectStart() {
    teardown();
    state_ = State::Connecting;
    const ZkServer& srv = servers_[cur_];
    fd_ = socket(AF_INET, SOCK_STREAM | SOCK_NONBLOCK | SOCK_CLOEXEC, 0);
    if (fd_ < 0) {
        serverFailed();
        return;
    }
    int one = 1;
    setsockopt(fd_, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
    struct sockaddr_in sa {};
    sa.sin_family = AF_INET;
    sa.sin_port = htons(srv.port);
    if (inet_pton(AF_INET, srv.host.c_str(), &sa.sin_addr) != 1) {
        /* resolve hostnames (ZK_HOST may not be an IP); blocking, but
         * only on the (re)connect path */
        struct addrinfo hints {};
        hints.ai_family = AF_INET;
        hints.ai_socktype = SOCK_STREAM;
        struct addrinfo* res = nullptr;
        int rc = getaddrinfo(srv.host.c_str(), nullptr, &hints, &res);
        if (rc != 0 || res == nullptr) {
            log_.error({{"host", Json(srv.host)},
                        {"server", Json(names_[cur_])}},
                       "cannot resolve ZK host");
            if (res) freeaddrinfo(res);
            serverFailed();
            return;
        }
        sa.sin_addr = ((struct sockaddr_in*)res->ai_addr)->sin_addr;
        freeaddrinfo(res);
    }
    int rv = ::connect(fd_, (struct sockaddr*)&sa, sizeof(sa));
    if (rv != 0 && errno != EINPROGRESS) {
        log_.debug(serverField(), "ZK connect failed; retrying");
        serverFailed();
        return;
    }
    loop_->addFd(fd_, EPOLLIN | EPOLLOUT,
                 [this](uint32_t ev) { onSockEvent(ev); });
    /* one deadline over TCP connect + ConnectResponse: a server that
     * accepts and stays silent, or a black-holed address, must not park
     * the client (the ping timer only runs once Connected) */
    int deadline = connectDeadlineMs();
    connectTimer_ = loop_->addTimer(deadline, [this, deadline]() {
        connectTimer_ = 0;
        if (state_ != State::Connecting && state_ != State::Handshaking)
            return;
        log_.warn({{"server", Json(names_[cur_])},
                   {"timeoutMs", Json((int64_t)deadline)}},
                  "ZK connect deadline expired");
        serverFailed();
    });
}

void ZkClient::sendHandshake() {
    state_ = State::Handshaking;
    Writer w;
    w.i32(0);                       // protocolVersion
    w.i64(lastZxid_);               // lastZxidSeen
    w.i32(cfg_.sessionTimeoutMs);   // timeOut
    w.i64(sessionId_);              // resume previous session if any
    if (passwd_.empty()) passwd_.assign(16, '\0');
    w.buffer(passwd_);
    w.boolean(false);               // readOnly
    sendPacket(w.buf);
    flush();
}

void ZkClient::onSockEvent(uint32_t events) {
    if (state_ == State::Connecting) {
        int err = 0;
        socklen_t elen = sizeof(err);
        getsockopt(fd_, SOL_SOCKET, SO_ERROR, &err, &elen);
        if (err != 0 || (events & (EPOLLERR | EPOLLHUP))) {
            log_.debug(serverField(), "ZK connect failed; retrying");
            serverFailed();
            return;
        }
        loop_->modFd(fd_, EPOLLIN);
        sendHandshake();
        return;
    }
    if (events & (EPOLLERR | EPOLLHUP)) {
        log_.warn(serverField(), "ZK connection lost");
        serverFailed();
        return;
    }
    if (events & EPOLLOUT) {
        writeBlocked_ = false;
        loop_->modFd(fd_, EPOLLIN);
        flush();
    }
    if (events & EPOLLIN) onReadable();
}

void ZkClient::onReadable() {
    char buf[65536];
    while (fd_ >= 0) {
        ssize_t nr = read(fd_, buf, sizeof(buf));
        if (nr > 0) {
            inBuf_.append(buf, (size_t)nr);
            continue;
        }
        if (nr < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) break;
        log_.warn(serverField(), "ZK connection closed by server");
        serverFailed();
        return;
    }
    lastPacketRecvMs_ = monotonicMillis();

    while (inBuf_.size() >= 4) {
        uint32_t plen = ((uint32_t)(uint8_t)inBuf_[0] << 24) |
                        ((uint32_t)(uint8_t)inBuf_[1] << 16) |
                        ((uint32_t)(uint8_t)inBuf_[2] << 8) |
                        (uint32_t)(uint8_t)inBuf_[3];
        if (plen > (64u << 20)) {
            log_.error(serverField(),
                       "ZK packet too large; dropping connection");
            serverFailed();
            return;
        }
        if (inBuf_.size() < 4 + plen) break;
        /* copy out: callbacks may mutate inBuf_ by issuing requests */
        std::string pkt = inBuf_.substr(4, plen);
        inBuf_.erase(0, 4 + plen);
        if (state_ == State::Handshaking)
            onConnectResponse((const uint8_t*)pkt.data(), pkt.size());
        else
            onPacket((const uint8_t*)pkt.data(), pkt.size());
        if (fd_ < 0) return;  // teardown happened in callback
    }
}

void ZkClient::onConnectResponse(const uint8_t* data, size_t len) {
    Reader r{data, len};
    int32_t proto = r.i32();
    int32_t timeout = r.i32();
    int64_t sid = r.i64();
    std::string pw = r.str();
    /* A real server always answers protocolVersion 0 with a sane
     * negotiated timeout; anything else is a broken/hostile peer, not
     * a session verdict — reconnect WITHOUT discarding the session so
     * a later healthy server can still resume it. */
    if (!r.ok || proto != 0 || timeout > 600000) {
        log_.warn(serverField(),
                  "malformed ZK connect response; reconnecting");
        serverFailed();
        return;
    }
    if (timeout <= 0 || sid == 0) {
        /* session expired (server refuses resume): start a fresh one.
         * This is a healthy server's verdict, not a failure: stay on it */
        log_.warn(serverField(),
                  "ZK session expired; creating a new session");
        sessionId_ = 0;
        passwd_.clear();
        lastZxid_ = 0;
        failures_ = 0;
        teardown();
        scheduleReconnect(cfg_.reconnectDelayMs);
        return;
    }
    bool isNew = sid != sessionId_;
    sessionId_ = sid;
    passwd_ = pw;
    negotiatedTimeout_ = timeout;
    state_ = State::Connected;
    sessions_++;
    if (connectTimer_) {
        loop_->cancelTimer(connectTimer_);
        connectTimer_ = 0;
    }
    /* a lost established connection is the first failure of its pass */
    failures_ = 0;
    if (lastSessionServer_ >= 0 && (size_t)lastSessionServer_ != cur_)
        switches_++;
    lastSessionServer_ = (int)cur_;
    log_.info({{"sessionId", Json((int64_t)sid)},
               {"timeout", Json((int64_t)timeout)},
               {"new", Json(isNew)},
               {"server", Json(names_[cur_])}},
              "ZK session established");
    armPingTimer();
    /* 'session' fires on every usable (re)connection — the mirror above
     * resyncs, which also covers resumed sessions with missed events. */
    if (sessionCb_) sessionCb_();
}

void ZkClient::armPingTimer() {
    if (pingTimer_) loop_->cancelTimer(pingTimer_);
    int t = negotiatedTimeout_ > 0 ? negotiatedTimeout_
                                   : cfg_.sessionTimeoutMs;
    pingTimer_ = loop_->addTimer(t / 3, [this]() {
        pingTimer_ = 0;
        if (state_ != State::Connected) return;
        int64_t silent = monotonicMillis() - lastPacketRecvMs_;
        int tt = negotiatedTimeout_ > 0 ? negotiatedTimeout_
                                        : cfg_.sessionTimeoutMs;
        if (silent > tt) {
            log_.warn(serverField(),
                      "ZK server unresponsive; reconnecting");
            serverFailed();
            return;
        }
        sendPing();
        armPingTimer();
    });
}

void ZkClient::sendPing() {
    Writer w;
    w.i32(XID_PING);
    w.i32(OP_PING);
    sendPacket(w.buf);
    flush();
}

void ZkClient::sendPacket(const std::string& body) {
    uint32_t n = (uint32_t)body.size();
    char b[4] = {(char)(n >> 24), (char)(n >> 16), (char)(n >> 8), (char)n};
    outBuf_.append(b, 4);
    outBuf_ += body;
}

void ZkClient::flush() {
    while (!outBuf_.empty() && fd_ >= 0) {
        ssize_t nw = write(fd_, outBuf_.data(), outBuf_.size());
        if (nw > 0) {
            outBuf_.erase(0, (size_t)nw);
            continue;
        }
        if (nw < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) {
            if (!writeBlocked_) {
                writeBlocked_ = true;
                loop_->modFd(fd_, EPOLLIN | EPOLLOUT);
            }
            return;
        }
        log_.debug(serverField(), "ZK write failed; retrying");
        serverFailed();
        return;
    }
}

void ZkClient::onPacket(const uint8_t* data, size_t len) {
    Reader r{data, len};
    int32_t xid = r.i32();
    int64_t zxid = r.i64();
    int32_t err = r.i32();
    if (!r.ok) return;
    if (zxid > 0) lastZxid_ = zxid;

    if (xid == XID_NOTIFICATION) {
        int32_t type = r.i32();
        int32_t st = r.i32();
        std::string path = r.str();
        (void)st;
        if (r.ok && watchCb_) watchCb_(type, path);
        return;
    }
    if (xid == XID_PING) return;

    auto it = pending_.find(xid);
    if (it == pending_.end()) {
        log_.warn({{"xid", Json((int64_t)xid)}},
                  "ZK reply for unknown xid");
        return;
    }
    Pending p = std::move(it->second);
    pending_.erase(it);

    static const Stat kStat;
    switch (p.op) {
    case OP_GETDATA: {
        if (err != ZOK) {
            p.dataCb(err, "", kStat);
            break;
        }
        std::string d = r.str();
        Stat s = r.stat();
        p.dataCb(r.ok ? ZOK : ZMARSHALLINGERROR, d, s);
        break;
    }
    case OP_GETCHILDREN: {
        if (err != ZOK) {
            p.childrenCb(err, {});
            break;
        }
        auto kids = r.strVec();
        p.childrenCb(r.ok ? ZOK : ZMARSHALLINGERROR, kids);
        break;
    }
    case OP_EXISTS: {
        if (err != ZOK) {
            p.statCb(err, kStat);
            break;
        }
        Stat s = r.stat();
        p.statCb(r.ok ? ZOK : ZMARSHALLINGERROR, s);
        break;
    }
    case OP_CREATE: {
        if (err != ZOK) {
            p.stringCb(err, "");
            break;
        }
        p.stringCb(ZOK, r.str());
        break;
    }
    case OP_SETDATA:
    case OP_DELETE: {
        p.voidCb(err);
        break;
    }
    default:
        break;
    }
}

/* ---------------- requests ---------------- */

void ZkClient::getData(const std::string& path, bool watch, DataCb cb) {
    if (state_ != State::Connected) {
        static const Stat kStat;
        loop_->defer([cb]() { cb(ZCONNECTIONLOSS, "", kStat); });
        return;
    }
    int32_t xid = nextXid();
    Writer w;
    w.i32(xid);
    w.i32(OP_GETDATA);
    w.str(path);
    w.boolean(watch);
    Pending p;
    p.xid = xid;
    p.op = OP_GETDATA;
    p.dataCb = std::move(cb);
    pending_[xid] = std::move(p);
    sendPacket(w.buf);
    flush();
}

void ZkClient::getChildren(const std::string& path, bool watch,
                           ChildrenCb cb) {
    if (state_ != State::Connected) {
        loop_->defer([cb]() { cb(ZCONNECTIONLOSS, {}); });
        return;
    }
    int32_t xid = nextXid();
    Writer w;
    w.i32(xid);
    w.i32(OP_GETCHILDREN);
    w.str(path);
    w.boolean(watch);
    Pending p;
    p.xid = xid;
    p.op = OP_GETCHILDREN;
    p.childrenCb = std::move(cb);
    pending_[xid] = std::move(p);
    sendPacket(w.buf);
    flush();
}

void ZkClient::exists(const std::string& path, bool watch, StatCb cb) {
    if (state_ != State::Connected) {
        static const Stat kStat;
        loop_->defer([cb]() { cb(ZCONNECTIONLOSS, kStat); });
        return;
    }
    int32_t xid = nextXid();
    Writer w;
    w.i32(xid);
    w.i32(OP_EXISTS);
    w.str(path);
    w.boolean(watch);
    Pending p;
    p.xid = xid;
    p.op = OP_EXISTS;
    p.statCb = std::move(cb);
    pending_[xid] = std::move(p);
    sendPacket(w.buf);
    flush();
}

void ZkClient::create(const std::string& path, const std::string& data,
                      int32_t flags, StringCb cb) {
    if (state_ != State::Connected) {
        loop_->defer([cb]() { cb(ZCONNECTIONLOSS, ""); });
        return;
    }
    int32_t xid = nextXid();
    Writer w;
    w.i32(xid);
    w.i32(OP_CREATE);
    w.str(path);
    w.buffer(data);
    writeOpenAcl(w);
    w.i32(flags);
    Pending p;
    p.xid = xid;
    p.op = OP_CREATE;
    p.stringCb = std::move(cb);
    pending_[xid] = std::move(p);
    sendPacket(w.buf);
    flush();
}

void ZkClient::setData(const std::string& path, const std::string& data,
                       int32_t version, VoidCb cb) {
    if (state_ != State::Connected) {
        loop_->defer([cb]() { cb(ZCONNECTIONLOSS); });
        return;
    }
    int32_t xid = nextXid();
    Writer w;
    w.i32(xid);
    w.i32(OP_SETDATA);
    w.str(path);
    w.buffer(data);
    w.i32(version);
    Pending p;
    p.xid = xid;
    p.op = OP_SETDATA;
    p.voidCb = std::move(cb);
    pending_[xid] = std::move(p);
    sendPacket(w.buf);
    flush();
}

void ZkClient::del(const std::string& path, int32_t version, VoidCb cb) {
    if (state_ != State::Connected) {
        loop_->defer([cb]() { cb(ZCONNECTIONLOSS); });
        return;
    }
    int32_t xid = nextXid();
    Writer w;
    w.i32(xid);
    w.i32(OP_DELETE);
    w.str(path);
    w.i32(version);
    Pending p;
    p.xid = xid;
    p.op = OP_DELETE;
    p.voidCb = std::move(cb);
    pending_[xid] = std::move(p);
    sendPacket(w.buf);
    flush();
}

}  // namespace bamd::zk
