/*
 * binder-amd: ZooKeeper client (zkstream equivalent).
 *
 * Single-threaded, event-loop driven. Capabilities used by the reference
 * (lib/zk.js:33-47, test/helper.js:98-166): session establishment with
 * timeout, automatic reconnect, a 'session' event on each (re)established
 * session driving full watch re-registration, getData/getChildren with
 * watches, create/setData/delete for tooling and tests, pings to hold
 * the session, and watch-event delivery.
 *
 * Reconnect model: on connection loss we retry with the previous session
 * id; if the server expired us (or we never had one) a fresh session is
 * created. In BOTH cases the 'session' callback fires, and the mirror
 * above re-arms every watch with fresh reads — so missed events during
 * the outage are swallowed by the resync (same recovery shape as
 * lib/zk.js:45-47 + rebind, zk.js:209-223).
 *
 * Server list. The client holds an ordered list of servers and is on one
 * of them at a time. Whatever makes a server fail us - connect refused,
 * unreachable or unresolvable, the connect deadline, a malformed
 * handshake, a write error, an unresponsive server, the loss of an
 * established connection - moves it to the next one, which is tried at
 * once, with the session id, password and last zxid kept so that a real
 * ensemble resumes the session there. After as many consecutive failures
 * as there are servers, with no session in between, it waits
 * reconnectDelayMs before the next pass; the loss of an established
 * connection is the first failure of its pass. With one server that is
 * the delay after every failure. A server that answers "session expired"
 * has not failed: the client stays on it and starts a fresh session after
 * the delay.
 *
 * A real ZooKeeper member that is behind this client's lastZxidSeen
 * refuses the handshake by closing the connection. That is a lost
 * connection like any other and moves on to the next member; no special
 * case.
 */
#pragma once

#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../common/log.hpp"
#include "../common/loop.hpp"
#include "hostlist.hpp"
#include "jute.hpp"

namespace bamd::zk {

struct ZkConfig {
    std::string host = "127.0.0.1";
    uint16_t port = 2181;
    int sessionTimeoutMs = 30000;  // lib/zk.js:37
    int reconnectDelayMs = 1000;
    /* More than one server: the list, tried in this order. Empty means
     * the one server {host, port} above. */
    std::vector<ZkServer> servers;
    /* TCP connect plus ConnectResponse must take no longer than this;
     * 0 = sessionTimeoutMs / number of servers (the Java client's rule) */
    int connectTimeoutMs = 0;
    /* permute the list once, at construction (spreads many clients over
     * the members) */
    bool shuffle = false;
};

class ZkClient {
  public:
    using SessionCb = std::function<void()>;
    using WatchCb =
        std::function<void(int32_t type, const std::string& path)>;
    using DataCb = std::function<void(int32_t rc, const std::string& data,
                                      const Stat& stat)>;
    using ChildrenCb = std::function<void(
        int32_t rc, const std::vector<std::string>& children)>;
    using StatCb = std::function<void(int32_t rc, const Stat& stat)>;
    using StringCb =
        std::function<void(int32_t rc, const std::string& value)>;
    using VoidCb = std::function<void(int32_t rc)>;

    ZkClient(EventLoop* loop, Logger log, ZkConfig cfg);
    ~ZkClient();

    void start();
    void close();

    bool connected() const { return state_ == State::Connected; }
    int64_t sessionId() const { return sessionId_; }

    /* Fired on every newly usable session (incl. reconnects). */
    void onSession(SessionCb cb) { sessionCb_ = std::move(cb); }
    /* All watch events funnel here (mirror routes by path). */
    void onWatch(WatchCb cb) { watchCb_ = std::move(cb); }

    void getData(const std::string& path, bool watch, DataCb cb);
    void getChildren(const std::string& path, bool watch, ChildrenCb cb);
    void exists(const std::string& path, bool watch, StatCb cb);
    void create(const std::string& path, const std::string& data,
                int32_t flags, StringCb cb);
    void setData(const std::string& path, const std::string& data,
                 int32_t version, VoidCb cb);
    void del(const std::string& path, int32_t version, VoidCb cb);

    /* The server this client is on or trying, as "h:p". */
    const std::string& currentServer() const { return names_[cur_]; }
    size_t serverCount() const { return servers_.size(); }
    /* Fired with the server's "h:p" each time a server fails us (see
     * "Server list" above), before the client moves on. */
    using FailureCb = std::function<void(const std::string& server)>;
    void onServerFailure(FailureCb cb) { failureCb_ = std::move(cb); }

    /* Stats for metrics/tests. */
    uint64_t reconnects() const { return reconnects_; }
    uint64_t sessionsEstablished() const { return sessions_; }
    /* sessions established on another server than the one before */
    uint64_t serverSwitches() const { return switches_; }

  private:
    enum class State { Closed, Connecting, Handshaking, Connected };

    struct Pending {
        int32_t xid;
        int32_t op;
        DataCb dataCb;
        ChildrenCb childrenCb;
        StatCb statCb;
        StringCb stringCb;
        VoidCb voidCb;
    };

    void connectStart();
    void onSockEvent(uint32_t events);
    void onReadable();
    void onPacket(const uint8_t* data, size_t len);
    void onConnectResponse(const uint8_t* data, size_t len);
    void sendHandshake();
    void sendPacket(const std::string& body);
    void flush();
    void failAllPending();
    void serverFailed();
    void scheduleReconnect(int delayMs);
    void teardown();
    int connectDeadlineMs() const;
    JsonObject serverField() const;
    void armPingTimer();
    void sendPing();
    int32_t nextXid() { return xid_++; }

    EventLoop* loop_;
    Logger log_;
    ZkConfig cfg_;
    State state_ = State::Closed;
    bool closing_ = false;

    std::vector<ZkServer> servers_;   // never empty
    std::vector<std::string> names_;  // "h:p" per server
    size_t cur_ = 0;
    size_t failures_ = 0;  // consecutive, since the last session or pause
    int lastSessionServer_ = -1;

    int fd_ = -1;
    std::string inBuf_;
    std::string outBuf_;
    bool writeBlocked_ = false;

    int64_t sessionId_ = 0;
    std::string passwd_;
    int negotiatedTimeout_ = 0;
    int64_t lastZxid_ = 0;
    int64_t lastPacketRecvMs_ = 0;

    int32_t xid_ = 1;
    std::map<int32_t, Pending> pending_;  // in-flight, FIFO by xid

    SessionCb sessionCb_;
    WatchCb watchCb_;

    FailureCb failureCb_;

    uint64_t reconnectTimer_ = 0;
    uint64_t pingTimer_ = 0;
    uint64_t connectTimer_ = 0;
    uint64_t reconnects_ = 0;
    uint64_t sessions_ = 0;
    uint64_t switches_ = 0;
};

}  // namespace bamd::zk
