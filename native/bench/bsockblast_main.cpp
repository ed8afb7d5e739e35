/*
 * bsockblast: server-tier load generator. Connects straight to one
 * binderd balancer socket and pipelines bsock1 QUERY frames, so the
 * number it reports is binderd's own (no balancer, no UDP generator in
 * the chain). It speaks only the protocol, so one binary measures any
 * binderd build.
 *
 * A fixed number of queries cycles through a names file (dnsblast -f
 * format: "<name> <qtype>" per line) with at most -w frames in flight.
 * Every reqId must come back exactly once as a NOERROR response, else
 * the run fails. Output: ONE JSON line on stdout with qps, queries and
 * binderd_cpu_ns_per_query - the growth of the server's utime+stime
 * (/proc/<pid>/stat, pid from -P) over the run divided by queries. That
 * figure includes libc and kernel time, which a gprof flat profile of
 * binderd does not show.
 *
 * usage: bsockblast -S <socket-path> [-f names-file] [-n queries]
 *        [-w window-frames] [-P binderd-pid] [-T stall-timeout-ms]
 */
#include <fcntl.h>
#include <poll.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../balancer/protocol.hpp"
#include "../dns/codec.hpp"

using namespace bamd;

namespace {

/* utime+stime of a process in nanoseconds; -1 when unreadable */
int64_t procCpuNs(long pid) {
    if (pid <= 0) return -1;
    std::ifstream f("/proc/" + std::to_string(pid) + "/stat");
    std::string line;
    if (!std::getline(f, line)) return -1;
    /* comm may contain spaces: fields resume after the last ')' */
    size_t rp = line.rfind(')');
    if (rp == std::string::npos) return -1;
    std::istringstream ss(line.substr(rp + 1));
    std::string tok;
    long long utime = 0, stime = 0;
    /* after ')': state is field 3; utime/stime are fields 14/15 */
    for (int field = 3; field <= 15 && (ss >> tok); ++field) {
        if (field == 14) utime = atoll(tok.c_str());
        if (field == 15) stime = atoll(tok.c_str());
    }
    long hz = sysconf(_SC_CLK_TCK);
    if (hz <= 0) hz = 100;
    return (int64_t)((utime + stime) * (1000000000LL / hz));
}

int fail(const char* what) {
    fprintf(stderr, "bsockblast: %s\n", what);
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    std::string sockPath, namesFile;
    uint64_t queries = 1000000;
    size_t window = 128;
    long pid = 0;
    int stallMs = 10000;
    int c;
    while ((c = getopt(argc, argv, "S:f:n:w:P:T:h")) != -1) {
        switch (c) {
        case 'S': sockPath = optarg; break;
        case 'f': namesFile = optarg; break;
        case 'n': queries = strtoull(optarg, nullptr, 10); break;
        case 'w': window = (size_t)strtoull(optarg, nullptr, 10); break;
        case 'P': pid = atol(optarg); break;
        case 'T': stallMs = atoi(optarg); break;
        default:
            fprintf(stderr,
                    "usage: bsockblast -S socket [-f names-file] "
                    "[-n queries] [-w window-frames] [-P binderd-pid] "
                    "[-T stall-timeout-ms]\n");
            return c == 'h' ? 0 : 1;
        }
    }
    if (sockPath.empty() || window == 0 || queries == 0 ||
        queries > 0xFFFFFFFFull)
        return fail("need -S, -w >= 1 and 1 <= -n < 2^32");

    /* one prebuilt QUERY frame per name; reqId and DNS id are patched
     * per send */
    std::vector<std::string> frames;
    auto addName = [&frames](const std::string& name, uint16_t qtype) {
        dns::Message q;
        dns::Question qq;
        qq.name = name;
        qq.qtype = qtype;
        q.questions.push_back(qq);
        std::vector<uint8_t> wire = q.encode(0);
        std::string payload;
        bsock::putU32(payload, 0);           /* reqId, patched */
        payload.push_back((char)4);          /* IPv4 */
        payload.push_back((char)0);          /* udp */
        bsock::putU16(payload, 5353);
        const char addr[16] = {127, 0, 0, 1};
        payload.append(addr, sizeof(addr));
        payload.append((const char*)wire.data(), wire.size());
        std::string frame;
        bsock::appendFrame(frame, bsock::FRAME_QUERY, payload);
        frames.push_back(std::move(frame));
    };
    if (!namesFile.empty()) {
        std::ifstream f(namesFile);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty()) continue;
            std::istringstream ss(line);
            std::string name, t;
            ss >> name >> t;
            uint16_t qt = dns::typeFromName(t.empty() ? "A" : t);
            addName(name, qt == 0 ? (uint16_t)dns::TYPE_A : qt);
        }
    }
    if (frames.empty()) addName("test.foo.com", dns::TYPE_A);

    int fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (fd < 0) return fail("socket() failed");
    struct sockaddr_un sa {};
    sa.sun_family = AF_UNIX;
    snprintf(sa.sun_path, sizeof(sa.sun_path), "%s", sockPath.c_str());
    if (connect(fd, (struct sockaddr*)&sa, sizeof(sa)) != 0)
        return fail("cannot connect to the balancer socket");
    int sz = 4 << 20;
    setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &sz, sizeof(sz));
    setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &sz, sizeof(sz));
    fcntl(fd, F_SETFL, fcntl(fd, F_GETFL) | O_NONBLOCK);

    std::vector<uint8_t> seen(queries, 0);
    std::string out;       /* frames built but not yet written */
    size_t outOff = 0;
    std::vector<uint8_t> in(1 << 20);
    size_t inLen = 0;
    uint64_t sent = 0, received = 0;
    size_t nameIdx = 0;

    int64_t cpu0 = procCpuNs(pid);
    auto t0 = std::chrono::steady_clock::now();

    while (received < queries) {
        /* top the window up: one buffer, one write */
        if (outOff == out.size()) {
            out.clear();
            outOff = 0;
            while (sent < queries && sent - received < window) {
                size_t at = out.size();
                const std::string& fr = frames[nameIdx];
                if (++nameIdx == frames.size()) nameIdx = 0;
                out += fr;
                uint32_t id = (uint32_t)sent;
                char* p = &out[at + bsock::kHeaderLen];
                p[0] = (char)id;
                p[1] = (char)(id >> 8);
                p[2] = (char)(id >> 16);
                p[3] = (char)(id >> 24);
                char* d = p + bsock::kQueryHeadLen;
                d[0] = (char)(id >> 8);
                d[1] = (char)id;
                ++sent;
            }
        }
        bool wantWrite = outOff < out.size();
        if (wantWrite) {
            ssize_t nw = write(fd, out.data() + outOff,
                               out.size() - outOff);
            if (nw > 0)
                outOff += (size_t)nw;
            else if (nw < 0 && errno != EAGAIN && errno != EWOULDBLOCK)
                return fail("write failed (server closed?)");
        }

        ssize_t nr = read(fd, in.data() + inLen, in.size() - inLen);
        if (nr == 0) return fail("server closed the connection");
        if (nr < 0) {
            if (errno != EAGAIN && errno != EWOULDBLOCK)
                return fail("read failed");
            struct pollfd pfd {fd, POLLIN, 0};
            if (outOff < out.size()) pfd.events |= POLLOUT;
            if (poll(&pfd, 1, stallMs) == 0)
                return fail("stalled: no reply within the timeout");
            continue;
        }
        inLen += (size_t)nr;
        size_t pos = 0;
        while (inLen - pos >= bsock::kHeaderLen) {
            const uint8_t* h = in.data() + pos;
            if (h[0] != bsock::kMagic) return fail("bad magic in reply");
            uint32_t plen = bsock::getU32(h + 2);
            if (plen > in.size() - bsock::kHeaderLen)
                return fail("oversized reply frame");
            if (inLen - pos < bsock::kHeaderLen + plen) break;
            if (h[1] == bsock::FRAME_REPLY) {
                const uint8_t* p = h + bsock::kHeaderLen;
                if (plen < 4 + 12) return fail("short REPLY frame");
                uint32_t id = bsock::getU32(p);
                const uint8_t* d = p + 4;
                if (id >= queries) return fail("unknown reqId in reply");
                if (seen[id]) return fail("reqId answered twice");
                seen[id] = 1;
                bool qr = (d[2] & 0x80) != 0;
                if (!qr || (d[3] & 0x0F) != 0)
                    return fail("reply is not a NOERROR response");
                if (d[0] != (uint8_t)(id >> 8) || d[1] != (uint8_t)id)
                    return fail("DNS id does not match the query");
                ++received;
            }
            pos += bsock::kHeaderLen + plen;
        }
        if (pos != 0) {
            memmove(in.data(), in.data() + pos, inLen - pos);
            inLen -= pos;
        }
    }

    double secs = std::chrono::duration<double>(
                      std::chrono::steady_clock::now() - t0).count();
    int64_t cpu1 = procCpuNs(pid);
    close(fd);

    double cpuPerQ = (cpu0 >= 0 && cpu1 >= 0)
                         ? (double)(cpu1 - cpu0) / (double)queries
                         : -1.0;
    printf("{\"qps\":%.1f,\"queries\":%llu,\"window\":%zu,"
           "\"names\":%zu,\"seconds\":%.4f,"
           "\"binderd_cpu_ns_per_query\":%.1f}\n",
           (double)queries / secs, (unsigned long long)queries, window,
           frames.size(), secs, cpuPerQ);
    return 0;
}
