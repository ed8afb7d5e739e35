/*
 * binder-amd: the ZooKeeper connect string, `host[:port](,host[:port])*`.
 *
 * One parser for every place that names registry servers: ZK_HOST and
 * zookeeper.host in binderd, `zktool -s`, and parse_zk_hosts in the
 * Python module (binder_amd/zkclient.py parse_hosts() is the same grammar
 * written again in Python; tests hold the two together).
 *
 *   host   an IPv4 literal or a hostname of [A-Za-z0-9._-], 1..255 chars
 *   port   decimal 1..65535, at most 5 digits; absent = the default port
 *
 * Blanks around an entry are trimmed; a repeated host:port is dropped and
 * the order of first appearance kept. Not supported, and said so in the
 * error instead of being guessed at: IPv6 literals (`[` `]`) and a chroot
 * suffix (`/`). Every error names the entry it is about.
 */
#pragma once

#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace bamd::zk {

struct ZkServer {
    std::string host;
    uint16_t port = 2181;
    bool operator==(const ZkServer& o) const {
        return port == o.port && host == o.host;
    }
};

/* "h:p", the form log fields and metric labels carry */
inline std::string serverName(const ZkServer& s) {
    return s.host + ":" + std::to_string(s.port);
}

/* A list that parseHostList() gives back unchanged. */
inline std::string formatHostList(const std::vector<ZkServer>& servers) {
    std::string out;
    for (const ZkServer& s : servers) {
        if (!out.empty()) out += ',';
        out += serverName(s);
    }
    return out;
}

namespace hostlist_detail {

inline bool isBlank(char c) {
    return c == ' ' || c == '\t' || c == '\r' || c == '\n';
}

inline bool isHostChar(char c) {
    return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') ||
           (c >= '0' && c <= '9') || c == '.' || c == '_' || c == '-';
}

inline std::string entryError(std::string_view entry, const char* what) {
    std::string e = "bad ZooKeeper server entry \"";
    e.append(entry);
    e += "\": ";
    e += what;
    return e;
}

/* One trimmed entry. Returns an empty string or the error. */
inline std::string parseEntry(std::string_view entry, uint16_t defaultPort,
                              ZkServer& out) {
    if (entry.empty()) return entryError(entry, "empty entry");
    size_t colons = 0, colon = std::string_view::npos;
    for (size_t i = 0; i < entry.size(); i++) {
        char c = entry[i];
        if (c == '[' || c == ']')
            return entryError(entry, "IPv6 literals are not supported");
        if (c == '/')
            return entryError(entry, "a chroot suffix is not supported");
        if (c == ':') {
            colons++;
            colon = i;
        }
    }
    if (colons > 1) return entryError(entry, "more than one ':'");
    std::string_view host =
        colons == 0 ? entry : entry.substr(0, colon);
    if (host.empty()) return entryError(entry, "empty host");
    if (host.size() > 255) return entryError(entry, "host too long");
    for (char c : host)
        if (!isHostChar(c))
            return entryError(entry, "invalid character in host");
    out.host.assign(host);
    out.port = defaultPort;
    if (colons == 1) {
        std::string_view port = entry.substr(colon + 1);
        if (port.empty()) return entryError(entry, "empty port");
        for (char c : port)
            if (c < '0' || c > '9')
                return entryError(entry, "port is not a number");
        uint32_t v = 0;
        if (port.size() <= 5)
            for (char c : port) v = v * 10 + (uint32_t)(c - '0');
        if (v < 1 || v > 65535)
            return entryError(entry, "port out of range (1..65535)");
        out.port = (uint16_t)v;
    }
    return {};
}

}  // namespace hostlist_detail

/* Parses `text` into `out` (cleared first). False, with `err` set and
 * `out` empty, when any entry is malformed. */
inline bool parseHostList(std::string_view text, uint16_t defaultPort,
                          std::vector<ZkServer>& out, std::string& err) {
    using namespace hostlist_detail;
    out.clear();
    err.clear();
    size_t pos = 0;
    for (;;) {
        size_t comma = text.find(',', pos);
        size_t end = comma == std::string_view::npos ? text.size() : comma;
        size_t b = pos, e = end;
        while (b < e && isBlank(text[b])) b++;
        while (e > b && isBlank(text[e - 1])) e--;
        ZkServer s;
        err = parseEntry(text.substr(b, e - b), defaultPort, s);
        if (!err.empty()) {
            out.clear();
            return false;
        }
        bool dup = false;
        for (const ZkServer& have : out) dup = dup || have == s;
        if (!dup) out.push_back(std::move(s));
        if (comma == std::string_view::npos) break;
        pos = comma + 1;
    }
    return true;
}

}  // namespace bamd::zk
