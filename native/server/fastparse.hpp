/*
 * binder-amd: the fast path's query parser.
 *
 * One wire query in, a FastQuery out: header and question checked,
 * the name as lowercase dotted [a-z0-9_-] labels. Anything it declines
 * (uppercase, compression, EDNS, other types and classes, an SRV name
 * that is not _svc._proto.domain) goes to the slow path. Header-only
 * and free of the server, so the Python bindings and the GPU batch
 * resolver's tests use the very parser binderd serves with.
 */
#pragma once

#include <cstddef>
#include <cstdint>
#include <string_view>

namespace bamd {

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

/* longest wire query the fast path looks at */
constexpr size_t kFastMaxQuery = 300;

inline bool parseFastQuery(const uint8_t* data, size_t len, FastQuery& q) {
    if (len < 17 || len > kFastMaxQuery) return false;
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

}  // namespace bamd
