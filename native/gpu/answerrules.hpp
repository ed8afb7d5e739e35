/*
 * binder-amd: the producer's rules for the GPU batch resolver, shared
 * by the host image (answerimage.hpp) and the update batch
 * (answerdelta.hpp): how a key is hashed, what a reply and a service
 * may hold, and what a finished blob must look like. The kernels trust
 * exactly this. No dependency on HIP.
 */
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "../server/answertab.hpp"

namespace bamd::gpu {

/* the default ceiling on a stored reply, and the range a producer may
 * choose one from: 4096 is the largest size the server ever grants a
 * query, so a longer body could only be answered truncated */
constexpr size_t kMaxReply = 512;
constexpr size_t kMaxReplyCeiling = 4096;
constexpr size_t kMinReply = 12;

/* a service member's first and second segment */
using Member = std::pair<std::string_view, std::string_view>;

[[noreturn]] inline void imageFail(const char* what) {
    throw std::runtime_error(std::string("answer image: ") + what);
}

/* DnsServer::answerHash on a dotted name: A on the whole name, SRV
 * on what follows the second label */
inline uint64_t hashOf(std::string_view qname, int qtype) {
    if (qtype != 1 && qtype != 33)
        throw std::invalid_argument("qtype must be 1 (A) or 33 (SRV)");
    if (qname.size() > AnswerTable::kMaxKey)
        throw std::invalid_argument("key longer than 255 bytes");
    if (qtype == 1)
        return AnswerTable::hashKey(qname.data(), qname.size(), 1);
    size_t d1 = qname.find('.');
    size_t d2 = d1 == std::string_view::npos
                    ? d1
                    : qname.find('.', d1 + 1);
    if (d2 == std::string_view::npos || d2 + 1 >= qname.size())
        throw std::invalid_argument(
            "SRV name is not _svc._proto.domain");
    return AnswerTable::hashKey(qname.data() + d2 + 1,
                                qname.size() - d2 - 1, 33);
}

/* a producer's ceiling: kMaxReply .. kMaxReplyCeiling */
inline size_t checkCeiling(size_t maxReply) {
    if (maxReply < kMaxReply || maxReply > kMaxReplyCeiling)
        throw std::invalid_argument("max_reply must be in [512, 4096]");
    return maxReply;
}

[[noreturn]] inline void tooLong(size_t maxReply) {
    throw std::invalid_argument("reply longer than " +
                                std::to_string(maxReply) + " bytes");
}

inline void checkReply(std::string_view reply, size_t maxReply) {
    if (reply.size() < kMinReply)
        throw std::invalid_argument("reply shorter than a header");
    if (reply.size() > maxReply) tooLong(maxReply);
}

/* Check a service's head and members and lay the members out as the
 * two segment lists serviceFill() takes (room for kMaxMembers each).
 * Returns the segments' bytes. */
inline size_t checkService(std::string_view head,
                           const std::vector<Member>& members,
                           size_t maxReply, answerbody::Seg* s1,
                           answerbody::Seg* s2) {
    size_t n = members.size();
    if (n > answerbody::kMaxMembers)
        throw std::invalid_argument("more than 64 members");
    if (head.size() < kMinReply)
        throw std::invalid_argument("head shorter than a header");
    size_t segBytes = 0;
    for (size_t i = 0; i < n; ++i) {
        const auto& [a, b] = members[i];
        s1[i] = {(const uint8_t*)a.data(), a.size()};
        s2[i] = {(const uint8_t*)b.data(), b.size()};
        segBytes += a.size() + b.size();
        if (segBytes > maxReply) break;
    }
    if (head.size() + segBytes > maxReply) tooLong(maxReply);
    return segBytes;
}

/* One finished blob `klen qtype key body` against the contract;
 * throws std::runtime_error naming the first rule broken. */
inline void verifyBlob(const uint8_t* b, size_t len, size_t maxReply) {
    using answerbody::get16;
    if (len < 2 || len < 2 + (size_t)b[0] + 4) imageFail("short blob");
    if (b[1] != 1 && b[1] != 33) imageFail("qtype not A or SRV");
    const uint8_t* body = b + 2 + b[0];
    size_t blen = len - 2 - b[0];
    size_t total = answerbody::total(body);
    if (total < kMinReply || total > maxReply) imageFail("bad total");
    if (answerbody::kind(body) == answerbody::kWire) {
        if (blen != answerbody::wireBodyLen(total))
            imageFail("wire body length");
        return;
    }
    if (answerbody::kind(body) != answerbody::kService)
        imageFail("unknown body kind");
    size_t n = body[1];
    if (n > answerbody::kMaxMembers || blen < 6 + 8 * n)
        imageFail("bad member count");
    size_t headLen = get16(body + 4);
    if (headLen < kMinReply || blen < 6 + 8 * n + headLen)
        imageFail("bad head");
    size_t segBytes = blen - 6 - 8 * n - headLen;
    size_t sum = headLen;
    for (size_t i = 0; i < 2 * n; ++i) {
        const uint8_t* e = body + 6 + 4 * i;
        if (get16(e) + get16(e + 2) > segBytes)
            imageFail("segment outside the blob");
        sum += get16(e + 2);
    }
    if (sum != total) imageFail("segments do not add up to total");
}

}  // namespace bamd::gpu
