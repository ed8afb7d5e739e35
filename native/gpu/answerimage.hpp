/*
 * binder-amd: host image of an answer table for the GPU batch resolver.
 *
 * A thin owner of a real AnswerTable, filled by hand instead of by the
 * server's fast path, whose slot array and arena are uploaded as they
 * are. The image is the producer's side of the contract with the two
 * kernels (resolve.cpp): what they trust is checked here, once, on the
 * host -
 *
 *   - every key is (qname, qtype) with qtype A or SRV and <= 255 bytes,
 *     hashed as DnsServer::answerHash does (A on the whole name, SRV on
 *     the name behind _svc._proto);
 *   - every body is a `wire` or `service` layout of answerbody::, its
 *     reply at least a DNS header (12 bytes, all in the head) and at
 *     most 512 bytes, at most 64 members, every segment inside the blob
 *     and the segment lengths adding up to `total`;
 *   - off + len of every slot lies inside the arena, and the slot array
 *     is a power of two loaded to at most 1/2 (so a probe always ends).
 *
 * add*() refuse what breaks these rules; verify() re-walks the finished
 * image before it is handed out. No dependency on HIP.
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

class AnswerImage {
  public:
    static constexpr size_t kMaxReply = 512;
    static constexpr size_t kMinReply = 12;

    using Member = std::pair<std::string_view, std::string_view>;

    size_t size() const { return tab_.size(); }
    const AnswerTable& table() const { return tab_; }

    /* home slot of the key's hash in the current slot array */
    size_t homeSlot(std::string_view qname, int qtype) const {
        uint64_t h = hashOf(qname, qtype);
        return tab_.slots() == 0 ? 0 : (size_t)(h & (tab_.slots() - 1));
    }

    void addReply(std::string_view qname, int qtype,
                  std::string_view reply) {
        uint64_t h = hashOf(qname, qtype);
        if (reply.size() < kMinReply)
            throw std::invalid_argument("reply shorter than a header");
        if (reply.size() > kMaxReply)
            throw std::invalid_argument("reply longer than 512 bytes");
        uint8_t* body = tab_.insert(
            h, (uint8_t)qtype, qname.data(), qname.size(),
            answerbody::wireBodyLen(reply.size()));
        if (body == nullptr)
            throw std::invalid_argument("answer table refused the entry");
        answerbody::wireFill(body, (const uint8_t*)reply.data(),
                             reply.size());
    }

    void addService(std::string_view qname, int qtype,
                    std::string_view head,
                    const std::vector<Member>& members) {
        uint64_t h = hashOf(qname, qtype);
        size_t n = members.size();
        if (n > answerbody::kMaxMembers)
            throw std::invalid_argument("more than 64 members");
        if (head.size() < kMinReply)
            throw std::invalid_argument("head shorter than a header");
        answerbody::Seg s1[answerbody::kMaxMembers];
        answerbody::Seg s2[answerbody::kMaxMembers];
        size_t segBytes = 0;
        for (size_t i = 0; i < n; ++i) {
            const auto& [a, b] = members[i];
            s1[i] = {(const uint8_t*)a.data(), a.size()};
            s2[i] = {(const uint8_t*)b.data(), b.size()};
            segBytes += a.size() + b.size();
            if (segBytes > kMaxReply) break;
        }
        if (head.size() + segBytes > kMaxReply)
            throw std::invalid_argument("reply longer than 512 bytes");
        uint8_t* body = tab_.insert(
            h, (uint8_t)qtype, qname.data(), qname.size(),
            answerbody::serviceBodyLen(n, head.size(), segBytes));
        if (body == nullptr)
            throw std::invalid_argument("answer table refused the entry");
        answerbody::serviceFill(body, n, (const uint8_t*)head.data(),
                                head.size(), s1, s2);
    }

    /* Walk the whole image against the contract above; throws
     * std::runtime_error naming the first rule broken. */
    void verify() const {
        size_t cap = tab_.slots(), used = tab_.arenaBytes();
        if (cap == 0) return;
        if ((cap & (cap - 1)) != 0 || cap > 0x80000000u)
            fail("slot count is not a power of two below 2^32");
        if (tab_.size() * 2 > cap) fail("load above 1/2");
        const SlotView* sl = (const SlotView*)tab_.slotData();
        const uint8_t* arena = tab_.arenaData();
        size_t live = 0;
        for (size_t i = 0; i < cap; ++i) {
            if (sl[i].len == 0) continue;
            ++live;
            if ((size_t)sl[i].off + sl[i].len > used)
                fail("blob outside the arena");
            verifyBlob(arena + sl[i].off, sl[i].len);
        }
        if (live != tab_.size()) fail("slot count mismatch");
    }

  private:
    struct SlotView {
        uint64_t hash;
        uint32_t off;
        uint32_t len;
    };

    [[noreturn]] static void fail(const char* what) {
        throw std::runtime_error(std::string("answer image: ") + what);
    }

    static void verifyBlob(const uint8_t* b, size_t len) {
        using answerbody::get16;
        if (len < 2 || len < 2 + (size_t)b[0] + 4) fail("short blob");
        if (b[1] != 1 && b[1] != 33) fail("qtype not A or SRV");
        const uint8_t* body = b + 2 + b[0];
        size_t blen = len - 2 - b[0];
        size_t total = answerbody::total(body);
        if (total < kMinReply || total > kMaxReply) fail("bad total");
        if (answerbody::kind(body) == answerbody::kWire) {
            if (blen != answerbody::wireBodyLen(total))
                fail("wire body length");
            return;
        }
        if (answerbody::kind(body) != answerbody::kService)
            fail("unknown body kind");
        size_t n = body[1];
        if (n > answerbody::kMaxMembers || blen < 6 + 8 * n)
            fail("bad member count");
        size_t headLen = get16(body + 4);
        if (headLen < kMinReply || blen < 6 + 8 * n + headLen)
            fail("bad head");
        size_t segBytes = blen - 6 - 8 * n - headLen;
        size_t sum = headLen;
        for (size_t i = 0; i < 2 * n; ++i) {
            const uint8_t* e = body + 6 + 4 * i;
            if (get16(e) + get16(e + 2) > segBytes)
                fail("segment outside the blob");
            sum += get16(e + 2);
        }
        if (sum != total) fail("segments do not add up to total");
    }

    /* DnsServer::answerHash on a dotted name: A on the whole name, SRV
     * on what follows the second label */
    static uint64_t hashOf(std::string_view qname, int qtype) {
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

    AnswerTable tab_;
};

}  // namespace bamd::gpu
