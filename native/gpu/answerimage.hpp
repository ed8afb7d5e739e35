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
 *     most max_reply bytes (512 unless the producer asks for a ceiling of
 *     up to 4096), at most 64 members, every segment inside the blob
 *     and the segment lengths adding up to `total`;
 *   - off + len of every slot lies inside the arena, and the slot array
 *     is a power of two loaded to at most 1/2 (so a probe always ends).
 *
 * add*() refuse what breaks these rules; verify() re-walks the finished
 * image before it is handed out. No dependency on HIP.
 */
#pragma once

#include "answerrules.hpp"

namespace bamd::gpu {

class AnswerImage {
  public:
    static constexpr size_t kMaxReply = gpu::kMaxReply;
    static constexpr size_t kMinReply = gpu::kMinReply;

    using Member = gpu::Member;

    explicit AnswerImage(size_t maxReply = gpu::kMaxReply)
        : maxReply_(checkCeiling(maxReply)) {}

    size_t maxReply() const { return maxReply_; }
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
        checkReply(reply, maxReply_);
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
        answerbody::Seg s1[answerbody::kMaxMembers];
        answerbody::Seg s2[answerbody::kMaxMembers];
        size_t segBytes = checkService(head, members, maxReply_, s1, s2);
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
            imageFail("slot count is not a power of two below 2^32");
        if (tab_.size() * 2 > cap) imageFail("load above 1/2");
        const SlotView* sl = (const SlotView*)tab_.slotData();
        const uint8_t* arena = tab_.arenaData();
        size_t live = 0;
        for (size_t i = 0; i < cap; ++i) {
            if (sl[i].len == 0) continue;
            ++live;
            if ((size_t)sl[i].off + sl[i].len > used)
                imageFail("blob outside the arena");
            verifyBlob(arena + sl[i].off, sl[i].len, maxReply_);
        }
        if (live != tab_.size()) imageFail("slot count mismatch");
    }

  private:
    struct SlotView {
        uint64_t hash;
        uint32_t off;
        uint32_t len;
    };

    AnswerTable tab_;
    size_t maxReply_;
};

}  // namespace bamd::gpu
