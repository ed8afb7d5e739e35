/*
 * binder-amd: a batch of changes to the device answer table of the GPU
 * batch resolver - the producer's side of the contract with the update
 * kernels (update.cpp), as answerimage.hpp is for the resolve kernels.
 *
 * Three operations, recorded in call order:
 *
 *   upsertReply / upsertService   add or replace one (qname, qtype)
 *   invalidate(domain)            what DnsServer::applyInvalidate does
 *                                 for a non-empty domain: drop (domain,
 *                                 A) and every SRV entry stored under
 *                                 hashKey(domain, 33) whose key is
 *                                 domain or ends in "." + domain
 *
 * The upserts are refused by the rules of answerrules.hpp, the same as
 * AnswerImage::add*, and every blob is verified as it is built.
 *
 * Normal form. The device applies a delta in two unordered phases -
 * all invalidations, then all upserts - so the delta is kept in the
 * form in which that equals the calls applied one by one:
 *
 *   - each domain is invalidated once, each key upserted once;
 *   - an upsert replaces a pending upsert of the same key;
 *   - an invalidation drops the pending upserts it covers, and is
 *     recorded: what the table held before the delta goes as well;
 *   - an upsert added after an invalidation that covers it stays,
 *     because phase 2 runs after phase 1.
 *
 * Packed form (pack()): domains end to end with int32 offsets and both
 * hashes (qtype 1, qtype 33) per domain; finished blobs `klen qtype key
 * body` end to end with int32 offsets and one hash per blob. The blob
 * section is byte for byte what goes into the arena. No dependency on
 * HIP.
 */
#pragma once

#include <map>
#include <set>

#include "answerrules.hpp"

namespace bamd::gpu {

class AnswerDelta {
  public:
    struct Packed {
        std::string ibuf;             /* domains end to end */
        std::vector<int32_t> ioff;    /* [I + 1] */
        std::vector<uint64_t> ihash;  /* [2 I]: hash A, hash SRV */
        std::string ubuf;             /* blobs end to end */
        std::vector<int32_t> uoff;    /* [U + 1] */
        std::vector<uint64_t> uhash;  /* [U] */
    };

    explicit AnswerDelta(size_t maxReply = kMaxReply)
        : maxReply_(checkCeiling(maxReply)) {}

    size_t maxReply() const { return maxReply_; }
    size_t size() const { return domains_.size() + upserts_.size(); }
    size_t invalidations() const { return domains_.size(); }
    size_t upserts() const { return upserts_.size(); }

    void clear() {
        domains_.clear();
        upserts_.clear();
        srvByHash_.clear();
    }

    void upsertReply(std::string_view qname, int qtype,
                     std::string_view reply) {
        uint64_t h = hashOf(qname, qtype);
        checkReply(reply, maxReply_);
        std::string blob = blobHead(
            qname, qtype, answerbody::wireBodyLen(reply.size()));
        answerbody::wireFill(body(blob, qname), (const uint8_t*)reply.data(),
                             reply.size());
        put(qname, qtype, h, std::move(blob));
    }

    void upsertService(std::string_view qname, int qtype,
                       std::string_view head,
                       const std::vector<Member>& members) {
        uint64_t h = hashOf(qname, qtype);
        answerbody::Seg s1[answerbody::kMaxMembers];
        answerbody::Seg s2[answerbody::kMaxMembers];
        size_t segBytes = checkService(head, members, maxReply_, s1, s2);
        std::string blob = blobHead(
            qname, qtype,
            answerbody::serviceBodyLen(members.size(), head.size(),
                                       segBytes));
        answerbody::serviceFill(body(blob, qname), members.size(),
                                (const uint8_t*)head.data(), head.size(),
                                s1, s2);
        put(qname, qtype, h, std::move(blob));
    }

    void invalidate(std::string_view domain) {
        if (domain.empty())
            throw std::invalid_argument("empty domain");
        if (domain.size() > AnswerTable::kMaxKey)
            throw std::invalid_argument("key longer than 255 bytes");
        upserts_.erase(modelKey(domain, 1));
        uint64_t h33 =
            AnswerTable::hashKey(domain.data(), domain.size(), 33);
        auto [lo, hi] = srvByHash_.equal_range(h33);
        while (lo != hi) {
            if (covers(domain, lo->second)) {
                upserts_.erase(modelKey(lo->second, 33));
                lo = srvByHash_.erase(lo);
            } else {
                ++lo;
            }
        }
        domains_.emplace(domain);
    }

    /* removeSuffix()'s key match: `key` is domain or ends in
     * "." + domain */
    static bool covers(std::string_view domain, std::string_view key) {
        return key.size() >= domain.size() &&
               key.substr(key.size() - domain.size()) == domain &&
               (key.size() == domain.size() ||
                key[key.size() - domain.size() - 1] == '.');
    }

    Packed pack() const {
        Packed p;
        p.ioff.push_back(0);
        for (const std::string& d : domains_) {
            p.ibuf += d;
            p.ioff.push_back(offset(p.ibuf.size()));
            p.ihash.push_back(AnswerTable::hashKey(d.data(), d.size(), 1));
            p.ihash.push_back(AnswerTable::hashKey(d.data(), d.size(), 33));
        }
        p.uoff.push_back(0);
        for (const auto& [key, up] : upserts_) {
            p.ubuf += up.blob;
            p.uoff.push_back(offset(p.ubuf.size()));
            p.uhash.push_back(up.hash);
        }
        return p;
    }

  private:
    struct Upsert {
        uint64_t hash;
        std::string blob;
    };

    static int32_t offset(size_t v) {
        if (v > 0x7FFFFFFFu)
            throw std::length_error("delta above 2^31 bytes");
        return (int32_t)v;
    }

    static std::string modelKey(std::string_view qname, int qtype) {
        return std::string(1, (char)qtype).append(qname);
    }

    static std::string blobHead(std::string_view qname, int qtype,
                                size_t bodyLen) {
        std::string blob(2 + qname.size() + bodyLen, '\0');
        blob[0] = (char)qname.size();
        blob[1] = (char)qtype;
        blob.replace(2, qname.size(), qname);
        return blob;
    }
    static uint8_t* body(std::string& blob, std::string_view qname) {
        return (uint8_t*)blob.data() + 2 + qname.size();
    }

    void put(std::string_view qname, int qtype, uint64_t h,
             std::string blob) {
        verifyBlob((const uint8_t*)blob.data(), blob.size(), maxReply_);
        auto [it, fresh] = upserts_.insert_or_assign(
            modelKey(qname, qtype), Upsert{h, std::move(blob)});
        if (fresh && qtype == 33) srvByHash_.emplace(h, qname);
    }

    std::set<std::string> domains_;
    std::map<std::string, Upsert> upserts_;   /* qtype byte + qname */
    std::multimap<uint64_t, std::string> srvByHash_;  /* pending SRV */
    size_t maxReply_;
};

}  // namespace bamd::gpu
