/*
 * binder-amd: device helpers shared by the two resolve kernel pairs
 * (resolve.cpp, resolveext.cpp): the streamed key and its hash, the
 * member-order generator and the copy plan of a service reply. Device
 * code only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bamd::gpu {

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kLenMul = 0xD6E8FEB86659FD93ull;
constexpr uint64_t kStepMul = 0xBF58476D1CE4E5B9ull;
constexpr uint64_t kSmMul2 = 0x94D049BB133111EBull;

/* Streams the dotted key out of the wire name. `pos` is the wire
 * position of the next key byte, `nextLen` the position of the next
 * length byte; that byte reads as '.', and its value says where the
 * one after it lies. With kFold a label byte 'A'-'Z' reads as its
 * lowercase. */
template <bool kFold>
struct KeyReaderT {
    const uint8_t* q;
    uint32_t pos;
    uint32_t nextLen;

    __device__ __forceinline__ uint32_t next() {
        uint32_t c = q[pos];
        if (pos == nextLen) {
            nextLen += c + 1;
            c = '.';
        } else if constexpr (kFold) {
            if (c - 'A' < 26u) c |= 0x20;
        }
        ++pos;
        return c;
    }
    __device__ __forceinline__ uint64_t word(uint32_t nbytes) {
        uint32_t lo = 0, hi = 0;
        for (uint32_t b = 0; b < nbytes && b < 4; ++b)
            lo |= next() << (8 * b);
        for (uint32_t b = 4; b < nbytes; ++b)
            hi |= next() << (8 * (b - 4));
        return ((uint64_t)hi << 32) | lo;
    }
};
using KeyReader = KeyReaderT<false>;
using FoldReader = KeyReaderT<true>;

/* AnswerTable::hashKey, bit for bit, over the streamed key */
template <class Reader>
__device__ __forceinline__ uint64_t hashKey(Reader r, uint32_t klen,
                                            uint32_t qtype) {
    uint64_t h = kGold ^ ((uint64_t)klen * kLenMul) ^
                 ((uint64_t)qtype << 56);
    uint32_t n = klen;
    while (n >= 8) {
        h = (h ^ r.word(8)) * kStepMul;
        h ^= h >> 32;
        n -= 8;
    }
    if (n != 0) {
        h = (h ^ r.word(n)) * kStepMul;
        h ^= h >> 32;
    }
    h ^= h >> 32;
    h *= kGold;
    h ^= h >> 29;
    h *= kStepMul;
    h ^= h >> 32;
    return h;
}

__device__ __forceinline__ uint32_t get16(const uint8_t* p) {
    return p[0] | ((uint32_t)p[1] << 8);
}

__device__ __forceinline__ uint64_t splitmix(uint64_t x) {
    x += kGold;
    uint64_t z = (x ^ (x >> 30)) * kStepMul;
    z = (z ^ (z >> 27)) * kSmMul2;
    return z ^ (z >> 31);
}

/* The member order of reply `index`: Fisher-Yates from the
 * counter-based generator. */
__device__ __forceinline__ void drawOrder(uint32_t n, uint64_t seed,
                                          uint64_t index, uint8_t* order) {
    for (uint32_t i = 0; i < n; ++i) order[i] = (uint8_t)i;
    uint64_t s0 = seed ^ (index * kLenMul);
    uint64_t k = 0;
    for (uint32_t i = n; i > 1;) {
        --i;
        uint64_t draw = splitmix(s0 + k * kGold);
        uint32_t j = (uint32_t)(draw >> 32) % (i + 1);
        uint8_t t = order[i];
        order[i] = order[j];
        order[j] = t;
        ++k;
    }
}

/* head + 64 first segments + 64 second segments */
constexpr int kMaxJobs = 129;

/* One copy of a service reply: `src` counts from the body's start,
 * `dst` from the reply's. */
struct Job {
    uint16_t src, dst, len;
};

/* Lane 0 of a group: draw the member order and lay out
 * answerbody::serviceAssemble's copies - head, first segments in order,
 * second segments in order. The head's first 12 bytes are left to the
 * header patch. */
__device__ inline void planService(const uint8_t* body, uint64_t seed,
                                   uint64_t index, uint8_t* order,
                                   Job* jobs) {
    uint32_t n = body[1];
    uint32_t headLen = get16(body + 4);
    const uint8_t* tab = body + 6;
    uint32_t headOff = 6 + 8 * n;
    uint32_t segOff = headOff + headLen;
    drawOrder(n, seed, index, order);
    jobs[0] = Job{(uint16_t)(headOff + 12), 12, (uint16_t)(headLen - 12)};
    uint32_t w = headLen;
    for (uint32_t pass = 0; pass < 2; ++pass) {
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t* e = tab + 8 * order[i] + 4 * pass;
            uint32_t len = get16(e + 2);
            jobs[1 + pass * n + i] = Job{(uint16_t)(segOff + get16(e)),
                                         (uint16_t)w, (uint16_t)len};
            w += len;
        }
    }
}

}  // namespace bamd::gpu
