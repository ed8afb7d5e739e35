/*
 * binder-amd: Python bindings of the GPU batch resolver's launchers
 * (binder_amd._gpuresolve). Device pointers and the stream cross as
 * integers, so nothing here links against a tensor library; the
 * caller (binder_amd/gpuresolve.py) owns every buffer.
 */
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

#include "resolve.hpp"
#include "resolveext.hpp"
#include "resolveframes.hpp"
#include "resolvefused.hpp"
#include "resolvefusedlim.hpp"
#include "resolvelarge.hpp"
#include "resolvepolicy.hpp"
#include "update.hpp"

namespace py = pybind11;
using namespace bamd::gpu;

namespace {

template <typename T>
T* ptr(uintptr_t v) {
    return reinterpret_cast<T*>(v);
}

void check(hipError_t e, const char* what) {
    if (e != hipSuccess)
        throw std::runtime_error(std::string(what) + ": " +
                                 hipGetErrorString(e));
}

Batch batch(uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n) {
    if (n < 0 || n > 0x7FFFFFFF || qbytes < 0 || qbytes > 0x7FFFFFFF)
        throw std::invalid_argument("batch out of range");
    return Batch{ptr<const uint8_t>(qbuf), ptr<const int32_t>(qoff), qbytes,
                 (int32_t)n};
}

/* a table the update kernels may write: a power-of-two slot array and
 * an arena below 2^32 bytes with its tombstone blob at `tomb` */
Table table(uintptr_t slots, uint64_t cap, uintptr_t arena, uint64_t tomb,
            uintptr_t counters) {
    if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
        throw std::invalid_argument("cap not a power of two");
    if (tomb > 0xFFFFFFFFu - kTombLen)
        throw std::invalid_argument("arena above 2^32 bytes");
    return Table{ptr<void>(slots), (uint32_t)cap, ptr<uint8_t>(arena),
                 (uint32_t)tomb, ptr<uint32_t>(counters)};
}

int32_t count(int64_t v) {
    if (v < 0 || v > 0x7FFFFFFF)
        throw std::invalid_argument("op batch out of range");
    return (int32_t)v;
}

}  // namespace

PYBIND11_MODULE(_gpuresolve, m) {
    m.doc() = "binder-amd GPU batch resolver launchers (gfx950)";
    m.attr("TILE") = kTile;
    m.attr("GROUP") = kGroup;
    m.attr("MAX_QUERY") = kMaxQuery;

    m.def("lookup",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t slots, uint64_t cap, uintptr_t arena,
             uintptr_t bodyOff, uintptr_t rlen, uintptr_t stream) {
              if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
                  throw std::invalid_argument("cap not a power of two");
              Image img{ptr<const void>(slots), (uint32_t)cap,
                        ptr<const uint8_t>(arena)};
              check(launchLookup(batch(qbuf, qoff, qbytes, n), img,
                                 ptr<uint32_t>(bodyOff), ptr<int32_t>(rlen),
                                 ptr<ihipStream_t>(stream)),
                    "bamd_resolve_lookup");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("body_off"), py::arg("rlen"), py::arg("stream"));

    m.def("emit",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t arena, uintptr_t bodyOff, uintptr_t rlen,
             uintptr_t roff, uintptr_t rbuf, uint64_t seed,
             uintptr_t stream) {
              Image img{nullptr, 0, ptr<const uint8_t>(arena)};
              check(launchEmit(batch(qbuf, qoff, qbytes, n), img,
                               ptr<const uint32_t>(bodyOff),
                               ptr<const int32_t>(rlen),
                               ptr<const int64_t>(roff), ptr<uint8_t>(rbuf),
                               seed, ptr<ihipStream_t>(stream)),
                    "bamd_resolve_emit");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("arena"), py::arg("body_off"), py::arg("rlen"),
          py::arg("roff"), py::arg("rbuf"), py::arg("seed"),
          py::arg("stream"));

    m.attr("ACCEPT_EDNS") = kAcceptEdns;
    m.attr("ACCEPT_ANYCASE") = kAcceptAnycase;

    m.def("lookup_ext",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t slots, uint64_t cap, uintptr_t arena,
             uint32_t accept, uintptr_t bodyOff, uintptr_t rlen,
             uintptr_t meta, uintptr_t stream) {
              if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
                  throw std::invalid_argument("cap not a power of two");
              if ((accept & ~kAcceptAll) != 0)
                  throw std::invalid_argument("unknown accept bits");
              Image img{ptr<const void>(slots), (uint32_t)cap,
                        ptr<const uint8_t>(arena)};
              check(launchLookupExt(batch(qbuf, qoff, qbytes, n), img,
                                    accept, ptr<uint32_t>(bodyOff),
                                    ptr<int32_t>(rlen), ptr<uint32_t>(meta),
                                    ptr<ihipStream_t>(stream)),
                    "bamd_resolve_lookup_ext");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("accept"), py::arg("body_off"), py::arg("rlen"),
          py::arg("meta"), py::arg("stream"));

    m.def("emit_ext",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t arena, uintptr_t bodyOff, uintptr_t rlen,
             uintptr_t meta, uintptr_t roff, uintptr_t rbuf, uint64_t seed,
             uintptr_t stream) {
              Image img{nullptr, 0, ptr<const uint8_t>(arena)};
              check(launchEmitExt(batch(qbuf, qoff, qbytes, n), img,
                                  ptr<const uint32_t>(bodyOff),
                                  ptr<const int32_t>(rlen),
                                  ptr<const uint32_t>(meta),
                                  ptr<const int64_t>(roff),
                                  ptr<uint8_t>(rbuf), seed,
                                  ptr<ihipStream_t>(stream)),
                    "bamd_resolve_emit_ext");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("arena"), py::arg("body_off"), py::arg("rlen"),
          py::arg("meta"), py::arg("roff"), py::arg("rbuf"),
          py::arg("seed"), py::arg("stream"));

    m.attr("LIST_ABOVE") = kListAbove;

    m.def("lookup_lim",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t slots, uint64_t cap, uintptr_t arena,
             uint32_t accept, uintptr_t bodyOff, uintptr_t rlen,
             uintptr_t meta, uintptr_t stream) {
              if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
                  throw std::invalid_argument("cap not a power of two");
              if ((accept & ~kAcceptAll) != 0)
                  throw std::invalid_argument("unknown accept bits");
              Image img{ptr<const void>(slots), (uint32_t)cap,
                        ptr<const uint8_t>(arena)};
              check(launchLookupLim(batch(qbuf, qoff, qbytes, n), img,
                                    accept, ptr<uint32_t>(bodyOff),
                                    ptr<int32_t>(rlen), ptr<uint32_t>(meta),
                                    ptr<ihipStream_t>(stream)),
                    "bamd_resolve_lookup_lim");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("accept"), py::arg("body_off"), py::arg("rlen"),
          py::arg("meta"), py::arg("stream"));

    /* list_above: kListAbove, or 2^32 - 1 for one group per reply */
    m.def("emit_lim",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t arena, uintptr_t bodyOff, uintptr_t rlen,
             uintptr_t meta, uintptr_t roff, uintptr_t rbuf, uint64_t seed,
             uintptr_t stream, uint32_t listAbove) {
              Image img{nullptr, 0, ptr<const uint8_t>(arena)};
              check(launchEmitLim(batch(qbuf, qoff, qbytes, n), img,
                                  ptr<const uint32_t>(bodyOff),
                                  ptr<const int32_t>(rlen),
                                  ptr<const uint32_t>(meta),
                                  ptr<const int64_t>(roff),
                                  ptr<uint8_t>(rbuf), seed, listAbove,
                                  ptr<ihipStream_t>(stream)),
                    "bamd_resolve_emit_lim");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("arena"), py::arg("body_off"), py::arg("rlen"),
          py::arg("meta"), py::arg("roff"), py::arg("rbuf"),
          py::arg("seed"), py::arg("stream"),
          py::arg("list_above") = kListAbove);

    m.attr("MAX_ZONE") = kMaxZone;
    m.attr("TALLY_WORDS") = (int)kTallyWords;

    /* zone: zlen bytes of wire form (0: no zone rule); tally: 0, or
     * TALLY_WORDS int64 counters that are added to */
    m.def("lookup_pol",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t slots, uint64_t cap, uintptr_t arena,
             uint32_t accept, uintptr_t zone, uint32_t zlen,
             uintptr_t bodyOff, uintptr_t rlen, uintptr_t meta,
             uintptr_t tally, uintptr_t stream) {
              if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
                  throw std::invalid_argument("cap not a power of two");
              if ((accept & ~kAcceptAll) != 0)
                  throw std::invalid_argument("unknown accept bits");
              if (zlen > kMaxZone || (zlen != 0 && zone == 0))
                  throw std::invalid_argument("zone above MAX_ZONE bytes");
              Image img{ptr<const void>(slots), (uint32_t)cap,
                        ptr<const uint8_t>(arena)};
              check(launchLookupPol(batch(qbuf, qoff, qbytes, n), img,
                                    accept, ptr<const uint8_t>(zone), zlen,
                                    ptr<uint32_t>(bodyOff),
                                    ptr<int32_t>(rlen), ptr<uint32_t>(meta),
                                    ptr<unsigned long long>(tally),
                                    ptr<ihipStream_t>(stream)),
                    "bamd_resolve_lookup_pol");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("accept"), py::arg("zone"), py::arg("zlen"),
          py::arg("body_off"), py::arg("rlen"), py::arg("meta"),
          py::arg("tally"), py::arg("stream"));

    m.def("emit_pol",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t arena, uintptr_t bodyOff, uintptr_t rlen,
             uintptr_t meta, uintptr_t roff, uintptr_t rbuf, uint64_t seed,
             uintptr_t stream) {
              Image img{nullptr, 0, ptr<const uint8_t>(arena)};
              check(launchEmitPol(batch(qbuf, qoff, qbytes, n), img,
                                  ptr<const uint32_t>(bodyOff),
                                  ptr<const int32_t>(rlen),
                                  ptr<const uint32_t>(meta),
                                  ptr<const int64_t>(roff),
                                  ptr<uint8_t>(rbuf), seed,
                                  ptr<ihipStream_t>(stream)),
                    "bamd_resolve_emit_pol");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("arena"), py::arg("body_off"), py::arg("rlen"),
          py::arg("meta"), py::arg("roff"), py::arg("rbuf"),
          py::arg("seed"), py::arg("stream"));

    m.attr("FUSED_TILE") = kFusedTile;

    m.def("fused",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t slots, uint64_t cap, uintptr_t arena,
             uint32_t accept, uint64_t seed, uintptr_t rbuf,
             uint64_t capacity, uintptr_t cursor, uintptr_t rstart,
             uintptr_t rlen, uintptr_t stream) {
              if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
                  throw std::invalid_argument("cap not a power of two");
              if ((accept & ~kAcceptAll) != 0)
                  throw std::invalid_argument("unknown accept bits");
              if (capacity >= (1ull << 63))
                  throw std::invalid_argument("capacity above 2^63");
              Image img{ptr<const void>(slots), (uint32_t)cap,
                        ptr<const uint8_t>(arena)};
              check(launchFused(batch(qbuf, qoff, qbytes, n), img, accept,
                                seed, ptr<uint8_t>(rbuf), capacity,
                                ptr<uint64_t>(cursor), ptr<int64_t>(rstart),
                                ptr<int32_t>(rlen),
                                ptr<ihipStream_t>(stream)),
                    "bamd_resolve_fused");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("accept"), py::arg("seed"), py::arg("rbuf"),
          py::arg("capacity"), py::arg("cursor"), py::arg("rstart"),
          py::arg("rlen"), py::arg("stream"));

    m.attr("FUSED_LIST_ABOVE") = kFusedListAbove;
    m.attr("FUSED_CHUNK") = kFusedChunk;
    m.attr("FUSED_MIN_CHUNK") = kFusedMinChunk;

    /* list_above, chunk: the defaults, or 2^32 - 1 for one group per
     * reply */
    m.def("fused_lim",
          [](uintptr_t qbuf, uintptr_t qoff, int64_t qbytes, int64_t n,
             uintptr_t slots, uint64_t cap, uintptr_t arena,
             uint32_t accept, uint64_t seed, uintptr_t rbuf,
             uint64_t capacity, uintptr_t cursor, uintptr_t rstart,
             uintptr_t rlen, uintptr_t stream, uint32_t listAbove,
             uint32_t chunk) {
              if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
                  throw std::invalid_argument("cap not a power of two");
              if ((accept & ~kAcceptAll) != 0)
                  throw std::invalid_argument("unknown accept bits");
              if (capacity >= (1ull << 63))
                  throw std::invalid_argument("capacity above 2^63");
              if (chunk < kFusedMinChunk)
                  throw std::invalid_argument("chunk below FUSED_MIN_CHUNK");
              Image img{ptr<const void>(slots), (uint32_t)cap,
                        ptr<const uint8_t>(arena)};
              check(launchFusedLim(batch(qbuf, qoff, qbytes, n), img, accept,
                                   seed, ptr<uint8_t>(rbuf), capacity,
                                   ptr<uint64_t>(cursor),
                                   ptr<int64_t>(rstart), ptr<int32_t>(rlen),
                                   listAbove, chunk,
                                   ptr<ihipStream_t>(stream)),
                    "bamd_resolve_fused_lim");
          },
          py::arg("qbuf"), py::arg("qoff"), py::arg("qbytes"), py::arg("n"),
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("accept"), py::arg("seed"), py::arg("rbuf"),
          py::arg("capacity"), py::arg("cursor"), py::arg("rstart"),
          py::arg("rlen"), py::arg("stream"),
          py::arg("list_above") = kFusedListAbove,
          py::arg("chunk") = kFusedChunk);

    m.attr("FRAMES_REPLY_MAX") = kFramesReplyMax;

    /* fbuf, foff: a run of bsock1 frames and its n + 1 frame starts;
     * cursor: four 64-bit words, zero; miss: n int32 */
    m.def("frames",
          [](uintptr_t fbuf, uintptr_t foff, int64_t fbytes, int64_t n,
             uintptr_t slots, uint64_t cap, uintptr_t arena,
             uint32_t accept, uint64_t seed, uintptr_t rbuf,
             uint64_t capacity, uintptr_t cursor, uintptr_t rstart,
             uintptr_t rlen, uintptr_t miss, uintptr_t stream,
             uint32_t listAbove, uint32_t chunk) {
              if (cap > 0x80000000u || (cap & (cap - 1)) != 0)
                  throw std::invalid_argument("cap not a power of two");
              if ((accept & ~kAcceptAll) != 0)
                  throw std::invalid_argument("unknown accept bits");
              if (capacity >= (1ull << 63))
                  throw std::invalid_argument("capacity above 2^63");
              if (chunk < kFusedMinChunk)
                  throw std::invalid_argument("chunk below FUSED_MIN_CHUNK");
              Image img{ptr<const void>(slots), (uint32_t)cap,
                        ptr<const uint8_t>(arena)};
              check(launchFrames(batch(fbuf, foff, fbytes, n), img, accept,
                                 seed, ptr<uint8_t>(rbuf), capacity,
                                 ptr<uint64_t>(cursor), ptr<int64_t>(rstart),
                                 ptr<int32_t>(rlen), ptr<int32_t>(miss),
                                 listAbove, chunk,
                                 ptr<ihipStream_t>(stream)),
                    "bamd_resolve_frames");
          },
          py::arg("fbuf"), py::arg("foff"), py::arg("fbytes"), py::arg("n"),
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("accept"), py::arg("seed"), py::arg("rbuf"),
          py::arg("capacity"), py::arg("cursor"), py::arg("rstart"),
          py::arg("rlen"), py::arg("miss"), py::arg("stream"),
          py::arg("list_above") = kFusedListAbove,
          py::arg("chunk") = kFusedChunk);

    m.attr("OP_BLOCK") = kOpBlock;
    m.attr("COUNTERS") = (int)kCounters;

    m.def("invalidate",
          [](uintptr_t slots, uint64_t cap, uintptr_t arena, uint64_t tomb,
             uintptr_t counters, uintptr_t ibuf, uintptr_t ioff,
             int64_t ibytes, uintptr_t ihash, int64_t n,
             uintptr_t stream) {
              check(launchInvalidate(
                        table(slots, cap, arena, tomb, counters),
                        ptr<const uint8_t>(ibuf), ptr<const int32_t>(ioff),
                        count(ibytes), ptr<const uint64_t>(ihash), count(n),
                        ptr<ihipStream_t>(stream)),
                    "bamd_update_invalidate");
          },
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("tomb"), py::arg("counters"), py::arg("ibuf"),
          py::arg("ioff"), py::arg("ibytes"), py::arg("ihash"),
          py::arg("n"), py::arg("stream"));

    m.def("insert",
          [](uintptr_t slots, uint64_t cap, uintptr_t arena, uint64_t tomb,
             uintptr_t counters, uint64_t used, uintptr_t uoff,
             int64_t ubytes, uintptr_t uhash, int64_t n,
             uintptr_t stream) {
              if (used + (uint64_t)count(ubytes) > tomb)
                  throw std::invalid_argument("batch outside the arena");
              check(launchInsert(table(slots, cap, arena, tomb, counters),
                                 (uint32_t)used, ptr<const int32_t>(uoff),
                                 count(ubytes), ptr<const uint64_t>(uhash),
                                 count(n), ptr<ihipStream_t>(stream)),
                    "bamd_update_insert");
          },
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("tomb"), py::arg("counters"), py::arg("used"),
          py::arg("uoff"), py::arg("ubytes"), py::arg("uhash"),
          py::arg("n"), py::arg("stream"));

    m.def("scan",
          [](uintptr_t slots, uint64_t cap, uintptr_t lens,
             uintptr_t totals, uintptr_t stream) {
              check(launchScan(table(slots, cap, 0, 0, 0),
                               ptr<int32_t>(lens),
                               ptr<unsigned long long>(totals),
                               ptr<ihipStream_t>(stream)),
                    "bamd_update_scan");
          },
          py::arg("slots"), py::arg("cap"), py::arg("lens"),
          py::arg("totals"), py::arg("stream"));

    m.def("move",
          [](uintptr_t slots, uint64_t cap, uintptr_t arena, uintptr_t lens,
             uintptr_t incl, uintptr_t nslots, uint64_t ncap,
             uintptr_t narena, uint64_t ntomb, uintptr_t counters,
             uintptr_t stream) {
              if (ncap == 0)
                  throw std::invalid_argument("no slots to move into");
              check(launchMove(table(slots, cap, arena, 0, 0),
                               ptr<const int32_t>(lens),
                               ptr<const int64_t>(incl),
                               table(nslots, ncap, narena, ntomb, counters),
                               ptr<ihipStream_t>(stream)),
                    "bamd_update_move");
          },
          py::arg("slots"), py::arg("cap"), py::arg("arena"),
          py::arg("lens"), py::arg("incl"), py::arg("nslots"),
          py::arg("ncap"), py::arg("narena"), py::arg("ntomb"),
          py::arg("counters"), py::arg("stream"));
}
