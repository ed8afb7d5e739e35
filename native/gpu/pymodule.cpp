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
}
