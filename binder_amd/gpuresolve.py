"""GPU batch resolver: a whole run of wire queries against a static
answer image, on the MI355X.

    image = _native.AnswerImage()        # filled on the host, verified
    table = GpuAnswerTable(image)        # uploaded once
    rbuf, roff = table.resolve(qbuf, qoff)

The work is two hand-written gfx950 kernels (native/gpu/resolve.cpp):
`bamd_resolve_lookup` parses, hashes and probes one query per lane,
`bamd_resolve_emit` copies or assembles the replies into one packed
buffer. torch is the plumbing only: it owns the buffers, the stream and
the prefix sum between the two kernels. A query the image does not
answer gets an empty reply (`roff[i + 1] == roff[i]`); the caller sends
it down the CPU path.

Nothing else in binder_amd imports this module: it needs the HIP
extension and a GPU, and says which one is missing.
"""
from __future__ import annotations

from . import require_native

try:
    import torch
except ImportError as e:  # pragma: no cover
    raise RuntimeError(f"binder_amd.gpuresolve needs torch: {e}") from e

try:
    from . import _gpuresolve
except ImportError as e:
    raise RuntimeError(
        "binder_amd._gpuresolve (the HIP extension) is not built; run "
        f"`make` on a machine with hipcc: {e}") from e

if not torch.cuda.is_available():
    raise RuntimeError("binder_amd.gpuresolve needs a GPU: "
                       "torch.cuda.is_available() is false")

_native = require_native()

TILE = _gpuresolve.TILE        # queries per lookup workgroup
GROUP = _gpuresolve.GROUP      # lanes per reply in emit
MAX_QUERY = _gpuresolve.MAX_QUERY


class GpuAnswerTable:
    """A static snapshot of an AnswerImage in device memory."""

    def __init__(self, image, device="cuda"):
        if not isinstance(image, _native.AnswerImage):
            raise TypeError("GpuAnswerTable takes an _native.AnswerImage")
        self.device = torch.device(device)
        slots, arena = image.slots(), image.arena()  # verified copies
        self.cap = len(slots) // 16
        self.entries = len(image)
        self._slots = self._upload(slots)
        self._arena = self._upload(arena)

    def _upload(self, data: bytes):
        if not data:
            return torch.empty(0, dtype=torch.uint8, device=self.device)
        host = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        return host.to(self.device)

    def resolve(self, qbuf, qoff, seed=0):
        """qbuf: uint8 query bytes end to end; qoff: int32 [N + 1].
        Returns (rbuf uint8, roff int64 [N + 1]) on the device."""
        dev = self.device
        if qbuf.dtype != torch.uint8 or qoff.dtype != torch.int32:
            raise TypeError("qbuf must be uint8 and qoff int32")
        if qoff.dim() != 1 or qoff.numel() < 1 or qbuf.dim() != 1:
            raise ValueError("qbuf and qoff must be 1-d, qoff [N + 1]")
        if qbuf.numel() >= 2 ** 31:
            raise ValueError("qbuf must be under 2^31 bytes")
        n = qoff.numel() - 1
        if n == 0:
            return (torch.empty(0, dtype=torch.uint8, device=dev),
                    torch.zeros(1, dtype=torch.int64, device=dev))
        qbuf = qbuf.to(dev).contiguous()
        qoff = qoff.to(dev).contiguous()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            body_off = torch.empty(n, dtype=torch.int32, device=dev)
            rlen = torch.empty(n, dtype=torch.int32, device=dev)
            _gpuresolve.lookup(
                qbuf.data_ptr(), qoff.data_ptr(), qbuf.numel(), n,
                self._slots.data_ptr(), self.cap, self._arena.data_ptr(),
                body_off.data_ptr(), rlen.data_ptr(), stream)
            roff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            roff[1:] = torch.cumsum(rlen, 0, dtype=torch.int64)
            rbuf = torch.empty(int(roff[-1]), dtype=torch.uint8, device=dev)
            if rbuf.numel() != 0:
                _gpuresolve.emit(
                    qbuf.data_ptr(), qoff.data_ptr(), qbuf.numel(), n,
                    self._arena.data_ptr(), body_off.data_ptr(),
                    rlen.data_ptr(), roff.data_ptr(), rbuf.data_ptr(),
                    seed & (2 ** 64 - 1), stream)
        return rbuf, roff

    def resolve_list(self, queries, seed=0):
        """One reply (bytes) or None per query."""
        offs = [0]
        for q in queries:
            offs.append(offs[-1] + len(q))
        qbuf = torch.frombuffer(bytearray(b"".join(queries) or b"\0"),
                                dtype=torch.uint8)[:offs[-1]]
        qoff = torch.tensor(offs, dtype=torch.int32)
        rbuf, roff = self.resolve(qbuf, qoff, seed)
        data, roff = rbuf.cpu().numpy().tobytes(), roff.tolist()
        return [data[a:b] if b > a else None
                for a, b in zip(roff, roff[1:])]
