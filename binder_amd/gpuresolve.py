"""GPU batch resolver: a whole run of wire queries against an answer
table in device memory, on the MI355X.

    image = _native.AnswerImage()        # filled on the host, verified
    table = GpuAnswerTable(image)        # uploaded once
    rbuf, roff = table.resolve(qbuf, qoff)
    delta = _native.AnswerDelta()        # invalidations and upserts
    table.apply(delta)                   # in place, on the device

The work is two hand-written gfx950 kernels (native/gpu/resolve.cpp):
`bamd_resolve_lookup` parses, hashes and probes one query per lane,
`bamd_resolve_emit` copies or assembles the replies into one packed
buffer. torch is the plumbing only: it owns the buffers, the stream and
the prefix sum between the two kernels. With `accept` set, resolve()
runs a second pair instead (native/gpu/resolveext.cpp),
`bamd_resolve_lookup_ext` and `bamd_resolve_emit_ext`, which also serve
queries that carry an EDNS0 OPT record (ACCEPT_EDNS) or uppercase in the
name (ACCEPT_ANYCASE). With `oversize=True` it runs a third pair
(native/gpu/resolvelarge.cpp), `bamd_resolve_lookup_lim` and
`bamd_resolve_emit_lim`, which serves an image built with a raised
ceiling, `_native.AnswerImage(max_reply=4096)`: replies of up to 4096
bytes, each held against what its query may take (512 bytes, or the OPT
record's size clamped to [512, 4096]) and truncated as the server
truncates when it does not fit: header with TC, the question, the OPT
tail. With `policy=ZonePolicy(b"foo.com")` on top of that it runs a
fourth pair (native/gpu/resolvepolicy.cpp), `bamd_resolve_lookup_pol` and
`bamd_resolve_emit_pol`, which also writes the replies the server builds
from the query alone: NOTIMP for a type it does not implement (AAAA, half
of a dual-stack stub's capture), REFUSED for an SRV name of the wrong
shape and for a name outside the zone. Those take no probe and no arena
read; `tally=` counts what became of the batch in five device words. The
table follows the registry through apply(): four more
kernels (native/gpu/update.cpp) tombstone
what a delta invalidates, claim or replace slots for what it upserts,
and compact the table when dead space has built up. A query the image does not
answer gets an empty reply (`roff[i + 1] == roff[i]`); the caller sends
it down the CPU path.

resolve() reads the replies' total back to size `rbuf`, which suits a
replay of a million queries. A serving loop's bursts go through a
workspace instead:

    burst = table.burst(64)              # buffers allocated once
    rbuf, rstart, rlen = burst.resolve(qbuf, qoff)

That is one launch of `bamd_resolve_fused` (native/gpu/resolvefused.cpp),
which looks up, places and writes a tile of queries in one workgroup,
with no allocation and no read back to the host. A workspace made with
`table.burst(64, oversize=True)` launches `bamd_resolve_fused_lim`
(native/gpu/resolvefusedlim.cpp) instead, which serves what
resolve(..., oversize=True) serves: replies of up to 4096 bytes, in full
or truncated. It deals the copies of a long reply (a 64-member service,
a 4 KiB wire reply in chunks) out to the whole workgroup. Without the
switch the burst path leaves entries above 512 bytes unserved, as
resolve() does.

What a serving loop holds is not bare DNS messages but a run of bsock1
frames (native/balancer/protocol.hpp), and what it owes the balancer is
REPLY frames. A third workspace takes and gives exactly that:

    frames = table.frames(64)            # buffers allocated once
    rbuf, rstart, rlen, miss = frames.resolve(fbuf, foff)

`foff` is where the frames start, from `_native.frame_index` on the host
(native/gpu/frameindex.hpp). One launch of `bamd_resolve_frames`
(native/gpu/resolveframes.cpp) checks every frame against that index,
reads the DNS message of a QUERY frame in place, serves it as the
oversize burst does, and writes the REPLY frame header with the reply.
A QUERY frame's `proto` byte says TCP or UDP, so TCP is served here: a
hit comes back in full whatever its size. `rbuf[:frames.end()]` is a
gap-free run of REPLY frames; `miss[:frames.misses()]` lists the frames
left to the CPU path.

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
FUSED_TILE = _gpuresolve.FUSED_TILE  # queries per fused workgroup
OP_BLOCK = _gpuresolve.OP_BLOCK  # ops per update workgroup
ACCEPT_EDNS = _gpuresolve.ACCEPT_EDNS        # ARCOUNT 1 with an OPT record
ACCEPT_ANYCASE = _gpuresolve.ACCEPT_ANYCASE  # 'A'-'Z' in the name
TALLY_WORDS = _gpuresolve.TALLY_WORDS  # counters of resolve(tally=...)


def _pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


class ZonePolicy:
    """What resolve(..., policy=...) answers from the query alone, as the
    server does: NOTIMP for a type other than A, SRV and PTR, REFUSED
    for an SRV name that is not _svc._proto.domain, and with a zone
    (the server's dnsDomain, bytes, e.g. b"foo.com") REFUSED for an A or
    SRV name that is not a label or more under it. b"" is no zone rule.

    The zone is lowercase [a-z0-9_-] labels of 1 to 63 bytes, at most
    255 bytes in wire form, which is what the device keeps."""

    _LABEL = frozenset(b"abcdefghijklmnopqrstuvwxyz0123456789_-")

    def __init__(self, zone=b"", device="cuda"):
        zone = bytes(zone)
        wire = b""
        if zone:
            for label in zone.split(b"."):
                if not 1 <= len(label) <= 63 or not self._LABEL.issuperset(
                        label):
                    raise ValueError(f"bad label in zone {zone!r}")
                wire += bytes([len(label)]) + label
            wire += b"\0"
            if len(wire) > _gpuresolve.MAX_ZONE:
                raise ValueError("zone above 255 bytes in wire form")
        self.zone, self.wire = zone, wire
        self._dev = torch.frombuffer(bytearray(wire or b"\0"),
                                     dtype=torch.uint8).to(device)


class GpuAnswerTable:
    """An AnswerImage in device memory, kept current with apply().

    Everything runs on the current stream: a resolve() after an apply()
    on the same stream sees the whole delta. apply(), compact() and
    resolve() are not safe concurrently on different streams."""

    MIN_SLOTS = 1024
    MIN_ARENA = 4096
    MAX_ARENA = 2 ** 32 - 16  # slot offsets are 32 bits

    def __init__(self, image, device="cuda", reserve_entries=0,
                 reserve_bytes=0):
        if not isinstance(image, _native.AnswerImage):
            raise TypeError("GpuAnswerTable takes an _native.AnswerImage")
        self.device = torch.device(device)
        slots, arena = image.slots(), image.arena()  # verified copies
        self.max_reply = image.max_reply  # the image's ceiling on a reply
        self.cap = len(slots) // 16
        self.entries = len(image)  # exact as of the last compaction
        self._slots = self._upload(slots)
        # the tombstone blob, two zero bytes, lies behind the arena
        self._used = len(arena)
        self._arena_cap = max(self._used, reserve_bytes)
        self._arena = torch.zeros(self._arena_cap + 2, dtype=torch.uint8,
                                  device=self.device)
        self._arena[:self._used].copy_(self._upload(arena))
        self._occ = self.entries    # upper bound: live + tombstones
        self._counters = torch.zeros(_gpuresolve.COUNTERS,
                                     dtype=torch.int32, device=self.device)
        self._seen = torch.zeros(_gpuresolve.COUNTERS,
                                 dtype=torch.int32).pin_memory()
        self._seen_event = None     # (event, used) of a read in flight
        self._last = ([0] * _gpuresolve.COUNTERS, self._used)
        self.compactions = 0
        want_slots = _pow2(2 * reserve_entries) if reserve_entries else 0
        if want_slots > self.cap:
            with torch.cuda.device(self.device):
                self._rebuild(min_slots=want_slots,
                              min_bytes=self._arena_cap)
            self.compactions = 0

    def _upload(self, data: bytes):
        if not data:
            return torch.empty(0, dtype=torch.uint8, device=self.device)
        host = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        return host.to(self.device)

    def _table(self):
        return (self._slots.data_ptr(), self.cap, self._arena.data_ptr(),
                self._arena_cap, self._counters.data_ptr())

    def _rebuild(self, extra_entries=0, extra_bytes=0, min_slots=0,
                 min_bytes=0):
        """Compact into fresh buffers with room for a batch of
        extra_entries blobs of extra_bytes: scan, torch's prefix sum,
        move. Reads the exact live counts back (one synchronise)."""
        dev = self.device
        stream = torch.cuda.current_stream().cuda_stream
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        lens = torch.empty(self.cap, dtype=torch.int32, device=dev)
        _gpuresolve.scan(self._slots.data_ptr(), self.cap, lens.data_ptr(),
                         totals.data_ptr(), stream)
        incl = torch.cumsum(lens, 0, dtype=torch.int64)
        live, live_bytes = totals.tolist()
        ncap = _pow2(max(4 * (live + extra_entries), min_slots,
                         self.MIN_SLOTS))
        nbytes = max(2 * (live_bytes + extra_bytes), min_bytes,
                     self.MIN_ARENA)
        if nbytes > self.MAX_ARENA or ncap > 2 ** 31:
            raise ValueError("answer table above 2^32 arena bytes")
        nslots = torch.zeros(ncap * 16, dtype=torch.uint8, device=dev)
        narena = torch.empty(nbytes + 2, dtype=torch.uint8, device=dev)
        _gpuresolve.move(self._slots.data_ptr(), self.cap,
                         self._arena.data_ptr(), lens.data_ptr(),
                         incl.data_ptr(), nslots.data_ptr(), ncap,
                         narena.data_ptr(), nbytes,
                         self._counters.data_ptr(), stream)
        self._slots, self.cap = nslots, ncap
        self._arena, self._arena_cap = narena, nbytes
        self._used, self._occ, self.entries = live_bytes, live, live
        self.compactions += 1
        self._seen_event = None
        self._last = ([0] * _gpuresolve.COUNTERS, self._used)

    def _crowded(self):
        """Dead bytes above live bytes, or tombstones above live
        entries, by the counters as the last finished apply() left
        them; no wait."""
        if self._seen_event is not None and self._seen_event[0].query():
            used = self._seen_event[1]
            self._last = ([c & 0xFFFFFFFF for c in self._seen.tolist()],
                          used)
            self._seen_event = None
        (tombs, dead, claims, _), used = self._last
        return dead > used - dead or tombs > self.entries + claims - tombs

    def apply(self, delta):
        """Apply an _native.AnswerDelta in place: all its invalidations,
        then all its upserts, by HIP kernels on the current stream.
        Makes room first (a compaction into larger buffers) when the
        batch could load the slot array above 1/2 or overrun the arena,
        and compacts when dead space has outgrown the live data. Not
        safe concurrently with resolve() on another stream."""
        if not isinstance(delta, _native.AnswerDelta):
            raise TypeError("apply takes an _native.AnswerDelta")
        if delta.max_reply > self.max_reply:
            raise ValueError(
                f"delta built for replies up to {delta.max_reply} bytes, "
                f"table for {self.max_reply}")
        p = delta.pack()
        ni, nu = len(p["ioff"]) // 4 - 1, len(p["uoff"]) // 4 - 1
        ibytes, ubytes = len(p["ibuf"]), len(p["ubuf"])
        if ni + nu == 0:
            return
        with torch.cuda.device(self.device):
            if 2 * (self._occ + nu) > self.cap or \
                    self._used + ubytes > self._arena_cap or self._crowded():
                self._rebuild(nu, ubytes)
            stream = torch.cuda.current_stream().cuda_stream
            # one upload: 8-byte hashes, 4-byte offsets, domain bytes
            ops = self._upload(p["ihash"] + p["uhash"] + p["ioff"] +
                               p["uoff"] + p["ibuf"])
            ihash = ops.data_ptr()
            uhash = ihash + 16 * ni
            ioff = uhash + 8 * nu
            uoff = ioff + 4 * (ni + 1)
            ibuf = uoff + 4 * (nu + 1)
            if ni:
                _gpuresolve.invalidate(*self._table(), ibuf, ioff, ibytes,
                                       ihash, ni, stream)
            if nu:
                # the blobs go into the arena as they are, end to end
                self._arena[self._used:self._used + ubytes].copy_(
                    torch.frombuffer(bytearray(p["ubuf"]),
                                     dtype=torch.uint8))
                _gpuresolve.insert(*self._table(), self._used, uoff, ubytes,
                                   uhash, nu, stream)
                self._used += ubytes
                self._occ += nu
            self._seen.copy_(self._counters, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            self._seen_event = (event, self._used)

    def compact(self, min_slots=0):
        """Rebuild slots and arena from the live entries on the device:
        no tombstones, no dead bytes, at least min_slots slots."""
        with torch.cuda.device(self.device):
            self._rebuild(min_slots=min_slots)

    def stats(self):
        """Exact counts; one small device read."""
        tombs, dead, claims, _ = (c & 0xFFFFFFFF
                                  for c in self._counters.tolist())
        return {"entries": self.entries + claims - tombs,
                "slots": self.cap, "tombstones": tombs,
                "arena_bytes": self._used, "dead_bytes": dead,
                "compactions": self.compactions}

    def resolve(self, qbuf, qoff, seed=0, accept=0, oversize=False,
                policy=None, tally=None):
        """qbuf: uint8 query bytes end to end; qoff: int32 [N + 1].
        Returns (rbuf uint8, roff int64 [N + 1]) on the device.

        accept is a set of ACCEPT_EDNS and ACCEPT_ANYCASE: what to serve
        beyond the CPU fast parser's queries. A query with a well-formed
        OPT record gets the server's OPT appended and ARCOUNT + 1, unless
        that passes the size it advertises; a name with uppercase is
        looked up folded and echoed as asked.

        Without oversize a hit above 512 bytes (the table then has a
        raised ceiling, max_reply) and a hit that passes the advertised
        size are left unserved. With oversize=True every accepted hit is
        served: in full when reply and OPT tail fit 512 bytes, or the
        advertised size clamped to [512, 4096], else truncated to the
        header with TC set, the question as asked and the OPT tail.

        policy is a ZonePolicy and needs oversize=True. Every accepted
        query that the server answers from the query alone then gets
        that answer, whatever the table holds: NOTIMP or REFUSED, the
        question as asked, and the OPT tail. Everything else is served
        as without it; PTR stays unserved. tally, with policy only, is
        an int64 device tensor of TALLY_WORDS counters that the call
        adds to and never clears: served in full, truncated, NOTIMP,
        REFUSED, unserved."""
        dev = self.device
        if accept & ~(ACCEPT_EDNS | ACCEPT_ANYCASE):
            raise ValueError(f"unknown accept bits: {accept:#x}")
        if policy is not None and not isinstance(policy, ZonePolicy):
            raise TypeError("policy must be a ZonePolicy")
        if policy is not None and not oversize:
            raise ValueError("policy needs oversize=True")
        if tally is not None:
            if policy is None:
                raise ValueError("tally needs policy")
            if tally.dtype != torch.int64 or tally.dim() != 1 or \
                    tally.numel() != TALLY_WORDS or \
                    not tally.is_contiguous() or tally.device.type != dev.type:
                raise TypeError("tally must be a contiguous int64 tensor of "
                                f"{TALLY_WORDS} words on the table's device")
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
            batch = (qbuf.data_ptr(), qoff.data_ptr(), qbuf.numel(), n)
            body_off = torch.empty(n, dtype=torch.int32, device=dev)
            rlen = torch.empty(n, dtype=torch.int32, device=dev)
            if policy is not None:
                meta = torch.empty(n, dtype=torch.int32, device=dev)
                zone = policy._dev.to(dev)  # held until the launch is queued
                _gpuresolve.lookup_pol(
                    *batch, self._slots.data_ptr(), self.cap,
                    self._arena.data_ptr(), accept, zone.data_ptr(),
                    len(policy.wire), body_off.data_ptr(), rlen.data_ptr(),
                    meta.data_ptr(),
                    0 if tally is None else tally.data_ptr(), stream)
            elif oversize:
                meta = torch.empty(n, dtype=torch.int32, device=dev)
                _gpuresolve.lookup_lim(
                    *batch, self._slots.data_ptr(), self.cap,
                    self._arena.data_ptr(), accept, body_off.data_ptr(),
                    rlen.data_ptr(), meta.data_ptr(), stream)
            elif accept:
                meta = torch.empty(n, dtype=torch.int32, device=dev)
                _gpuresolve.lookup_ext(
                    *batch, self._slots.data_ptr(), self.cap,
                    self._arena.data_ptr(), accept, body_off.data_ptr(),
                    rlen.data_ptr(), meta.data_ptr(), stream)
            else:
                _gpuresolve.lookup(
                    *batch, self._slots.data_ptr(), self.cap,
                    self._arena.data_ptr(), body_off.data_ptr(),
                    rlen.data_ptr(), stream)
            roff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            roff[1:] = torch.cumsum(rlen, 0, dtype=torch.int64)
            rbuf = torch.empty(int(roff[-1]), dtype=torch.uint8, device=dev)
            if rbuf.numel() != 0 and policy is not None:
                _gpuresolve.emit_pol(
                    *batch, self._arena.data_ptr(), body_off.data_ptr(),
                    rlen.data_ptr(), meta.data_ptr(), roff.data_ptr(),
                    rbuf.data_ptr(), seed & (2 ** 64 - 1), stream)
            elif rbuf.numel() != 0 and oversize:
                _gpuresolve.emit_lim(
                    *batch, self._arena.data_ptr(), body_off.data_ptr(),
                    rlen.data_ptr(), meta.data_ptr(), roff.data_ptr(),
                    rbuf.data_ptr(), seed & (2 ** 64 - 1), stream)
            elif rbuf.numel() != 0 and accept:
                _gpuresolve.emit_ext(
                    *batch, self._arena.data_ptr(), body_off.data_ptr(),
                    rlen.data_ptr(), meta.data_ptr(), roff.data_ptr(),
                    rbuf.data_ptr(), seed & (2 ** 64 - 1), stream)
            elif rbuf.numel() != 0:
                _gpuresolve.emit(
                    *batch, self._arena.data_ptr(), body_off.data_ptr(),
                    rlen.data_ptr(), roff.data_ptr(), rbuf.data_ptr(),
                    seed & (2 ** 64 - 1), stream)
        return rbuf, roff

    def burst(self, max_queries, max_bytes=None, rbuf=None, oversize=False):
        """A reusable ResolveBurst workspace for batches of at most
        max_queries queries; see there. For a serving loop's bursts of
        tens to thousands of queries. On a million-query replay the
        fused kernel is several times slower than resolve()
        (profiles/GPURESOLVE.md): replay keeps resolve(). oversize is
        resolve()'s switch; it belongs to the workspace because it
        sizes the default buffer."""
        return ResolveBurst(self, max_queries, max_bytes, rbuf, oversize)

    def frames(self, max_frames, max_bytes=None, rbuf=None):
        """A reusable FrameBurst workspace for runs of at most max_frames
        bsock1 frames; see there. What a serving loop holds goes in as
        it lies in the ring, and REPLY frames come out."""
        return FrameBurst(self, max_frames, max_bytes, rbuf)

    def resolve_list(self, queries, seed=0, accept=0, oversize=False,
                     policy=None, tally=None):
        """One reply (bytes) or None per query."""
        offs = [0]
        for q in queries:
            offs.append(offs[-1] + len(q))
        qbuf = torch.frombuffer(bytearray(b"".join(queries) or b"\0"),
                                dtype=torch.uint8)[:offs[-1]]
        qoff = torch.tensor(offs, dtype=torch.int32)
        rbuf, roff = self.resolve(qbuf, qoff, seed, accept, oversize, policy,
                                  tally)
        data, roff = rbuf.cpu().numpy().tobytes(), roff.tolist()
        return [data[a:b] if b > a else None
                for a, b in zip(roff, roff[1:])]


class ResolveBurst:
    """Buffers for GpuAnswerTable's single-launch resolve, allocated
    once: `rbuf` of max_bytes (by default max_queries x (512 + 11), the
    largest reply with the OPT tail, or with oversize=True max_queries x
    4096, the upper end of what a query may take: neither can overflow),
    or the caller's own uint8 device tensor, whose length is then the
    capacity;
    `rstart` int64 and `rlen` int32 per query; two two-word cursors.

    resolve() on device inputs is one kernel launch and one reset of a
    cursor (a small fill behind the launch, for the next call) on the
    current stream: no allocation, no read back, so bursts queue behind
    each other. It reads the table's buffers at call time:
    a workspace made before an apply() that rebuilt the table serves the
    new one. The stream rule is the table's: current stream, and not
    concurrent with apply() on another stream. One workspace serves one
    call at a time and stays on one stream: the fill that readies the
    next call's cursor is queued behind this call's launch.

    Replies of one tile of FUSED_TILE consecutive queries are packed in
    query order; tiles lie in `rbuf` in the order the device placed them.
    A batch of at most FUSED_TILE queries therefore has resolve()'s
    bytes and offsets. A tile that finds no room in `rbuf` is left
    unserved as a whole and counted in dropped().

    With oversize=True every call launches `bamd_resolve_fused_lim` and
    serves every accepted hit, in full or truncated, as
    GpuAnswerTable.resolve(..., oversize=True) does; on an image with
    the default ceiling that only adds the truncation of replies that
    pass the advertised size."""

    REPLY_MAX = 512 + 11
    REPLY_MAX_OVERSIZE = 4096

    def __init__(self, table, max_queries, max_bytes=None, rbuf=None,
                 oversize=False):
        if max_queries < 1 or max_queries >= 2 ** 31:
            raise ValueError("max_queries must be in [1, 2^31)")
        dev = table.device
        if rbuf is None:
            if max_bytes is None:
                max_bytes = max_queries * (
                    self.REPLY_MAX_OVERSIZE if oversize else self.REPLY_MAX)
            rbuf = torch.empty(max_bytes, dtype=torch.uint8, device=dev)
        elif max_bytes is not None:
            raise ValueError("give max_bytes or rbuf, not both")
        elif rbuf.dtype != torch.uint8 or rbuf.dim() != 1 or \
                not rbuf.is_contiguous() or rbuf.device.type != dev.type:
            raise TypeError("rbuf must be a contiguous 1-d uint8 tensor "
                            "on the table's device")
        self.table, self.max_queries = table, max_queries
        self.oversize = bool(oversize)
        self._launch = (_gpuresolve.fused_lim if oversize
                        else _gpuresolve.fused)
        self.rbuf = rbuf
        self.rstart = torch.zeros(max_queries, dtype=torch.int64, device=dev)
        self.rlen = torch.zeros(max_queries, dtype=torch.int32, device=dev)
        # two cursors { bytes claimed, hits dropped }, used in turn: a
        # call launches on one and then clears the other for the next
        # call, so no fill stands between the caller and its kernel
        self._cursor = torch.zeros(2, 2, dtype=torch.int64, device=dev)
        self._cur = (self._cursor[0], self._cursor[1])
        self._turn = 0
        self._out = tuple(
            (rbuf.data_ptr(), rbuf.numel(), c.data_ptr(),
             self.rstart.data_ptr(), self.rlen.data_ptr())
            for c in self._cur)

    def resolve(self, qbuf, qoff, seed=0, accept=0):
        """qbuf, qoff, seed and accept as in GpuAnswerTable.resolve().
        A workspace made without oversize does not serve a hit above 512
        bytes or past the advertised size (rlen[i] == 0); one made with
        it serves them in full or truncated.
        Returns (rbuf, rstart [N], rlen [N]): views of the workspace,
        valid until the next call on it. Reply i is
        rbuf[rstart[i]:rstart[i] + rlen[i]]; rlen[i] == 0 means query i
        is not served, and rstart[i] then means nothing."""
        t = self.table
        if accept & ~(ACCEPT_EDNS | ACCEPT_ANYCASE):
            raise ValueError(f"unknown accept bits: {accept:#x}")
        if qbuf.dtype != torch.uint8 or qoff.dtype != torch.int32:
            raise TypeError("qbuf must be uint8 and qoff int32")
        if qoff.dim() != 1 or qoff.numel() < 1 or qbuf.dim() != 1:
            raise ValueError("qbuf and qoff must be 1-d, qoff [N + 1]")
        if qbuf.numel() >= 2 ** 31:
            raise ValueError("qbuf must be under 2^31 bytes")
        n = qoff.numel() - 1
        if n > self.max_queries:
            raise ValueError(f"{n} queries in a workspace for "
                             f"{self.max_queries}")
        if n == 0:
            return self.rbuf, self.rstart[:0], self.rlen[:0]
        qbuf = qbuf.to(t.device).contiguous()
        qoff = qoff.to(t.device).contiguous()
        k = self._turn
        self._turn = k ^ 1
        with torch.cuda.device(t.device):
            self._launch(
                qbuf.data_ptr(), qoff.data_ptr(), qbuf.numel(), n,
                t._slots.data_ptr(), t.cap, t._arena.data_ptr(), accept,
                seed & (2 ** 64 - 1), *self._out[k],
                torch.cuda.current_stream().cuda_stream)
            self._cur[k ^ 1].zero_()
        return self.rbuf, self.rstart[:n], self.rlen[:n]

    def dropped(self):
        """Hits of the last non-empty resolve() that found no room in
        `rbuf`. The one call here that synchronises."""
        return int(self._cur[self._turn ^ 1][1])


class FrameBurst:
    """Buffers for GpuAnswerTable's single-launch resolve of a run of
    bsock1 frames (native/balancer/protocol.hpp), allocated once: `rbuf`
    of max_bytes (by default max_frames x REPLY_MAX, the longest REPLY
    frame, which cannot overflow), or the caller's own uint8 device
    tensor, whose length is then the capacity; `rstart` int64, `rlen`
    and `miss` int32 per frame; two four-word cursors.

    resolve() on device inputs is one launch of `bamd_resolve_frames`
    and one reset of a cursor on the current stream: no allocation, no
    read back. Streams, the table's buffers and "one call at a time"
    are as for ResolveBurst.

    A QUERY frame whose DNS message the table answers gets a REPLY
    frame with its req_id. proto 0 is served as
    burst(oversize=True) serves the bare message: in full when it fits
    512 bytes or the advertised size, else truncated. Any other proto is
    TCP, and a hit comes back in full whatever its size. `rbuf[:end()]`
    is a gap-free run of whole REPLY frames, ready for the reply ring in
    one copy: a tile's in frame order, tiles in the order the device
    placed them. Every other frame (PING and the other types, a QUERY
    that is malformed, not accepted or not in the table, a tile that
    found no room in `rbuf`) is listed once in `miss[:misses()]`, for
    the CPU path."""

    REPLY_MAX = _gpuresolve.FRAMES_REPLY_MAX

    def __init__(self, table, max_frames, max_bytes=None, rbuf=None):
        if max_frames < 1 or max_frames >= 2 ** 31:
            raise ValueError("max_frames must be in [1, 2^31)")
        dev = table.device
        if rbuf is None:
            if max_bytes is None:
                max_bytes = max_frames * self.REPLY_MAX
            rbuf = torch.empty(max_bytes, dtype=torch.uint8, device=dev)
        elif max_bytes is not None:
            raise ValueError("give max_bytes or rbuf, not both")
        elif rbuf.dtype != torch.uint8 or rbuf.dim() != 1 or \
                not rbuf.is_contiguous() or rbuf.device.type != dev.type:
            raise TypeError("rbuf must be a contiguous 1-d uint8 tensor "
                            "on the table's device")
        self.table, self.max_frames = table, max_frames
        self.rbuf = rbuf
        self.rstart = torch.zeros(max_frames, dtype=torch.int64, device=dev)
        self.rlen = torch.zeros(max_frames, dtype=torch.int32, device=dev)
        self.miss = torch.zeros(max_frames, dtype=torch.int32, device=dev)
        # two cursors { bytes claimed, hits dropped, end of the stream,
        # misses }, used in turn as ResolveBurst's are
        self._cursor = torch.zeros(2, 4, dtype=torch.int64, device=dev)
        self._cur = (self._cursor[0], self._cursor[1])
        self._turn = 0
        self._out = tuple(
            (rbuf.data_ptr(), rbuf.numel(), c.data_ptr(),
             self.rstart.data_ptr(), self.rlen.data_ptr(),
             self.miss.data_ptr())
            for c in self._cur)

    def resolve(self, fbuf, foff, seed=0, accept=0):
        """fbuf: uint8 frame bytes as they lie in the ring; foff: int32
        [N + 1] frame starts, as _native.frame_index gives them; seed and
        accept as in GpuAnswerTable.resolve().
        Returns (rbuf, rstart [N], rlen [N], miss [N]): views of the
        workspace, valid until the next call on it. Frame i's REPLY
        frame is rbuf[rstart[i]:rstart[i] + rlen[i]]; rlen[i] == 0 means
        it has none and i is in miss[:misses()]."""
        t = self.table
        if accept & ~(ACCEPT_EDNS | ACCEPT_ANYCASE):
            raise ValueError(f"unknown accept bits: {accept:#x}")
        if fbuf.dtype != torch.uint8 or foff.dtype != torch.int32:
            raise TypeError("fbuf must be uint8 and foff int32")
        if foff.dim() != 1 or foff.numel() < 1 or fbuf.dim() != 1:
            raise ValueError("fbuf and foff must be 1-d, foff [N + 1]")
        if fbuf.numel() >= 2 ** 31:
            raise ValueError("fbuf must be under 2^31 bytes")
        n = foff.numel() - 1
        if n > self.max_frames:
            raise ValueError(f"{n} frames in a workspace for "
                             f"{self.max_frames}")
        if n == 0:
            return self.rbuf, self.rstart[:0], self.rlen[:0], self.miss[:0]
        fbuf = fbuf.to(t.device).contiguous()
        foff = foff.to(t.device).contiguous()
        k = self._turn
        self._turn = k ^ 1
        with torch.cuda.device(t.device):
            _gpuresolve.frames(
                fbuf.data_ptr(), foff.data_ptr(), fbuf.numel(), n,
                t._slots.data_ptr(), t.cap, t._arena.data_ptr(), accept,
                seed & (2 ** 64 - 1), *self._out[k],
                torch.cuda.current_stream().cuda_stream)
            self._cur[k ^ 1].zero_()
        return self.rbuf, self.rstart[:n], self.rlen[:n], self.miss[:n]

    # of the last non-empty resolve(); these three synchronise

    def end(self):
        """Where the run of REPLY frames in `rbuf` ends."""
        return int(self._cur[self._turn ^ 1][2])

    def misses(self):
        """How many frames are listed in `miss`."""
        return int(self._cur[self._turn ^ 1][3])

    def dropped(self):
        """Hits that found no room in `rbuf`; they are in `miss` too."""
        return int(self._cur[self._turn ^ 1][1])

    def resolve_bytes(self, data, seed=0, accept=0):
        """Index the whole frames at the front of `data`, at most
        max_frames of them (_native.frame_index), upload, resolve and
        read back: (the REPLY frames as bytes, the sorted indices of the
        frames left to the CPU path, bytes of `data` consumed). For
        replay and tests; a caller that must tell a cut frame from a bad
        one behind `consumed` runs frame_index itself."""
        foff, consumed, _ = _native.frame_index(data, self.max_frames)
        n = len(foff) // 4 - 1
        if n == 0:
            return b"", [], consumed
        rbuf, _, _, miss = self.resolve(
            torch.frombuffer(bytearray(data[:consumed]), dtype=torch.uint8),
            torch.frombuffer(bytearray(foff), dtype=torch.int32),
            seed, accept)
        return (rbuf[:self.end()].cpu().numpy().tobytes(),
                sorted(miss[:self.misses()].tolist()), consumed)
