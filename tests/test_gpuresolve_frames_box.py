"""GpuAnswerTable.frames (native/gpu/resolveframes.cpp): a run of bsock1
frames in, REPLY frames out, against the oversize test's Python
reference with the frame rules in front of it. Exact bytes per frame; the
REPLY stream and the miss list by their contract."""
import struct
from itertools import accumulate

import pytest

from test_answer_image import wire
from test_gpuresolve_accept_box import (ANYCASE, EDNS, OPT_TAIL, edns,  # noqa
                                        gr)
from test_gpuresolve_oversize_box import LimRef, fill, mixed_queries

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEFCAFEF00D


def frame(body, req_id=None, proto=0, ftype=1, plen=None):
    """A bsock1 frame; with a req_id, `body` is a QUERY's DNS message."""
    if req_id is not None:
        body = struct.pack("<IBBH16x", req_id, 4, proto, 5353) + body
    return struct.pack("<BBI", 0xB5, ftype,
                       len(body) if plen is None else plen) + body


class FrameRef(LimRef):
    def answer_frame(self, f, index, seed, accept):
        """The REPLY frame for frame f, or b"" where it is unserved."""
        dns = f[30:]
        if len(f) < 6 + 24 + 17 or len(dns) > 300 or f[:2] != b"\xb5\x01" or \
                int.from_bytes(f[2:6], "little") != len(f) - 6:
            return b""
        r = self.answer_lim(dns, index, seed, accept)
        if r and f[11]:
            # TCP is held against 65535: the same queries are served, none
            # truncated. answer_ext puts no limit on a query without an
            # OPT, so take that reply and count the tail in as it does
            end = 12
            while 0 < dns[end] < 64:
                end += 1 + dns[end]
            r = self.answer_ext(dns[:10] + b"\0\0" + dns[12:end + 5], index,
                                seed, accept & ANYCASE)
            if dns[10:12] == b"\0\1":
                ar = (int.from_bytes(r[10:12], "big") + 1) & 0xFFFF
                r = r[:10] + ar.to_bytes(2, "big") + r[12:] + OPT_TAIL
        return r and struct.pack("<BBI", 0xB5, 2, 4 + len(r)) + f[6:10] + r


@pytest.fixture(scope="module")
def big():
    return fill(FrameRef(), True)


@pytest.fixture(scope="module")
def table(gr, big):
    return gr.GpuAnswerTable(big.image)


def batch(n):
    """mixed_queries as UDP and TCP QUERY frames in turn; every seventh
    position is a frame of another kind."""
    fs = []
    for i, q in enumerate(mixed_queries(n)):
        fs.append(frame(q, 1000 + i, proto=i % 2) if i % 7 != 6 else [
            frame(b"", ftype=3), frame(q, 1000 + i, ftype=9),
            frame(bytes(23)), frame(q, 1000 + i, plen=24 + len(q) - 1),
            frame(q, 1000 + i, proto=7)][i // 7 % 5])
    return fs


def run(big, table, fs, accept, rbuf=None, shift=0):
    """One burst; every output held against the reference. Returns the
    reference's frames and the workspace."""
    import torch
    ws = table.frames(len(fs), rbuf=rbuf)
    fbuf = torch.frombuffer(bytearray(bytes(shift) + b"".join(fs)),
                            dtype=torch.uint8).cuda()[shift:]
    foff = torch.tensor(list(accumulate(map(len, fs), initial=0)),
                        dtype=torch.int32).cuda()
    want = [big.answer_frame(f, i, SEED, accept) for i, f in enumerate(fs)]
    check(ws, ws.resolve(fbuf, foff, SEED, accept), want, rbuf is None)
    return want, ws


def check(ws, out, want, roomy=True):
    data, end = out[0].cpu().numpy().tobytes(), ws.end()
    rstart, rlen = out[1].tolist(), out[2].tolist()
    got = [data[s:s + n] if n else b"" for s, n in zip(rstart, rlen)]
    served = [i for i, n in enumerate(rlen) if n]
    if roomy:
        assert got == want and ws.dropped() == 0
    assert all(got[i] == want[i] for i in served)
    assert len(served) + ws.dropped() == sum(map(bool, want))
    assert sorted(out[3][:ws.misses()].tolist()) == \
        [i for i, n in enumerate(rlen) if not n]
    stream, at = [], 0  # whole REPLY frames: the served ones, each once
    while at < end:
        assert data[at:at + 2] == b"\xb5\x02"
        stream.append(data[at:at + 6 + int.from_bytes(data[at + 2:at + 6],
                                                      "little")])
        at += len(stream[-1])
    assert at == end == sum(rlen) <= len(data)
    assert sorted(stream) == sorted(got[i] for i in served)


@pytest.mark.parametrize("n", [1, 64, 65, 3 * 64 + 5])
@pytest.mark.parametrize("accept", [0, EDNS | ANYCASE])
def test_frame_kinds(big, table, accept, n):
    want, _ = run(big, table, batch(n), accept)
    assert want[0] and (n == 1 or not all(want))
    if n > 64:  # kinds 0..3 are unserved, proto 7 is served as TCP is
        assert [bool(want[i]) for i in range(6, 35, 7)] == \
            [False] * 4 + [accept != 0]
        assert not accept or max(map(len, want)) > 4096


def test_all_miss_tile_claims_nothing(big, table):
    fs = batch(64) + [frame(wire(b"absent%d.foo.com" % i), i)
                      for i in range(64)] + batch(5)
    want, _ = run(big, table, fs, EDNS)
    assert any(want[:64]) and not any(want[64:128]) and any(want[128:])


def test_tcp_size_edges(big, table):
    stored, fs, lens = [512, 513, 4085, 4086, 4096], [], []
    for t in stored:
        q = wire(b"t%d.foo.com" % t, qid=t)
        for j, (query, lim, e) in enumerate(
                [(q, 512, 0), (edns(q, size=512), 512, 11),
                 (edns(q, size=4096), 4096, 11)]):
            fs += [frame(query, 8 * t + j), frame(query, 8 * t + j + 4, 1)]
            lens += [10 + (t + e if t + e <= lim else len(q) + e),
                     10 + t + e]
    # 131 copy jobs and 3904 bytes: listed, cut and dealt out
    fs.append(frame(wire(b"_s._tcp.m64.foo.com", 33), 7, proto=1))
    lens.append(10 + 37 + 3857)
    want, ws = run(big, table, fs, EDNS)
    assert [len(w) for w in want] == lens and max(lens) == ws.REPLY_MAX
    assert ws.rbuf.numel() == len(fs) * ws.REPLY_MAX
    data = b"".join(fs)  # one tile: the stream is in frame order
    assert ws.resolve_bytes(data + fs[0][:40], SEED, EDNS) == \
        (b"".join(want), [], len(data))


@pytest.mark.parametrize("shift,long", [(1, 0), (2, 0), (3, 0), (0, 1),
                                        (3, 1)])
def test_alignment_and_unstaged_tile(big, table, shift, long):
    fs = batch(70)
    if long:  # tile 0 spans more than LDS holds: read from global memory
        fs[6] = frame(bytes(20000), ftype=9)
    want, _ = run(big, table, fs, EDNS | ANYCASE, shift=shift)
    assert sum(map(bool, want)) > 50


def test_capacity(big, table):
    import torch
    fs = batch(3 * 64 + 5)
    cap = sum(len(big.answer_frame(f, i, SEED, 3))
              for i, f in enumerate(fs)) // 2
    guard = torch.full((cap + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    _, ws = run(big, table, fs, 3, rbuf=guard[:cap])
    assert guard[cap:].tolist() == [0xAA] * 64
    assert ws.dropped() > 0 and 0 < ws.end() <= cap


def test_no_host_round_trip_and_arguments(big, table):
    import torch
    fs = batch(70)
    fbuf = torch.frombuffer(bytearray(b"".join(fs)), dtype=torch.uint8).cuda()
    foff = torch.tensor(list(accumulate(map(len, fs), initial=0)),
                        dtype=torch.int32).cuda()
    ws = table.frames(len(fs))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ws.resolve(fbuf, foff, SEED, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(ws, out, [big.answer_frame(f, i, SEED, 3)
                    for i, f in enumerate(fs)])
    for bad, args in [(ValueError, (fbuf, foff, 0, 4)),
                      (TypeError, (fbuf, foff.long())),
                      (ValueError, (fbuf[None], foff))]:
        with pytest.raises(bad):
            ws.resolve(*args)
    with pytest.raises(ValueError):
        table.frames(len(fs) - 1).resolve(fbuf, foff)
