"""resolve(..., oversize=True) (native/gpu/resolvelarge.cpp) on an image
with a 4096-byte ceiling, against the accept test's Python reference
with its size rule replaced by the server's: a hit is served in full
when reply and OPT tail fit what the query may take, else truncated.
Exact bytes, exact offsets."""
from itertools import accumulate

import pytest

from binder_amd import _native
from test_answer_image import wire
from test_gpuresolve_accept_box import (ANYCASE, EDNS, OPT_TAIL, AcceptRef,
                                        edns, gr)  # noqa: F401
from test_gpuresolve_box import dotted, rnd

pytestmark = pytest.mark.gpu


def tensors(queries):
    import torch
    return (torch.frombuffer(bytearray(b"".join(queries)), dtype=torch.uint8),
            torch.tensor(list(accumulate(map(len, queries), initial=0)),
                         dtype=torch.int32))


class LimRef(AcceptRef):
    def __init__(self):
        super().__init__()
        self.image = _native.AnswerImage(max_reply=4096)

    def answer_lim(self, q, index, seed, accept):
        end = 12
        while end < len(q) and 0 < q[end] < 64:
            end += 1 + q[end]
        end += 1  # the root byte: the name is q[12:end]
        norm, limit, tail = q, 512, b""
        if accept & ANYCASE:
            norm = q[:12] + q[12:end].lower() + q[end:]
        if accept & EDNS and q[10:12] == b"\0\1":
            o = q[end + 4:]
            if len(q) > 300 or len(o) < 11 or o[:3] != b"\0\0\x29" or \
                    o[5:7] != b"\0\0" or \
                    11 + int.from_bytes(o[9:11], "big") > len(o):
                return b""
            limit = min(max(int.from_bytes(o[3:5], "big"), 512), 4096)
            norm, tail = norm[:10] + b"\0\0" + norm[12:end + 4], OPT_TAIL
        r = self.answer(norm, index, seed)
        if r and len(r) + len(tail) > limit:  # truncated: TC, the question
            return (r[:2] + bytes([r[2] | 2, r[3], 0, 1, 0, 0, 0, 0, 0,
                                   len(tail) and 1]) + q[12:end + 4] + tail)
        if r and norm[12:end] != q[12:end]:  # echo, clipped to the head
            p = _native.parse_fast(norm)
            k = min(end, len(self.table[p[0], 33 if p[1] else 1][0]))
            r = r[:12] + q[12:k] + r[k:]
        if r and tail:
            ar = (int.from_bytes(r[10:12], "big") + 1) & 0xFFFF
            r = r[:10] + ar.to_bytes(2, "big") + r[12:] + tail
        return r

    def check_lim(self, gr, queries, accept, seed=0, table=None):
        table = table or gr.GpuAnswerTable(self.image)
        rbuf, roff = table.resolve(*tensors(queries), seed, accept=accept,
                                   oversize=True)
        want = [self.answer_lim(q, i, seed, accept)
                for i, q in enumerate(queries)]
        assert roff.tolist() == list(accumulate(map(len, want), initial=0))
        assert rbuf.cpu().numpy().tobytes() == b"".join(want)
        assert table.resolve_list(queries, seed, accept, oversize=True) == \
            [w or None for w in want]
        return want


def members(n):
    """Uneven segments: 9 of them make 484 bytes, 64 make 3857."""
    return [(rnd(32 + m % 23, m), rnd(16 + m % 5, 300 + m)) for m in range(n)]


def fill(ref, large):
    """Hosts and an 8-member service, and with `large` wire replies at the
    size edges and services of 33 and 64 members."""
    for i in range(40):
        ref.reply(b"h%d.foo.com" % i, 1, rnd(29 + i, i))
    ref.service(b"_s._tcp.m8.foo.com", 33, rnd(40, 1), members(8))
    for t in (512, 513, 4085, 4086, 4096) if large else (512,):
        ref.reply(b"t%d.foo.com" % t, 1, rnd(t, t))
    for n in (33, 64) if large else ():
        ref.service(b"_s._tcp.m%d.foo.com" % n, 33, rnd(37, n), members(n))
        ref.service(b"m%d.foo.com" % n, 1, rnd(25, n),
                    [(a, b"") for a, _ in members(n)])
    return ref


@pytest.fixture(scope="module")
def big():
    return fill(LimRef(), True)


@pytest.mark.parametrize("t", [512, 513, 4085, 4086, 4096])
def test_size_edges(gr, big, t):
    q = wire(b"t%d.foo.com" % t)
    sizes = [0, 512, 523, 524, 4095, 4096, 65535]
    got = big.check_lim(gr, [q] + [edns(q, size=s) for s in sizes], EDNS)
    limits = [512] + [min(max(s, 512), 4096) for s in sizes]
    assert [len(g) for g in got] == [
        t + e if t + e <= lim else len(q) + e
        for lim, e in zip(limits, [0] + [11] * 7)]


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("n", [9, 33, 64])
def test_services(gr, n, seed):
    """9 members stay with their group in emit, 33 and 64 are drained by
    the workgroup; the same query twice draws two orders."""
    ref = LimRef()
    ref.service(b"_x._tcp.s.foo", 33, rnd(37, 7), members(n))
    ref.service(b"s.foo", 1, rnd(25, 8), [(a, b"") for a, _ in members(n)])
    ref.reply(b"w.foo", 1, rnd(45, 9))
    qs = [wire(b"_x._tcp.s.foo", 33, qid=1), wire(b"s.foo", qid=2, flags=0),
          wire(b"w.foo")]
    got = ref.check_lim(gr, ([edns(q, size=4096) for q in qs] + qs) * 2,
                        EDNS, seed)
    # without an OPT: header, question; the 9-member A form fits 512
    assert [len(g) for g in got[3:6]] == [12 + 19, 349 if n == 9 else 12 + 11,
                                          45]
    assert got[0] != got[6] and sorted(got[0]) == sorted(got[6])
    if n == 64:
        assert 2048 < len(got[0]) <= 4096 and got[3] == got[9]


def mixed_queries(n):
    qs = []
    for i in range(n):
        host = b"h%d.foo.com" % (i * 7 % 40)
        qs.append([
            wire(b"_s._tcp.m64.foo.com", 33, qid=i),             # truncated
            wire(host, qid=i),
            edns(wire(b"_s._tcp.m64.foo.com", 33, qid=i), size=4096),
            wire(b"absent%d.foo.com" % i, qid=i),
            wire(host.upper(), qid=i, flags=0),
            edns(wire(b"m33.foo.com", qid=i), size=1000),        # truncated
            edns(wire(host, qid=i), rdata=b"\0\x0a\0\x08" + rnd(8, i)),
            edns(wire(b"_S._tcp.M33.foo.com", 33, qid=i), size=4096),
            wire(b"_s._tcp.m8.foo.com", 33, qid=i),
            edns(wire(b"T4086.foo.com", qid=i), size=4096)][i % 10])
    return qs


@pytest.mark.parametrize("n", [1, 17, 129])  # one emit block + 1, TILE + 1
@pytest.mark.parametrize("accept", [0, EDNS | ANYCASE])
def test_mixed_batch(gr, big, accept, n):
    got = big.check_lim(gr, mixed_queries(n), accept, seed=5)
    assert [bool(g) for g in got] == [
        (i % 10 in (0, 1, 8)) or (accept != 0 and i % 10 != 3)
        for i in range(n)]


def test_truncated_longest_name(gr):
    """255 wire bytes of name, asked in mixed case: id, RD and the
    question come from the query, flags and rcode from the stored head."""
    ref, key = LimRef(), dotted(253)
    head = b"\0\0\x84\x03" + rnd(8, 1)
    ref.reply(key, 1, head + rnd(600, 2))
    asked = key[:100] + key[100:].upper()
    qs = [wire(asked, qid=0x1234, flags=0x0100), wire(asked, qid=0x4321,
                                                      flags=0),
          edns(wire(asked, qid=7), size=600), wire(key, qid=8)]
    assert len(qs[0]) == 12 + 255 + 4
    got = ref.check_lim(gr, qs, EDNS | ANYCASE)
    assert got[0] == b"\x12\x34\x87\x03\0\1" + bytes(6) + qs[0][12:]
    assert got[1] == b"\x43\x21\x86\x03\0\1" + bytes(6) + qs[1][12:]
    assert got[2] == (b"\0\x07\x87\x03\0\1\0\0\0\0\0\1" + qs[0][12:] +
                      OPT_TAIL)
    assert ref.check_lim(gr, qs, 0)[:3] == [b""] * 3


@pytest.mark.parametrize("accept", [0, EDNS | ANYCASE])
def test_without_the_switch(gr, big, accept):
    """oversize=False on the large table: entries above 512 bytes are not
    served, the rest is the default image's answer, burst included."""
    small = fill(AcceptRef(), False)
    qs = mixed_queries(40) + [wire(b"t%d.foo.com" % t) for t in (512, 513)]
    want = small.check_ext(gr, qs, accept, seed=5)
    assert sum(map(bool, want)) == (17 if accept else 9)
    table = gr.GpuAnswerTable(big.image)
    assert table.max_reply == 4096
    assert table.resolve_list(qs, 5, accept) == [w or None for w in want]
    rbuf, rstart, rlen = table.burst(64).resolve(*tensors(qs), 5, accept)
    data = rbuf.cpu().numpy().tobytes()
    assert [data[a:a + n] for a, n in zip(rstart.tolist(), rlen.tolist())] \
        == want


def test_apply_large_delta(gr, big):
    table = gr.GpuAnswerTable(big.image)
    ref, mem = fill(LimRef(), True), members(49)
    head = rnd(3000 - sum(len(a) + len(b) for a, b in mem), 3)
    delta = _native.AnswerDelta(max_reply=4096)
    delta.upsert_service(b"_s._tcp.new.foo.com", 33, head, mem)
    ref.table[b"_s._tcp.new.foo.com", 33] = (head, mem)
    qs = [edns(wire(b"_s._tcp.new.foo.com", 33), size=4096),
          wire(b"_s._tcp.new.foo.com", 33), wire(b"h1.foo.com")]
    table.apply(delta)
    got = ref.check_lim(gr, qs, EDNS, 9, table)
    assert len(got[0]) == 3000 + 11 and got[1][2] & 2
    delta = _native.AnswerDelta(max_reply=513)
    delta.invalidate(b"new.foo.com")
    del ref.table[b"_s._tcp.new.foo.com", 33]
    table.apply(delta)
    assert list(map(len, ref.check_lim(gr, qs, EDNS, 9, table))) == [0, 0, 30]
    with pytest.raises(ValueError):
        gr.GpuAnswerTable(_native.AnswerImage()).apply(delta)
