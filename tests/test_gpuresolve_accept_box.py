"""The GPU batch resolver's opt-in kernel pair (native/gpu/resolveext.cpp,
resolve(..., accept=...)) against the box test's Python reference: the
name is lowercased and the OPT record dropped, the bound CPU parser and
the dict answer as before, and the echo, ARCOUNT, tail and size-limit
rules are applied to that answer. Exact bytes, exact offsets."""
import struct
from itertools import accumulate

import pytest

import dnswire
from binder_amd import _native
from test_answer_image import wire
from test_gpuresolve_box import Ref, dotted, rnd

pytestmark = pytest.mark.gpu

EDNS, ANYCASE = 1, 2
OPT_TAIL = bytes.fromhex("0000290578000000000000")


@pytest.fixture(scope="module")
def gr():
    from binder_amd import gpuresolve
    assert (gpuresolve.ACCEPT_EDNS, gpuresolve.ACCEPT_ANYCASE) == (1, 2)
    return gpuresolve


def opt(size=1232, rdata=b"", xrcode=0, version=0, flags=0, name=b"\0",
        rtype=41, rdlen=None):
    return name + struct.pack(">HHBBHH", rtype, size, xrcode, version, flags,
                              len(rdata) if rdlen is None else rdlen) + rdata


def edns(q, ar=1, **kw):
    """q with ARCOUNT `ar` and one OPT record behind it."""
    return q[:10] + struct.pack(">H", ar) + q[12:] + opt(**kw)


class AcceptRef(Ref):
    def answer_ext(self, q, index, seed, accept):
        end = 12
        while end < len(q) and 0 < q[end] < 64:
            end += 1 + q[end]
        end += 1  # the root byte: the name is q[12:end]
        norm, limit = q, None
        if accept & ANYCASE:
            norm = q[:12] + q[12:end].lower() + q[end:]
        if accept & EDNS and q[10:12] == b"\0\1":
            o = q[end + 4:]
            if len(q) > 300 or len(o) < 11 or o[:3] != b"\0\0\x29" or \
                    o[5:7] != b"\0\0" or \
                    11 + int.from_bytes(o[9:11], "big") > len(o):
                return b""
            limit = min(max(int.from_bytes(o[3:5], "big"), 512), 4096)
            norm = norm[:10] + b"\0\0" + norm[12:end + 4]
        r = self.answer(norm, index, seed)
        if r and norm[12:end] != q[12:end]:  # echo, clipped to the head
            p = _native.parse_fast(norm)
            k = min(end, len(self.table[p[0], 33 if p[1] else 1][0]))
            r = r[:12] + q[12:k] + r[k:]
        if r and limit is not None:
            if len(r) + 11 > limit:
                return b""
            ar = (int.from_bytes(r[10:12], "big") + 1) & 0xFFFF
            r = r[:10] + ar.to_bytes(2, "big") + r[12:] + OPT_TAIL
        return r

    def check_ext(self, gr, queries, accept, seed=0):
        import torch
        qbuf = torch.frombuffer(bytearray(b"".join(queries)),
                                dtype=torch.uint8)
        qoff = torch.tensor(list(accumulate(map(len, queries), initial=0)),
                            dtype=torch.int32)
        rbuf, roff = gr.GpuAnswerTable(self.image).resolve(
            qbuf, qoff, seed, accept=accept)
        want = [self.answer_ext(q, i, seed, accept)
                for i, q in enumerate(queries)]
        assert roff.tolist() == list(accumulate(map(len, want), initial=0))
        assert rbuf.cpu().numpy().tobytes() == b"".join(want)
        return want


@pytest.fixture(scope="module")
def mixed():
    ref = AcceptRef()
    for i in range(300):
        ref.reply(b"h%d.bench.foo.com" % i, 1, rnd(29 + i % 40, i))
    mem = [(rnd(16 + m, m), rnd(20 - m, 50 + m)) for m in range(8)]
    ref.service(b"_http._tcp.svc.foo.com", 33, rnd(40, 1), mem)
    ref.service(b"svc.foo.com", 1, rnd(30, 2), [(a, b"") for a, _ in mem])
    for total in (501, 502, 512):
        ref.reply(b"t%d.foo.com" % total, 1, rnd(total, total))
    return ref


# what each kind of the mixed batch needs in `accept`; None is the miss
NEEDS = [0, ANYCASE, EDNS, EDNS | ANYCASE, EDNS, None, ANYCASE]


def mixed_queries(n):
    qs = []
    for i in range(n):
        host = b"h%d.bench.foo.com" % (i * 13 % 300)
        qs.append([
            wire(host, qid=i),
            wire(host.upper(), qid=i),
            edns(wire(b"svc.foo.com", qid=i, flags=0)),
            edns(wire(host.replace(b"bench", b"bEnCh"), qid=i), size=4096),
            edns(wire(host, qid=i), rdata=b"\0\x0a\0\x08" + rnd(8, i)),
            wire(b"absent%d.foo.com" % i, qid=i),
            wire(b"_Http._TCP.svc.foo.com", 33, qid=i)][i % 7])
    return qs


@pytest.mark.parametrize("n", [1, 65, 129])  # 129 = TILE + 1
@pytest.mark.parametrize("accept", [0, 1, 2, 3])
def test_mixed_batch(gr, mixed, accept, n):
    assert gr.TILE + 1 == 129
    qs = mixed_queries(n)
    got = mixed.check_ext(gr, qs, accept, seed=5)
    assert [bool(g) for g in got] == [
        NEEDS[i % 7] is not None and NEEDS[i % 7] & ~accept == 0
        for i in range(n)]
    if accept == 0:  # the default path, unchanged
        assert got == mixed.check(gr, qs, seed=5)
    with pytest.raises(ValueError):
        gr.GpuAnswerTable(mixed.image).resolve_list(qs, accept=4)


@pytest.mark.parametrize("total", [501, 502, 512])
def test_opt_advertised_size(gr, mixed, total):
    sizes = [0, 511, 512, 522, 523, 4096, 65535]
    got = mixed.check_ext(gr, [edns(wire(b"t%d.foo.com" % total), size=s)
                               for s in sizes], EDNS)
    assert [bool(g) for g in got] == [
        total + 11 <= min(max(s, 512), 4096) for s in sizes]


def test_opt_edges(gr, mixed):
    q = wire(b"h7.bench.foo.com")
    e = edns(q)
    cases = [(edns(q, rdata=b"abcd", rdlen=5), False),
             (edns(q, rdata=b"abcd"), True),
             (edns(q, version=1), False), (edns(q, xrcode=1), False),
             (edns(q, flags=0x8000), True),
             (edns(q, ar=2) + opt(), False),
             (edns(q, name=b"\1a\0"), False), (edns(q, rtype=42), False),
             (e[:-1], False), (q[:10] + b"\0\1" + q[12:], False),
             (e + b"\0" * (300 - len(e)), True),
             (e + b"\0" * (301 - len(e)), False),
             (e + b"\0" * 40000, False)]  # its tile is read unstaged
    qs = []
    for c, _ in cases:
        qs += [c, e]
    got = mixed.check_ext(gr, qs, EDNS | ANYCASE)
    assert [bool(g) for g in got] == [x for _, s in cases for x in (s, True)]


@pytest.mark.parametrize("klen", [7, 8, 9, 17, 255])
def test_fold_in_every_hash_word(gr, klen):
    """One uppercase byte at the first and last byte of each 8-byte hash
    word and of the tail word."""
    ref = AcceptRef()
    key = dotted(klen)
    ref.reply(key, 1, rnd(12 + klen + 6 + 16, klen))
    at = sorted({p for w in range(0, klen, 8)
                 for p in (w, min(w + 7, klen - 1)) if key[p:p + 1] != b"."})
    qs = [wire(key[:p] + key[p:p + 1].upper() + key[p + 1:]) for p in at]
    got = ref.check_ext(gr, qs, ANYCASE)
    assert all(got) and len(set(got)) == len(at)
    assert ref.check_ext(gr, qs, EDNS) == [b""] * len(at)


def test_case_and_header_edges(gr):
    """Range edges, the echo clamp, ARCOUNT's carry and wrap."""
    ref = AcceptRef()
    ref.reply(b"h7.foo", 1, rnd(30, 0))
    ref.reply(b"abc", 1, rnd(12, 1))
    ref.reply(b"abd", 1, rnd(13, 2))
    ref.service(b"s.foo", 1, rnd(12 + 7 - 1, 3), [(rnd(5, 4), b""),
                                                 (rnd(6, 5), b"")])
    ref.reply(b"carry", 1, rnd(10, 6) + b"\x00\xff" + rnd(20, 7))
    ref.reply(b"wrap", 1, rnd(10, 8) + b"\xff\xff" + rnd(20, 9))
    cases = [(wire(b"h7.fo" + bytes([c])), False) for c in b"@[`{"] + [
        (wire(b"H7.FOO"), True), (edns(wire(b"ABC")), True),
        (wire(b"aBd"), True), (edns(wire(b"S.Foo")), True),
        (edns(wire(b"carry")), True), (edns(wire(b"WRAP")), True)]
    got = ref.check_ext(gr, [c for c, _ in cases], EDNS | ANYCASE, seed=3)
    assert [bool(g) for g in got] == [s for _, s in cases]
    assert got[-2][10:12] == b"\x01\x00" and got[-1][10:12] == b"\x00\x00"


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("n", [1, 64])
def test_services(gr, n, seed):
    ref = AcceptRef()
    mem = [(rnd(2 + m % 3, m), rnd(1 + m % 2, 300 + m)) for m in range(n)]
    ref.service(b"_x._tcp.s.foo", 33, rnd(37, 7), mem)
    ref.service(b"s.foo", 1, rnd(25, 8), [(rnd(3 + m % 5, m), b"")
                                         for m in range(n)])
    plain = [wire(b"_x._tcp.s.foo", 33, qid=1), wire(b"s.foo", qid=2)] * 3
    base = ref.check_ext(gr, plain, 0, seed)
    got = ref.check_ext(gr, [edns(q) for q in plain], EDNS | ANYCASE, seed)
    for b, g in zip(base, got):  # the base path's draw, then the tail
        assert g[:10] + b[10:12] + g[12:] == b + OPT_TAIL
    ref.check_ext(gr, [edns(wire(b"_X._tCp.S.fOO", 33)), wire(b"S.FOO")] * 3,
                  EDNS | ANYCASE, seed)


def test_reply_parses(gr):
    """A real reply, asked for in mixed case with an OPT."""
    name = dnswire.labels("example.foo.com")
    asked = dnswire.labels("ExAmPlE.foo.com")
    msg = dnswire.Msg(0, dnswire.flags(qr=True, aa=True),
                      [dnswire.Question(name, dnswire.A)],
                      [dnswire.RR(name, dnswire.A, dnswire.IN, 30,
                                  bytes([10, 0, 0, k])) for k in (1, 2)])
    ref = AcceptRef()
    ref.reply(b"example.foo.com", 1, dnswire.build(msg, compress=True))
    q = edns(wire(b"ExAmPlE.foo.com", qid=0x1234))
    got = dnswire.parse(ref.check_ext(gr, [q], EDNS | ANYCASE)[0])
    assert got.id == 0x1234 and got.flags & dnswire.RD
    assert got.questions == [dnswire.Question(asked, dnswire.A)]
    assert [(r.name, r.rdata) for r in got.answers] == [
        (asked, bytes([10, 0, 0, 1])), (asked, bytes([10, 0, 0, 2]))]
    assert got.additionals == [dnswire.RR((), dnswire.OPT, 1400, 0, b"")]
