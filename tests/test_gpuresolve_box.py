"""GPU batch resolver (native/gpu/resolve.cpp) against a plain Python
reference: the bound CPU parser decides accept/reject and the name, a
dict holds the table, and the assembly and member-order generator are
written out below. Exact bytes, exact offsets."""
import random

import pytest

from binder_amd import _native
from test_answer_image import wire

pytestmark = pytest.mark.gpu

M64 = 2 ** 64 - 1
GOLD = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def gr():
    from binder_amd import gpuresolve
    return gpuresolve


def sm(x):
    x = (x + GOLD) & M64
    z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def member_order(n, seed, index):
    s0 = seed ^ ((index * 0xD6E8FEB86659FD93) & M64)
    order, k = list(range(n)), 0
    for i in range(n - 1, 0, -1):
        j = (sm((s0 + k * GOLD) & M64) >> 32) % (i + 1)
        order[i], order[j] = order[j], order[i]
        k += 1
    return order


class Ref:
    """The image under test and the dict that mirrors it."""

    def __init__(self):
        self.image, self.table = _native.AnswerImage(), {}

    def reply(self, name, qtype, reply):
        self.image.add_reply(name, qtype, reply)
        self.table[name, qtype] = (reply, None)

    def service(self, name, qtype, head, members):
        self.image.add_service(name, qtype, head, members)
        self.table[name, qtype] = (head, members)

    def answer(self, q, index, seed):
        p = _native.parse_fast(q)
        ent = p and self.table.get((p[0], 33 if p[1] else 1))
        if not ent:
            return b""
        r, members = ent
        if members is not None:
            order = member_order(len(members), seed, index)
            r = r + b"".join(members[m][0] for m in order) + \
                b"".join(members[m][1] for m in order)
        return q[:2] + bytes([r[2] | (q[2] & 1)]) + r[3:]

    def check(self, gr, queries, seed=0):
        """Resolve on the GPU; compare with the reference; return the
        replies."""
        import torch
        offs = [0]
        for q in queries:
            offs.append(offs[-1] + len(q))
        qbuf = torch.frombuffer(bytearray(b"".join(queries)),
                                dtype=torch.uint8)
        rbuf, roff = gr.GpuAnswerTable(self.image).resolve(
            qbuf, torch.tensor(offs, dtype=torch.int32), seed)
        want = [self.answer(q, i, seed) for i, q in enumerate(queries)]
        woff = [0]
        for w in want:
            woff.append(woff[-1] + len(w))
        assert roff.dtype == torch.int64 and roff.tolist() == woff
        assert rbuf.cpu().numpy().tobytes() == b"".join(want)
        return want


def rnd(n, salt):
    return random.Random(salt).randbytes(n)


def dotted(length, fill=b"k"):
    """A name of exactly `length` bytes in labels of at most 63."""
    labels, left = [], length
    while left > 0:
        n = min(63, left if left <= 63 or left >= 65 else 62)
        labels.append(fill * n)
        left -= n + 1
    return b".".join(labels)


@pytest.fixture(scope="module")
def mixed():
    ref = Ref()
    for i in range(300):
        ref.reply(b"h%d.bench.foo.com" % i, 1, rnd(29 + i % 40, i))
    mem = [(rnd(16 + m, m), rnd(20 - m, 50 + m)) for m in range(8)]
    ref.service(b"_http._tcp.svc.foo.com", 33, rnd(40, 1), mem)
    ref.service(b"svc.foo.com", 1, rnd(30, 2), [(a, b"") for a, _ in mem])
    return ref


def mixed_queries(n):
    qs = []
    for i in range(n):
        kind = i % 7
        if kind == 3:
            qs.append(wire(b"_http._tcp.svc.foo.com", 33, qid=i))
        elif kind == 5:
            qs.append(wire(b"svc.foo.com", qid=i, flags=0))
        elif kind == 6:
            qs.append(wire(b"absent%d.foo.com" % i, qid=i))
        else:
            qs.append(wire(b"h%d.bench.foo.com" % (i * 13 % 300), qid=i))
    return qs


def test_empty_batch_and_api(gr):
    import torch
    t = gr.GpuAnswerTable(Ref().image)
    rbuf, roff = t.resolve(torch.empty(0, dtype=torch.uint8),
                           torch.zeros(1, dtype=torch.int32))
    assert rbuf.numel() == 0 and roff.tolist() == [0]
    assert t.resolve_list([wire(b"a.b"), b""]) == [None, None]
    with pytest.raises(TypeError):
        gr.GpuAnswerTable(b"raw bytes")


@pytest.mark.parametrize("tiles,plus", [(0, 1), (0, 63), (0, 64), (0, 65),
                                        (1, -1), (1, 0), (1, 1), (2, 3)])
def test_batch_sizes(gr, mixed, tiles, plus):
    """1, 63, 64, 65, T-1, T, T+1, 2T+3 queries over a mixed table."""
    n = tiles * gr.TILE + plus
    qs = mixed_queries(n)
    got = mixed.check(gr, qs, seed=5)
    assert sum(1 for g in got if g) == sum(1 for i in range(n) if i % 7 != 6)
    t = gr.GpuAnswerTable(mixed.image)
    assert t.resolve_list(qs, seed=5) == [g or None for g in got]


@pytest.mark.parametrize("klen", [1, 7, 8, 9, 15, 16, 17, 63, 64, 249, 255])
def test_key_lengths(gr, klen):
    """The hash's 8-byte steps, for A and SRV keys of klen bytes, plus
    near misses of the same length; each query also padded with
    trailing bytes to 300 (served) and 301 (not)."""
    ref = Ref()
    key = dotted(klen)
    names = [(key, 1)]
    if klen <= 249:  # _s._t. + key fits 255
        names.append((b"_s._t." + key, 33))
    for i, (name, qt) in enumerate(names):
        ref.reply(name, qt, rnd(40 + i, klen))
    qs = []
    for name, qt in names:
        q = wire(name, qt)
        other = name[:-1] + b"z"
        qs += [q, wire(other, qt), q + b"\0" * (300 - len(q)),
               q + b"\0" * (301 - len(q)), wire(name, 34 - qt)]
    got = ref.check(gr, qs)
    assert [bool(g) for g in got[:5]] == [True, False, True, False, False]


def test_longest_name_and_root(gr):
    """256 dotted bytes pass the parser but no key can be that long;
    the root name (the shortest valid query, 17 bytes) is a key."""
    ref = Ref()
    ref.reply(b"", 1, rnd(17, 0))
    ref.reply(dotted(255), 1, rnd(18, 1))
    longest = dotted(254, b"m") + b".x"
    assert len(_native.parse_fast(wire(longest))[0]) == 256
    got = ref.check(gr, [wire(longest), wire(b""), wire(dotted(255)),
                         wire(dotted(254, b"m") + b".xy")])
    assert [len(g) for g in got] == [0, 17, 18, 0]


def test_probe_chains(gr):
    """Chains that wrap past the last of 1024 slots, three SRV names on
    one hash, A and SRV of one name, an absent name inside a chain."""
    ref = Ref()
    ref.reply(b"seed", 1, rnd(12, 0))  # brings the 1024 slots
    tail = [b"h%d" % i for i in range(5000)
            if ref.image.home_slot(b"h%d" % i, 1) >= 1022]
    assert len(tail) >= 6
    for i, name in enumerate(tail[::2]):
        ref.reply(name, 1, rnd(20 + i, i))
    for i, name in enumerate([b"_a._tcp.d", b"_b._tcp.d", b"_c._udp.d"]):
        ref.reply(name, 33, rnd(30 + i, 100 + i))
    ref.reply(b"_a._tcp.d", 1, rnd(34, 200))
    ref.reply(b"d", 1, rnd(35, 201))
    assert len(ref.image.slots()) == 1024 * 16
    qs = [wire(n) for n in tail] + [
        wire(b"_c._udp.d", 33), wire(b"_a._tcp.d", 33), wire(b"_a._tcp.d"),
        wire(b"_b._tcp.d", 33), wire(b"_d._tcp.d", 33), wire(b"d"),
        wire(b"d", 33), wire(b"_b._tcp.d")]
    got = ref.check(gr, qs)
    assert [bool(g) for g in got[:len(tail)]] == \
        [i % 2 == 0 for i in range(len(tail))]
    assert [len(g) for g in got[len(tail):]] == [32, 30, 34, 31, 0, 35, 0, 0]


def test_empty_image(gr):
    assert Ref().check(gr, mixed_queries(9)) == [b""] * 9


def test_not_served_wires(gr, mixed):
    """Every reject rule once, between hits."""
    hit = wire(b"h7.bench.foo.com")
    srv = wire(b"_http._tcp.svc.foo.com", 33)
    ptr = hit[:12] + b"\x02h7\xc0\x0c" + hit[-4:]
    bad = [wire(b"H7.bench.foo.com"), ptr,
           wire(b"h7.bench.foo.com", counts=(1, 0, 0, 1)),
           wire(b"h7.bench.foo.com", 28), wire(b"h7.bench.foo.com", qclass=3),
           wire(b"h7.bench.foo.com", flags=0x8100),
           hit[:12], hit[:20], hit[:-4], hit[:-2], hit[:-1],
           wire(b"_http", 33), wire(b"_http._tcp", 33),
           wire(b"_ht_tp._tcp.svc.foo.com", 33),
           wire(b"_http._t_cp.svc.foo.com", 33),
           wire(b"http._tcp.svc.foo.com", 33)]
    assert all(_native.parse_fast(b) is None for b in bad)
    qs = [hit, srv]
    for b in bad:
        qs += [b, hit, srv]
    got = mixed.check(gr, qs)
    assert [bool(g) for g in got[2:]] == [False, True, True] * len(bad)


def test_copy_alignment(gr):
    """Wire replies of the edge lengths at every source residue mod 4,
    each fetched at every destination residue mod 4."""
    ref, used, seen = Ref(), 0, set()
    ref.reply(b"f", 1, rnd(13, 99))  # filler: moves dst on by one mod 4
    used += 2 + 1 + 4 + 13
    names = []
    for length in [12, 13, 14, 15, 16, 17, 31, 33, 511, 512]:
        for res in range(4):
            name = b"r%d-%d" % (length, res)
            name += b"x" * ((res - (used + 6 + len(name))) % 4)
            ref.reply(name, 1, rnd(length, length * 4 + res))
            names.append((name, length, (used + 6 + len(name)) % 4))
            used += 6 + len(name) + length
    arena = ref.image.arena()
    assert len(arena) == used
    qs, cursor = [], 0
    for name, length, src in names:
        assert arena.find(rnd(length, length * 4 + src)) % 4 == src
        for dst in range(4):
            while cursor % 4 != dst:
                qs.append(wire(b"f"))
                cursor += 13
            qs.append(wire(name))
            seen.add((length, src, cursor % 4))
            cursor += length
    assert len(seen) == 10 * 16
    ref.check(gr, qs)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_services(gr, n, seed):
    """A form (no second segments) and SRV form, unequal segments; the
    same query twice draws two orders."""
    ref = Ref()
    mem = [(rnd(2 + m % 3, m), rnd(1 + m % 2, 300 + m)) for m in range(n)]
    ref.service(b"_x._tcp.s.foo", 33, rnd(37, 7), mem)
    ref.service(b"s.foo", 1, rnd(25, 8), [(rnd(3 + m % 5, m), b"")
                                         for m in range(n)])
    ref.reply(b"w.foo", 1, rnd(45, 9))
    qs = [wire(b"_x._tcp.s.foo", 33, qid=1), wire(b"s.foo", qid=2, flags=0),
          wire(b"w.foo"), wire(b"_x._tcp.s.foo", 33, qid=1),
          wire(b"s.foo", qid=2, flags=0), wire(b"nope.foo")] * 3
    got = ref.check(gr, qs, seed)
    if n == 64:
        assert got[0] != got[3] and got[1] != got[4]
        assert sorted(got[0]) == sorted(got[3])
