"""resolve(..., oversize=True, policy=ZonePolicy(zone))
(native/gpu/resolvepolicy.cpp) against the oversize test's reference for
what the table answers, and against the real engine for what the server
answers from the query alone: a short classifier says which queries
those are, _native.StubEngine gives their bytes, and the accept test's
ARCOUNT + 1 and OPT tail rule is applied to them. Exact bytes, exact
offsets, exact tally."""
from itertools import accumulate

import pytest

from binder_amd import _native
from test_answer_image import wire
from test_gpuresolve_accept_box import (ANYCASE, EDNS, OPT_TAIL, edns, gr,  # noqa: F401,E501
                                        opt)
from test_gpuresolve_box import dotted
from test_gpuresolve_oversize_box import LimRef, fill, tensors

pytestmark = pytest.mark.gpu

NOTIMP, REFUSED = 4, 5
FULL, TRUNCATED, UNSERVED = "full", "truncated", None  # and the two rcodes
KINDS = [FULL, TRUNCATED, NOTIMP, REFUSED, UNSERVED]    # the tally's order
ENGINES = {}


def question_end(q):
    end = 12
    while end < len(q) and 0 < q[end] < 64:
        end += 1 + q[end]
    return end + 1  # behind the root byte


def policy_rcode(q, accept, zone):
    """The rcode the server answers q with from q alone, or None."""
    end = question_end(q)
    norm = q[:12] + (q[12:end].lower() if accept & ANYCASE else q[12:end])
    if accept & EDNS and q[10:12] == b"\0\1":
        o = q[end + 4:]
        if len(q) > 300 or len(o) < 11 or o[:3] != b"\0\0\x29" or \
                o[5:7] != b"\0\0" or \
                11 + int.from_bytes(o[9:11], "big") > len(o):
            return None
        norm, q = norm[:10] + b"\0\0" + norm[12:], q[:end + 4]
    # a candidate, whatever its type? The server drops a name above 255
    p = _native.parse_fast(norm + b"\0\1" + q[end + 2:])
    if not p or end - 12 > 255:
        return None
    name, qtype = p[0], int.from_bytes(q[end:end + 2], "big")
    if qtype not in (1, 12, 33):
        return NOTIMP
    if qtype == 33:
        labels = name.split(b".")
        if len(labels) < 3 or any(lab[:1] != b"_" or b"_" in lab[1:]
                                  for lab in labels[:2]):
            return REFUSED
        name = b".".join(labels[2:])
    if qtype != 12 and zone and not name.endswith(b"." + zone):
        return REFUSED
    return None


class PolRef(LimRef):
    def answer_pol(self, q, index, seed, accept, zone):
        """(reply, kind)"""
        rcode = policy_rcode(q, accept, zone)
        cut = question_end(q) + 4
        if rcode is None:
            r = self.answer_lim(q, index, seed, accept)
            # truncated: header and question, which no stored reply here
            # is as short as, and the tail of a served query with an OPT
            short = len(r) == cut + (11 if q[10:12] == b"\0\1" else 0)
            return r, (TRUNCATED if short else FULL) if r else UNSERVED
        bare = q[:10] + b"\0\0" + q[12:cut]
        got = set()
        for recursion in (False, True):  # and a store that is not ready
            key = zone, recursion
            if key not in ENGINES:
                ENGINES[key] = _native.StubEngine(zone.decode(), "dc1",
                                                  recursion)
                ENGINES[key].set_ready(not recursion)
            r, action = ENGINES[key].query_wire(bare)
            assert action == "respond" and r[3] == rcode, (q, r, action)
            got.add(r)
        assert len(got) == 1
        if q[10:12] == b"\0\1":
            r = r[:10] + b"\0\1" + r[12:] + OPT_TAIL
        return r, rcode

    def check_pol(self, gr, queries, accept, zone, seed=0):
        import torch
        table = gr.GpuAnswerTable(self.image)
        tally = torch.zeros(gr.TALLY_WORDS, dtype=torch.int64, device="cuda")
        want = [self.answer_pol(q, i, seed, accept, zone)
                for i, q in enumerate(queries)]
        for call in (1, 2):  # the tally is added to
            rbuf, roff = table.resolve(
                *tensors(queries), seed, accept=accept, oversize=True,
                policy=gr.ZonePolicy(zone), tally=tally)
            assert roff.tolist() == list(
                accumulate((len(w) for w, _ in want), initial=0))
            assert rbuf.cpu().numpy().tobytes() == b"".join(
                w for w, _ in want)
            assert tally.tolist() == [
                call * sum(k == kind for _, k in want) for kind in KINDS]
        return [kind for _, kind in want]


@pytest.fixture(scope="module")
def big():
    return fill(PolRef(), True)


def mixed_queries(n):
    qs = []
    for i in range(n):
        host = b"h%d.foo.com" % (i * 7 % 40)
        qs.append([
            wire(host, 28, qid=i),                            # AAAA, inside
            wire(host, qid=i),
            wire(b"_s._tcp.m64.foo.com", 33, qid=i),          # truncated
            edns(wire(b"x%d.bar.org" % i, 28, qid=i, flags=0)),
            wire(b"x.y.foo.com", 33, qid=i),                  # SRV shape
            wire(b"h%d.bar.org" % i, qid=i),                  # outside
            wire(b"absent%d.foo.com" % i, qid=i),
            wire(b"4.3.2.1.in-addr.arpa", 12, qid=i),
            wire(host.upper(), 28, qid=i),
            edns(wire(host, qid=i), size=4096)][i % 10])
    return qs


@pytest.mark.parametrize("n", [1, 65, 129])  # 129 = TILE + 1
@pytest.mark.parametrize("accept", [0, EDNS | ANYCASE])
def test_mixed_batch(gr, big, accept, n):
    qs = mixed_queries(n)
    kinds = [NOTIMP, FULL, TRUNCATED, accept and NOTIMP, REFUSED, REFUSED,
             UNSERVED, UNSERVED, accept and NOTIMP, accept and FULL]
    assert big.check_pol(gr, qs, accept, b"foo.com", seed=5) == [
        kinds[i % 10] or UNSERVED for i in range(n)]
    big.check_lim(gr, qs, accept, seed=5)  # policy=None: as before


@pytest.mark.parametrize("qtype", [0, 2, 16, 28, 65, 255, 0x0101, 0x0121,
                                   1, 33, 12])
def test_qtypes(gr, big, qtype):
    """Both type bytes count, and the zone does not for NOTIMP."""
    qs = [wire(b"h1.foo.com", qtype), wire(b"_s._tcp.m8.foo.com", qtype),
          wire(b"h1.bar.org", qtype, flags=0)]
    want = {1: [FULL, UNSERVED, REFUSED], 33: [REFUSED, FULL, REFUSED],
            12: [UNSERVED] * 3}.get(qtype, [NOTIMP] * 3)
    assert big.check_pol(gr, qs, 0, b"foo.com") == want


IN253, IN255 = (dotted(n - 8) + b".foo.com" for n in (253, 255))
EDGES = [  # name, type, what zone foo.com makes of it, what no zone does
    (b"foo.com", 1, REFUSED, UNSERVED), (b"a.foo.com", 1, UNSERVED, UNSERVED),
    (b"afoo.com", 1, REFUSED, UNSERVED), (b"com", 1, REFUSED, UNSERVED),
    (b"a.foo.com.x", 1, REFUSED, UNSERVED), (b"m", 1, REFUSED, UNSERVED),
    (b"", 1, REFUSED, UNSERVED), (b"a.FOO.com", 1, UNSERVED, UNSERVED),
    (b"h1.foo.com", 1, FULL, FULL), (b"h1.foo.com", 28, NOTIMP, NOTIMP),
    (IN253, 1, UNSERVED, UNSERVED), (dotted(253), 1, REFUSED, UNSERVED),
    # 257 wire bytes: the server drops the query
    (IN255, 1, UNSERVED, UNSERVED), (dotted(255), 1, UNSERVED, UNSERVED),
    (dotted(255), 28, UNSERVED, UNSERVED), (dotted(253), 28, NOTIMP, NOTIMP),
    (b"_a._b.foo.com", 33, REFUSED, UNSERVED),
    (b"_a._b.x.foo.com", 33, UNSERVED, UNSERVED),
    (b"_a._b", 33, REFUSED, REFUSED), (b"x.y.foo.com", 33, REFUSED, REFUSED),
    (b"_a._b_.x.foo.com", 33, REFUSED, REFUSED)]


@pytest.mark.parametrize("accept", [0, ANYCASE])
@pytest.mark.parametrize("zone", [b"foo.com", b""])
def test_zone_edges(gr, big, zone, accept):
    assert len(IN253) == 253 and len(wire(dotted(255))) == 12 + 257 + 4
    assert _native.StubEngine("foo.com").query_wire(wire(dotted(255))) == \
        (b"", "drop")
    got = big.check_pol(gr, [wire(n, t) for n, t, _, _ in EDGES], accept,
                        zone)
    assert got == [no_zone if zone == b"" else in_zone
                   for _, _, in_zone, no_zone in EDGES]


def test_zone_length_byte_is_no_label_byte(gr, big):
    """A zone whose first label has 45 bytes begins with 0x2D on the wire,
    which is '-': the match must begin at a label."""
    zone = b"k" * 45 + b".com"
    qs = [wire(b"x-" + zone), wire(b"x." + zone), wire(zone)]
    assert big.check_pol(gr, qs, 0, zone) == [REFUSED, UNSERVED, REFUSED]


@pytest.mark.parametrize("accept", [0, EDNS])
def test_edns(gr, big, accept):
    q = wire(b"h1.foo.com", 28)
    with_opt = NOTIMP if accept else UNSERVED
    cases = [(edns(q, size=s), with_opt) for s in (0, 512, 4096)] + [
        (edns(wire(b"x.bar.org"), rdata=b"abcd"), accept and REFUSED),
        (edns(q, version=1), UNSERVED), (edns(q, ar=2) + opt(), UNSERVED),
        (edns(q)[:-1], UNSERVED), (wire(b"h1.foo.com", 28, qclass=3), UNSERVED),
        (q + bytes(300 - len(q)), NOTIMP), (q + bytes(301 - len(q)), UNSERVED)]
    assert big.check_pol(gr, [c for c, _ in cases], accept, b"foo.com") == \
        [kind or UNSERVED for _, kind in cases]


def test_interface(gr, big):
    table = gr.GpuAnswerTable(big.image)
    with pytest.raises(ValueError):
        table.resolve_list([wire(b"a.b", 28)], policy=gr.ZonePolicy(b"b"))
    assert table.resolve_list([wire(b"a.b", 28, qid=7)], oversize=True,
                              policy=gr.ZonePolicy()) == [
        b"\0\x07\x85\x04\0\1" + bytes(6) + wire(b"a.b", 28)[12:]]
    for zone in (b"Foo.com", b"foo..com", b"foo.com.", b"k" * 64 + b".com",
                 dotted(254), b"foo.c\0m"):
        with pytest.raises(ValueError):
            gr.ZonePolicy(zone)
    assert len(gr.ZonePolicy(dotted(253)).wire) == 255
