"""The native DNS codec against tests/dnswire.py, in process.

Three kinds of evidence, none of which decodes a message with the codec
that produced it:

  * byte images written out by hand from RFC 1035/2782/3596/6891 (the
    derivation stands next to each), which check the oracle itself and
    are then fed to the native decoder;
  * native encode -> strict parse, and oracle build (with compression
    the native encoder never emits) -> native decode, over the goldens
    and over 2,000 seeded random messages each way;
  * wire the decoder must refuse.
"""
import random
import socket
import struct

import pytest

from binder_amd import require_native

import dnswire as w
from dnswire import RR, Msg, Question, RawName, WireError, labels

n = require_native()


def hx(*parts):
    return bytes.fromhex("".join(parts).replace(" ", ""))


# ------------------------------------------------------------------
# Hand-written images. Offsets are counted from the start of the
# message; the header is 12 octets (RFC 1035 4.1.1), so the first
# question name starts at offset 12 = 0x0c.
#
# web.foo.com as a question name (RFC 1035 3.1: length octet, label,
# ..., zero octet):
#   offset 12: 03 'w' 'e' 'b'     16: 03 'f' 'o' 'o'
#          20: 03 'c' 'o' 'm'     24: 00
# then QTYPE and QCLASS at 25..28, so the first record starts at 29.
QNAME_WEB = "03 776562 03 666f6f 03 636f6d 00"
WEB = labels("web.foo.com")
FOO = labels("foo.com")

# _http._tcp.foo.com:
#   12: 05 '_http'  18: 04 '_tcp'  23: 03 'foo'  27: 03 'com'  31: 00
# QTYPE/QCLASS at 32..35, first record at 36.
QNAME_SRV = "05 5f68747470 04 5f746370 03 666f6f 03 636f6d 00"

# 1.0.168.192.in-addr.arpa
QNAME_ARPA = ("01 31 01 30 03 313638 03 313932 "
              "07 696e2d61646472 04 61727061 00")

# flags 0x8400: QR (bit 15) and AA (bit 10), RFC 1035 4.1.1
GOLDEN = {
    # A, RFC 1035 3.4.1: owner is a pointer (c0 0c) to offset 12; type 1,
    # class 1, TTL 0x01020304, RDLENGTH 4, 192.168.0.1
    "A": (hx("1234 8400 0001 0001 0000 0000", QNAME_WEB, "0001 0001",
             "c00c 0001 0001 01020304 0004 c0a80001"),
          Msg(0x1234, 0x8400, [Question(WEB, w.A)],
              [RR(WEB, w.A, 1, 0x01020304, bytes([192, 168, 0, 1]))])),
    # the largest TTL the field holds
    "A-ttl-max": (
        hx("0001 8400 0001 0001 0000 0000", QNAME_WEB, "0001 0001",
           "c00c 0001 0001 ffffffff 0004 0a000001"),
        Msg(1, 0x8400, [Question(WEB, w.A)],
            [RR(WEB, w.A, 1, 0xFFFFFFFF, bytes([10, 0, 0, 1]))])),
    # AAAA, RFC 3596 2.2: type 28 = 0x1c, 16 octets, 2001:db8::1
    "AAAA": (hx("1235 8400 0001 0001 0000 0000", QNAME_WEB, "001c 0001",
                "c00c 001c 0001 00000e10 0010",
                "20010db8 00000000 00000000 00000001"),
             Msg(0x1235, 0x8400, [Question(WEB, w.AAAA)],
                 [RR(WEB, w.AAAA, 1, 3600,
                     hx("20010db8000000000000000000000001"))])),
    # NS, RFC 1035 3.3.11. Owner foo.com = pointer to offset 16 (c0 10),
    # into the middle of the question name. Target ns1.foo.com =
    # 03 'ns1' + pointer to 16: 4 + 2 = 6 octets. TTL 86400 = 0x15180.
    "NS": (hx("1236 8400 0001 0001 0000 0000", QNAME_WEB, "0002 0001",
              "c010 0002 0001 00015180 0006 03 6e7331 c010"),
           Msg(0x1236, 0x8400, [Question(WEB, w.NS)],
               [RR(FOO, w.NS, 1, 86400, labels("ns1.foo.com"))])),
    # CNAME, RFC 1035 3.3.1: www2.foo.com = 04 'www2' + c0 10: 7 octets
    "CNAME": (hx("1237 8400 0001 0001 0000 0000", QNAME_WEB, "0005 0001",
                 "c00c 0005 0001 0000003c 0007 04 77777732 c010"),
              Msg(0x1237, 0x8400, [Question(WEB, w.CNAME)],
                  [RR(WEB, w.CNAME, 1, 60, labels("www2.foo.com"))])),
    # PTR, RFC 1035 3.3.12: type 12; the target spelled out in full:
    # 4 + 4 + 4 + 1 = 13 = 0x0d octets
    "PTR": (hx("1238 8400 0001 0001 0000 0000", QNAME_ARPA, "000c 0001",
               "c00c 000c 0001 0000001e 000d", QNAME_WEB),
            Msg(0x1238, 0x8400,
                [Question(labels("1.0.168.192.in-addr.arpa"), w.PTR)],
                [RR(labels("1.0.168.192.in-addr.arpa"), w.PTR, 1, 30,
                    WEB)])),
    # TXT, RFC 1035 3.3.14: two <character-string>s, 05 'hello' and
    # 03 'abc': 6 + 4 = 10 octets. TTL 300 = 0x12c.
    "TXT": (hx("1239 8400 0001 0001 0000 0000", QNAME_WEB, "0010 0001",
               "c00c 0010 0001 0000012c 000a 05 68656c6c6f 03 616263"),
            Msg(0x1239, 0x8400, [Question(WEB, w.TXT)],
                [RR(WEB, w.TXT, 1, 300, (b"hello", b"abc"))])),
    # SRV, RFC 2782: type 33 = 0x21; priority, weight, port, then the
    # target, never compressed: lb0.foo.com = 4 + 4 + 4 + 1 = 13, so
    # RDLENGTH = 6 + 13 = 19 = 0x13. The record starts at 36: owner 2,
    # type/class/ttl/rdlength 10, so rdata at 48 and the target at 54 =
    # 0x36. The additional A is owned by a pointer to that target: a
    # name compressed into an earlier rdata name.
    "SRV": (hx("123a 8400 0001 0001 0000 0001", QNAME_SRV, "0021 0001",
               "c00c 0021 0001 00000e11 0013 0102 0304 0506",
               "03 6c6230 03 666f6f 03 636f6d 00",
               "c036 0001 0001 00000007 0004 0a000001"),
            Msg(0x123a, 0x8400,
                [Question(labels("_http._tcp.foo.com"), w.SRV)],
                [RR(labels("_http._tcp.foo.com"), w.SRV, 1, 0xe11,
                    (0x0102, 0x0304, 0x0506, labels("lb0.foo.com")))],
                [],
                [RR(labels("lb0.foo.com"), w.A, 1, 7,
                    bytes([10, 0, 0, 1]))])),
    # SOA, RFC 1035 3.3.13, in the authority section. MNAME ns1.foo.com
    # = 03 'ns1' c0 10 (6 octets), RNAME hostmaster.foo.com = 0a
    # 'hostmaster' c0 10 (13 octets), five 32-bit numbers (20):
    # RDLENGTH 39 = 0x27. The record starts at 29, its rdata at 41 =
    # 0x29, where the label 'ns1' begins; the additional A points there.
    "SOA": (hx("123b 8400 0001 0000 0001 0001", QNAME_WEB, "0006 0001",
               "c010 0006 0001 00000e10 0027",
               "03 6e7331 c010  0a 686f73746d6173746572 c010",
               "78000001 00002a30 00000e10 00093a80 0000003c",
               "c029 0001 0001 00000005 0004 0a000002"),
            Msg(0x123b, 0x8400, [Question(WEB, w.SOA)], [],
                [RR(FOO, w.SOA, 1, 3600,
                    (labels("ns1.foo.com"), labels("hostmaster.foo.com"),
                     0x78000001, 10800, 3600, 604800, 60))],
                [RR(labels("ns1.foo.com"), w.A, 1, 5,
                    bytes([10, 0, 0, 2]))])),
    # OPT, RFC 6891 6.1.2: root owner (00), type 41 = 0x29, CLASS = the
    # sender's UDP payload size (4096 = 0x1000), TTL = extended rcode,
    # version, DO (0x8000) and Z; one empty option, code 65001 = 0xfde9
    # (RFC 6891 9: local use), length 0.
    # A query: flags 0x0100 is RD alone.
    "OPT": (hx("beef 0100 0001 0000 0000 0001", QNAME_WEB, "0001 0001",
               "00 0029 1000 00008000 0004 fde9 0000"),
            Msg(0xbeef, 0x0100, [Question(WEB, w.A)], [], [],
                [RR((), w.OPT, 4096, 0x8000, hx("fde90000"))])),
}

# RFC 1035 4.1.1, header bits from the most significant:
#   QR | Opcode x4 | AA | TC | RD | RA | Z x3 | RCODE x4
# 0x8000 0x7800 0x0400 0x0200 0x0100 0x0080 0x0070 0x000f
HEADERS = [
    ("0007", "8000", dict(id=7, qr=True)),
    ("0007", "0400", dict(id=7, aa=True)),
    ("0007", "0200", dict(id=7, tc=True)),
    ("0007", "0100", dict(id=7, rd=True)),
    ("0007", "0080", dict(id=7, ra=True)),
    ("0007", "1000", dict(id=7, opcode=2)),  # 2 << 11
    ("0007", "8000", dict(id=7, qr=True, rcode=0)),
    ("0007", "8001", dict(id=7, qr=True, rcode=1)),
    ("0007", "8002", dict(id=7, qr=True, rcode=2)),
    ("0007", "8003", dict(id=7, qr=True, rcode=3)),
    ("0007", "8004", dict(id=7, qr=True, rcode=4)),
    ("0007", "8005", dict(id=7, qr=True, rcode=5)),
    ("0000", "0000", dict(id=0)),
    ("ffff", "0000", dict(id=0xFFFF)),
]
HEADER_FIELDS = {}
for _id, _flags, _f in HEADERS:
    HEADER_FIELDS.setdefault(f"hdr-{_id}-{_flags}", {}).update(_f)
    GOLDEN[f"hdr-{_id}-{_flags}"] = (
        hx(_id, _flags, "0001 0000 0000 0000", QNAME_WEB, "0001 0001"),
        Msg(int(_id, 16), int(_flags, 16), [Question(WEB, w.A)]))

NAMES = sorted(GOLDEN)

# ------------------------------------------------- oracle <-> native dict

TYPE_NAMES = {1: "A", 2: "NS", 5: "CNAME", 6: "SOA", 12: "PTR", 15: "MX",
              16: "TXT", 28: "AAAA", 33: "SRV", 41: "OPT", 255: "ANY"}
RCODE_NAMES = ["NOERROR", "FORMERR", "SERVFAIL", "NXDOMAIN", "NOTIMP",
               "REFUSED"]


def pres(name):
    return b".".join(name).decode("ascii")


def native_record(rr):
    d = {"name": pres(rr.name), "type": TYPE_NAMES[rr.rtype],
         "class": rr.rclass, "ttl": rr.ttl}
    t, rd = rr.rtype, rr.rdata
    if t == w.A:
        d["address"] = socket.inet_ntop(socket.AF_INET, rd)
    elif t == w.AAAA:
        d["address"] = socket.inet_ntop(socket.AF_INET6, rd)
    elif t in (w.NS, w.CNAME, w.PTR):
        d["target"] = pres(rd)
    elif t == w.TXT:
        d["target"] = b"".join(rd).decode("ascii")
    elif t == w.SRV:
        d.update(priority=rd[0], weight=rd[1], port=rd[2],
                 target=pres(rd[3]))
    elif t == w.SOA:
        d.update(mname=pres(rd[0]), rname=pres(rd[1]), serial=rd[2],
                 refresh=rd[3], retry=rd[4], expire=rd[5], minimum=rd[6])
    elif t == w.OPT:
        d.update(udp_size=rr.rclass, rdata=list(rd))
    else:
        raise AssertionError(t)
    return d


def native_dict(m):
    """What decode_message must return for m, and what encode_message
    takes to produce it."""
    rc = m.rcode
    return {
        "id": m.id, "qr": bool(m.flags & w.QR), "opcode": m.opcode,
        "aa": bool(m.flags & w.AA), "tc": bool(m.flags & w.TC),
        "rd": bool(m.flags & w.RD), "ra": bool(m.flags & w.RA),
        "rcode": RCODE_NAMES[rc] if rc < 6 else f"RCODE{rc}",
        "questions": [{"name": pres(q.name), "type": TYPE_NAMES[q.qtype],
                       "class": q.qclass} for q in m.questions],
        "answers": [native_record(r) for r in m.answers],
        "authorities": [native_record(r) for r in m.authorities],
        "additionals": [native_record(r) for r in m.additionals],
    }


def txt_as_encoded(m):
    """The native encoder takes TXT as one string and cuts it into
    255-octet character-strings (RFC 1035 3.3: <character-string> holds
    at most 255); the same message with every TXT cut that way."""
    def fix(rr):
        if rr.rtype != w.TXT:
            return rr
        text = b"".join(rr.rdata)
        cut = tuple(text[i:i + 255] for i in range(0, len(text), 255))
        return RR(rr.name, rr.rtype, rr.rclass, rr.ttl, cut or (b"",))
    return Msg(m.id, m.flags, list(m.questions),
               *([fix(r) for r in sec] for sec in m.sections()))


# ----------------------------------------------------- the oracle itself

@pytest.mark.parametrize("name", NAMES)
def test_oracle_reads_the_hand_written_images(name):
    wire, want = GOLDEN[name]
    got = w.parse(wire)
    assert got == want
    assert wire[got.qspan[0]:got.qspan[1]] == \
        wire[12:12 + sum(w.name_wire_len(q.name) + 4
                         for q in want.questions)]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_writes_the_hand_written_images(name):
    """build() with the greedy chooser picks the pointers the images
    use: the longest earlier suffix, at its first occurrence."""
    wire, want = GOLDEN[name]
    assert w.build(want, compress=True) == wire


def test_oracle_writes_uncompressed_and_reads_it_back():
    for name in NAMES:
        wire, want = GOLDEN[name]
        flat = w.build(want)
        assert len(flat) >= len(wire)
        assert w.parse(flat) == want


def bad(reason, wire):
    with pytest.raises(WireError, match=reason):
        w.parse(wire)


def test_oracle_refuses():
    a_wire, a_msg = GOLDEN["A"]
    bad("header shorter", a_wire[:11])
    bad("section counts", a_wire[:-1])
    bad("section counts", w.build(a_msg, counts=(1, 2, 0, 0)))
    bad("after the last", a_wire + b"\0")
    bad("after the last", w.build(a_msg, counts=(1, 0, 0, 0)))
    q = lambda raw: w.build(Msg(1, 0, [Question(RawName(raw), w.A)]))
    bad("label type 01", q(b"\x40" + b"a" * 64 + b"\0"))
    bad("label type 10", q(b"\x80\0"))
    long256 = labels(".".join(["a" * 63] * 3 + ["b" * 62]))
    bad("255 octets", w.build(Msg(1, 0, [Question(long256, w.A)])))
    # 251 octets in the question, then an owner of 250 octets that
    # ends in a pointer to it: 501 in all
    tail = labels(".".join(["c" * 49] * 5))  # 5 * 50 + 1 = 251
    head = RawName(b"".join(bytes([49]) + b"d" * 49 for _ in range(5))
                   + b"\xc0\x0c")
    bad("255 octets", w.build(Msg(
        1, w.QR, [Question(tail, w.A)],
        [RR(head, w.A, 1, 0, bytes(4))])))
    bad("pointer at 12 to 14", q(b"\xc0\x0e\0"))  # forward
    bad("pointer at 12 to 12", q(b"\xc0\x0c"))  # itself
    bad("pointer", q(b"\x01a\xc0\x0c"))  # back into its own name
    # onto the second octet of a label, not its start
    bad("not the start", w.build(Msg(
        1, w.QR, [Question(WEB, w.A)],
        [RR(RawName(b"\xc0\x0d"), w.A, 1, 0, bytes(4))])))
    bad("past the end", q(b"\x05ab"))
    for rtype, rdata in ((w.CNAME, WEB), (w.TXT, (b"abc",)),
                         (w.SRV, (1, 2, 3, WEB)),
                         (w.SOA, (WEB, FOO, 1, 2, 3, 4, 5))):
        rr = RR(WEB, rtype, 1, 0, rdata)
        m = Msg(1, w.QR, [], [rr])
        real = len(w.build(m)) - 12 - 13 - 10
        bad("rdlength", w.build(m, rdlength={id(rr): real - 1}) + b"")
        bad("rdlength", w.build(m, rdlength={id(rr): real + 1}) + b"\x07")
    for rtype, n_oct in ((w.A, 5), (w.A, 3), (w.AAAA, 15)):
        bad("octets", w.build(Msg(1, w.QR, [], [
            RR(WEB, rtype, 1, 0, bytes(n_oct))])))
    bad("TXT without", w.build(Msg(1, w.QR, [], [
        RR(WEB, w.TXT, 1, 0, b"")])))
    # SRV target as a pointer to the question name
    bad("compressed SRV", w.build(Msg(1, w.QR, [Question(WEB, w.SRV)], [
        RR(WEB, w.SRV, 1, 0, struct.pack(">HHH", 1, 2, 3) + b"\xc0\x0c")])))
    opt = RR((), w.OPT, 1232, 0, b"")
    bad("OPT outside", w.build(Msg(1, w.QR, [], [opt])))
    bad("OPT outside", w.build(Msg(1, w.QR, [], [], [opt])))
    bad("more than one OPT", w.build(Msg(1, 0, [], [], [], [opt, opt])))
    bad("not the root", w.build(Msg(1, 0, [], [], [], [
        RR(FOO, w.OPT, 1232, 0, b"")])))
    bad("Z bit", w.build(Msg(1, w.QR | w.Z, [Question(WEB, w.A)])))
    # ... which a query may carry as far as this parser cares
    w.parse(w.build(Msg(1, w.Z, [Question(WEB, w.A)])))


def test_oracle_against_dnspython():
    """An extra: the same images through a third implementation."""
    pytest.importorskip("dns")
    import dns.message
    import dns.name
    for name in NAMES:
        wire, want = GOLDEN[name]
        m = dns.message.from_wire(wire)
        assert m.id == want.id
        assert m.flags == want.flags
        assert [(dns.name.Name(q.name + (b"",)), q.qtype)
                for q in want.questions] == \
            [(rrset.name, int(rrset.rdtype)) for rrset in m.question]
        for sec, got in zip((want.answers, want.authorities),
                            (m.answer, m.authority)):
            # (RFC 2181 8: a TTL with the top bit set is read as zero)
            assert [(dns.name.Name(r.name + (b"",)), r.rtype,
                     r.ttl if r.ttl < 1 << 31 else 0)
                    for r in sec] == \
                [(rrset.name, int(rrset.rdtype), rrset.ttl)
                 for rrset in got]
    srv = dns.message.from_wire(GOLDEN["SRV"][0]).answer[0][0]
    assert (srv.priority, srv.weight, srv.port) == (0x0102, 0x0304, 0x0506)
    assert srv.target == dns.name.from_text("lb0.foo.com.")
    soa = dns.message.from_wire(GOLDEN["SOA"][0]).authority[0][0]
    assert (soa.serial, soa.refresh, soa.retry, soa.expire, soa.minimum) \
        == (0x78000001, 10800, 3600, 604800, 60)


# --------------------------------------------------------- decode goldens

@pytest.mark.parametrize("name", NAMES)
def test_native_decodes_golden(name):
    wire, want = GOLDEN[name]
    got = n.decode_message(wire)
    assert got == native_dict(want)
    if name in HEADER_FIELDS:  # bit by bit, not through dnswire's masks
        fields = dict(qr=False, opcode=0, aa=False, tc=False, rd=False,
                      ra=False, rcode=0)
        fields.update(HEADER_FIELDS[name])
        fields["rcode"] = RCODE_NAMES[fields["rcode"]]
        assert {k: got[k] for k in fields} == fields


@pytest.mark.parametrize("name", NAMES)
def test_native_decodes_golden_uncompressed(name):
    """The same message with every name spelled out in full."""
    _, want = GOLDEN[name]
    assert n.decode_message(w.build(want)) == native_dict(want)


# --------------------------------------------------------- encode goldens

@pytest.mark.parametrize("name", NAMES)
def test_native_encode_strict_parses_to_input(name):
    _, want = GOLDEN[name]
    wire = n.encode_message(native_dict(want))
    assert w.parse(wire) == txt_as_encoded(want)


def test_single_question_queries_are_fully_determined():
    """No name to point at, so only one encoding exists."""
    assert n.encode_message(
        {"id": 0xbeef, "rd": True,
         "questions": [{"name": "web.foo.com", "type": "A"}]}) == \
        hx("beef 0100 0001 0000 0000 0000", QNAME_WEB, "0001 0001")
    assert n.encode_message(
        {"id": 0, "questions": [{"name": "_http._tcp.foo.com",
                                 "type": "SRV"}]}) == \
        hx("0000 0000 0001 0000 0000 0000", QNAME_SRV, "0021 0001")
    assert n.encode_message(
        {"id": 0xFFFF, "questions": [{"name": "1.0.168.192.in-addr.arpa",
                                      "type": "PTR"}]}) == \
        hx("ffff 0000 0001 0000 0000 0000", QNAME_ARPA, "000c 0001")
    for name in NAMES:
        if name.startswith("hdr-"):
            wire, want = GOLDEN[name]
            assert n.encode_message(native_dict(want)) == wire


# ----------------------------------------------------- seeded differential

ALPHABET = (b"abcdefghijklmnopqrstuvwxyz"
            b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-")
TYPED = (w.A, w.AAAA, w.NS, w.CNAME, w.PTR, w.TXT, w.SRV, w.SOA)
QTYPES = sorted(TYPE_NAMES)
N_MESSAGES = 2000


class Gen:
    def __init__(self, seed):
        self.rng = random.Random(seed)

    def chars(self, size):
        return bytes(self.rng.choice(ALPHABET) for _ in range(size))

    def label(self, most=63):
        r = self.rng
        size = r.choice((1, 63)) if r.random() < 0.1 else \
            r.randint(1, r.choice((4, 12, 63)))
        return self.chars(min(size, most))

    def name(self, pool):
        """A fresh name, or labels in front of a suffix of one drawn
        before (what gives compression something to do); now and then
        one filled up to the 255-octet limit exactly."""
        r = self.rng
        base = ()
        if pool and r.random() < 0.7:
            base = r.choice(pool)
            base = base[r.randint(0, len(base)):]
        if r.random() < 0.03 and not base:
            name = ()
        else:
            # octets left for labels in front, each one more than its
            # size (RFC 1035 2.3.4)
            room = 255 - w.name_wire_len(base)
            front = []
            if r.random() < 0.08:
                while room >= 2:
                    size = min(63, room - 1)
                    if room > 64:
                        size = r.randint(1, 63)
                        if room - 1 - size == 1:  # no label fits in one
                            size -= 1
                    front.append(self.chars(size))
                    room -= 1 + size
            else:
                for _ in range(r.randint(0, 4)):
                    if room < 2:
                        break
                    front.append(self.label(min(63, room - 1)))
                    room -= 1 + len(front[-1])
            name = tuple(front) + base
        assert w.name_wire_len(name) <= 255
        if name:
            pool.append(name)
        return name

    def record(self, pool):
        r = self.rng
        t = r.choice(TYPED)
        if t == w.A:
            rd = r.randbytes(4)
        elif t == w.AAAA:
            rd = r.randbytes(16)
        elif t in (w.NS, w.CNAME, w.PTR):
            rd = self.name(pool)
        elif t == w.TXT:
            total = r.choice((0, 1, 255, 256, 600)) if r.random() < 0.2 \
                else r.randint(0, 80)
            text = bytes(r.choice(ALPHABET) for _ in range(total))
            rd = []
            while text:  # any tiling; encode re-cuts it (txt_as_encoded)
                k = r.randint(0, min(255, len(text)))
                rd.append(text[:k])
                text = text[k:]
            rd = tuple(rd) or (b"",)
        elif t == w.SRV:
            rd = (r.randrange(65536), r.randrange(65536),
                  r.randrange(65536), self.name(pool))
        else:
            rd = (self.name(pool), self.name(pool)) + tuple(
                r.choice((0, 0xFFFFFFFF, r.randrange(1 << 32)))
                for _ in range(5))
        return RR(self.name(pool), t, r.randrange(65536),
                  r.choice((0, 0xFFFFFFFF, r.randrange(1 << 32))), rd)

    def message(self):
        r = self.rng
        pool = []
        m = Msg(r.choice((0, 0xFFFF, r.randrange(65536))),
                w.flags(qr=r.random() < .5, opcode=r.randrange(16),
                        aa=r.random() < .5, tc=r.random() < .5,
                        rd=r.random() < .5, ra=r.random() < .5,
                        rcode=r.randrange(16)))
        for _ in range(r.randint(0, 2)):
            m.questions.append(Question(self.name(pool), r.choice(QTYPES),
                                        r.randrange(65536)))
        for sec in m.sections():
            for _ in range(r.randint(0, 6)):
                sec.append(self.record(pool))
        if r.random() < 0.5:
            m.additionals.insert(
                r.randint(0, len(m.additionals)),
                RR((), w.OPT, r.randrange(65536), r.randrange(1 << 32),
                   r.randbytes(r.choice((0, 0, 4, 11)))))
        return m


def test_generator_reaches_the_edges():
    """The differential below is only as good as what it draws."""
    g = Gen(0xD1F0)
    lens, label_lens, counts = set(), set(), set()
    for _ in range(300):
        m = g.message()
        for sec in m.sections():
            counts.add(len([r for r in sec if r.rtype != w.OPT]))
            for rr in sec:
                lens.add(w.name_wire_len(rr.name))
                label_lens.update(len(x) for x in rr.name)
    assert {1, 255} <= lens and {1, 63} <= label_lens
    assert counts >= set(range(7))


def test_differential_native_encode_strict_parse():
    g = Gen(0xE2C0DE)
    for i in range(N_MESSAGES):
        m = g.message()
        wire = n.encode_message(native_dict(m))
        try:
            got = w.parse(wire)
        except WireError as e:
            raise AssertionError(f"message {i}: {e}\n{m}\n{wire.hex()}")
        assert got == txt_as_encoded(m), (i, wire.hex())


def test_differential_oracle_build_native_decode():
    g = Gen(0xDEC0DE)
    choose = w.random_legal(random.Random(0xC0))
    pointers = 0
    for i in range(N_MESSAGES):
        m = g.message()
        wire = w.build(m, compress=choose)
        flat = w.build(m)
        pointers += len(flat) > len(wire)
        assert w.parse(wire) == m, i  # the input is legal
        assert n.decode_message(wire) == native_dict(m), (i, wire.hex())
        assert n.decode_message(flat) == native_dict(m), (i, flat.hex())
    assert pointers > N_MESSAGES // 2  # compression was in play


# -------------------------------------------------------------- boundaries

def name_of(*sizes):
    return tuple(bytes([ord("a") + i]) * s for i, s in enumerate(sizes))


N255 = name_of(63, 63, 63, 61)  # 64 + 64 + 64 + 62 + 1 = 255
N256 = name_of(63, 63, 63, 62)
N257 = name_of(63, 63, 63, 63)


def test_name_of_255_octets_round_trips():
    assert w.name_wire_len(N255) == 255
    m = Msg(9, w.QR, [Question(N255, w.A)],
            [RR(N255, w.CNAME, 1, 5, N255[1:])])
    wire = n.encode_message(native_dict(m))
    assert w.parse(wire) == m
    for wire in (w.build(m), w.build(m, compress=True)):
        assert n.decode_message(wire) == native_dict(m)


@pytest.mark.parametrize("name", [N256, N257], ids=["256", "257"])
def test_longer_names_do_not_decode(name):
    assert w.name_wire_len(name) in (256, 257)
    assert n.decode_message(
        w.build(Msg(9, 0, [Question(name, w.A)]))) is None
    assert n.decode_message(w.build(
        Msg(9, w.QR, [Question(WEB, w.A)],
            [RR(WEB, w.CNAME, 1, 5, name)]))) is None


def test_name_over_255_through_a_pointer_does_not_decode():
    """255 octets counted across the pointer (RFC 1035 4.1.4 saves
    octets in the message, not in the name)."""
    tail = name_of(49, 49, 49, 49, 49)  # 5 * 50 + 1 = 251
    for front, ok in ((b"\x02zz", True), (b"\x03zzz", True),
                      (b"\x04zzzz", False)):
        # 3, 4 or 5 octets in front of a pointer to the 251 at offset 12
        wire = w.build(Msg(
            9, w.QR, [Question(tail, w.A)],
            [RR(RawName(front + b"\xc0\x0c"), w.A, 1, 0, bytes(4))]))
        assert (n.decode_message(wire) is not None) == ok
        if ok:
            assert w.name_wire_len(w.parse(wire).answers[0].name) == \
                len(front) + 251
        else:
            bad("255 octets", wire)


@pytest.mark.parametrize("name", [N256, N257], ids=["256", "257"])
def test_longer_names_are_not_emitted(name):
    """The SERVFAIL path of an over-long label (Message::encodeInto):
    the header and the question, rcode 2, no records."""
    d = native_dict(Msg(9, w.QR, [Question(WEB, w.A)],
                        [RR(WEB, w.A, 1, 5, bytes(4))]))
    d["answers"][0]["name"] = pres(name)
    assert w.parse(n.encode_message(d)) == \
        Msg(9, w.flags(qr=True, rcode=2), [Question(WEB, w.A)])
    # the same answer with an over-long label, for comparison
    d["answers"][0]["name"] = "b" * 64 + ".foo.com"
    assert w.parse(n.encode_message(d)) == \
        Msg(9, w.flags(qr=True, rcode=2), [Question(WEB, w.A)])
    # a question that cannot be written is left out as well
    d = {"id": 9, "questions": [{"name": pres(name), "type": "A"}]}
    assert w.parse(n.encode_message(d)) == Msg(9, w.flags(qr=True, rcode=2))


def test_label_length_boundary():
    ok = w.build(Msg(1, 0, [Question((b"a" * 63, b"com"), w.A)]))
    assert n.decode_message(ok)["questions"][0]["name"] == "a" * 63 + ".com"
    over = w.build(Msg(1, 0, [Question(
        RawName(b"\x40" + b"a" * 64 + b"\x03com\0"), w.A)]))
    assert n.decode_message(over) is None


# -------------------------------------------------------------- rejections

@pytest.mark.parametrize("name", NAMES)
def test_every_proper_prefix_is_refused(name):
    """The oracle shows the images end with their last record, so any
    prefix promises more than it holds."""
    wire, _ = GOLDEN[name]
    w.parse(wire)
    for cut in range(len(wire)):
        assert n.decode_message(wire[:cut]) is None, cut


RDATA = {
    "CNAME": (w.CNAME, WEB),
    "SRV": (w.SRV, (1, 2, 3, WEB)),
    "SOA": (w.SOA, (WEB, FOO, 1, 2, 3, 4, 5)),
    "TXT": (w.TXT, (b"abc", b"de")),
}


@pytest.mark.parametrize("delta", [-1, 1], ids=["short", "long"])
@pytest.mark.parametrize("kind", sorted(RDATA))
def test_wrong_rdlength_is_refused(kind, delta):
    """rdlength off by one, the record last in the message. One longer
    comes with one more octet in the message (0x07: no whole
    character-string, no root label), so the rdata is all there."""
    rtype, rdata = RDATA[kind]
    rr = RR(FOO, rtype, 1, 60, rdata)
    m = Msg(3, w.QR, [Question(FOO, rtype)], [rr])
    good = w.build(m)
    assert n.decode_message(good) == native_dict(m)
    real = struct.unpack(">H", good[12 + 13 + 9 + 8:][:2])[0]
    assert 12 + 13 + 9 + 10 + real == len(good)
    wire = w.build(m, rdlength={id(rr): real + delta})
    if delta > 0:
        wire += b"\x07"
    assert len(wire) >= 12 + 13 + 9 + 10 + real + delta
    bad("rdlength", wire)
    assert n.decode_message(wire) is None


def test_rdata_name_may_not_cross_rdlength():
    """Two records; the first one's CNAME target ends one octet past its
    rdlength, in the octet the second record's owner starts with."""
    rr = RR(FOO, w.CNAME, 1, 60, WEB)
    m = Msg(3, w.QR, [], [rr, RR((), w.A, 1, 0, bytes(4))])
    # the target's root octet doubles as the second owner's root name
    wire = bytearray(w.build(Msg(3, w.QR, [], [rr])))
    struct.pack_into(">H", wire, 12 + 9 + 8, 12)  # real: 13
    struct.pack_into(">H", wire, 6, 2)
    wire += struct.pack(">HHIH", w.A, 1, 0, 4) + bytes(4)
    bad("past rdlength", bytes(wire))
    assert n.decode_message(bytes(wire)) is None
    assert n.decode_message(w.build(m)) == native_dict(m)


@pytest.mark.parametrize("raw", [
    b"\xc0\x0e\x01a\0",      # forward, to offset 14
    b"\xc0\x0c",             # to itself, offset 12
    b"\x01a\xc0\x10\xc0\x0e",  # 14 -> 16 -> 14
    b"\x01a\xc0\x0c",        # back onto its own first label: endless
], ids=["forward", "self", "two-step", "own-label"])
def test_pointer_loops_are_refused(raw):
    wire = w.build(Msg(1, 0, [Question(RawName(raw), w.A)]))
    bad("pointer", wire)
    assert n.decode_message(wire) is None


@pytest.mark.parametrize("name", [
    (b"web.foo", b"com"), (b"a.", b"foo", b"com"),
    (b"x..y", b"foo", b"com"), (b".",), (b".a", b"com")],
    ids=["mid", "trailing", "double", "alone", "leading"])
def test_label_holding_a_dot_is_refused(name):
    """0x2E inside a label is legal DNS (RFC 1035 3.1) but has no
    dotted-string form, which is what the engine keys on; the decoder
    refuses it, and the server drops the query (docs/PARITY.md)."""
    wire = w.build(Msg(1, 0, [Question(name, w.A)]))
    assert w.parse(wire).questions[0].name == name
    assert n.decode_message(wire) is None
    wire = w.build(Msg(1, w.QR, [Question(WEB, w.A)],
                       [RR(WEB, w.CNAME, 1, 0, name)]))
    w.parse(wire)
    assert n.decode_message(wire) is None
