"""A strict DNS message reader and writer, written from the RFCs.

The oracle of tests/test_dns_golden.py and tests/test_dns_wire_served.py.
Standard library only, and nothing from binder_amd: it shares no code
with the codec it judges (the spirit of tests/zkwire.py). Each rule
names the RFC section it comes from.

parse() accepts only what a careful resolver accepts and raises
WireError naming the rule broken. build() writes a message with the
compression of every single name under the caller's control, so tests
can feed the native decoder legal encodings the native encoder never
produces, and illegal ones on purpose.

Names are tuples of label bytes, never joined: a "." inside a label
stays one label. The root name is the empty tuple.
"""
import struct
from dataclasses import dataclass, field

# RR types: RFC 1035 3.2.2, RFC 3596 2.1, RFC 2782, RFC 6891 6.1.1
A, NS, CNAME, SOA, PTR, MX, TXT, AAAA, SRV, OPT, ANY = \
    1, 2, 5, 6, 12, 15, 16, 28, 33, 41, 255
IN = 1  # RFC 1035 3.2.4

# RFC 1035 4.1.1, the second 16 bits of the header:
#   QR(1) Opcode(4) AA(1) TC(1) RD(1) RA(1) Z(1) AD(1) CD(1) RCODE(4)
# (AD and CD: RFC 4035 3.2; the one bit left of Z's three is 0x0040)
QR, AA, TC, RD, RA, Z = 0x8000, 0x0400, 0x0200, 0x0100, 0x0080, 0x0040


def flags(qr=False, opcode=0, aa=False, tc=False, rd=False, ra=False,
          rcode=0):
    return ((QR if qr else 0) | ((opcode & 0xF) << 11) | (AA if aa else 0)
            | (TC if tc else 0) | (RD if rd else 0) | (RA if ra else 0)
            | (rcode & 0xF))


class WireError(ValueError):
    """The message breaks a rule; str() names the rule."""


@dataclass(frozen=True)
class Question:
    name: tuple
    qtype: int
    qclass: int = IN


@dataclass(frozen=True)
class RR:
    """rdata by type: A and AAAA the address bytes; NS, CNAME and PTR a
    name; SOA (mname, rname, serial, refresh, retry, expire, minimum);
    SRV (priority, weight, port, target); TXT a tuple of
    character-strings; anything else, OPT included, the raw bytes."""
    name: tuple
    rtype: int
    rclass: int
    ttl: int
    rdata: object


@dataclass
class Msg:
    id: int = 0
    flags: int = 0
    questions: list = field(default_factory=list)
    answers: list = field(default_factory=list)
    authorities: list = field(default_factory=list)
    additionals: list = field(default_factory=list)
    # [start, end) of the question section in the parsed bytes
    qspan: tuple = field(default=(12, 12), compare=False)

    @property
    def rcode(self):
        return self.flags & 0xF

    @property
    def opcode(self):
        return (self.flags >> 11) & 0xF

    def sections(self):
        return (self.answers, self.authorities, self.additionals)


def name_wire_len(name):
    """RFC 1035 2.3.4/3.1: every length octet, every label octet and
    the root octet count toward the 255 limit."""
    return sum(1 + len(label) for label in name) + 1


# ---------------------------------------------------------------- parse

class _Parser:
    def __init__(self, data):
        self.d = bytes(data)
        self.pos = 0
        # offsets at which a (non-root) label of an already parsed name
        # began: the only legal pointer targets
        self.label_starts = set()

    def take(self, n, what, limit=None):
        end = len(self.d) if limit is None else limit
        if self.pos + n > end:
            raise WireError(f"{what}: runs past the end "
                            f"(RFC 1035 4.1)" if limit is None else
                            f"{what}: runs past rdlength (RFC 1035 3.2.1)")
        out = self.d[self.pos:self.pos + n]
        self.pos += n
        return out

    def u16(self, what, limit=None):
        return struct.unpack(">H", self.take(2, what, limit))[0]

    def u32(self, what, limit=None):
        return struct.unpack(">I", self.take(4, what, limit))[0]

    def name(self, limit=None, allow_pointer=True):
        """A name at self.pos. `limit`: the end of the enclosing rdata,
        which the octets written in place must not cross."""
        d = self.d
        end_in_place = len(d) if limit is None else limit
        past = ("name runs past rdlength (RFC 1035 3.2.1)"
                if limit is not None else
                "name runs past the end of the message (RFC 1035 4.1)")
        labels = []
        new_starts = []
        wire_len = 0
        p = self.pos
        after = None  # where parsing resumes, once a pointer was taken
        visited = set()
        while True:
            bound = end_in_place if after is None else len(d)
            if p >= bound:
                raise WireError(past)
            octet = d[p]
            kind = octet & 0xC0
            if kind == 0xC0:  # RFC 1035 4.1.4
                if p + 2 > bound:
                    raise WireError(past)
                if not allow_pointer:
                    raise WireError(
                        "compressed SRV target (RFC 2782, Target)")
                target = ((octet & 0x3F) << 8) | d[p + 1]
                if p in visited:
                    raise WireError("pointer chain revisits an offset "
                                    "(RFC 1035 4.1.4)")
                visited.add(p)
                if after is None:
                    after = p + 2
                # 4.1.4: "a pointer to a prior occurance of the same
                # name": strictly backwards, and onto a label of a name
                # parsed before this one
                if target >= p or target not in self.label_starts:
                    raise WireError(
                        f"pointer at {p} to {target}: not the start of "
                        f"a label of an earlier name (RFC 1035 4.1.4)")
                p = target
                continue
            if kind != 0:  # 01 and 10
                raise WireError(f"label type {kind >> 6:02b} "
                                f"(RFC 1035 4.1.4: reserved)")
            # kind == 0: octet <= 63 (RFC 1035 2.3.4) by construction
            if octet == 0:
                wire_len += 1
                p += 1
                break
            if p + 1 + octet > bound:
                raise WireError(past)
            if after is None:
                new_starts.append(p)
            labels.append(d[p + 1:p + 1 + octet])
            wire_len += 1 + octet
            if wire_len + 1 > 255:
                raise WireError("name longer than 255 octets "
                                "(RFC 1035 2.3.4)")
            p += 1 + octet
        self.pos = p if after is None else after
        self.label_starts.update(new_starts)
        return tuple(labels)

    def rdata(self, rtype, rdlen):
        start = self.pos
        end = start + rdlen
        if end > len(self.d):
            raise WireError("rdata runs past the end of the message "
                            "(RFC 1035 3.2.1)")
        if rtype == A:  # RFC 1035 3.4.1
            if rdlen != 4:
                raise WireError("A rdata is not 4 octets (RFC 1035 3.4.1)")
            out = self.take(4, "A")
        elif rtype == AAAA:  # RFC 3596 2.2
            if rdlen != 16:
                raise WireError("AAAA rdata is not 16 octets "
                                "(RFC 3596 2.2)")
            out = self.take(16, "AAAA")
        elif rtype in (NS, CNAME, PTR):  # RFC 1035 3.3.11, 3.3.1, 3.3.12
            out = self.name(limit=end)
        elif rtype == SOA:  # RFC 1035 3.3.13
            mname = self.name(limit=end)
            rname = self.name(limit=end)
            out = (mname, rname) + tuple(
                self.u32("SOA " + f, end) for f in
                ("serial", "refresh", "retry", "expire", "minimum"))
        elif rtype == SRV:  # RFC 2782
            prio = self.u16("SRV priority", end)
            weight = self.u16("SRV weight", end)
            port = self.u16("SRV port", end)
            out = (prio, weight, port,
                   self.name(limit=end, allow_pointer=False))
        elif rtype == TXT:  # RFC 1035 3.3.14, 3.3: <character-string>
            strings = []
            if rdlen == 0:
                raise WireError("TXT without a character-string "
                                "(RFC 1035 3.3.14: one or more)")
            while self.pos < end:
                n = self.take(1, "TXT length", end)[0]
                strings.append(self.take(n, "TXT character-string", end))
            out = tuple(strings)
        else:
            out = self.take(rdlen, "rdata")
        if self.pos != end:
            raise WireError(
                f"type {rtype} rdata used {self.pos - start} octets, "
                f"rdlength says {rdlen} (RFC 1035 3.2.1)")
        return out

    def record(self):
        name = self.name()
        rtype = self.u16("RR type")
        rclass = self.u16("RR class")
        ttl = self.u32("RR ttl")
        rdlen = self.u16("RR rdlength")
        return RR(name, rtype, rclass, ttl, self.rdata(rtype, rdlen))


def parse(data):
    p = _Parser(data)
    if len(p.d) < 12:
        raise WireError("header shorter than 12 octets (RFC 1035 4.1.1)")
    m = Msg()
    m.id, m.flags, qd, an, ns, ar = struct.unpack(">HHHHHH", p.take(12, ""))
    try:
        for _ in range(qd):  # RFC 1035 4.1.2
            name = p.name()
            m.questions.append(
                Question(name, p.u16("qtype"), p.u16("qclass")))
        m.qspan = (12, p.pos)
        for count, out in zip((an, ns, ar), m.sections()):
            for _ in range(count):  # RFC 1035 4.1.3
                out.append(p.record())
    except WireError as e:
        if "past the end" in str(e):
            raise WireError(f"section counts {qd}/{an}/{ns}/{ar} promise "
                            f"more than is present: {e}") from None
        raise
    if p.pos != len(p.d):
        raise WireError(f"{len(p.d) - p.pos} octets after the last counted "
                        f"record (RFC 1035 4.1)")
    # RFC 6891 6.1.1: at most one OPT, in the additional section, owned
    # by the root
    for sec in (m.answers, m.authorities):
        if any(r.rtype == OPT for r in sec):
            raise WireError("OPT outside the additional section "
                            "(RFC 6891 6.1.1)")
    opts = [r for r in m.additionals if r.rtype == OPT]
    if len(opts) > 1:
        raise WireError("more than one OPT (RFC 6891 6.1.1)")
    if opts and opts[0].name != ():
        raise WireError("OPT owner is not the root (RFC 6891 6.1.2)")
    # RFC 1035 4.1.1: Z "must be zero in all queries and responses"
    if (m.flags & QR) and (m.flags & Z):
        raise WireError("Z bit set in a response (RFC 1035 4.1.1)")
    return m


# ---------------------------------------------------------------- build

class RawName:
    """A name given as its literal wire octets: for illegal encodings."""

    def __init__(self, wire, labels=()):
        self.wire = bytes(wire)
        self.labels = tuple(labels)


def greedy(name, candidates):
    """The longest earlier suffix, at its first occurrence."""
    return min(candidates) if candidates else None


def random_legal(rng):
    """A chooser that draws among "uncompressed" and every legal
    pointer, so a name may point into the middle of an earlier one or
    spell labels out that it could have saved."""
    def choose(name, candidates):
        if not candidates or rng.random() < 0.3:
            return None
        return rng.choice(candidates)
    return choose


class _Builder:
    def __init__(self, choose):
        self.out = bytearray()
        self.choose = choose
        self.suffixes = {}  # tuple of labels -> [offset, ...]

    def name(self, name, compress=True):
        if isinstance(name, RawName):
            self.out += name.wire
            return
        choice = None
        if compress and self.choose is not None:
            # (k, offset): spell k labels out, then point at offset
            candidates = [(k, off) for k in range(len(name))
                          for off in self.suffixes.get(name[k:], ())]
            choice = self.choose(name, candidates)
        spelled = len(name) if choice is None else choice[0]
        for k in range(spelled):
            label = name[k]
            if len(self.out) < 0x4000:  # 14-bit offsets (RFC 1035 4.1.4)
                self.suffixes.setdefault(name[k:], []).append(
                    len(self.out))
            self.out.append(len(label))
            self.out += label
        if choice is None:
            self.out.append(0)
        else:
            self.out += struct.pack(">H", 0xC000 | choice[1])

    def rdata(self, rr):
        t, rd = rr.rtype, rr.rdata
        if isinstance(rd, (bytes, bytearray)):
            self.out += rd
        elif t in (NS, CNAME, PTR):
            self.name(rd)
        elif t == SOA:
            self.name(rd[0])
            self.name(rd[1])
            self.out += struct.pack(">IIIII", *rd[2:])
        elif t == SRV:
            self.out += struct.pack(">HHH", *rd[:3])
            self.name(rd[3], compress=False)  # RFC 2782
        elif t == TXT:
            for s in rd:
                self.out.append(len(s))
                self.out += s
        else:
            raise TypeError(f"no rdata writer for type {t}: {rd!r}")

    def record(self, rr, rdlength=None):
        self.name(rr.name)
        self.out += struct.pack(">HHI", rr.rtype, rr.rclass, rr.ttl)
        at = len(self.out)
        self.out += b"\0\0"
        self.rdata(rr)
        real = len(self.out) - at - 2
        struct.pack_into(">H", self.out, at,
                         real if rdlength is None else rdlength)


def build(msg, compress=None, counts=None, rdlength=None):
    """The wire form of msg.

    compress: None or False writes every name out in full; True points
    every name at the longest earlier suffix; a callable
    choose(name, candidates) -> None | (k, offset) decides per name,
    where each candidate (k, offset) means "spell the first k labels
    out, then point at offset", one per earlier occurrence of each
    suffix. A name given as RawName is copied as it stands. SRV targets
    are never offered compression (RFC 2782).

    counts: (qd, an, ns, ar) to write in place of the true ones.
    rdlength: {id(rr): value} to write in place of the true rdlength.
    """
    choose = greedy if compress is True else (compress or None)
    b = _Builder(choose)
    true_counts = (len(msg.questions), len(msg.answers),
                   len(msg.authorities), len(msg.additionals))
    b.out += struct.pack(">HHHHHH", msg.id, msg.flags,
                         *(counts or true_counts))
    for q in msg.questions:
        b.name(q.name)
        b.out += struct.pack(">HH", q.qtype, q.qclass)
    for sec in msg.sections():
        for rr in sec:
            b.record(rr, (rdlength or {}).get(id(rr)))
    return bytes(b.out)


def labels(text):
    """"a.b.c" -> (b"a", b"b", b"c"); "" is the root. For tests whose
    names hold no dots inside labels."""
    if isinstance(text, str):
        text = text.encode()
    return tuple(text.split(b".")) if text else ()
