"""Replies as real binderd processes send them, judged by
tests/dnswire.py alone: the queries are written by dnswire.build, go out
over this file's own UDP and TCP sockets, and every reply is
strict-parsed. The native codec is nowhere on the path, so a mistake
that its encoder and decoder share, or a hand-assembled reply whose
rdlength is off (the fast path builds its replies without the encoder),
cannot pass by decoding fine in our own hands.

What the replies must hold is worked out here from the tree and from
the rules that tests/test_engine_policy.py pins, never from a server's
output. The same checks run at three log levels: warn (fast path and
memoised hits), info (fast path, logging) and debug (slow path only).

Run against a sanitizer build with BINDERD_BIN (`make
check-wire-asan`); a daemon that exits on its own or writes a sanitizer
report to its log fails the tests here.
"""
import json
import os
import random
import shutil
import socket
import struct
import subprocess
import time
from collections import Counter

import pytest

from binder_amd.harness import BALANCERD, BinderProcess, free_port

import dnswire as w
import test_balancer_hotpath as hp
from dnswire import RR, Msg, Question, labels

LEVELS = ("warn", "info", "debug")

# ------------------------------------------------------------ the tree

SVC_TTL = 60
MEMBERS = {  # name -> (address, ttl of its own or None, ports or None)
    "m0": ("10.4.0.1", None, None),
    "m1": ("10.4.0.2", 10, None),
    "m2": ("10.4.0.3", None, [53, 8053]),
}
SVC_PORT = 80

# The big service's A reply: 12 octets of header, the question
# big.foo.com (4 + 4 + 4 + 1) with type and class (4), and per member an
# owner that is at best a 2-octet pointer, 10 octets of type, class, TTL
# and rdlength, and 4 of address. The smallest count that cannot fit in
# 512 octets (RFC 1035 4.2.1) however well it is compressed:
BIG_FIXED = 12 + 13 + 4
BIG_PER_MEMBER = 2 + 10 + 4
BIG_MEMBERS = (512 - BIG_FIXED) // BIG_PER_MEMBER + 1


def big_addr(j):
    return f"10.6.{j // 200}.{j % 200 + 1}"


def make_tree():
    tree = {
        "foo.com": None,
        "web.foo.com": {"type": "host", "host": {"address": "10.1.0.1"}},
        "pg.foo.com": {"type": "database", "ttl": 20, "database": {
            "primary": "tcp://postgres@10.99.99.14:5432/postgres"}},
        "svc.foo.com": {"type": "service", "service": {
            "srvce": "_http", "proto": "_tcp", "port": SVC_PORT,
            "ttl": SVC_TTL}},
        "big.foo.com": {"type": "service", "service": {
            "srvce": "_x", "proto": "_tcp", "port": 81, "ttl": SVC_TTL}},
    }
    for name, (addr, ttl, ports) in MEMBERS.items():
        rec = {"type": "rr_host", "rr_host": {"address": addr}}
        if ttl is not None:
            rec["ttl"] = ttl
        if ports is not None:
            rec["rr_host"]["ports"] = ports
        tree[f"{name}.svc.foo.com"] = rec
    for j in range(BIG_MEMBERS):
        tree[f"b{j}.big.foo.com"] = {
            "type": "rr_host", "rr_host": {"address": big_addr(j)}}
    return tree


def ip(text):
    return socket.inet_aton(text)


# ------------------------------------- what the policy says comes back
# Flags of every answer: QR, AA set, RA clear, opcode and RD echoed
# (test_engine_policy.py and Engine::handle; RA: the reference clears
# it), plus the rcode.

def reply_flags(rd=False, rcode=0, tc=False, opcode=0):
    return w.flags(qr=True, aa=True, rd=rd, ra=False, rcode=rcode, tc=tc,
                   opcode=opcode)


def a_rr(name, addr, ttl):
    return RR(labels(name), w.A, w.IN, ttl, ip(addr))


# host and database: one A, the record's TTL or the default 30
# (test_host_a_record, test_database_record_parses_url)
WEB_A = [a_rr("web.foo.com", "10.1.0.1", 30)]
PG_A = [a_rr("pg.foo.com", "10.99.99.14", 20)]
# A for a service: each member under the service's name, TTL the smaller
# of the service's and the member's own
# (test_service_a_uses_min_of_service_and_member_ttl)
SVC_A = [a_rr("svc.foo.com", addr, min(SVC_TTL, ttl or SVC_TTL))
         for addr, ttl, _ in MEMBERS.values()]
# SRV: one record per member port at the service's TTL, priority 0 and
# weight 10, and one additional A per member (not per port) at the
# member's own TTL, else the service's (test_service_srv,
# test_multi_port_member_gets_one_srv_per_port)
SVC_SRV = [RR(labels("_http._tcp.svc.foo.com"), w.SRV, w.IN, SVC_TTL,
              (0, 10, port, labels(f"{name}.svc.foo.com")))
           for name, (_, _, ports) in MEMBERS.items()
           for port in (ports or [SVC_PORT])]
SVC_EXTRA = [a_rr(f"{name}.svc.foo.com", addr, ttl or SVC_TTL)
             for name, (addr, ttl, _) in MEMBERS.items()]
BIG_A = [a_rr("big.foo.com", big_addr(j), SVC_TTL)
         for j in range(BIG_MEMBERS)]
# SRV asked of a name that is no service: NODATA with a SOA for negative
# caching, owned by the name, TTL and MINIMUM the record's TTL, MNAME the
# zone, RNAME hostmaster.<zone>, the other numbers zero
# (test_srv_on_non_service_nodata_with_soa, Engine::addSoaAuthority)
WEB_SOA = [RR(labels("web.foo.com"), w.SOA, w.IN, 30,
              (labels("foo.com"), labels("hostmaster.foo.com"),
               0, 0, 0, 0, 30))]
WEB_PTR = [RR(labels("1.0.1.10.in-addr.arpa"), w.PTR, w.IN, 30,
              labels("web.foo.com"))]

NOERROR, SERVFAIL, NXDOMAIN, NOTIMP, REFUSED = 0, 2, 3, 4, 5

# (qname, qtype) -> (rcode, answers, authorities, additionals)
EXPECT = {
    ("web.foo.com", w.A): (NOERROR, WEB_A, [], []),
    ("pg.foo.com", w.A): (NOERROR, PG_A, [], []),
    ("svc.foo.com", w.A): (NOERROR, SVC_A, [], []),
    ("_http._tcp.svc.foo.com", w.SRV): (NOERROR, SVC_SRV, [], SVC_EXTRA),
    # the wrong proto on a name we own (test_srv_wrong_proto_nxdomain)
    ("_http._udp.svc.foo.com", w.SRV): (NXDOMAIN, [], [], []),
    ("_http._tcp.web.foo.com", w.SRV): (NOERROR, [], WEB_SOA, []),
    # test_unsupported_types_notimp
    ("web.foo.com", w.AAAA): (NOTIMP, [], [], []),
    ("web.foo.com", w.TXT): (NOTIMP, [], [], []),
    ("web.foo.com", w.ANY): (NOTIMP, [], [], []),
    # test_host_ptr_forward_reverse, test_ptr_unknown_ip_refused
    ("1.0.1.10.in-addr.arpa", w.PTR): (NOERROR, WEB_PTR, [], []),
    ("9.9.9.10.in-addr.arpa", w.PTR): (REFUSED, [], [], []),
    # test_unknown_name_refused_not_nxdomain, and the apex, which fails
    # the ".foo.com" suffix test (test_invalid_record_servfail)
    ("nothere.foo.com", w.A): (REFUSED, [], [], []),
    ("foo.com", w.A): (REFUSED, [], [], []),
}


def expected(name, qtype, qid=0, rd=False, opt=False):
    """The whole reply. (For big.foo.com: where it is not truncated.)"""
    rcode, an, ns, ar = (NOERROR, BIG_A, [], []) \
        if (name, qtype) == ("big.foo.com", w.A) else EXPECT[(name, qtype)]
    ar = list(ar)
    if opt:  # the server's own payload size: 1400
        ar.append(RR((), w.OPT, 1400, 0, b""))
    return Msg(qid, reply_flags(rd=rd, rcode=rcode),
               [Question(labels(name), qtype)], list(an), list(ns), ar)


def canon(m):
    """A reply with the order inside each section taken out: members
    are served shuffled."""
    return (m.id, m.flags, tuple(m.questions),
            tuple(Counter(sec) for sec in m.sections()))


def query(name, qtype, qid=1, rd=False, opt=None):
    m = Msg(qid, w.flags(rd=rd),
            [Question(name if isinstance(name, tuple) else labels(name),
                      qtype)])
    if opt is not None:
        m.additionals.append(RR((), w.OPT, opt, 0, b""))
    return w.build(m)


# ------------------------------------------------------------- daemons

STARTED = []  # (what, BinderProcess or Popen, log path)


def scan_log(what, log):
    text = open(log, errors="replace").read()
    for mark in ("Sanitizer", "runtime error:"):
        assert mark not in text, f"{what}: {text[-4000:]}"


def check_daemon(what, proc, log):
    popen = getattr(proc, "proc", proc)
    assert popen is not None and popen.poll() is None, \
        f"{what} exited on its own: {popen and popen.returncode}"
    scan_log(what, log)


class Server:
    def __init__(self, tmp, level, balancer_socket=None):
        store = tmp / "tree.json"
        if not store.exists():
            store.write_text(json.dumps(make_tree()))
        self.log = tmp / f"binderd-{level}-{len(STARTED)}.log"
        self.proc = BinderProcess(
            store=f"file:{store}", workdir=tmp, log_level=level,
            log_path=str(self.log), balancer_socket=balancer_socket)
        self.proc.start()
        STARTED.append((f"binderd at {level}", self.proc, self.log))
        self.proc.wait_ready(f"b{BIG_MEMBERS - 1}.big.foo.com", timeout=20)
        self.port = self.proc.port

    def stop(self):
        self.proc.stop()


def udp_client(port):
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    s.connect(("127.0.0.1", port))
    return s


def ask(s, wire, timeout=2.0):
    """The reply to `wire` over a connected UDP socket, as bytes. UDP:
    asked again if nothing comes, and answers to earlier askings are
    passed over by id... which is why callers vary the id."""
    for _ in range(3):
        s.send(wire)
        s.settimeout(timeout)
        try:
            while True:
                data = s.recv(65535)
                if data[:2] == wire[:2]:
                    return data
        except socket.timeout:
            continue
    raise AssertionError(f"no reply to {wire.hex()}")


def tcp_read(s, count):
    """`count` length-prefixed messages (RFC 1035 4.2.2) and what is
    left over."""
    buf = b""
    out = []
    s.settimeout(5)
    while len(out) < count:
        while len(buf) >= 2 and \
                len(buf) >= 2 + struct.unpack(">H", buf[:2])[0]:
            size = struct.unpack(">H", buf[:2])[0]
            out.append(buf[2:2 + size])
            buf = buf[2 + size:]
        if len(out) >= count:
            break
        part = s.recv(65536)
        assert part, "connection closed before the reply"
        buf += part
    return out, buf


@pytest.fixture(scope="module")
def tmp():
    path = hp.short_tmpdir()
    yield path
    shutil.rmtree(path, ignore_errors=True)


@pytest.fixture(scope="module")
def servers(tmp):
    out = {}
    try:
        for level in LEVELS:
            out[level] = Server(tmp, level)
        yield out
        for level, s in out.items():
            check_daemon(f"binderd at {level}", s.proc, s.log)
    finally:
        for s in out.values():
            s.stop()
    for level, s in out.items():  # what it wrote on its way out
        scan_log(f"binderd at {level}", s.log)


@pytest.fixture(params=LEVELS)
def server(request, servers):
    return servers[request.param]


_ids = iter(range(0x100, 0xFF00))


def next_id():
    return next(_ids)


# ---------------------------------------------------------- the checks

def test_big_service_is_the_smallest_that_cannot_fit():
    """BIG_MEMBERS is computed, not guessed: the best-compressed reply
    is over 512 octets, and one member fewer would fit."""
    m = expected("big.foo.com", w.A)
    assert len(w.build(m, compress=True)) > 512
    m.answers = BIG_A[:-1]
    assert len(w.build(m, compress=True)) <= 512


def test_host_a_miss_then_memoised_hits(server):
    """Three times: the first is built, the later ones come from the
    answer table where there is one. Byte for byte the same but for the
    id."""
    with udp_client(server.port) as s:
        replies = []
        for _ in range(3):
            qid = next_id()
            data = ask(s, query("pg.foo.com", w.A, qid))
            assert w.parse(data) == expected("pg.foo.com", w.A, qid)
            replies.append(data)
        assert replies[1][2:] == replies[0][2:]
        assert replies[2][2:] == replies[0][2:]
        data = ask(s, query("web.foo.com", w.A, 7))
        assert w.parse(data) == expected("web.foo.com", w.A, 7)


@pytest.mark.parametrize("name,qtype", [
    ("svc.foo.com", w.A), ("_http._tcp.svc.foo.com", w.SRV),
    ("_http._udp.svc.foo.com", w.SRV)], ids=["A", "SRV", "wrong-proto"])
def test_service_replies(server, name, qtype):
    with udp_client(server.port) as s:
        for _ in range(4):  # built, then assembled from the table
            qid = next_id()
            got = w.parse(ask(s, query(name, qtype, qid)))
            assert canon(got) == canon(expected(name, qtype, qid))
            if qtype == w.SRV:
                for rr in got.answers:
                    assert rr.rdata[:2] == (0, 10)
                assert {rr.rdata[3] for rr in got.answers} == \
                    {rr.name for rr in got.additionals}


def test_header_echo(server):
    with udp_client(server.port) as s:
        for qid in (0x0000, 0x00FF, 0xFFFF):
            for rd in (False, True):
                got = w.parse(ask(s, query("web.foo.com", w.A, qid, rd)))
                assert got == expected("web.foo.com", w.A, qid, rd)
                assert got.id == qid
                assert bool(got.flags & w.RD) == rd
                assert got.flags & w.AA and got.flags & w.QR
                assert not got.flags & w.RA and not got.flags & w.TC


def test_uppercase_qname_is_echoed_byte_for_byte(server):
    """The owned part of the name is folded for the lookup
    (test_suffix_check_case_sensitive_pre_lowercase); the question goes
    back as it came."""
    wire = query("WeB.foo.com", w.A, 9)
    with udp_client(server.port) as s:
        data = ask(s, wire)
    got = w.parse(data)
    assert data[got.qspan[0]:got.qspan[1]] == wire[12:]
    assert got.questions == [Question(labels("WeB.foo.com"), w.A)]
    assert got.rcode == NOERROR
    assert got.answers == WEB_A  # the owner: the folded name


@pytest.mark.parametrize("name,qtype", [
    ("web.foo.com", w.A), ("_http._tcp.svc.foo.com", w.SRV),
    ("nothere.foo.com", w.A)], ids=["A", "SRV", "miss"])
def test_edns_one_opt_in_additional(server, name, qtype):
    with udp_client(server.port) as s:
        got = w.parse(ask(s, query(name, qtype, 11, opt=4096)))
    assert canon(got) == canon(expected(name, qtype, 11, opt=True))
    opts = [rr for rr in got.additionals if rr.rtype == w.OPT]
    assert opts == [RR((), w.OPT, 1400, 0, b"")]


OTHERS = sorted(k for k in EXPECT if k not in (
    ("web.foo.com", w.A), ("pg.foo.com", w.A), ("svc.foo.com", w.A),
    ("_http._tcp.svc.foo.com", w.SRV), ("_http._udp.svc.foo.com", w.SRV)))


@pytest.mark.parametrize("name,qtype", OTHERS,
                         ids=[f"{a}-{b}" for a, b in OTHERS])
def test_other_qtypes_follow_the_policy(server, name, qtype):
    with udp_client(server.port) as s:
        for rd in (False, True):
            qid = next_id()
            got = w.parse(ask(s, query(name, qtype, qid, rd)))
            assert got == expected(name, qtype, qid, rd)


def test_big_service_truncates_over_udp(server):
    wire = query("big.foo.com", w.A, 21)
    with udp_client(server.port) as s:
        data = ask(s, wire)
        got = w.parse(data)
        assert got == Msg(21, reply_flags(tc=True),
                          [Question(labels("big.foo.com"), w.A)])
        assert data[got.qspan[0]:got.qspan[1]] == wire[12:]
        assert len(data) == len(wire)
        # RFC 6891 6.2.3: with a larger payload size on offer, all of it
        data = ask(s, query("big.foo.com", w.A, 22, opt=4096))
        assert len(data) > 512
        want = expected("big.foo.com", w.A, 22, opt=True)
        assert canon(w.parse(data)) == canon(want)


def test_big_service_over_tcp_and_pipelining(server):
    want = expected("big.foo.com", w.A, 23)
    with socket.create_connection(("127.0.0.1", server.port),
                                  timeout=5) as s:
        wire = query("big.foo.com", w.A, 23)
        s.sendall(struct.pack(">H", len(wire)) + wire)
        (data,), rest = tcp_read(s, 1)
        assert rest == b""
        assert len(data) > 512
        assert canon(w.parse(data)) == canon(want)  # parse: no octet over
        # two queries in one write, two framed replies, nothing else
        q1 = query("web.foo.com", w.A, 24)
        q2 = query("_http._tcp.svc.foo.com", w.SRV, 25)
        s.sendall(struct.pack(">H", len(q1)) + q1 +
                  struct.pack(">H", len(q2)) + q2)
        (d1, d2), rest = tcp_read(s, 2)
        assert rest == b""
        assert w.parse(d1) == expected("web.foo.com", w.A, 24)
        assert canon(w.parse(d2)) == \
            canon(expected("_http._tcp.svc.foo.com", w.SRV, 25))
        s.settimeout(0.05)
        with pytest.raises(socket.timeout):
            s.recv(1)


def test_same_structures_at_every_level(servers):
    """Fast, memoised and slow replies parse to the same thing, member
    order aside."""
    questions = sorted(EXPECT) + [("big.foo.com", w.A)]
    seen = {}
    for level in LEVELS:
        with udp_client(servers[level].port) as s:
            for rnd in range(2):
                for k, (name, qtype) in enumerate(questions):
                    for opt in (None, 4096):
                        qid = 0x4000 + k
                        got = canon(w.parse(ask(
                            s, query(name, qtype, qid, opt=opt))))
                        first = seen.setdefault((name, qtype, opt), got)
                        assert got == first, (level, rnd, name, qtype, opt)


# --------------------------------------------------- through the balancer

class Chain:
    """One binderd at warn behind one one-worker balancer, the way
    tests/test_bal_shm.py sets its chains up; `flags` reach the
    balancer (-M 0 switches the shared-memory hop off)."""

    def __init__(self, tmp, tag, flags=()):
        self.bal = None
        self.server = None
        sockdir = tmp / f"socks-{tag}"
        sockdir.mkdir()
        try:
            self.server = Server(tmp, "warn",
                                 balancer_socket=str(sockdir / "b0"))
            self.port = free_port()
            self.stats = tmp / f"stats-{tag}.sock"
            self.log = tmp / f"bal-{tag}.log"
            self.bal = subprocess.Popen(
                [str(BALANCERD), "-p", str(self.port), "-H", "127.0.0.1",
                 "-s", str(sockdir), "-S", str(self.stats), "-r", "100",
                 *flags],
                env=dict(os.environ, LOG_LEVEL="warn"),
                stdout=open(self.log, "ab"), stderr=subprocess.STDOUT)
            STARTED.append((f"balancer {tag}", self.bal, self.log))
            deadline = time.time() + 20
            while True:
                try:
                    if [b["ok"] for b in
                            hp.balstat(self.stats)["backends"]] == [True]:
                        break
                except (OSError, ValueError):
                    pass
                assert time.time() < deadline, "balancer saw no backend"
                time.sleep(0.05)
            with udp_client(self.port) as s:  # forwarding has begun
                ask(s, query("web.foo.com", w.A, 1))
        except BaseException:
            self.close()
            raise

    def transport(self, want, timeout=5):
        """The switch to the rings takes a round trip after connect."""
        deadline = time.time() + timeout
        while True:
            got = [b["transport"]
                   for b in hp.balstat(self.stats)["backends"]]
            if got == [want] or time.time() > deadline:
                return got
            time.sleep(0.05)

    def close(self):
        if self.bal is not None:
            self.bal.terminate()
            try:
                self.bal.wait(timeout=5)
            except subprocess.TimeoutExpired:
                self.bal.kill()
        if self.server is not None:
            self.server.stop()


@pytest.fixture(scope="module", params=["shm", "stream"])
def chain(request, tmp):
    c = Chain(tmp, request.param,
              flags=() if request.param == "shm" else ("-M", "0"))
    try:
        assert c.transport(request.param) == [request.param]
        yield c
        check_daemon("balancer", c.bal, c.log)
        check_daemon("binderd behind it", c.server.proc, c.server.log)
    finally:
        c.close()
    scan_log("binderd behind the balancer", c.server.log)


def test_through_the_balancer_equals_direct(chain, servers):
    direct = servers["warn"]
    cases = [("pg.foo.com", w.A), ("_http._tcp.svc.foo.com", w.SRV),
             ("big.foo.com", w.A)]
    with udp_client(chain.port) as via, udp_client(direct.port) as s:
        for name, qtype in cases:
            for rnd in range(3):
                qid = next_id()
                wire = query(name, qtype, qid)
                a = w.parse(ask(via, wire))
                b = w.parse(ask(s, wire))
                assert canon(a) == canon(b), (name, rnd)
                if name == "big.foo.com":
                    assert a == Msg(qid, reply_flags(tc=True),
                                    [Question(labels(name), qtype)])
                else:
                    assert canon(a) == canon(expected(name, qtype, qid))
    with socket.create_connection(("127.0.0.1", chain.port),
                                  timeout=5) as t:
        wire = query("big.foo.com", w.A, 31)
        t.sendall(struct.pack(">H", len(wire)) + wire)
        (data,), rest = tcp_read(t, 1)
        assert rest == b""
        want = expected("big.foo.com", w.A, 31)
        assert canon(w.parse(data)) == canon(want)


# --------------------------------------------------- hostile-name sweep

SWEEP = 300
SERVED_QTYPES = (w.A, w.SRV, w.PTR, w.AAAA, w.TXT, w.ANY)


def hostile_queries():
    """(wire, has_dot): a valid header, one question, labels of any
    octets with '.', NUL and upper case over-weighted, every second one
    with an OPT."""
    rng = random.Random(0x2E2E)
    heavy = b".\0" + b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"

    def label(dot):
        size = rng.choice((1, 2, 3, 5, 8, 20, 63))
        raw = bytearray(
            rng.choice(heavy) if rng.random() < 0.3 else rng.randrange(256)
            for _ in range(size))
        if not dot:
            raw = raw.replace(b".", b"x")
        elif b"." not in raw:
            raw[rng.randrange(size)] = 0x2E
        return bytes(raw)

    out = []
    for k in range(SWEEP):
        dot = rng.random() < 0.12
        front = [label(False) for _ in range(rng.randint(0, 3))]
        if rng.random() < 0.3:  # a served name, its case disturbed
            base = rng.choice(("web", "svc", "_http._tcp.svc", "pg"))
            front += [bytes(c ^ 0x20 if 0x61 <= c <= 0x7a and
                            rng.random() < 0.3 else c for c in lab)
                      for lab in base.encode().split(b".")]
        if dot or not front:
            front.insert(rng.randint(0, len(front)), label(dot))
        tail = rng.choice((labels("foo.com"), labels("foo.com"),
                           labels("FOO.com"), labels("in-addr.arpa"), ()))
        while w.name_wire_len(tuple(front) + tail) > 255:
            front.pop(0)
        name = tuple(front) + tail
        assert name
        m = Msg(0x1000 + k, w.flags(rd=rng.random() < 0.5),
                [Question(name, rng.choice(SERVED_QTYPES))])
        if k % 2:
            m.additionals.append(
                RR((), w.OPT, rng.choice((0, 512, 1232, 4096, 65535)), 0,
                   b""))
        wire = w.build(m)
        assert w.parse(wire) == m  # hostile, but well-formed
        out.append((wire, any(b"." in lab for lab in name)))
    return out


@pytest.mark.parametrize("level", ["warn", "debug"])
def test_hostile_names(servers, level):
    """Engine::handle answers every query the decoder accepts and that is
    no response (DnsServer::slowPath drops `!parsed` and QR=1 only; with
    recursion off nothing is answered later), so every query here must
    get a reply except those with 0x2E inside a label, which the decoder
    refuses by design (docs/PARITY.md) and which must get none.

    A drop is shown without a guess at timing: onUdpReadable takes
    datagrams off the one socket in order, answers each before it looks
    at the next and sends the replies in that order, so the reply to a
    sentinel sent after the hostile query ends the wait."""
    cases = hostile_queries()
    must = [c for c in cases if not c[1]]
    assert len(must) >= 0.8 * SWEEP, len(must)
    assert len(must) < SWEEP  # and some that must be dropped
    sentinel_want = expected("web.foo.com", w.A, 0xFFFE)
    with udp_client(servers[level].port) as s:
        s.settimeout(5)
        for wire, has_dot in cases:
            s.send(wire)
            s.send(query("web.foo.com", w.A, 0xFFFE))
            got = []
            while True:
                data = s.recv(65535)
                if data[:2] == b"\xff\xfe":
                    assert w.parse(data) == sentinel_want
                    break
                got.append(data)
            if has_dot:
                assert got == [], (wire.hex(), got[0].hex())
                continue
            assert len(got) == 1, (wire.hex(), len(got))
            reply = w.parse(got[0])
            assert reply.id == struct.unpack(">H", wire[:2])[0]
            asked = w.parse(wire)
            assert got[0][reply.qspan[0]:reply.qspan[1]] == \
                wire[asked.qspan[0]:asked.qspan[1]], wire.hex()
            assert reply.flags & w.QR


# ------------------------------------------------------------ the end

def test_daemons_stayed_up_and_wrote_no_sanitizer_report(servers):
    """Last in the file: every daemon started above is still running
    (none exited on its own) and no log holds a sanitizer report."""
    checked = 0
    for what, proc, log in STARTED:
        popen = getattr(proc, "proc", proc)
        if popen is None or (isinstance(popen, subprocess.Popen) and
                             popen.returncode is not None and
                             not any(proc is s.proc
                                     for s in servers.values())):
            # stopped by its fixture, which checked it then; the log
            # stays to be read
            scan_log(what, log)
        else:
            check_daemon(what, proc, log)
        checked += 1
    assert checked >= len(LEVELS)
