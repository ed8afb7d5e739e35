"""binderd's balancer-socket ingress, spoken to directly in bsock1.

The receive side parses frames with a cursor over one buffer and writes
REPLY frames in place; these tests pin what that must not change:
answers equal to the UDP listener's, stream reassembly at every split
point, the write-blocked path past the socket buffer, large and bad
frames, client identity in the log lines, and a recursion reply whose
connection is gone.
"""
import json
import socket
import time

import pytest

from binder_amd import require_native
from binder_amd.harness import BinderProcess

MAGIC = 0xB5
QUERY, REPLY, PING, PONG = 1, 2, 3, 4
MAX_PAYLOAD = 1 << 20

TREE = {
    "foo.com": None,
    "web.foo.com": {"type": "host", "host": {"address": "1.2.3.4"}},
    "db.foo.com": {"type": "database",
                   "database": {"primary": "tcp://u@9.8.7.6:5432/x"},
                   "ttl": 20},
    "svc.foo.com": {"type": "service",
                    "service": {"srvce": "_x", "proto": "_tcp",
                                "port": 80, "ttl": 60}},
    "m0.svc.foo.com": {"type": "rr_host",
                       "rr_host": {"address": "10.0.0.9"}},
    "m1.svc.foo.com": {"type": "rr_host", "ttl": 7,
                       "rr_host": {"address": "10.0.0.10"}},
    "m2.svc.foo.com": {"type": "rr_host",
                       "rr_host": {"address": "10.0.0.11",
                                   "ports": [8080, 8081]}},
    # 12 members x (SRV + additional A) is well past 512 bytes
    "big.foo.com": {"type": "service",
                    "service": {"srvce": "_big", "proto": "_tcp",
                                "port": 443}},
}
for _i in range(12):
    TREE[f"member{_i:02d}.big.foo.com"] = {
        "type": "rr_host", "rr_host": {"address": f"10.7.0.{_i + 1}"}}

V4_SRC = bytes([127, 0, 0, 55]) + b"\x00" * 12
V6_SRC = socket.inet_pton(socket.AF_INET6, "2001:db8::55")


def query_frame(req_id, wire, family=4, proto=0, port=5353, src=V4_SRC):
    payload = (req_id.to_bytes(4, "little") + bytes([family, proto]) +
               port.to_bytes(2, "little") + src + wire)
    return bytes([MAGIC, QUERY]) + len(payload).to_bytes(4, "little") + \
        payload


def ping_frame():
    return bytes([MAGIC, PING, 0, 0, 0, 0])


def dns_wire(name, qtype="A", qid=1, rd=False, edns=None):
    msg = {"id": qid, "rd": rd,
           "questions": [{"name": name, "type": qtype}]}
    if edns is not None:
        msg["additionals"] = [{"name": "", "type": "OPT",
                               "udp_size": edns}]
    return require_native().encode_message(msg)


class FrameReader:
    """Reassembles bsock1 frames from a connected socket."""

    def __init__(self, sock):
        self.sock = sock
        self.buf = bytearray()
        self.eof = False

    def frames(self):
        """Frames completed by one more recv (possibly none)."""
        chunk = self.sock.recv(1 << 20)
        if not chunk:
            self.eof = True
            return []
        self.buf += chunk
        out = []
        pos = 0
        while len(self.buf) - pos >= 6:
            assert self.buf[pos] == MAGIC
            plen = int.from_bytes(self.buf[pos + 2:pos + 6], "little")
            if len(self.buf) - pos < 6 + plen:
                break
            out.append((self.buf[pos + 1],
                        bytes(self.buf[pos + 6:pos + 6 + plen])))
            pos += 6 + plen
        del self.buf[:pos]
        return out

    def collect(self, n_replies, n_pongs=0):
        """Read until the expected frame counts are in. Returns
        ({reqId: dns bytes}, pongs); a reqId seen twice fails."""
        replies, pongs = {}, 0
        while len(replies) < n_replies or pongs < n_pongs:
            got = self.frames()
            assert not self.eof, \
                f"closed after {len(replies)} replies, {pongs} pongs"
            for ftype, payload in got:
                if ftype == PONG:
                    pongs += 1
                    continue
                assert ftype == REPLY
                rid = int.from_bytes(payload[:4], "little")
                assert rid not in replies, f"reqId {rid} answered twice"
                replies[rid] = payload[4:]
        return replies, pongs


def connect(path, timeout=10):
    s = socket.socket(socket.AF_UNIX)
    s.settimeout(timeout)
    s.connect(str(path))
    return s


def normalized(wire):
    """Decoded reply with the member order taken out."""
    r = require_native().decode_message(wire)
    assert r is not None
    key = lambda rec: json.dumps(rec, sort_keys=True)  # noqa: E731
    r["answers"] = sorted(r["answers"], key=key)
    r["additionals"] = sorted(r["additionals"], key=key)
    return r


@pytest.fixture(scope="module")
def server(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bsock")
    store = tmp / "tree.json"
    store.write_text(json.dumps(TREE))
    sock = tmp / "b0"
    srv = BinderProcess(store=f"file:{store}", workdir=tmp,
                        log_level="warn", balancer_socket=str(sock))
    srv.start()
    srv.sock_path = sock
    yield srv
    srv.stop()


# (name, qtype, edns): hits, misses, label mismatches, case, EDNS and an
# oversize answer, on the fast and the slow path; each runs RD clear
# and RD set
KINDS = [
    ("web.foo.com", "A", None),
    ("db.foo.com", "A", None),
    ("svc.foo.com", "A", None),
    ("_x._tcp.svc.foo.com", "SRV", None),
    ("_y._tcp.svc.foo.com", "SRV", None),    # wrong _svc
    ("_x._udp.svc.foo.com", "SRV", None),    # wrong _proto
    ("_big._tcp.big.foo.com", "SRV", None),  # > 512 bytes: TC on UDP
    ("big.foo.com", "A", None),
    ("missing.foo.com", "A", None),
    ("WEB.foo.com", "A", None),
    ("web.foo.com", "A", 4096),
    ("_big._tcp.big.foo.com", "SRV", 4096),
]


def udp_raw(server, wire):
    with socket.socket(socket.AF_INET, socket.SOCK_DGRAM) as s:
        s.settimeout(3)
        s.sendto(wire, (server.host, server.port))
        return s.recvfrom(65535)[0]


@pytest.mark.parametrize("rd", [False, True])
def test_same_answers_as_udp(server, rd):
    with connect(server.sock_path) as s:
        rdr = FrameReader(s)
        for i, (name, qtype, edns) in enumerate(KINDS):
            qid = 4000 + i
            wire = dns_wire(name, qtype, qid=qid, rd=rd, edns=edns)
            s.sendall(query_frame(i, wire))
            replies, _ = rdr.collect(1)
            udp_reply = udp_raw(server, wire)
            via_bsock = normalized(replies[i])
            via_udp = normalized(udp_reply)
            # id, flags, rcode, counts and record sets in one dict
            assert via_bsock == via_udp, (name, qtype, edns, rd)
            assert via_bsock["id"] == qid
            assert via_bsock["rd"] == rd
            assert len(replies[i]) == len(udp_reply)


def test_oversize_srv_served_whole_for_tcp_clients(server):
    """proto=tcp lifts the 512-byte rule: the reply is written in place
    as one large frame and must equal the TCP listener's answer."""
    wire = dns_wire("_big._tcp.big.foo.com", "SRV", qid=77)
    with connect(server.sock_path) as s:
        s.sendall(query_frame(1, wire, proto=1))
        replies, _ = FrameReader(s).collect(1)
    r = normalized(replies[1])
    assert len(replies[1]) > 512 and not r["tc"]
    assert len(r["answers"]) == 12 and len(r["additionals"]) == 12
    t = server.dig("_big._tcp.big.foo.com", "SRV", tcp=True, qid=77)
    key = lambda rec: json.dumps(rec, sort_keys=True)  # noqa: E731
    assert r["answers"] == sorted(t["answers"], key=key)
    assert r["additionals"] == sorted(t["additionals"], key=key)


def mixed_stream(n_frames=300):
    """300 frames: the query kinds above (both RD values) with a PING
    every seventh frame. Returns (bytes, reply reqIds, ping count)."""
    out = []
    ids = []
    pings = 0
    for i in range(n_frames):
        if i % 7 == 3:
            out.append(ping_frame())
            pings += 1
            continue
        name, qtype, edns = KINDS[i % len(KINDS)]
        wire = dns_wire(name, qtype, qid=i, rd=bool(i & 1), edns=edns)
        out.append(query_frame(i, wire))
        ids.append(i)
    return b"".join(out), ids, pings


@pytest.fixture(scope="module")
def unsplit(server):
    stream, ids, pings = mixed_stream()
    with connect(server.sock_path) as s:
        s.sendall(stream)
        replies, pongs = FrameReader(s).collect(len(ids), pings)
    assert pongs == pings
    assert sorted(replies) == ids
    return stream, ids, pings, replies


@pytest.mark.parametrize("chunk", [1, 5, 6, 7, 29, 30, 31, 4096])
def test_split_points(server, unsplit, chunk):
    stream, ids, pings, whole = unsplit
    with connect(server.sock_path) as s:
        for off in range(0, len(stream), chunk):
            s.sendall(stream[off:off + chunk])
        # a closing PING: its PONG is the last frame the server writes,
        # so a reqId answered twice would have shown up before it
        s.sendall(ping_frame())
        replies, pongs = FrameReader(s).collect(len(ids), pings + 1)
    assert pongs == pings + 1
    assert sorted(replies) == ids
    for rid in ids:
        if replies[rid] == whole[rid]:
            continue
        # only the per-reply member shuffle may differ
        assert len(replies[rid]) == len(whole[rid]), rid
        assert normalized(replies[rid]) == normalized(whole[rid]), rid


def test_past_event_cap_and_socket_buffer(server):
    """~100,000 frames in one sendall with nobody reading: about 6 MB
    of replies against a 4 MiB send buffer, so the server must park on
    EPOLLOUT and resume from its write cursor."""
    n = 100_000
    wire = bytearray(dns_wire("web.foo.com", "A", qid=0))
    parts = []
    for i in range(n):
        wire[0] = (i >> 8) & 0xFF
        wire[1] = i & 0xFF
        parts.append(query_frame(i, bytes(wire)))
    blob = b"".join(parts)
    with connect(server.sock_path, timeout=30) as s:
        s.sendall(blob)  # returns only once the server has taken it all
        rdr = FrameReader(s)
        seen = bytearray(n)
        got = 0
        while got < n:
            frames = rdr.frames()
            assert not rdr.eof, f"closed after {got} replies"
            for ftype, payload in frames:
                assert ftype == REPLY
                rid = int.from_bytes(payload[:4], "little")
                assert not seen[rid], f"reqId {rid} answered twice"
                seen[rid] = 1
                d = payload[4:]
                assert d[2] & 0x80 and (d[3] & 0x0F) == 0, rid  # NOERROR
                assert (d[0] << 8 | d[1]) == (rid & 0xFFFF)
                got += 1
    assert got == n and all(seen)


def assert_serving(server):
    wire = dns_wire("web.foo.com", "A", qid=9)
    with connect(server.sock_path) as s:
        s.sendall(query_frame(5, wire))
        replies, _ = FrameReader(s).collect(1)
    r = normalized(replies[5])
    assert r["rcode"] == "NOERROR"
    assert r["answers"][0]["address"] == "1.2.3.4"


def test_large_garbage_frame_then_valid_query(server):
    garbage = bytes((i * 131 + 7) & 0xFF for i in range(200_000))
    good = dns_wire("web.foo.com", "A", qid=321)
    with connect(server.sock_path) as s:
        s.sendall(query_frame(1, garbage) + query_frame(2, good))
        replies, _ = FrameReader(s).collect(1)
        assert list(replies) == [2], "garbage payload must get no reply"
        r = normalized(replies[2])
        assert r["id"] == 321 and r["rcode"] == "NOERROR"
        assert r["answers"][0]["address"] == "1.2.3.4"
        # connection still open and serving
        s.sendall(ping_frame())
        _, pongs = FrameReader(s).collect(0, 1)
        assert pongs == 1


def test_maximum_size_frame_is_accepted(server):
    """plen == kMaxPayload is legal: the buffer grows to hold it."""
    garbage = b"\xff" * (MAX_PAYLOAD - 24)
    frame = query_frame(1, garbage)
    assert len(frame) == MAX_PAYLOAD + 6
    with connect(server.sock_path) as s:
        s.sendall(frame + ping_frame())
        _, pongs = FrameReader(s).collect(0, 1)
        assert pongs == 1


def expect_closed(s):
    try:
        assert s.recv(64) == b""
    except ConnectionError:
        pass


def test_oversize_length_closes_connection(server):
    with connect(server.sock_path) as s:
        s.sendall(bytes([MAGIC, QUERY]) +
                  (MAX_PAYLOAD + 1).to_bytes(4, "little"))
        expect_closed(s)
    assert_serving(server)


def test_wrong_magic_closes_connection(server):
    good = query_frame(1, dns_wire("web.foo.com"))
    with connect(server.sock_path) as s:
        s.sendall(bytes([0xB4]) + good[1:])
        expect_closed(s)
    assert_serving(server)


def test_client_identity_in_info_log_lines(tmp_path):
    store = tmp_path / "tree.json"
    store.write_text(json.dumps(TREE))
    log = tmp_path / "b.log"
    sock = tmp_path / "b0"
    srv = BinderProcess(store=f"file:{store}", workdir=tmp_path,
                        log_level="info", log_path=str(log),
                        balancer_socket=str(sock))
    srv.start()
    try:
        cases = [  # (reqId/qid, name, family, proto, port, src)
            (11, "web.foo.com", 4, 0, 5353, V4_SRC),   # fast path
            (12, "WEB.foo.com", 4, 0, 5353, V4_SRC),   # slow path
            (13, "web.foo.com", 6, 1, 40000, V6_SRC),  # fast path
            (14, "WEB.foo.com", 6, 1, 40000, V6_SRC),  # slow path
        ]
        with connect(sock) as s:
            for rid, name, fam, proto, port, src in cases:
                s.sendall(query_frame(
                    rid, dns_wire(name, "A", qid=rid), family=fam,
                    proto=proto, port=port, src=src))
            FrameReader(s).collect(len(cases))
        # the UDP and TCP listeners format lazily too
        srv.dig("web.foo.com", qid=15)
        srv.dig("web.foo.com", qid=16, tcp=True)
        want = {11: ("127.0.0.55", "5353/udp"),
                12: ("127.0.0.55", "5353/udp"),
                13: ("2001:db8::55", "40000/tcp"),
                14: ("2001:db8::55", "40000/tcp")}
        seen = {}
        deadline = time.time() + 5
        while time.time() < deadline and len(seen) < 6:
            for ln in log.read_text().splitlines():
                try:
                    d = json.loads(ln)
                except ValueError:
                    continue
                if d.get("msg") == "DNS query":
                    seen[d["req_id"]] = (d["client"], d["port"])
            if len(seen) < 6:
                time.sleep(0.02)
        for rid, fields in want.items():
            assert seen.get(rid) == fields, (rid, seen)
        assert seen[15][0] == "127.0.0.1" and seen[15][1].endswith("/udp")
        assert seen[16][0] == "127.0.0.1" and seen[16][1].endswith("/tcp")
    finally:
        srv.stop()


def test_recursion_reply_after_balancer_connection_closed(tmp_path):
    """A query handed to recursion over the balancer socket whose
    connection closes before the upstream answers: the late reply is
    discarded, nothing crashes, and recursion still works for the next
    connection."""
    n = require_native()
    up = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    up.bind(("127.0.0.2", 0))
    up.settimeout(5)
    tree = tmp_path / "local.json"
    tree.write_text(json.dumps({"foo.com": None}))
    sock = tmp_path / "b0"
    srv = BinderProcess(
        dns_domain="foo.com", datacenter="dc1",
        store=f"file:{tree}", workdir=tmp_path,
        balancer_socket=str(sock),
        config={"recursion": {
            "source": "static", "regionName": "r1",
            "dnsDomain": "foo.com",
            "upstreamPort": up.getsockname()[1],
            "dcs": {"dc2": ["127.0.0.2"]},
        }})
    srv.start()

    def answer(data, addr):
        q = n.decode_message(data)
        up.sendto(n.encode_message({
            "id": q["id"], "qr": True,
            "questions": [dict(q["questions"][0])],
            "answers": [{"name": q["questions"][0]["name"], "type": "A",
                         "ttl": 30, "address": "10.22.0.1"}],
        }), addr)

    try:
        wire = dns_wire("web.dc2.foo.com", "A", qid=50, rd=True)
        s = connect(sock)
        s.sendall(query_frame(1, wire))
        data, addr = up.recvfrom(4096)  # the query is now in recursion
        s.close()
        # a round trip on a new connection: the server has been through
        # its event loop since the close
        with connect(sock) as s2:
            s2.sendall(ping_frame())
            assert FrameReader(s2).collect(0, 1)[1] == 1
            answer(data, addr)  # late answer for the closed connection
            # same path again, connection kept open this time
            s2.sendall(query_frame(2, wire))
            answer(*up.recvfrom(4096))
            replies, _ = FrameReader(s2).collect(1)
        r = normalized(replies[2])
        assert r["rcode"] == "NOERROR" and r["id"] == 50
        assert r["answers"][0]["address"] == "10.22.0.1"
        assert srv.proc.poll() is None
    finally:
        srv.stop()
        up.close()
