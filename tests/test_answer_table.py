"""binderd's answer table and the balancer-socket serving pipeline.

The table memoises the fast path's finished replies per (qname, qtype);
info-level logging bypasses it. Every check here therefore compares a
binderd at warn level (table on) with a twin at info level (table off)
that mirrors the same ZooKeeper tree: same answers on a miss and on a
hit, the new answer after every kind of tree change, no memo for the
forms the fast path declines, replies complete and in request order at
the pipeline's edges, and the per-reply member shuffle intact.
"""
import json
import re
import shutil
import socket
import tempfile
import time
from pathlib import Path

import pytest

from binder_amd import require_native
from binder_amd.harness import BinderProcess
from binder_amd.stubzk import StubZk

REPO = Path(__file__).resolve().parent.parent
MAGIC = 0xB5
QUERY, REPLY, PING, PONG = 1, 2, 3, 4
V4_SRC = bytes([127, 0, 0, 55]) + b"\x00" * 12

N_HOSTS = 40
N_SVCS = 4
N_MEMBERS = 4
BIG_MEMBERS = 12  # 12 x (SRV + additional A) is well past 512 bytes


def pipe_depth():
    """K, the pipeline's lookahead, as compiled into binderd."""
    text = (REPO / "native" / "server" / "server.hpp").read_text()
    return int(re.search(r"kPipeDepth\s*=\s*(\d+)", text).group(1))


K = pipe_depth()


def jput(zk, path, obj):
    zk.put(path, json.dumps(obj).encode())


def host(addr):
    return {"type": "host", "host": {"address": addr}}


def member(addr):
    return {"type": "rr_host", "rr_host": {"address": addr}}


SERVICE = {"type": "service",
           "service": {"srvce": "_x", "proto": "_tcp", "port": 80,
                       "ttl": 60}}


def build_tree(zk):
    zk.mkdirp("/com/foo")
    for i in range(N_HOSTS):
        jput(zk, f"/com/foo/h{i}", host(f"10.1.0.{i + 1}"))
    for i in range(N_SVCS):
        jput(zk, f"/com/foo/s{i}", SERVICE)
        for j in range(N_MEMBERS):
            jput(zk, f"/com/foo/s{i}/m{j}", member(f"10.9.{i}.{j + 1}"))
    jput(zk, "/com/foo/big", SERVICE)
    for j in range(BIG_MEMBERS):
        jput(zk, f"/com/foo/big/member{j:02d}", member(f"10.7.0.{j + 1}"))


def all_names():
    names = [(f"h{i}.foo.com", "A") for i in range(N_HOSTS)]
    for i in range(N_SVCS):
        names.append((f"s{i}.foo.com", "A"))
        names.append((f"_x._tcp.s{i}.foo.com", "SRV"))
    return names


class Pair:
    """A table-on binderd, its table-off twin, and their tree."""

    def __init__(self):
        # short directory: the balancer sockets live in it
        self.tmp = Path(tempfile.mkdtemp(prefix="bt-"))
        self.zk = StubZk().start()
        build_tree(self.zk)
        self.memo = self._binderd("warn", "m")
        self.plain = self._binderd("info", "p")
        last = f"member{BIG_MEMBERS - 1:02d}.big.foo.com"
        for b in (self.memo, self.plain):
            b.wait_ready(last, timeout=30)
            b.wait_ready(f"h{N_HOSTS - 1}.foo.com", timeout=30)

    def _binderd(self, level, tag):
        sock = self.tmp / tag
        b = BinderProcess(store="zk", zk_host="127.0.0.1",
                          zk_port=self.zk.port, workdir=self.tmp,
                          log_level=level, balancer_socket=str(sock),
                          log_path=str(self.tmp / f"{tag}.log"))
        b.start()
        b.sock_path = sock
        return b

    def close(self):
        self.memo.stop()
        self.plain.stop()
        self.zk.stop()
        shutil.rmtree(self.tmp, ignore_errors=True)


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    p.close()


def view(r):
    """What two replies to the same question must agree on: flags,
    rcode, question, counts and the record sets without their order."""
    key = lambda rec: json.dumps(rec, sort_keys=True)  # noqa: E731
    out = {k: v for k, v in r.items()
           if k not in ("id", "answers", "additionals")}
    out["answers"] = sorted(r["answers"], key=key)
    out["additionals"] = sorted(r["additionals"], key=key)
    return out


def same_as_twin(pair, name, qtype="A", **kw):
    """Ask both servers; the memo server's reply is returned once it
    has been found equal to the twin's."""
    got = pair.memo.dig(name, qtype, **kw)
    want = pair.plain.dig(name, qtype, **kw)
    assert view(got) == view(want), (name, qtype, kw)
    return got


# ---------------- parity, miss then hit ----------------

def test_parity_with_table_bypassed(pair):
    qid = 100
    for rd in (False, True):
        for name, qtype in all_names():
            for _ in range(2):  # first ask of a name misses, then hits
                qid += 1
                r = same_as_twin(pair, name, qtype, rd=rd, qid=qid)
                assert r["id"] == qid
                assert r["rd"] == rd
                assert r.status == "NOERROR"
                if qtype == "SRV":
                    assert len(r.answers) == N_MEMBERS
                    assert len(r["additionals"]) == N_MEMBERS
                elif name.startswith("s"):
                    assert len(r.answers) == N_MEMBERS
                else:
                    assert len(r.answers) == 1


# ---------------- invalidation through the mirror ----------------

def converge(pair, name, qtype, expect):
    """After a tree change: the twin reaches the expected state, the
    memo server follows it and then stays there."""
    deadline = time.time() + 12
    while not expect(pair.plain.dig(name, qtype)):
        assert time.time() < deadline, f"twin never saw {name} change"
    while view(pair.memo.dig(name, qtype)) != \
            view(pair.plain.dig(name, qtype)):
        assert time.time() < deadline, \
            f"{name} {qtype}: still the memoised answer"
    for _ in range(4):
        r = same_as_twin(pair, name, qtype)
        assert expect(r), (name, qtype, r)


def addresses(r):
    return sorted(a["address"] for a in r.answers)


def extra_addresses(r):
    return sorted(a["address"] for a in r["additionals"])


def test_invalidation_through_the_mirror():
    p = Pair()
    try:
        zk = p.zk
        svc_a, svc_srv = "s0.foo.com", "_x._tcp.s0.foo.com"
        # memoise everything that is about to change
        for name, qtype in [("h0.foo.com", "A"), ("h1.foo.com", "A"),
                            (svc_a, "A"), (svc_srv, "SRV"),
                            ("s1.foo.com", "A"),
                            ("_x._tcp.s1.foo.com", "SRV")]:
            for _ in range(2):
                same_as_twin(p, name, qtype)

        # a host's address
        jput(zk, "/com/foo/h0", host("10.1.9.9"))
        converge(p, "h0.foo.com", "A",
                 lambda r: addresses(r) == ["10.1.9.9"])

        # a member's address: the service's A and SRV answers follow
        jput(zk, "/com/foo/s0/m0", member("10.9.0.77"))
        converge(p, svc_a, "A", lambda r: "10.9.0.77" in addresses(r)
                 and "10.9.0.1" not in addresses(r))
        converge(p, svc_srv, "SRV",
                 lambda r: "10.9.0.77" in extra_addresses(r)
                 and "10.9.0.1" not in extra_addresses(r))

        # a member added
        jput(zk, "/com/foo/s0/m4", member("10.9.0.5"))
        converge(p, svc_a, "A",
                 lambda r: len(r.answers) == N_MEMBERS + 1
                 and "10.9.0.5" in addresses(r))
        converge(p, svc_srv, "SRV",
                 lambda r: len(r.answers) == N_MEMBERS + 1
                 and "10.9.0.5" in extra_addresses(r))

        # a member removed
        zk.rmr("/com/foo/s0/m1")
        converge(p, svc_a, "A",
                 lambda r: len(r.answers) == N_MEMBERS
                 and "10.9.0.2" not in addresses(r))
        converge(p, svc_srv, "SRV",
                 lambda r: len(r.answers) == N_MEMBERS
                 and "10.9.0.2" not in extra_addresses(r))

        # a host deleted: no longer answered, from the table or at all
        zk.rmr("/com/foo/h1")
        converge(p, "h1.foo.com", "A",
                 lambda r: r.status != "NOERROR" and not r.answers)

        # a service deleted: both of its entries go
        zk.rmr("/com/foo/s1")
        converge(p, "s1.foo.com", "A",
                 lambda r: r.status != "NOERROR" and not r.answers)
        converge(p, "_x._tcp.s1.foo.com", "SRV",
                 lambda r: r.status != "NOERROR" and not r.answers)

        # untouched names still answer as before
        same_as_twin(p, "h2.foo.com")
        same_as_twin(p, "_x._tcp.s2.foo.com", "SRV")
    finally:
        p.close()


# ---------------- forms the table must not memoise ----------------

def test_uppercase_name_is_not_memoised(pair):
    for name in ("H3.foo.com", "h3.foo.com", "h3.foo.com", "H3.FOO.com",
                 "h3.foo.com"):
        r = same_as_twin(pair, name)
        assert r["questions"][0]["name"] == name
        if name == name.lower():  # whatever the other forms get
            assert r.status == "NOERROR"
            assert addresses(r) == ["10.1.0.4"]


def test_edns_query_is_not_memoised(pair):
    def has_opt(r):
        return any(a["type"] == "OPT" for a in r["additionals"])

    for name, qtype in (("h4.foo.com", "A"),
                        ("_x._tcp.s3.foo.com", "SRV")):
        assert has_opt(same_as_twin(pair, name, qtype, edns=4096))
        for _ in range(2):
            assert not has_opt(same_as_twin(pair, name, qtype))
        assert has_opt(same_as_twin(pair, name, qtype, edns=4096))


def test_oversize_service_is_not_memoised(pair):
    name = "_x._tcp.big.foo.com"
    for _ in range(2):
        udp = same_as_twin(pair, name, "SRV")
        assert udp["tc"], udp
    # whole over TCP, where the 512-byte rule does not apply ...
    for _ in range(2):
        tcp = same_as_twin(pair, name, "SRV", tcp=True)
        assert len(tcp.answers) == BIG_MEMBERS and not tcp["tc"]
    # ... and the TCP answer did not become UDP's
    assert same_as_twin(pair, name, "SRV")["tc"]
    # the same service's A answer fits and is served normally
    for _ in range(2):
        assert len(same_as_twin(pair, "big.foo.com").answers) == \
            BIG_MEMBERS


# ---------------- pipeline edges over the balancer socket ----------------

def query_frame(req_id, wire, proto=0):
    payload = (req_id.to_bytes(4, "little") + bytes([4, proto]) +
               (5353).to_bytes(2, "little") + V4_SRC + wire)
    return bytes([MAGIC, QUERY]) + len(payload).to_bytes(4, "little") + \
        payload


PING_FRAME = bytes([MAGIC, PING, 0, 0, 0, 0])


def dns_wire(name, qtype, qid):
    return require_native().encode_message(
        {"id": qid, "rd": False,
         "questions": [{"name": name, "type": qtype}]})


class Stream:
    """bsock1 frames off a connected socket, in arrival order."""

    def __init__(self, path):
        self.sock = socket.socket(socket.AF_UNIX)
        self.sock.settimeout(10)
        self.sock.connect(str(path))
        self.buf = bytearray()

    def close(self):
        self.sock.close()

    def send(self, data):
        self.sock.sendall(data)

    def take(self, count):
        """The next `count` frames as ("pong",) or ("reply", reqId,
        decoded message)."""
        out = []
        while len(out) < count:
            while True:
                if len(self.buf) >= 6:
                    assert self.buf[0] == MAGIC
                    plen = int.from_bytes(self.buf[2:6], "little")
                    if len(self.buf) >= 6 + plen:
                        break
                chunk = self.sock.recv(1 << 20)
                assert chunk, f"closed after {len(out)} frames"
                self.buf += chunk
            ftype, payload = self.buf[1], bytes(self.buf[6:6 + plen])
            del self.buf[:6 + plen]
            if ftype == PONG:
                out.append(("pong",))
            else:
                assert ftype == REPLY
                msg = require_native().decode_message(payload[4:])
                assert msg is not None, "undecodable reply"
                out.append(("reply", int.from_bytes(payload[:4], "little"),
                            msg))
        return out


@pytest.fixture()
def stream(pair):
    s = Stream(pair.memo.sock_path)
    yield s
    s.close()


def batch_names(count):
    pool = all_names()
    # hosts, service A and SRV interleaved
    return [pool[(i * 7) % len(pool)] for i in range(count)]


def check_replies(pair, frames, asked, base_id):
    """frames: take() output holding only replies; asked: the (name,
    qtype) of each request, in request order."""
    assert len(frames) == len(asked)
    for i, (frame, (name, qtype)) in enumerate(zip(frames, asked)):
        kind, req_id, msg = frame
        assert kind == "reply"
        assert req_id == base_id + i, "replies out of request order"
        assert msg["id"] == (base_id + i) & 0xFFFF
        assert msg["questions"][0]["name"] == name
        want = pair.plain.dig(name, qtype)
        got = dict(msg)
        assert view(got) == view(want), (i, name, qtype)


@pytest.mark.parametrize(
    "count", sorted({1, max(1, K - 1), K, K + 1, 3 * K + 1}))
def test_one_write_of_n_frames(pair, stream, count):
    base = 7000
    asked = batch_names(count)
    # the whole batch twice: first cold for some names, then all hits
    for _ in range(2):
        stream.send(b"".join(
            query_frame(base + i, dns_wire(n, t, base + i))
            for i, (n, t) in enumerate(asked)))
        check_replies(pair, stream.take(count), asked, base)


def test_ping_in_the_middle_of_a_batch(pair, stream):
    base = 8000
    asked = batch_names(2 * K + 1)
    frames = [query_frame(base + i, dns_wire(n, t, base + i))
              for i, (n, t) in enumerate(asked)]
    at = K // 2 + 1
    stream.send(b"".join(frames[:at]) + PING_FRAME + b"".join(frames[at:]))
    got = stream.take(len(asked) + 1)
    assert got[at] == ("pong",), "PONG left its place in the order"
    check_replies(pair, got[:at] + got[at + 1:], asked, base)


def test_fast_path_miss_in_the_middle_of_a_batch(pair, stream):
    base = 9000
    asked = batch_names(2 * K + 1)
    at = K // 2 + 1
    asked[at] = ("nope.foo.com", "A")       # unknown: slow path
    asked[at + 2] = ("H5.foo.com", "A")     # uppercase: slow path
    stream.send(b"".join(
        query_frame(base + i, dns_wire(n, t, base + i))
        for i, (n, t) in enumerate(asked)))
    got = stream.take(len(asked))
    check_replies(pair, got, asked, base)
    assert got[at][2]["rcode"] != "NOERROR"
    assert got[at + 2][2]["rcode"] == "NOERROR"


def test_frame_split_at_every_byte_offset(pair, stream):
    """The frame's first part ends one read: a PING rides in front of
    it and its PONG is awaited before the rest is sent, so the server
    has provably parsed up to the partial frame."""
    name, qtype = "_x._tcp.s2.foo.com", "SRV"
    before, after = ("h6.foo.com", "A"), ("s3.foo.com", "A")
    want = view(pair.plain.dig(name, qtype))
    whole = query_frame(2, dns_wire(name, qtype, 2))
    for cut in range(1, len(whole)):
        stream.send(query_frame(1, dns_wire(*before, 1)) + PING_FRAME +
                    whole[:cut])
        first = stream.take(2)
        assert first[0][:2] == ("reply", 1) and first[1] == ("pong",)
        stream.send(whole[cut:] + query_frame(3, dns_wire(*after, 3)))
        second = stream.take(2)
        assert [f[1] for f in second] == [2, 3], cut
        assert view(second[0][2]) == want, cut
        assert second[1][2]["questions"][0]["name"] == after[0]


# ---------------- shuffle ----------------

def test_every_member_reaches_every_position(pair):
    name = "_x._tcp.s0.foo.com"
    seen_srv = [set() for _ in range(N_MEMBERS)]
    seen_add = [set() for _ in range(N_MEMBERS)]
    seen_a = [set() for _ in range(N_MEMBERS)]
    for _ in range(300):
        r = pair.memo.dig(name, "SRV")
        assert len(r.answers) == N_MEMBERS
        for pos, a in enumerate(r.answers):
            seen_srv[pos].add(a["target"])
        for pos, a in enumerate(r["additionals"]):
            seen_add[pos].add(a["address"])
        # SRV records and their additional A records share one order
        assert [a["target"] for a in r.answers] == \
            [a["name"] for a in r["additionals"]]
        r = pair.memo.dig("s0.foo.com", "A")
        for pos, a in enumerate(r.answers):
            seen_a[pos].add(a["address"])
    for seen in (seen_srv, seen_add, seen_a):
        for pos in range(N_MEMBERS):
            assert len(seen[pos]) == N_MEMBERS, (pos, seen[pos])
