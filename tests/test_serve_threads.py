"""binderd's pool of serving threads (BINDER_SERVE_THREADS >= 2).

Balancer connections are spread over threads that each own an event
loop and a private answer table; everything that is not a table hit
runs under one serving lock, at its frame's place in the batch. These
tests pin what the pool must not change - reply order per connection,
answers equal to a table-bypassed twin's, invalidation seen on every
connection once it has been seen on one, exact metrics, recursion
replies across threads, churn and a clean SIGTERM - and that info-level
logging switches the pool off.

Every daemon writes to a log file which is checked for ThreadSanitizer
reports after it stops: with a plain build that finds nothing, with the
`make check-serve-threads` build it is the race check.
"""
import json
import re
import shutil
import socket
import tempfile
import threading
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
PING_FRAME = bytes([MAGIC, PING, 0, 0, 0, 0])

T = 3
N_HOSTS = 40
N_SVCS = 4
N_MEMBERS = 4
K = int(re.search(
    r"kPipeDepth\s*=\s*(\d+)",
    (REPO / "native" / "server" / "server.hpp").read_text()).group(1))


# ---------------- tree ----------------

def host(addr):
    return {"type": "host", "host": {"address": addr}}


def member(addr):
    return {"type": "rr_host", "rr_host": {"address": addr}}


SERVICE = {"type": "service",
           "service": {"srvce": "_x", "proto": "_tcp", "port": 80,
                       "ttl": 60}}


def tree_records():
    """domain -> record, the same tree for the file and the zk store"""
    recs = {"foo.com": None}
    for i in range(N_HOSTS):
        recs[f"h{i}.foo.com"] = host(f"10.1.0.{i + 1}")
    for i in range(N_SVCS):
        recs[f"s{i}.foo.com"] = SERVICE
        for j in range(N_MEMBERS):
            recs[f"m{j}.s{i}.foo.com"] = member(f"10.9.{i}.{j + 1}")
    return recs


def zk_path(domain):
    return "/" + "/".join(reversed(domain.split(".")))


def all_names():
    names = [(f"h{i}.foo.com", "A") for i in range(N_HOSTS)]
    for i in range(N_SVCS):
        names.append((f"s{i}.foo.com", "A"))
        names.append((f"_x._tcp.s{i}.foo.com", "SRV"))
    return names


# ---------------- daemons ----------------

def assert_no_tsan(log_path):
    text = Path(log_path).read_text(errors="replace")
    assert "ThreadSanitizer" not in text, text[-4000:]


class Daemon:
    """A binderd with a balancer socket and a log file; stop() also
    checks the log for ThreadSanitizer reports."""

    def __init__(self, tmp, tag, threads, level="warn", **kw):
        self.sock_path = Path(tmp) / tag
        self.log_path = Path(tmp) / f"{tag}.log"
        self.proc = BinderProcess(workdir=tmp, log_level=level,
                                  balancer_socket=str(self.sock_path),
                                  log_path=str(self.log_path), **kw)
        self.proc.env["BINDER_SERVE_THREADS"] = str(threads)
        self.proc.start()

    def stop(self):
        self.proc.stop()
        assert_no_tsan(self.log_path)


@pytest.fixture()
def tmp():
    # short directory: the balancer sockets live in it
    d = Path(tempfile.mkdtemp(prefix="st-"))
    yield d
    shutil.rmtree(d, ignore_errors=True)


def file_store(tmp):
    p = Path(tmp) / "tree.json"
    p.write_text(json.dumps(tree_records()))
    return f"file:{p}"


# ---------------- bsock1 ----------------

def query_frame(req_id, wire, proto=0):
    payload = (req_id.to_bytes(4, "little") + bytes([4, proto]) +
               (5353).to_bytes(2, "little") + V4_SRC + wire)
    return bytes([MAGIC, QUERY]) + len(payload).to_bytes(4, "little") + \
        payload


def dns_wire(name, qtype="A", qid=1, rd=False):
    return require_native().encode_message(
        {"id": qid & 0xFFFF, "rd": rd,
         "questions": [{"name": name, "type": qtype}]})


class Stream:
    """bsock1 frames off a connected socket, in arrival order."""

    def __init__(self, path, timeout=20):
        self.sock = socket.socket(socket.AF_UNIX)
        self.sock.settimeout(timeout)
        self.sock.connect(str(path))
        self.buf = bytearray()

    def close(self):
        self.sock.close()

    def send(self, data):
        self.sock.sendall(data)

    def take_raw(self, count):
        """The next `count` frames as (type, payload)."""
        out = []
        pos = 0
        while len(out) < count:
            if len(self.buf) - pos >= 6:
                assert self.buf[pos] == MAGIC
                plen = int.from_bytes(self.buf[pos + 2:pos + 6], "little")
                if len(self.buf) - pos >= 6 + plen:
                    out.append((self.buf[pos + 1],
                                bytes(self.buf[pos + 6:pos + 6 + plen])))
                    pos += 6 + plen
                    continue
            chunk = self.sock.recv(1 << 20)
            assert chunk, f"closed after {len(out)} frames"
            self.buf += chunk
        del self.buf[:pos]
        return out

    def take(self, count):
        """... as ("pong",) or ("reply", reqId, decoded message)."""
        out = []
        for ftype, payload in self.take_raw(count):
            if ftype == PONG:
                out.append(("pong",))
                continue
            assert ftype == REPLY
            msg = require_native().decode_message(payload[4:])
            assert msg is not None, "undecodable reply"
            out.append(("reply", int.from_bytes(payload[:4], "little"),
                        msg))
        return out

    def ask(self, name, qtype="A", req_id=1):
        self.send(query_frame(req_id, dns_wire(name, qtype, req_id)))
        (kind, rid, msg), = self.take(1)
        assert kind == "reply" and rid == req_id
        return msg


def view(r):
    """What two replies to one question agree on: everything but the
    id and the member order."""
    key = lambda rec: json.dumps(rec, sort_keys=True)  # noqa: E731
    out = {k: v for k, v in dict(r).items()
           if k not in ("id", "answers", "additionals")}
    out["answers"] = sorted(r["answers"], key=key)
    out["additionals"] = sorted(r["additionals"], key=key)
    return out


def addresses(msg):
    return sorted(a["address"] for a in msg["answers"])


def extra_addresses(msg):
    return sorted(a["address"] for a in msg["additionals"])


def run_threads(fns):
    """Run the callables concurrently; re-raise the first failure."""
    errors = []

    def wrap(fn):
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=wrap, args=(fn,)) for fn in fns]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads), "driver thread stuck"
    if errors:
        raise errors[0]


# ---------------- 1. order and parity ----------------

def test_order_and_parity_on_four_connections(tmp):
    store = file_store(tmp)
    pooled = Daemon(tmp, "m", T, store=store)
    plain = Daemon(tmp, "p", 1, level="info", store=store)
    try:
        pool = all_names()
        # the twin's answer to everything that will be asked, taken once
        # and shared by the four drivers
        want = {}
        for name, qtype in pool + [("nope.foo.com", "A"),
                                   ("H5.foo.com", "A")]:
            want[(name, qtype)] = view(plain.proc.dig(name, qtype))

        def drive(conn_no):
            s = Stream(pooled.sock_path)
            try:
                base = 100000 * (conn_no + 1)
                for count in (K - 1, K, K + 1, 3 * K + 1):
                    asked = [pool[(i * 7 + conn_no * 3 + count) % len(pool)]
                             for i in range(count)]
                    at = count // 2
                    asked[at - 1] = ("nope.foo.com", "A")  # unknown name
                    asked[at + 1] = ("H5.foo.com", "A")    # uppercase
                    frames = [query_frame(base + i,
                                          dns_wire(n, t, base + i))
                              for i, (n, t) in enumerate(asked)]
                    blob = b"".join(frames[:at]) + PING_FRAME + \
                        b"".join(frames[at:])
                    for _ in range(2):  # cold, then hits
                        s.send(blob)
                        got = s.take(count + 1)
                        assert got[at] == ("pong",), \
                            "PONG left its place in the order"
                        replies = got[:at] + got[at + 1:]
                        for i, (frame, q) in enumerate(zip(replies, asked)):
                            assert frame[0] == "reply"
                            assert frame[1] == base + i, \
                                "replies out of request order"
                            assert frame[2]["id"] == (base + i) & 0xFFFF
                            assert view(frame[2]) == want[q], (i, q)
                    base += 1000
            finally:
                s.close()

        run_threads([lambda n=n: drive(n) for n in range(4)])
    finally:
        pooled.stop()
        plain.stop()


# ---------------- 2. invalidation across threads ----------------

def test_invalidation_reaches_every_thread():
    tmp = Path(tempfile.mkdtemp(prefix="st-"))
    zk = StubZk().start()
    d = None
    streams = []
    try:
        for domain, rec in tree_records().items():
            path = zk_path(domain)
            if rec is None:
                zk.mkdirp(path)
            else:
                zk.put(path, json.dumps(rec).encode())
        d = Daemon(tmp, "m", T, store="zk", zk_host="127.0.0.1",
                   zk_port=zk.port)
        d.proc.wait_ready(f"m{N_MEMBERS - 1}.s{N_SVCS - 1}.foo.com",
                          timeout=30)
        d.proc.wait_ready(f"h{N_HOSTS - 1}.foo.com", timeout=30)
        # opened one after the other: accepted round-robin, so the
        # three connections belong to three threads
        for _ in range(T):
            s = Stream(d.sock_path)
            assert s.ask("h0.foo.com")["rcode"] == "NOERROR"
            streams.append(s)
        a, b, c = streams
        srv = "_x._tcp.s0.foo.com"
        rid = 10
        for rnd in range(30):
            # a host's address
            addr = f"10.4.{rnd}.7"
            for s in streams:  # memoised on all three threads
                for _ in range(2):
                    s.ask("h1.foo.com", "A", rid)
            zk.put("/com/foo/h1", json.dumps(host(addr)).encode())
            deadline = time.time() + 10
            while addresses(a.ask("h1.foo.com", "A", rid)) != [addr]:
                assert time.time() < deadline, "A never saw the new host"
            rid += 1
            for s in (b, c):
                assert addresses(s.ask("h1.foo.com", "A", rid)) == [addr], \
                    f"round {rnd}: old answer after the new one was seen"

            # a service's SRV answer after a member change
            maddr = f"10.5.{rnd}.9"
            for s in streams:
                for _ in range(2):
                    s.ask(srv, "SRV", rid)
            zk.put("/com/foo/s0/m0", json.dumps(member(maddr)).encode())
            deadline = time.time() + 10
            while maddr not in extra_addresses(a.ask(srv, "SRV", rid)):
                assert time.time() < deadline, "A never saw the member"
            rid += 1
            for s in (b, c):
                assert maddr in extra_addresses(s.ask(srv, "SRV", rid)), \
                    f"round {rnd}: old SRV after the new one was seen"
    finally:
        for s in streams:
            s.close()
        try:
            if d is not None:
                d.stop()
        finally:
            zk.stop()
            shutil.rmtree(tmp, ignore_errors=True)


# ---------------- 3. metrics ----------------

def completed(text):
    """binder_requests_completed by type label"""
    out = {}
    for ln in text.splitlines():
        m = re.match(r'binder_requests_completed\{.*type="(\w+)"\} (\d+)',
                     ln)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def test_scrape_counts_every_reply_received(tmp):
    d = Daemon(tmp, "m", T, store=file_store(tmp))
    streams = [Stream(d.sock_path) for _ in range(3)]
    try:
        names = [("h2.foo.com", "A"), ("s1.foo.com", "A"),
                 ("_x._tcp.s1.foo.com", "SRV")]
        for s in streams:  # warm: the 300 below are hits
            for n, t in names:
                s.ask(n, t)
        before = completed(d.proc.metrics())
        n_total, n_srv = 300, 0
        sent = [0, 0, 0]
        for i in range(n_total):
            n, t = names[i % 3] if i % 5 else names[2]
            n_srv += t == "SRV"
            k = i % 3
            streams[k].send(query_frame(i, dns_wire(n, t, i)))
            sent[k] += 1
        for s, k in zip(streams, sent):
            assert len(s.take_raw(k)) == k
        after = completed(d.proc.metrics())
        assert after.get("SRV", 0) - before.get("SRV", 0) == n_srv
        assert after.get("A", 0) - before.get("A", 0) == n_total - n_srv
        # the histograms count the same events
        text = d.proc.metrics()
        for metric in ("binder_request_latency_seconds_count",
                       "binder_response_size_bytes_count"):
            got = sum(int(m.group(1)) for m in re.finditer(
                metric + r'\{[^}]*\} (\d+)', text))
            assert got == sum(after.values()), metric
    finally:
        for s in streams:
            s.close()
        d.stop()


# ---------------- 4. recursion ----------------

def test_recursion_replies_cross_threads(tmp):
    n = require_native()
    up = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    up.bind(("127.0.0.2", 0))
    up.settimeout(5)
    tree = tmp / "local.json"
    tree.write_text(json.dumps({"foo.com": None,
                                "web.foo.com": host("1.2.3.4")}))
    d = Daemon(tmp, "m", T, dns_domain="foo.com", datacenter="dc1",
               store=f"file:{tree}",
               config={"recursion": {
                   "source": "static", "regionName": "r1",
                   "dnsDomain": "foo.com",
                   "upstreamPort": up.getsockname()[1],
                   "dcs": {"dc2": ["127.0.0.2"]},
               }})

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
        # answered: the upstream's reply arrives on the main thread and
        # is written by the connection's own
        s = Stream(d.sock_path)
        s.send(query_frame(1, wire))
        answer(*up.recvfrom(4096))
        (kind, rid, msg), = s.take(1)
        assert (kind, rid) == ("reply", 1)
        assert msg["rcode"] == "NOERROR" and msg["id"] == 50
        assert msg["answers"][0]["address"] == "10.22.0.1"
        # a local hit on the same connection still works
        assert addresses(s.ask("web.foo.com", "A", 2)) == ["1.2.3.4"]

        # closed before the upstream answers
        s.send(query_frame(3, wire))
        data, addr = up.recvfrom(4096)
        s.close()
        # T further connections: one lands on the closed connection's
        # thread, and each has been through its loop after the close
        others = [Stream(d.sock_path) for _ in range(T)]
        try:
            for o in others:
                o.send(PING_FRAME)
                assert o.take(1) == [("pong",)]
            answer(data, addr)  # late answer for the closed connection
            for i, o in enumerate(others):
                o.send(query_frame(10 + i, wire))
                answer(*up.recvfrom(4096))
                (kind, rid, msg), = o.take(1)
                assert (kind, rid) == ("reply", 10 + i)
                assert msg["answers"][0]["address"] == "10.22.0.1"
        finally:
            for o in others:
                o.close()
        assert d.proc.proc.poll() is None
    finally:
        d.stop()
        up.close()


# ---------------- 5. churn and shutdown ----------------

def test_churn_then_sigterm(tmp):
    d = Daemon(tmp, "m", T, store=file_store(tmp))
    pool = all_names()
    n_stream = 20000
    seen = bytearray(n_stream)

    def streamer():
        s = Stream(d.sock_path, timeout=60)
        try:
            step = 500
            for base in range(0, n_stream, step):
                s.send(b"".join(
                    query_frame(i, dns_wire(*pool[i % len(pool)], qid=i))
                    for i in range(base, base + step)))
                for i, (ftype, payload) in enumerate(s.take_raw(step)):
                    assert ftype == REPLY
                    rid = int.from_bytes(payload[:4], "little")
                    assert rid == base + i, "stream out of order"
                    assert payload[4 + 3] & 0x0F == 0  # NOERROR
                    seen[rid] = 1
        finally:
            s.close()

    def churner():
        blob = b"".join(
            query_frame(i, dns_wire(*pool[i % len(pool)], qid=i))
            for i in range(200))
        for _ in range(50):
            s = Stream(d.sock_path)
            s.send(blob)
            s.take_raw(3)  # some replies are in, most are not
            s.close()

    keep = [Stream(d.sock_path) for _ in range(T)]  # open at SIGTERM
    try:
        run_threads([streamer, churner])
        assert all(seen), "the stream lost replies"
        for s in keep:
            assert s.ask("h0.foo.com")["rcode"] == "NOERROR"
        proc = d.proc.proc
        t0 = time.time()
        d.proc.sigterm()
        assert proc.wait(timeout=5) == 0
        assert time.time() - t0 < 5
    finally:
        for s in keep:
            s.close()
        d.stop()


# ---------------- 6. info level: pool off ----------------

def test_info_level_serves_without_the_pool(tmp):
    d = Daemon(tmp, "m", T, level="info", store=file_store(tmp))
    try:
        streams = [Stream(d.sock_path) for _ in range(2)]
        try:
            rid = 40
            for s in streams:
                for name, qtype, want in (
                        ("h3.foo.com", "A", 1),
                        ("_x._tcp.s2.foo.com", "SRV", N_MEMBERS),
                        ("H3.foo.com", "A", 1)):
                    for _ in range(2):
                        rid += 1
                        msg = s.ask(name, qtype, rid)
                        assert msg["rcode"] == "NOERROR"
                        assert len(msg["answers"]) == want
        finally:
            for s in streams:
                s.close()
        first, last = 41, rid
        deadline = time.time() + 5
        seen = set()
        while time.time() < deadline and len(seen) < last - first + 1:
            text = d.log_path.read_text()
            for ln in text.splitlines():
                try:
                    rec = json.loads(ln)
                except ValueError:
                    continue
                if rec.get("msg") == "DNS query":
                    seen.add(rec["req_id"])
            if len(seen) < last - first + 1:
                time.sleep(0.02)
        assert seen >= set(range(first, last + 1)), sorted(seen)
        assert "served by a thread pool" not in text
    finally:
        d.stop()
