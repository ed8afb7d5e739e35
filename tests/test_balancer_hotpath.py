"""The balancer's UDP hot path end to end: reply runs gathered over a
whole backend read, one route per datagram, receive buffers parsed in
place. A real balancer in front of one binderd on a file store.

The grouping rules themselves are checked by `make check-replyruns`;
here the point is that every reply reaches the socket that asked, with
the answer for its own name, whatever the mix of sizes, sockets and
address families - and that the stats socket accounts for all of them.
"""
import json
import os
import shutil
import signal
import socket
import struct
import subprocess
import tempfile
import time
from pathlib import Path

import pytest

from binder_amd import require_native
from binder_amd.harness import BALANCERD, BinderProcess, free_port

UDP_SEGMENT = 103

# names of three lengths, ten hosts each, plus one service of three
HOSTS = ([f"h{i}" for i in range(10)] +
         [f"h{i}" for i in range(10, 20)] +
         [f"h{i}" for i in range(100, 110)])
MEMBERS = 3


def addr_of(host):
    i = int(host[1:])
    return f"10.1.{i // 250}.{i % 250 + 1}"


def make_tree():
    tree = {"foo.com": None,
            "svc.foo.com": {"type": "service",
                            "service": {"srvce": "_x", "proto": "_tcp",
                                        "port": 80, "ttl": 60}}}
    for h in HOSTS:
        tree[f"{h}.foo.com"] = {"type": "host",
                                "host": {"address": addr_of(h)}}
    for j in range(MEMBERS):
        tree[f"m{j}.svc.foo.com"] = {
            "type": "rr_host", "rr_host": {"address": f"10.4.0.{j + 1}"}}
    return tree


# (name, type) by position: three A lengths and the SRV interleaved
QUESTIONS = [(f"{h}.foo.com", "A") for h in HOSTS] + \
    [("_x._tcp.svc.foo.com", "SRV")] * 6


def question(i):
    return QUESTIONS[(i * 7) % len(QUESTIONS)]


def balstat(path):
    with socket.socket(socket.AF_UNIX) as s:
        s.settimeout(2)
        s.connect(str(path))
        buf = b""
        while True:
            part = s.recv(1 << 20)
            if not part:
                break
            buf += part
    return json.loads(buf.decode())


def short_tmpdir():
    base = tempfile.gettempdir()
    if len(base) > 48 and os.access("/tmp", os.W_OK | os.X_OK):
        base = "/tmp"
    return Path(tempfile.mkdtemp(prefix="bt-", dir=base))


class Chain:
    """n binderd on one file store behind a one-worker balancer."""

    def __init__(self, n_backends=1, host="127.0.0.1"):
        self.native = require_native()
        self.tmp = short_tmpdir()
        self.received = 0  # UDP replies the tests took off their sockets
        self.backends = []
        self.bal = None
        try:
            self._start(n_backends, host)
        except BaseException:
            self.close()
            raise

    def _start(self, n_backends, host):
        store = self.tmp / "tree.json"
        store.write_text(json.dumps(make_tree()))
        sockdir = self.tmp / "socks"
        sockdir.mkdir()
        for i in range(n_backends):
            b = BinderProcess(store=f"file:{store}", workdir=self.tmp,
                              log_level="warn",
                              balancer_socket=str(sockdir / f"b{i}"),
                              log_path=str(self.tmp / f"b{i}.log"))
            b.start()
            self.backends.append(b)
        for b in self.backends:
            b.wait_ready("h109.foo.com", timeout=20)
        self.port = free_port()
        self.stats = self.tmp / "stats.sock"
        cmd = [str(BALANCERD), "-p", str(self.port), "-s", str(sockdir),
               "-S", str(self.stats), "-r", "100"]
        if host:
            cmd += ["-H", host]
        self.bal = subprocess.Popen(
            cmd, env=dict(os.environ, LOG_LEVEL="warn"),
            stdout=open(self.tmp / "bal.log", "ab"),
            stderr=subprocess.STDOUT)
        deadline = time.time() + 20
        while True:
            try:
                st = balstat(self.stats)
                if sum(1 for b in st["backends"] if b["ok"]) == n_backends:
                    break
            except (OSError, ValueError):
                pass
            assert time.time() < deadline, "balancer never saw its backends"
            time.sleep(0.05)
        # the chain is up once a query gets through; every reply the
        # balancer sends from here on is counted in self.received
        with self.client() as s:
            got = self.ask(s, range(1), timeout=10, retry=True)
            assert 0 in got, "balancer never forwarded"
            self.drain(s, got, 0.3)  # a re-asked probe's second answer

    def close(self):
        if self.bal is not None:
            self.bal.terminate()
            try:
                self.bal.wait(timeout=5)
            except subprocess.TimeoutExpired:
                self.bal.kill()
        for b in self.backends:
            b.stop()
        shutil.rmtree(self.tmp, ignore_errors=True)

    def client(self, family=socket.AF_INET):
        s = socket.socket(family, socket.SOCK_DGRAM)
        # room for a whole burst of replies even if this process is not
        # scheduled while they arrive (the default holds ~200 datagrams)
        s.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 8 << 20)
        s.connect(("::1" if family == socket.AF_INET6 else "127.0.0.1",
                   self.port))
        return s

    def wire(self, qid):
        name, qtype = question(qid)
        return self.native.encode_message(
            {"id": qid, "questions": [{"name": name, "type": qtype}]})

    def drain(self, s, got, wait):
        """Take what has arrived (waiting up to `wait` s for the first
        datagram) into got: id -> list of decoded replies."""
        first = True
        while True:
            s.settimeout(wait if first else 0)
            try:
                data = s.recv(65535)
            except (BlockingIOError, socket.timeout):
                return
            first = False
            self.received += 1
            m = self.native.decode_message(data)
            assert m is not None, data
            got.setdefault(m["id"], []).append(m)

    def ask(self, s, ids, timeout=5.0, retry=False):
        """Send one query per id without waiting for answers in between
        (arrivals are only taken off the socket every 50 sends, so its
        receive buffer cannot overflow), then collect. Returns id ->
        list of replies."""
        ids = list(ids)
        got = {}
        for k, qid in enumerate(ids):
            s.send(self.wire(qid))
            if k % 50 == 49:
                self.drain(s, got, 0)
        deadline = time.time() + timeout
        while len(got) < len(ids) and time.time() < deadline:
            self.drain(s, got, 0.25)
            if retry and not got:
                s.send(self.wire(ids[0]))
        return got


def check_replies(got, ids):
    """Every id exactly once, each with the answer for its own name."""
    ids = list(ids)
    missing = [i for i in ids if i not in got]
    assert not missing, f"{len(missing)} of {len(ids)} unanswered"
    assert set(got) == set(ids), sorted(set(got) - set(ids))[:10]
    for qid in ids:
        assert len(got[qid]) == 1, (qid, len(got[qid]))
        m = got[qid][0]
        name, qtype = question(qid)
        assert m["rcode"] == "NOERROR", m
        assert m["questions"][0]["name"] == name, (qid, m)
        if qtype == "A":
            assert [a["address"] for a in m["answers"]] == \
                [addr_of(name.split(".")[0])], (qid, m)
        else:
            assert len(m["answers"]) == MEMBERS, (qid, m)
            assert sorted(a["address"] for a in m["additionals"]) == \
                [f"10.4.0.{j + 1}" for j in range(MEMBERS)], (qid, m)


@pytest.fixture(scope="module")
def chain():
    c = Chain()
    yield c
    c.close()


def test_mixed_sizes_one_socket(chain):
    """600 queries in flight from one socket over three name lengths
    plus SRV: one destination, four reply sizes interleaved."""
    ids = range(1000, 1600)
    with chain.client() as s:
        got = chain.ask(s, ids)
    check_replies(got, ids)


def test_eight_sockets_interleaved(chain):
    """Eight sockets, 100 ids each, sends interleaved across them: each
    socket receives its own ids and nothing else."""
    socks = [chain.client() for _ in range(8)]
    try:
        mine = [range(2000 + 100 * k, 2100 + 100 * k) for k in range(8)]
        got = [{} for _ in socks]
        for j in range(100):
            for k, s in enumerate(socks):
                s.send(chain.wire(mine[k][j]))
            if j % 25 == 24:
                for k, s in enumerate(socks):
                    chain.drain(s, got[k], 0)
        deadline = time.time() + 5
        for k, s in enumerate(socks):
            while len(got[k]) < 100 and time.time() < deadline:
                chain.drain(s, got[k], 0.25)
        for k in range(8):
            check_replies(got[k], mine[k])
    finally:
        for s in socks:
            s.close()


def gso_send(s, wires):
    seg = len(wires[0])
    assert all(len(w) == seg for w in wires)
    try:
        s.sendmsg([b"".join(wires)],
                  [(socket.IPPROTO_UDP, UDP_SEGMENT,
                    struct.pack("H", seg))])
    except OSError:
        pytest.skip("kernel without UDP_SEGMENT")


def test_gso_ingress_two_sockets(chain):
    """A UDP_SEGMENT super-packet of 8 queries from socket A, then one
    from socket B: 16 answers, each on the socket that asked (the route
    is taken once per datagram, the reply address per segment)."""
    # equal-size queries: ids whose names all have the same length
    same_len = [i for i in range(3000, 3400)
                if question(i)[1] == "A" and len(question(i)[0]) == 11]
    ids_a, ids_b = same_len[:8], same_len[8:16]
    with chain.client() as a, chain.client() as b:
        gso_send(a, [chain.wire(i) for i in ids_a])
        gso_send(b, [chain.wire(i) for i in ids_b])
        got_a, got_b = {}, {}
        deadline = time.time() + 5
        while (len(got_a) < 8 or len(got_b) < 8) and \
                time.time() < deadline:
            chain.drain(a, got_a, 0.1)
            chain.drain(b, got_b, 0.1)
    check_replies(got_a, ids_a)
    check_replies(got_b, ids_b)


def test_stats_conservation(chain):
    """Every UDP reply is counted once, as a run segment or a single;
    the total is what the tests took off their sockets."""
    ids = range(4000, 4300)
    with chain.client() as s:
        check_replies(chain.ask(s, ids), ids)
    st = balstat(chain.stats)
    print({k: st[k] for k in ("udp_queries", "udp_replies", "drops",
                              "reply_runs", "reply_run_segments",
                              "reply_singles", "backend_reads",
                              "udp_rx_msgs")}, "received", chain.received)
    assert st["reply_run_segments"] + st["reply_singles"] == \
        st["udp_replies"], st
    assert st["udp_replies"] == chain.received, (st, chain.received)
    assert st["drops"] == 0, st
    assert st["reply_runs"] <= st["reply_run_segments"] // 2
    assert st["backend_reads"] > 0
    assert 0 < st["udp_rx_msgs"] <= st["udp_queries"]
    assert len(st["per_worker"]) == st["workers"] == 1
    for k in ("reply_runs", "reply_run_segments", "reply_singles",
              "backend_reads", "udp_rx_msgs", "udp_replies"):
        assert st["per_worker"][0][k] == st[k], k


def test_ipv6_beside_ipv4():
    """A ::1 client and a 127.0.0.1 client through one dual-stack
    balancer, queries interleaved: both families' reply addresses are
    rebuilt correctly."""
    try:
        with socket.socket(socket.AF_INET6, socket.SOCK_DGRAM) as probe:
            probe.bind(("::1", 0))
    except OSError:
        pytest.skip("no IPv6 loopback")
    c = Chain(host="")
    try:
        with c.client(socket.AF_INET6) as s6, c.client() as s4:
            ids6, ids4 = range(5000, 5100), range(5100, 5200)
            got6, got4 = {}, {}
            for q6, q4 in zip(ids6, ids4):
                s6.send(c.wire(q6))
                s4.send(c.wire(q4))
            deadline = time.time() + 5
            while (len(got6) < 100 or len(got4) < 100) and \
                    time.time() < deadline:
                c.drain(s6, got6, 0.1)
                c.drain(s4, got4, 0.1)
        check_replies(got6, ids6)
        check_replies(got4, ids4)
        st = balstat(c.stats)
        assert st["reply_run_segments"] + st["reply_singles"] == \
            st["udp_replies"] == c.received, (st, c.received)
    finally:
        c.close()


def test_backend_kill_reroutes_same_source():
    """Two backends; the one serving this source is killed between two
    bursts. The next queries from the same source reach the survivor:
    the per-datagram route cache does not outlive its backend."""
    c = Chain(n_backends=2)
    try:
        with c.client() as s:
            ids = range(6000, 6200)
            check_replies(c.ask(s, ids), ids)
            st = balstat(c.stats)
            serving = [b for b in st["backends"] if b["queries"] > 0]
            assert len(serving) == 1, st["backends"]
            victim = next(b for b in c.backends
                          if serving[0]["path"] in b.cmd)
            victim.proc.send_signal(signal.SIGKILL)
            victim.proc.wait(timeout=5)
            # the balancer sees the hangup on its own; a query sent
            # before it does is lost with the backend, so ask until one
            # is answered, then the burst must come back whole
            first = c.ask(s, range(6500, 6501), timeout=10, retry=True)
            assert 6500 in first
            ids = range(7000, 7200)
            check_replies(c.ask(s, ids), ids)
        st = balstat(c.stats)
        by_path = {b["path"]: b for b in st["backends"]}
        survivor = next(b for p, b in by_path.items()
                        if p != serving[0]["path"])
        assert survivor["replies"] >= 201, st["backends"]
        assert st["reply_run_segments"] + st["reply_singles"] == \
            st["udp_replies"], st
    finally:
        c.close()
