"""The balancer <-> binderd hop over shared-memory rings (bsock1 types
5-7, native/common/shmpipe.hpp): real daemons on the CPU, a tree of a
few dozen records, warn level so the answer table is in play.

The rings themselves are checked by `make check-shmpipe`; here the point
is the negotiation (and every way of staying on the stream), that the
answers are the same either way, that a 4 KiB ring carries bursts and
replies larger than itself can hold at once, and that a dead backend is
still noticed and leaves nothing behind.
"""
import json
import os
import shutil
import signal
import socket
import struct
import subprocess
import tempfile
import threading
import time
from pathlib import Path

import pytest

from binder_amd.harness import BALANCERD, BinderProcess, free_port
from binder_amd.stubzk import StubZk

import test_balancer_hotpath as hp
import test_serve_threads as sth

BIG_MEMBERS = 7  # SRV reply of the "big" service: just under 512 bytes


def make_tree():
    tree = hp.make_tree()
    tree["big.foo.com"] = {"type": "service",
                           "service": {"srvce": "_x", "proto": "_tcp",
                                       "port": 80, "ttl": 60}}
    for j in range(BIG_MEMBERS):
        tree[f"member-number-{j}.big.foo.com"] = {
            "type": "rr_host", "rr_host": {"address": f"10.6.0.{j + 1}"}}
    return tree


ALL_QUESTIONS = [(f"{h}.foo.com", "A") for h in hp.HOSTS] + [
    ("svc.foo.com", "A"), ("_x._tcp.svc.foo.com", "SRV"),
    ("_x._tcp.big.foo.com", "SRV"), ("nosuch.foo.com", "A"),
    ("m0.svc.foo.com", "A")]


class ShmChain(hp.Chain):
    """hp.Chain with a say in each daemon's environment and flags."""

    def __init__(self, n_backends=1, bal_env=None, be_envs=None,
                 bal_flags=(), be_config=None):
        self.bal_env = bal_env or {}
        self.be_envs = be_envs or [{}] * n_backends
        self.be_config = be_config
        self.bal_flags = list(bal_flags)
        super().__init__(n_backends=n_backends)

    def _start(self, n_backends, host):
        store = self.tmp / "tree.json"
        store.write_text(json.dumps(make_tree()))
        self.sockdir = self.tmp / "socks"
        self.sockdir.mkdir()
        for i in range(n_backends):
            b = BinderProcess(store=f"file:{store}", workdir=self.tmp,
                              log_level="warn",
                              balancer_socket=str(self.sockdir / f"b{i}"),
                              log_path=str(self.tmp / f"b{i}.log"),
                              config=self.be_config)
            b.env.update(self.be_envs[i])
            b.start()
            self.backends.append(b)
        for b in self.backends:
            b.wait_ready("h109.foo.com", timeout=20)
        self.port = free_port()
        self.stats = self.tmp / "stats.sock"
        cmd = [str(BALANCERD), "-p", str(self.port), "-H", host,
               "-s", str(self.sockdir), "-S", str(self.stats),
               "-r", "100"] + self.bal_flags
        self.bal = subprocess.Popen(
            cmd, env=dict(os.environ, LOG_LEVEL="warn", **self.bal_env),
            stdout=open(self.tmp / "bal.log", "ab"),
            stderr=subprocess.STDOUT)
        deadline = time.time() + 20
        while True:
            try:
                st = hp.balstat(self.stats)
                if sum(1 for b in st["backends"] if b["ok"]) == n_backends:
                    break
            except (OSError, ValueError):
                pass
            assert time.time() < deadline, "balancer never saw its backends"
            time.sleep(0.05)
        with self.client() as s:
            got = self.ask(s, range(1), timeout=10, retry=True)
            assert 0 in got, "balancer never forwarded"
            self.drain(s, got, 0.3)

    def transports(self):
        return {Path(b["path"]).name: b["transport"]
                for b in hp.balstat(self.stats)["backends"]}

    def wait_transport(self, want, timeout=5):
        """The switch takes one round trip after the connect."""
        deadline = time.time() + timeout
        while True:
            got = self.transports()
            if got == want or time.time() > deadline:
                return got
            time.sleep(0.05)

    def resolve(self, s, name, qtype, qid):
        wire = self.native.encode_message(
            {"id": qid, "questions": [{"name": name, "type": qtype}]})
        for _ in range(5):
            s.send(wire)
            s.settimeout(1)
            try:
                while True:
                    data = s.recv(65535)
                    self.received += 1
                    m = self.native.decode_message(data)
                    if m["id"] == qid:
                        return m, len(data)
            except socket.timeout:
                continue
        raise AssertionError(f"no answer for {name} {qtype}")


def view(m):
    """What must not depend on the transport: rcode, counts, and the
    records as sets (SRV members are served in a shuffled order)."""
    def recs(section):
        return sorted(json.dumps(r, sort_keys=True) for r in m[section])
    return (m["rcode"], len(m["answers"]), len(m["additionals"]),
            recs("answers"), recs("additionals"))


@pytest.fixture(scope="module")
def chain_shm():
    c = ShmChain()
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain_stream():
    """balancer switched off by its flag, binderd left at its default"""
    c = ShmChain(bal_flags=["-M", "0"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain_small():
    """4 KiB rings: wrap and full within a handful of queries"""
    c = ShmChain(bal_env={"BINDER_BAL_SHM_RING": "4096"})
    yield c
    c.close()


def test_transport_is_shm_when_both_allow(chain_shm):
    assert chain_shm.wait_transport({"b0": "shm"}) == {"b0": "shm"}


def test_stream_when_balancer_is_off(chain_stream):
    ids = range(100, 200)
    with chain_stream.client() as s:
        hp.check_replies(chain_stream.ask(s, ids), ids)
    assert chain_stream.transports() == {"b0": "stream"}
    st = hp.balstat(chain_stream.stats)
    assert st["shm_doorbells"] == 0 and st["shm_drains"] == 0, st


def test_same_replies_shm_on_and_off(chain_shm, chain_stream):
    assert chain_shm.wait_transport({"b0": "shm"}) == {"b0": "shm"}
    assert chain_stream.transports() == {"b0": "stream"}
    with chain_shm.client() as a, chain_stream.client() as b:
        for k, (name, qtype) in enumerate(ALL_QUESTIONS):
            for rnd in range(2):  # second round: from the answer table
                ma, _ = chain_shm.resolve(a, name, qtype, 300 + 2 * k + rnd)
                mb, _ = chain_stream.resolve(b, name, qtype,
                                             300 + 2 * k + rnd)
                assert view(ma) == view(mb), (name, qtype, ma, mb)
        # the comparison was of answers, not of two ways of failing
        m, _ = chain_shm.resolve(a, "h5.foo.com", "A", 999)
        assert m["rcode"] == "NOERROR" and \
            m["answers"][0]["address"] == hp.addr_of("h5"), m
        m, _ = chain_shm.resolve(a, "nosuch.foo.com", "A", 998)
        assert m["rcode"] != "NOERROR", m


def test_stream_when_binderd_is_off():
    """Two backends behind one balancer, one of them switched off by its
    environment: each connection settles on its own transport, and both
    serve."""
    c = ShmChain(n_backends=2, be_envs=[{}, {"BINDER_BAL_SHM": "0"}])
    try:
        want = {"b0": "shm", "b1": "stream"}
        assert c.wait_transport(want) == want
        # sources 127.0.0.x pin to the less loaded backend in turn
        for k in range(2):
            with socket.socket(socket.AF_INET, socket.SOCK_DGRAM) as s:
                s.bind((f"127.0.0.{k + 2}", 0))
                s.connect(("127.0.0.1", c.port))
                ids = range(400 + 100 * k, 500 + 100 * k)
                hp.check_replies(c.ask(s, ids), ids)
        st = hp.balstat(c.stats)
        assert all(b["replies"] >= 100 for b in st["backends"]), st
        assert c.transports() == want
    finally:
        c.close()


@pytest.mark.parametrize("kw,want", [
    # binderd's config key alone
    (dict(be_config={"balancerShm": False}), "stream"),
    # binderd's environment wins over its config key
    (dict(be_config={"balancerShm": False},
          be_envs=[{"BINDER_BAL_SHM": "1"}]), "shm"),
    (dict(be_config={"balancerShm": True},
          be_envs=[{"BINDER_BAL_SHM": "0"}]), "stream"),
    # the balancer takes its default from the environment ...
    (dict(bal_env={"BINDER_BAL_SHM": "0"}), "stream"),
    # ... and its flag wins over it, both ways
    (dict(bal_env={"BINDER_BAL_SHM": "0"}, bal_flags=["-M", "1"]), "shm"),
    (dict(bal_env={"BINDER_BAL_SHM": "1"}, bal_flags=["-M", "0"]),
     "stream"),
], ids=["binderd-config-off", "binderd-env-on-over-config",
        "binderd-env-off-over-config", "balancer-env-off",
        "balancer-flag-on-over-env", "balancer-flag-off-over-env"])
def test_every_switch_and_its_precedence(kw, want):
    c = ShmChain(**kw)
    try:
        assert c.wait_transport({"b0": want},
                                timeout=5 if want == "shm" else 0.5) == \
            {"b0": want}
        ids = range(800, 900)
        with c.client() as s:
            hp.check_replies(c.ask(s, ids), ids)
        assert c.transports() == {"b0": want}
    finally:
        c.close()


def test_stream_when_peer_ignores_the_offer():
    """A bsock1 peer that knows types 1-4 only: it skips the offer, goes
    on answering PINGs on the stream, and the balancer keeps the
    connection there."""
    tmp = hp.short_tmpdir()
    sockdir = tmp / "socks"
    sockdir.mkdir()
    lsock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    lsock.bind(str(sockdir / "b0"))
    lsock.listen(4)
    seen = []  # frame types, in order
    stop = threading.Event()

    def peer():
        lsock.settimeout(0.2)
        conn = None
        while not stop.is_set() and conn is None:
            try:
                conn, _ = lsock.accept()
            except socket.timeout:
                pass
        if conn is None:
            return
        conn.settimeout(0.2)
        buf = b""
        while not stop.is_set():
            try:
                part = conn.recv(65536)
            except socket.timeout:
                continue
            except OSError:
                break
            if not part:
                break
            buf += part
            while len(buf) >= 6:
                plen = struct.unpack("<I", buf[2:6])[0]
                if len(buf) < 6 + plen:
                    break
                assert buf[0] == 0xB5
                seen.append(buf[1])
                if buf[1] == 3:  # PING -> PONG
                    conn.sendall(bytes([0xB5, 4, 0, 0, 0, 0]))
                buf = buf[6 + plen:]
        conn.close()

    t = threading.Thread(target=peer, daemon=True)
    t.start()
    stats = tmp / "stats.sock"
    bal = subprocess.Popen(
        [str(BALANCERD), "-p", str(free_port()), "-H", "127.0.0.1",
         "-s", str(sockdir), "-S", str(stats), "-r", "100"],
        env=dict(os.environ, LOG_LEVEL="warn"),
        stdout=open(tmp / "bal.log", "ab"), stderr=subprocess.STDOUT)
    try:
        deadline = time.time() + 10
        while not (seen[:1] == [5] and 3 in seen):
            assert time.time() < deadline, seen
            time.sleep(0.05)
        st = hp.balstat(stats)
        assert [b["transport"] for b in st["backends"]] == ["stream"], st
        assert st["backends"][0]["ok"], st
        assert 7 not in seen, seen  # no SHM_GO without a SHM_OK
        assert bal.poll() is None
    finally:
        stop.set()
        bal.terminate()
        bal.wait(timeout=5)
        t.join()
        lsock.close()
        shutil.rmtree(tmp, ignore_errors=True)


def test_small_ring_burst_larger_than_the_ring(chain_small):
    """600 queries (some 36 KB of frames, 60 KB of replies) through
    4 KiB rings: partial accepts, full rings and the doorbell for room,
    in both directions."""
    assert chain_small.wait_transport({"b0": "shm"}) == {"b0": "shm"}
    ids = range(1000, 1600)
    with chain_small.client() as s:
        hp.check_replies(chain_small.ask(s, ids), ids)


def test_small_ring_large_reply_crosses_the_wrap(chain_small):
    """Replies near 512 bytes, forty in a row: 4 KiB holds eight, so the
    frames cross the ring's end several times, and each must arrive
    whole."""
    assert chain_small.wait_transport({"b0": "shm"}) == {"b0": "shm"}
    with chain_small.client() as s:
        sizes = set()
        for k in range(40):
            m, size = chain_small.resolve(s, "_x._tcp.big.foo.com", "SRV",
                                          2000 + k)
            sizes.add(size)
            assert m["rcode"] == "NOERROR", m
            assert len(m["answers"]) == BIG_MEMBERS, m
            assert sorted(a["address"] for a in m["additionals"]) == \
                sorted(f"10.6.0.{j + 1}" for j in range(BIG_MEMBERS)), m
    assert all(400 <= n <= 512 for n in sizes), sizes
    # and pipelined, so that several are in the ring at once
    big = chain_small.native.encode_message(
        {"id": 1, "questions": [{"name": "_x._tcp.big.foo.com",
                                 "type": "SRV"}]})
    with chain_small.client() as s:
        for k in range(60):
            s.send(struct.pack(">H", 3000 + k) + big[2:])
        got = {}
        deadline = time.time() + 5
        while len(got) < 60 and time.time() < deadline:
            chain_small.drain(s, got, 0.25)
    assert sorted(got) == list(range(3000, 3060))
    for replies in got.values():
        assert len(replies) == 1
        assert len(replies[0]["answers"]) == BIG_MEMBERS
        assert len(replies[0]["additionals"]) == BIG_MEMBERS


def test_small_ring_tcp_query(chain_small):
    assert chain_small.wait_transport({"b0": "shm"}) == {"b0": "shm"}
    wire = chain_small.native.encode_message(
        {"id": 77, "questions": [{"name": "h7.foo.com", "type": "A"}]})
    with socket.create_connection(("127.0.0.1", chain_small.port),
                                  timeout=5) as s:
        s.sendall(struct.pack(">H", len(wire)) + wire)
        buf = b""
        while len(buf) < 2 or len(buf) < 2 + struct.unpack(">H", buf[:2])[0]:
            part = s.recv(4096)
            assert part, "connection closed before the reply"
            buf += part
    m = chain_small.native.decode_message(buf[2:])
    assert m["id"] == 77 and m["rcode"] == "NOERROR", m
    assert [a["address"] for a in m["answers"]] == [hp.addr_of("h7")], m


def test_conservation_with_shm(chain_shm):
    """The identity of test_balancer_hotpath.py, over rings."""
    assert chain_shm.wait_transport({"b0": "shm"}) == {"b0": "shm"}
    ids = range(4000, 4600)
    with chain_shm.client() as s:
        hp.check_replies(chain_shm.ask(s, ids), ids)
    st = hp.balstat(chain_shm.stats)
    print({k: st[k] for k in ("udp_queries", "udp_replies", "drops",
                              "reply_runs", "reply_run_segments",
                              "reply_singles", "backend_reads",
                              "udp_rx_msgs", "shm_doorbells",
                              "shm_drains")}, "received",
          chain_shm.received)
    assert st["reply_run_segments"] + st["reply_singles"] == \
        st["udp_replies"], st
    assert st["udp_replies"] == chain_shm.received, (st, chain_shm.received)
    assert st["drops"] == 0, st
    # every reply of this chain came through the ring but the first few
    # (the readiness probe may have beaten the switch)
    assert 0 < st["shm_drains"] <= st["backend_reads"], st
    assert st["shm_doorbells"] > 0, st
    for k in ("shm_doorbells", "shm_drains"):
        assert st["per_worker"][0][k] == st[k], k


def fd_census(pid):
    kinds = {"eventfd": 0, "memfd": 0, "total": 0}
    for name in os.listdir(f"/proc/{pid}/fd"):
        try:
            target = os.readlink(f"/proc/{pid}/fd/{name}")
        except OSError:
            continue  # closed meanwhile
        kinds["total"] += 1
        if "eventfd" in target:
            kinds["eventfd"] += 1
        if "memfd:" in target:
            kinds["memfd"] += 1
    with open(f"/proc/{pid}/maps") as f:
        kinds["maps"] = sum(1 for line in f if "bsock1-rings" in line)
    return kinds


def test_backend_killed_between_bursts_leaves_nothing():
    """kill -9 of the serving backend: the balancer notices through the
    socket, traffic moves to the other backend, and the dead
    connection's region and doorbells are gone."""
    c = ShmChain(n_backends=2)
    try:
        want = {"b0": "shm", "b1": "shm"}
        assert c.wait_transport(want) == want
        with c.client() as s:
            ids = range(6000, 6200)
            hp.check_replies(c.ask(s, ids), ids)
            st = hp.balstat(c.stats)
            serving = [b for b in st["backends"] if b["queries"] > 0]
            assert len(serving) == 1, st["backends"]
            before = fd_census(c.bal.pid)
            assert before["maps"] == 2 and before["memfd"] == 0, before
            victim = next(b for b in c.backends
                          if serving[0]["path"] in b.cmd)
            victim.proc.send_signal(signal.SIGKILL)
            victim.proc.wait(timeout=5)
            first = c.ask(s, range(6500, 6501), timeout=10, retry=True)
            assert 6500 in first
            ids = range(7000, 7200)
            hp.check_replies(c.ask(s, ids), ids)
        st = hp.balstat(c.stats)
        survivor = next(b for b in st["backends"]
                        if b["path"] != serving[0]["path"])
        assert survivor["replies"] >= 201, st["backends"]
        assert survivor["transport"] == "shm", st["backends"]
        # one socket and two doorbells fewer, one region unmapped (the
        # balancer keeps trying the dead socket's path, so a connect
        # attempt may be in flight at the instant of a look)
        expect = dict(before, total=before["total"] - 3,
                      eventfd=before["eventfd"] - 2, maps=1)
        deadline = time.time() + 3
        while True:
            after = fd_census(c.bal.pid)
            if after == expect or time.time() > deadline:
                break
            time.sleep(0.05)
        assert after == expect, (before, after)
    finally:
        c.close()


def udp_ask(native, s, name, qtype, qid):
    wire = native.encode_message(
        {"id": qid & 0xFFFF, "questions": [{"name": name, "type": qtype}]})
    for _ in range(5):
        s.send(wire)
        s.settimeout(2)
        try:
            while True:
                m = native.decode_message(s.recv(65535))
                if m["id"] == qid & 0xFFFF:
                    return m
        except socket.timeout:
            continue
    raise AssertionError(f"no answer for {name}")


def test_invalidation_reaches_every_thread_over_rings():
    """The check of test_serve_threads.py with the connections on rings:
    three balancers, so three connections on three serving threads of
    one binderd. After a record changes, no connection serves the old
    answer once another has served the new one (an invalidation posted
    before bytes were taken from a ring applies before they are
    answered)."""
    tmp = Path(tempfile.mkdtemp(prefix="st-"))
    (tmp / "stats").mkdir()
    zk = StubZk().start()
    d = None
    bals, socks = [], []
    native = hp.require_native()
    try:
        for domain, rec in sth.tree_records().items():
            path = sth.zk_path(domain)
            if rec is None:
                zk.mkdirp(path)
            else:
                zk.put(path, json.dumps(rec).encode())
        d = sth.Daemon(tmp, "m", sth.T, store="zk", zk_host="127.0.0.1",
                       zk_port=zk.port)
        d.proc.wait_ready(f"m{sth.N_MEMBERS - 1}.s{sth.N_SVCS - 1}.foo.com",
                          timeout=30)
        d.proc.wait_ready(f"h{sth.N_HOSTS - 1}.foo.com", timeout=30)
        # started one after the other: accepted round-robin, so the
        # three connections belong to three threads
        for k in range(sth.T):
            port = free_port()
            stats = tmp / "stats" / f"s{k}"
            bals.append(subprocess.Popen(
                [str(BALANCERD), "-p", str(port), "-H", "127.0.0.1",
                 "-s", str(tmp), "-S", str(stats), "-r", "100"],
                env=dict(os.environ, LOG_LEVEL="warn"),
                stdout=open(tmp / f"bal{k}.log", "ab"),
                stderr=subprocess.STDOUT))
            deadline = time.time() + 10
            while True:
                try:
                    st = hp.balstat(stats)
                    if [b["transport"] for b in st["backends"]] == ["shm"]:
                        break
                except (OSError, ValueError):
                    pass
                assert time.time() < deadline, "never switched to rings"
                time.sleep(0.05)
            s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
            s.connect(("127.0.0.1", port))
            assert udp_ask(native, s, "h0.foo.com", "A", 1)["rcode"] == \
                "NOERROR"
            socks.append(s)
        a, b, c = socks
        srv = "_x._tcp.s0.foo.com"
        rid = 10
        for rnd in range(30):
            addr = f"10.4.{rnd}.7"
            for s in socks:  # memoised on all three threads
                for _ in range(2):
                    udp_ask(native, s, "h1.foo.com", "A", rid)
            zk.put("/com/foo/h1", json.dumps(sth.host(addr)).encode())
            deadline = time.time() + 10
            while sth.addresses(
                    udp_ask(native, a, "h1.foo.com", "A", rid)) != [addr]:
                assert time.time() < deadline, "A never saw the new host"
            rid += 1
            for s in (b, c):
                assert sth.addresses(
                    udp_ask(native, s, "h1.foo.com", "A", rid)) == [addr], \
                    f"round {rnd}: old answer after the new one was seen"

            maddr = f"10.5.{rnd}.9"
            for s in socks:
                for _ in range(2):
                    udp_ask(native, s, srv, "SRV", rid)
            zk.put("/com/foo/s0/m0", json.dumps(sth.member(maddr)).encode())
            deadline = time.time() + 10
            while maddr not in sth.extra_addresses(
                    udp_ask(native, a, srv, "SRV", rid)):
                assert time.time() < deadline, "A never saw the member"
            rid += 1
            for s in (b, c):
                assert maddr in sth.extra_addresses(
                    udp_ask(native, s, srv, "SRV", rid)), \
                    f"round {rnd}: old SRV after the new one was seen"
    finally:
        for s in socks:
            s.close()
        for p in bals:
            p.terminate()
        for p in bals:
            p.wait(timeout=5)
        try:
            if d is not None:
                d.stop()
        finally:
            zk.stop()
            shutil.rmtree(tmp, ignore_errors=True)
