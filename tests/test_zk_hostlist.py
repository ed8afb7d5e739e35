"""ZooKeeper server list: connect-string parsing, failover rotation and
its pacing, the connect deadline, and what shows which server a binderd
is on (log fields, /metrics).

binderd runs with the list in the given order (ZK_SHUFFLE=0) so that
"first" and "second" mean something. Fake endpoints are plain sockets
speaking bytes built with tests/zkwire.py; registries are StubZk.
"""
import json
import os
import selectors
import socket
import struct
import subprocess
import sys
import threading
import time

import pytest

from zkwire import be32, be64, connect_request, jstr, packet, read_packet

from binder_amd import REPO_ROOT, _native, zkclient
from binder_amd.harness import BinderProcess, free_port
from binder_amd.stubzk import StubZk

ZKTOOL = REPO_ROOT / "bin" / "zktool"
RENDER = REPO_ROOT / "deploy" / "render-config.py"
GOLDEN = REPO_ROOT / "tests" / "golden"


def host(addr):
    return json.dumps({"type": "host", "host": {"address": addr}}).encode()


def stub_with(records, port=0):
    zk = StubZk(port=port).start()
    zk.mkdirp("/com/foo")
    for name, addr in records.items():
        zk.put(f"/com/foo/{name}", host(addr))
    return zk


def closed_port():
    """A port nothing listens on: connections are refused."""
    return free_port()


def binderd(tmp_path, zk_host=None, config=None, log_level="info",
            shuffle="0"):
    b = BinderProcess(store="zk", zk_host=zk_host, workdir=tmp_path,
                      config=config, log_level=log_level,
                      log_path=str(tmp_path / "binderd.log"))
    # nothing of the caller's environment: the harness sets ZK_HOST
    # itself when zk_host is given
    b.env.pop("ZK_PORT", None)
    b.env.pop("ZK_SHUFFLE", None)
    if zk_host is None:
        b.env.pop("ZK_HOST", None)
    if shuffle is not None:
        b.env["ZK_SHUFFLE"] = shuffle
    return b


def log_lines(b):
    out = []
    with open(b.log_path, "rb") as f:
        for raw in f:
            try:
                out.append(json.loads(raw))
            except ValueError:
                pass
    return out


def wait_log(b, pred, timeout=10.0):
    """The first log line for which pred(line) holds."""
    deadline = time.time() + timeout
    while True:
        for line in log_lines(b):
            if pred(line):
                return line
        if time.time() > deadline:
            raise AssertionError(
                "no such log line; log:\n" +
                "\n".join(json.dumps(ln) for ln in log_lines(b)[-30:]))
        time.sleep(0.02)


def wait_address(b, name, addr, timeout=10.0):
    deadline = time.time() + timeout
    got = None
    while time.time() < deadline:
        r = b.dig(name)
        got = [a["address"] for a in r.answers] if r.answers else r.status
        if got == [addr]:
            return
        time.sleep(0.02)
    raise AssertionError(f"{name} never became {addr}: last {got}")


def metric(b, name):
    return [ln for ln in b.metrics().splitlines()
            if ln.startswith(name + "{") or ln.startswith(name + " ")]


def session_on(server):
    return lambda ln: ln.get("msg") == "ZK session established" and \
        ln.get("server") == server


# --- 1. parser table --------------------------------------------------

# text -> the list with default port 2181, the list with default port 7
ACCEPTED = {
    "a": ([("a", 2181)], [("a", 7)]),
    "a:1": ([("a", 1)], [("a", 1)]),
    "a:65535": ([("a", 65535)], [("a", 65535)]),
    "10.0.0.1:2181, b ,c:3": (
        [("10.0.0.1", 2181), ("b", 2181), ("c", 3)],
        [("10.0.0.1", 2181), ("b", 7), ("c", 3)]),
    "a,a:2181,a": ([("a", 2181)], [("a", 7), ("a", 2181)]),
}
REJECTED = {
    "": '""', ",": '""', "a,,b": '""', "a:": '"a:"', "a:0": '"a:0"',
    "a:65536": '"a:65536"', "a:x": '"a:x"', "a:1:2": '"a:1:2"',
    "[::1]:2181": '"[::1]:2181"', "a:2181/chroot": '"a:2181/chroot"',
    "a b": '"a b"',
}


@pytest.mark.parametrize("text", list(ACCEPTED))
def test_parsers_accept(text):
    want, want7 = ACCEPTED[text]
    assert [tuple(e) for e in _native.parse_zk_hosts(text, 2181)] == want
    assert zkclient.parse_hosts(text, 2181) == want
    # the default port reaches exactly the entries that name none
    assert [tuple(e) for e in _native.parse_zk_hosts(text, 7)] == want7
    assert zkclient.parse_hosts(text, 7) == want7


@pytest.mark.parametrize("text", list(REJECTED))
def test_parsers_reject(text):
    with pytest.raises(ValueError) as native_err:
        _native.parse_zk_hosts(text, 2181)
    with pytest.raises(ValueError) as py_err:
        zkclient.parse_hosts(text, 2181)
    # the message names the offending entry, and is the same message
    assert REJECTED[text] in str(native_err.value)
    assert str(py_err.value) == str(native_err.value)


def test_parsers_say_what_is_unsupported():
    with pytest.raises(ValueError, match="chroot"):
        _native.parse_zk_hosts("a:2181/chroot", 2181)
    with pytest.raises(ValueError, match="IPv6"):
        _native.parse_zk_hosts("[::1]:2181", 2181)


# --- 2. dead first entry ----------------------------------------------

def check_dead_first(b, dead, live):
    r = b.wait_ready("web.foo.com")
    assert r.answers[0]["address"] == "10.0.0.1"
    lines = log_lines(b)
    assert any(ln.get("msg", "").startswith("ZK connect failed") and
               ln.get("server") == dead for ln in lines), lines
    assert any(session_on(live)(ln) for ln in lines), lines
    assert not any(session_on(dead)(ln) for ln in lines)
    fails = [ln for ln in metric(b, "binder_zk_connect_failures")
             if f'server="{dead}"' in ln]
    assert len(fails) == 1, metric(b, "binder_zk_connect_failures")
    assert int(fails[0].rsplit(" ", 1)[1]) >= 1
    # a label name appears once per series: the server list's label
    # takes the place of the static server-uuid label
    assert fails[0].count("server=") == 1, fails[0]
    assert metric(b, "binder_zk_server_switches")[0].endswith(" 0")


def test_dead_first_entry(tmp_path):
    zk = stub_with({"web": "10.0.0.1"})
    dead = f"127.0.0.1:{closed_port()}"
    live = f"127.0.0.1:{zk.port}"
    b = binderd(tmp_path, zk_host=f"{dead},{live}", log_level="debug")
    try:
        b.start()
        check_dead_first(b, dead, live)
    finally:
        b.stop()
        zk.stop()


# --- 3. failover and wrap-around --------------------------------------

def test_failover_and_wrap_around(tmp_path):
    a = stub_with({"web": "10.0.0.1"})
    bz = stub_with({"web": "10.0.0.2", "neu": "10.0.0.3"})
    a_port = a.port
    b = binderd(tmp_path, zk_host=f"127.0.0.1:{a_port},127.0.0.1:{bz.port}")
    try:
        b.start()
        wait_address(b, "web.foo.com", "10.0.0.1")
        assert b.dig("neu.foo.com").status == "REFUSED"

        a.stop()
        # stale-serve: the mirror keeps answering while it moves on
        assert b.dig("web.foo.com").answers[0]["address"] == "10.0.0.1"
        wait_address(b, "web.foo.com", "10.0.0.2")
        wait_address(b, "neu.foo.com", "10.0.0.3")
        assert metric(b, "binder_zk_server_switches")[0].endswith(" 1")
        lost = [ln for ln in metric(b, "binder_zk_connect_failures")
                if f'server="127.0.0.1:{a_port}"' in ln]
        assert lost and int(lost[0].rsplit(" ", 1)[1]) == 1, lost

        # wrap from the last entry back to the first
        a = stub_with({"web": "10.0.0.1"}, port=a_port)
        bz.stop()
        wait_address(b, "web.foo.com", "10.0.0.1")
        assert metric(b, "binder_zk_server_switches")[0].endswith(" 2")
    finally:
        b.stop()
        a.stop()
        bz.stop()


# --- 4. silent server -------------------------------------------------

def test_silent_server_hits_connect_deadline(tmp_path):
    silent = socket.socket()
    silent.bind(("127.0.0.1", 0))
    silent.listen(8)
    held = []

    def hold():
        try:
            while True:
                held.append(silent.accept()[0])  # and never write
        except OSError:
            pass

    threading.Thread(target=hold, daemon=True).start()
    zk = stub_with({"web": "10.0.0.1"})
    mute = f"127.0.0.1:{silent.getsockname()[1]}"
    live = f"127.0.0.1:{zk.port}"
    b = binderd(tmp_path, zk_host=f"{mute},{live}",
                config={"zookeeper": {"connectTimeoutMs": 300}})
    try:
        t0 = time.time()
        b.start()
        b.wait_ready("web.foo.com")
        took = time.time() - t0
        wait_log(b, session_on(live))
        warn = wait_log(b, lambda ln: ln.get("server") == mute and
                        "deadline" in ln.get("msg", ""))
        assert warn["level"] == 40
        assert warn["timeoutMs"] == 300
        assert held, "the silent endpoint was never connected to"
        # 300 ms, not the 15 s that sessionTimeoutMs / 2 would give
        assert took < 5, took
    finally:
        b.stop()
        zk.stop()
        silent.close()
        for s in held:
            s.close()


# --- 5. golden bytes, fresh session at the second server --------------

def listener(backlog=8):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    s.listen(backlog)
    s.settimeout(10)
    return s, f"127.0.0.1:{s.getsockname()[1]}"


def test_golden_fresh_session_at_second_server():
    e1, n1 = listener()
    e2, n2 = listener()
    golden = connect_request(timeout_ms=10000, read_only=False)[4:]
    proc = subprocess.Popen(
        [str(ZKTOOL), "-s", f"{n1},{n2}", "get", "/com"],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    try:
        c1, _ = e1.accept()
        c1.settimeout(10)
        assert read_packet(c1) == golden
        c1.close()  # a server that fails the client before any session

        c2, _ = e2.accept()
        c2.settimeout(10)
        got = read_packet(c2)
        assert got == golden, \
            f"ConnectRequest at the second server drifted:\n {got.hex()}"
        c2.sendall(packet(be32(0) + be32(30000) +
                          be64(0x0100000000000042) + jstr(b"\xab" * 16) +
                          b"\x00"))
        assert read_packet(c2) == be32(1) + be32(4) + jstr("/com") + \
            b"\x00"
        stat = be64(5) + be64(7) + be64(1000) + be64(2000) + \
            be32(1) + be32(0) + be32(0) + be64(0) + be32(5) + \
            be32(0) + be64(7)
        c2.sendall(packet(be32(1) + be64(7) + be32(0) + jstr(b"hello") +
                          stat))
        out, err = proc.communicate(timeout=10)
        assert proc.returncode == 0, err.decode()
        assert out == b"hello\n"
        c2.close()
    finally:
        proc.kill()
        proc.wait(timeout=5)
        e1.close()
        e2.close()


# --- 6. golden bytes, resume at the second server ---------------------

def test_golden_resume_at_second_server(tmp_path):
    a = stub_with({"web": "10.0.0.1"})
    e, name = listener()
    b = binderd(tmp_path, zk_host=f"127.0.0.1:{a.port},{name}")
    try:
        b.start()
        b.wait_ready("web.foo.com")
        sid = wait_log(b, session_on(f"127.0.0.1:{a.port}"))["sessionId"]
        assert sid != 0
        a.stop()

        c1, _ = e.accept()
        c1.settimeout(10)
        got = read_packet(c1)
        proto, zxid, timeout, got_sid = struct.unpack(">iqiq", got[:24])
        assert (proto, timeout, got_sid) == (0, 30000, sid)
        assert zxid > 0
        assert got[24:] == jstr(b"\x01" * 16) + b"\x00"
        # the spec's expired image: session 0, timeout 0
        c1.sendall(packet(be32(0) + be32(0) + be64(0) +
                          jstr(b"\x00" * 16) + b"\x00"))

        # a verdict, not a failure: the client stays on this server
        c2, _ = e.accept()
        c2.settimeout(10)
        got = read_packet(c2)
        assert got == connect_request(timeout_ms=30000,
                                      read_only=False)[4:], got.hex()
        c1.close()
        c2.close()
    finally:
        b.stop()
        a.stop()
        e.close()


# --- 7. pass pacing ---------------------------------------------------

def test_pass_pacing():
    """Two servers that fail every attempt: both are tried at once, then
    the client waits reconnectDelayMs (1000) before the next pass. Passes
    start at about 0, 1 and 2 s, so 2.5 s hold 6 attempts; 4 <= n <= 8
    follows from that rule: fewer means no immediate rotation or no
    further passes, more means a pass without its pause."""
    e1, n1 = listener(64)
    e2, n2 = listener(64)
    sel = selectors.DefaultSelector()
    for e in (e1, e2):
        e.setblocking(False)
        sel.register(e, selectors.EVENT_READ)
    proc = subprocess.Popen(
        [str(ZKTOOL), "-s", f"{n1},{n2}", "get", "/com"],
        stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    accepted = []
    try:
        first = None
        hard_stop = time.time() + 10
        while time.time() < hard_stop:
            if first is not None and time.time() - first >= 2.5:
                break
            for key, _ in sel.select(timeout=0.05):
                conn, _ = key.fileobj.accept()
                now = time.time()
                conn.close()
                if first is None:
                    first = now
                if now - first < 2.5:
                    accepted.append((round(now - first, 3),
                                     key.fileobj is e2))
        print("accepted:", accepted)
        assert first is not None, "zktool never connected"
        assert 4 <= len(accepted) <= 8, accepted
        # listed order: the first attempt goes to the first entry, and
        # the two alternate
        assert [second for _, second in accepted[:4]] == \
            [False, True, False, True], accepted
    finally:
        proc.kill()
        proc.wait(timeout=5)
        sel.close()
        e1.close()
        e2.close()


# --- 8. malformed list ------------------------------------------------

def test_malformed_list_is_fatal(tmp_path):
    b = binderd(tmp_path, zk_host="a:2181/chroot")
    b.start(wait_ready=False)
    try:
        assert b.proc.wait(timeout=10) == 1
        fatal = [ln for ln in log_lines(b) if ln.get("level") == 60]
        assert len(fatal) == 1, fatal
        assert '"a:2181/chroot"' in fatal[0]["msg"]
        assert "chroot" in fatal[0]["msg"]
    finally:
        b.stop()


# --- 9. zookeeper.servers in the config file --------------------------

def test_config_servers_array(tmp_path):
    zk = stub_with({"web": "10.0.0.1"})
    dead_port = closed_port()
    servers = [{"host": "127.0.0.1", "port": dead_port},
               {"host": "127.0.0.1", "port": zk.port}]
    b = binderd(tmp_path, log_level="debug", shuffle=None,
                config={"zookeeper": {"servers": servers,
                                      "shuffle": False}})
    assert "ZK_HOST" not in b.env
    try:
        b.start()
        check_dead_first(b, f"127.0.0.1:{dead_port}",
                         f"127.0.0.1:{zk.port}")
    finally:
        b.stop()
        zk.stop()


def test_zk_host_wins_over_config_servers(tmp_path):
    zk = stub_with({"web": "10.0.0.1"})
    other = stub_with({"web": "10.0.0.9"})
    b = binderd(tmp_path, zk_host=f"127.0.0.1:{zk.port}",
                config={"zookeeper": {"servers": [
                    {"host": "127.0.0.1", "port": other.port}]}})
    try:
        b.start()
        r = b.wait_ready("web.foo.com")
        assert r.answers[0]["address"] == "10.0.0.1"
        assert other.stats["sessions"] == 0
    finally:
        b.stop()
        zk.stop()
        other.stop()


def test_shuffle_is_the_default_with_a_list(tmp_path):
    """Without ZK_SHUFFLE and zookeeper.shuffle a list is permuted: which
    server comes first is the draw's business, that the mirror comes up
    on a live one is ours. One of the three entries is dead, so a draw
    that puts it first rotates too."""
    zk1 = stub_with({"web": "10.0.0.1"})
    zk2 = stub_with({"web": "10.0.0.1"})
    live = {f"127.0.0.1:{zk1.port}", f"127.0.0.1:{zk2.port}"}
    b = binderd(tmp_path, shuffle=None, zk_host=",".join(
        sorted(live) + [f"127.0.0.1:{closed_port()}"]))
    assert "ZK_SHUFFLE" not in b.env
    try:
        b.start()
        b.wait_ready("web.foo.com")
        line = wait_log(b, lambda ln: ln.get("msg") ==
                        "ZK session established")
        assert line["server"] in live
    finally:
        b.stop()
        zk1.stop()
        zk2.stop()


# --- 10. the Python client --------------------------------------------

def test_zkconn_takes_a_list():
    zk = stub_with({"web": "10.0.0.1"})
    try:
        text = f"127.0.0.1:{closed_port()},127.0.0.1:{zk.port}"
        with zkclient.ZkConn(text) as c:
            assert c.server == f"127.0.0.1:{zk.port}"
            assert c.get("/com/foo/web") == host("10.0.0.1")
        # `port` is the port of entries without one
        with zkclient.ZkConn("127.0.0.1", zk.port) as c:
            assert c.server == f"127.0.0.1:{zk.port}"
    finally:
        zk.stop()
    with pytest.raises(OSError):
        zkclient.ZkConn(f"127.0.0.1:{closed_port()},"
                        f"127.0.0.1:{closed_port()}", timeout=2)
    with pytest.raises(ValueError, match="chroot"):
        zkclient.ZkConn("127.0.0.1:2181/binder")


# --- 11. render-config.py ---------------------------------------------

def render(env_extra, meta=GOLDEN / "render_config_meta.json"):
    env = {k: v for k, v in os.environ.items()
           if k not in ("ZK_SERVERS", "ZK_PORT")}
    env.update(env_extra)
    return subprocess.run(
        [sys.executable, str(RENDER),
         str(REPO_ROOT / "etc" / "config.json.in"), str(meta)],
        env=env, capture_output=True, text=True, timeout=30, check=True
    ).stdout


def test_render_config_without_servers_is_unchanged():
    # render_config_parent.json is what the renderer and template gave
    # for this metadata before either knew about ZK_SERVERS
    assert render({}) == (GOLDEN / "render_config_parent.json").read_text()


def test_render_config_with_servers(tmp_path):
    want = [{"host": "10.0.0.1", "port": 2181},
            {"host": "zk2", "port": 2182},
            {"host": "zk3", "port": 2183}]
    out = json.loads(render({"ZK_SERVERS": "10.0.0.1:2181, zk2 ,zk3:2183",
                             "ZK_PORT": "2182"}))
    assert out["zookeeper"] == {"servers": want}
    parent = json.loads((GOLDEN / "render_config_parent.json").read_text())
    del out["zookeeper"]
    assert out == parent
    # the metadata file may carry the list too, as the array itself
    meta = json.loads((GOLDEN / "render_config_meta.json").read_text())
    meta["ZK_SERVERS"] = want
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    out = json.loads(render({}, meta=tmp_path / "meta.json"))
    assert out["zookeeper"] == {"servers": want}
