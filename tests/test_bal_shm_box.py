"""The shared-memory backend hop under generator load, on the bench box.

One binderd on a file store behind a 4-worker balancer with the default
ring, dnsblast in closed loop with GSO bursts: 200,000 queries, every
one answered NOERROR, none timed out, the balancer's books balance, all
connections on rings - and fewer doorbells rung than batches taken off
the reply rings, i.e. looking at the rings once more before sleeping
does save wakeups under load.
"""
import json
import os
import subprocess
import time

import pytest

from binder_amd import REPO_ROOT
from binder_amd.digclient import dig
from binder_amd.harness import BALANCERD, BinderProcess, free_port

from test_balancer_hotpath import balstat

pytestmark = pytest.mark.gpu

N_HOSTS = 1000
N_QUERIES = 200_000


def test_rings_behind_generator_lose_nothing_and_save_wakeups(tmp_path):
    tree = {"foo.com": None}
    for i in range(N_HOSTS):
        tree[f"h{i}.foo.com"] = {
            "type": "host",
            "host": {"address": f"10.1.{i // 250}.{i % 250 + 1}"}}
    store = tmp_path / "tree.json"
    store.write_text(json.dumps(tree))
    (tmp_path / "names.txt").write_text(
        "\n".join(f"h{i}.foo.com A" for i in range(N_HOSTS)))
    sockdir = tmp_path / "socks"
    sockdir.mkdir()
    stats_path = tmp_path / "stats.sock"

    env = {k: v for k, v in os.environ.items()
           if k not in ("BINDER_BAL_SHM", "BINDER_BAL_SHM_RING")}
    b = BinderProcess(store=f"file:{store}", workdir=tmp_path,
                      log_level="warn",
                      balancer_socket=str(sockdir / "b0"),
                      log_path=str(tmp_path / "b0.log"))
    for k in ("BINDER_BAL_SHM", "BINDER_BAL_SHM_RING"):
        b.env.pop(k, None)  # the defaults are what is under test
    b.start()
    bal = None
    try:
        b.wait_ready(f"h{N_HOSTS - 1}.foo.com", timeout=30)
        port = free_port()
        bal = subprocess.Popen(
            [str(BALANCERD), "-p", str(port), "-H", "127.0.0.1",
             "-s", str(sockdir), "-S", str(stats_path), "-r", "100",
             "-w", "4"],
            env=dict(env, LOG_LEVEL="warn"),
            stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT)
        # the chain is up once a query gets through it
        deadline = time.time() + 10
        while True:
            try:
                if dig("h0.foo.com", "A", server="127.0.0.1", port=port,
                       timeout=0.25).status == "NOERROR":
                    break
            except OSError:
                pass
            assert time.time() < deadline, "balancer never forwarded"
        # all four workers' connections have moved onto their rings
        deadline = time.time() + 5
        while True:
            st = balstat(stats_path)
            if st["workers"] == 4 and \
                    [x["transport"] for x in st["backends"]] == ["shm"]:
                break
            assert time.time() < deadline, st["backends"]
            time.sleep(0.05)
        out = subprocess.run(
            [str(REPO_ROOT / "bin" / "dnsblast"),
             "-s", "127.0.0.1", "-p", str(port),
             "-n", str(N_QUERIES), "-c", "64", "-t", "4",
             "-f", str(tmp_path / "names.txt")],
            capture_output=True, text=True, timeout=60, check=True)
        stats = json.loads(out.stdout.strip().splitlines()[-1])
        print(stats)
        assert stats["sent"] >= N_QUERIES
        assert stats["received"] == stats["sent"], stats
        assert stats["noerror"] == stats["received"], stats
        assert stats["timeouts"] == 0, stats
        assert b.proc.poll() is None and bal.poll() is None

        # workers other than the one serving the stats socket publish
        # their counters on the 100 ms sweep tick
        deadline = time.time() + 5
        while True:
            st = balstat(stats_path)
            if st["udp_replies"] >= stats["received"] or \
                    time.time() > deadline:
                break
            time.sleep(0.02)
        print({k: v for k, v in st.items()
               if k not in ("backends", "remotes")})
        assert st["workers"] == 4
        assert st["udp_replies"] >= stats["received"], st
        assert st["reply_run_segments"] + st["reply_singles"] == \
            st["udp_replies"], st
        assert st["drops"] == 0, st
        for w in st["per_worker"]:
            assert w["reply_run_segments"] + w["reply_singles"] == \
                w["udp_replies"], w
        assert [x["transport"] for x in st["backends"]] == ["shm"], st
        assert st["shm_drains"] > 0, st
        assert st["shm_doorbells"] < st["shm_drains"], st
    finally:
        if bal is not None:
            bal.terminate()
            bal.wait(timeout=5)
        b.stop()
