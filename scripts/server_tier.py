#!/usr/bin/env python3
"""Server tier A/B: bsockblast straight into one binderd's balancer
socket, with the bench's own serving shape - ZK mirror store, the
10,000-record bench tree, and bench.build_tree's name mix (plus
hosts-only, SRV-only and 50-name cache-hot subsets of it). Every build
named on the command line gets its own binderd on the same tree, and
the builds are interleaved run by run, so their rows compare.

Prints one JSON row per run (qps, binderd CPU ns/query from /proc),
appends them to OUT.jsonl, and ends with a per-case summary.

usage: server_tier.py OUT.jsonl RUNS name=path/to/binderd ...
  e.g. server_tier.py /tmp/st.jsonl 3 parent=/tmp/parent/bin/binderd \
           new=bin/binderd
"""
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import bench  # noqa: E402
from binder_amd.harness import BinderProcess, NativeZkd  # noqa: E402
from binder_amd.zkclient import ZkConn  # noqa: E402


def main():
    out_path = Path(sys.argv[1])
    runs = int(sys.argv[2])
    builds = [a.split("=", 1) for a in sys.argv[3:]]
    queries = 2_000_000
    tmp = Path(tempfile.mkdtemp(prefix="st-"))
    zkd = NativeZkd().start()
    conn = ZkConn("127.0.0.1", zkd.port)
    names_file = tmp / "names.txt"
    bench.build_tree(conn, names_file, 10000)
    names = names_file.read_text().splitlines()
    hosts = [n for n in names if n.startswith("h")]
    svca = [n for n in names if n.startswith("s")]
    srv = [n for n in names if n.endswith("SRV")]
    sets = {
        "mix": names,
        "hosts": hosts,
        "srv": srv,
        # same mix, 50 names, spread over the tree
        "mix50": hosts[::139][:36] + svca[::143][:7] + srv[::143][:7],
        "hosts50": hosts[::100][:50],
        "srv50": srv[::20][:50],
    }
    files = {}
    for k, v in sets.items():
        files[k] = tmp / f"{k}.txt"
        files[k].write_text("\n".join(v))
    procs = {}
    for name, path in builds:
        b = BinderProcess(dns_domain="foo.com", datacenter="coal",
                          store="zk", zk_host="127.0.0.1",
                          zk_port=zkd.port, workdir=tmp, log_level="warn",
                          balancer_socket=str(tmp / f"b-{name}"),
                          log_path=str(tmp / f"{name}.log"))
        b.cmd[0] = str(Path(path).resolve())
        b.start(wait_ready=False)
        procs[name] = b
    for name, b in procs.items():
        b.wait_listening(timeout=30)
        b.wait_ready("h4999.foo.com", timeout=120)
        b.wait_ready("_x._tcp.s999.foo.com", timeout=60, qtype="SRV")
    cases = [("mix", 128), ("mix", 4096), ("hosts", 1024), ("srv", 1024),
             ("mix", 1024), ("mix50", 1024), ("hosts50", 1024),
             ("srv50", 1024)]
    rows = []
    try:
        # one untimed pass per build: page in, fill caches/memo
        for name, b in procs.items():
            subprocess.run([str(REPO / "bin" / "bsockblast"), "-S",
                            str(tmp / f"b-{name}"), "-f", str(files["mix"]),
                            "-n", "500000", "-w", "1024"],
                           capture_output=True, check=True)
        for run in range(runs):
            for setname, window in cases:
                for name, b in procs.items():
                    r = subprocess.run(
                        [str(REPO / "bin" / "bsockblast"), "-S",
                         str(tmp / f"b-{name}"), "-f", str(files[setname]),
                         "-n", str(queries), "-w", str(window),
                         "-P", str(b.proc.pid)],
                        capture_output=True, text=True, check=True)
                    row = json.loads(r.stdout.strip().splitlines()[-1])
                    row.update(build=name, run=run, names_set=setname)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    time.sleep(0.05)
    finally:
        for b in procs.values():
            b.stop()
        conn.close()
        zkd.stop()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    with open(out_path, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    # summary
    print("\nset window build qps(M) cpu_ns")
    for setname, window in cases:
        for name in procs:
            sel = [r for r in rows if r["build"] == name and
                   r["names_set"] == setname and r["window"] == window]
            print(setname, window, name,
                  " / ".join(f"{r['qps'] / 1e6:.2f}" for r in sel), "|",
                  " / ".join(f"{r['binderd_cpu_ns_per_query']:.0f}"
                             for r in sel))


if __name__ == "__main__":
    main()
