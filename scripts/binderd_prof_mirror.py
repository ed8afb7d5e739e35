#!/usr/bin/env python3
"""gprof flat profile of binderd in the bench's own serving shape: ZK
mirror store, the 10,000-record bench tree and bench.build_tree's name
mix, driven closed-loop by bsockblast (8 M queries). This is the
profile to read before touching the serving core; binderd_prof.sh
(file store, host names only) does not walk the mirror or the service
answers and under-reports the per-query cost several times over.

Each build is a binderd compiled with -pg into a scratch BUILD dir
(never into bin/), e.g.
  make BUILD=/tmp/pg CXXFLAGS="-O2 -g -pg -std=c++20 -fPIC \
      -fno-omit-frame-pointer -Wall -Wextra -Wno-unused-parameter \
      -MMD -MP" bin/binderd && mv bin/binderd /tmp/binderd-prof && \
      make bin/binderd
Writes OUTDIR/gprof_mirror_<name>.txt (top of the flat profile plus the
bsockblast row with binderd's CPU ns/query, which unlike gprof covers
libc and kernel time).

usage: binderd_prof_mirror.py OUTDIR name=path/to/binderd-prof ...
"""
import json
import os
import signal
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import bench  # noqa: E402
from binder_amd.harness import BinderProcess, NativeZkd  # noqa: E402
from binder_amd.zkclient import ZkConn  # noqa: E402


def main():
    out = Path(sys.argv[1])
    out.mkdir(parents=True, exist_ok=True)
    builds = [a.split("=", 1) for a in sys.argv[2:]]
    tmp = Path(tempfile.mkdtemp(prefix="gp-"))
    zkd = NativeZkd().start()
    conn = ZkConn("127.0.0.1", zkd.port)
    names_file = tmp / "names.txt"
    bench.build_tree(conn, names_file, 10000)
    try:
        for name, path in builds:
            binary = str(Path(path).resolve())
            cwd = tmp / name
            cwd.mkdir()
            b = BinderProcess(dns_domain="foo.com", datacenter="coal",
                              store="zk", zk_host="127.0.0.1",
                              zk_port=zkd.port, workdir=cwd,
                              log_level="warn",
                              balancer_socket=str(cwd / "b0"))
            b.cmd[0] = binary
            b.proc = subprocess.Popen(b.cmd, env=b.env, cwd=str(cwd),
                                      stdout=subprocess.DEVNULL,
                                      stderr=subprocess.STDOUT)
            b.wait_listening(timeout=30)
            b.wait_ready("h4999.foo.com", timeout=120)
            b.wait_ready("_x._tcp.s999.foo.com", timeout=60, qtype="SRV")
            r = subprocess.run(
                [str(REPO / "bin" / "bsockblast"), "-S", str(cwd / "b0"),
                 "-f", str(names_file), "-n", "8000000", "-w", "1024",
                 "-P", str(b.proc.pid)],
                capture_output=True, text=True, check=True)
            row = json.loads(r.stdout.strip().splitlines()[-1])
            b.proc.send_signal(signal.SIGTERM)
            b.proc.wait(timeout=20)
            g = subprocess.run(["gprof", "-b", "-p", binary,
                                str(cwd / "gmon.out")],
                               capture_output=True, text=True)
            lines = g.stdout.splitlines()[:45]
            (out / f"gprof_mirror_{name}.txt").write_text(
                f"# binderd ({name}), mirror store, bench mix, 8 M "
                f"queries via bsockblast -w 1024\n# {json.dumps(row)}\n" +
                "\n".join(lines) + "\n")
            print(name, json.dumps(row))
            print("\n".join(lines[:16]))
    finally:
        conn.close()
        zkd.stop()
    os.sync()


if __name__ == "__main__":
    main()
