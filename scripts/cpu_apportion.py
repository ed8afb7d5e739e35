#!/usr/bin/env python3
"""Apportion the cgroup CPU quota across the bench chain: sample
utime+stime of every process (binderd / balancer / zkd / dnsblast)
while a sustained closed-loop run is in flight, and print cores
consumed per component — the denominator that bounds qps on the
quota-capped bench boxes (profiles/SCALING.md round 2).

usage: cpu_apportion.py [--procs 8] [--workers 8] [--threads 6]
                        [--window 256] [--ramp 2] [--tag NAME]

Every component is reported as total cores and split into user and
system time. For the balancer and for binderd the cost per query
(core-us, user and system) is added, and from the balancer's stats
socket the shape of its hot path over the window: mean reply-run
length, share of replies that left singly, replies per backend read,
queries per received UDP message, and - with the backend hop on
shared-memory rings - doorbells rung, ring drains, doorbells per drain
and the transports in use.
BALANCER_BIN selects the balancer binary (binder_amd/harness.py), so a
parent build and a new one can alternate inside one box visit.

The generator is given far more queries than any window can use: a
budget that runs out inside the window (100 M did, once the chain
passed 12.5 M qps) reads as a *lower* rate the faster the chain is.
"""
import argparse
import json
import socket
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import bench  # noqa: E402

HZ = 100  # USER_HZ


def cpu_of(pid):
    try:
        parts = open(f"/proc/{pid}/stat").read().rsplit(") ", 1)[1]
        f = parts.split()
        return int(f[11]) / HZ, int(f[12]) / HZ  # utime, stime (s)
    except (OSError, IndexError, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--threads", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--window", type=int, default=256,
                    help="dnsblast in-flight queries per socket")
    ap.add_argument("--ramp", type=float, default=2.0,
                    help="seconds of load before the sampling window")
    ap.add_argument("--no-gso", action="store_true")
    ap.add_argument("--tag", default=None,
                    help="copied into the output row (e.g. the build)")
    args = ap.parse_args()

    from binder_amd.harness import free_port, NativeZkd
    from binder_amd.zkclient import ZkConn

    tmp = Path(tempfile.mkdtemp(prefix="cpu-apportion-"))
    names_file = tmp / "names.txt"
    zkd = NativeZkd().start()
    conn = ZkConn("127.0.0.1", zkd.port)
    bench.build_tree(conn, names_file, 10000)
    backends, sockdir = bench.start_backends(args.procs, tmp, zkd.port)
    port = free_port()
    bal = bench.start_balancer(tmp, sockdir, port,
                               workers=args.workers)
    bench.wait_balancer_ready(port, args.procs, tmp)

    cmd = [str(REPO / "bin" / "dnsblast"), "-s", "127.0.0.1",
           "-p", str(port), "-n", "4000000000", "-c", str(args.window),
           "-t", str(args.threads), "-P", "8", "-f", str(names_file),
           "-B", "127.0.1.1", "-T", "10000"]
    if args.no_gso:
        cmd.append("-g")
    blast = subprocess.Popen(cmd, stdout=subprocess.DEVNULL)

    def balstat():
        with socket.socket(socket.AF_UNIX) as s:
            s.settimeout(2)
            s.connect(str(tmp / "stats.sock"))
            return json.loads(s.recv(1 << 20).decode())
    try:
        time.sleep(args.ramp)
        pids = {"dnsblast": [blast.pid], "balancer": [bal.pid],
                "zkd": [zkd.proc.pid],
                "binderd": [b.proc.pid for b in backends]}
        t0 = time.time()
        before = {k: [cpu_of(p) for p in v] for k, v in pids.items()}
        st0 = balstat()
        time.sleep(args.seconds)
        dt = time.time() - t0
        after = {k: [cpu_of(p) for p in v] for k, v in pids.items()}
        st1 = balstat()
        out = {"window_s": round(dt, 2), "procs": args.procs,
               "workers": args.workers, "threads": args.threads,
               "window": args.window, "ramp_s": args.ramp, "gso": not args.no_gso,
               "qps": round((st1["udp_replies"] -
                             st0["udp_replies"]) / dt)}
        if args.tag:
            out["tag"] = args.tag
        total = 0.0
        split = {}
        for k in pids:
            pairs = [(a, b) for a, b in zip(after[k], before[k])
                     if a is not None and b is not None]
            user = sum(a[0] - b[0] for a, b in pairs) / dt
            syst = sum(a[1] - b[1] for a, b in pairs) / dt
            split[k] = (user, syst)
            out[k + "_cores"] = round(user + syst, 2)
            out[k + "_user_cores"] = round(user, 2)
            out[k + "_sys_cores"] = round(syst, 2)
            total += user + syst
        out["total_cores"] = round(total, 2)
        if out["qps"] > 0:
            per_q = 1e6 / out["qps"]  # cores -> core-us per query
            for k in ("balancer", "binderd"):
                user, syst = split[k]
                out[k + "_core_us_per_query"] = round(
                    (user + syst) * per_q, 4)
                out[k + "_user_us_per_query"] = round(user * per_q, 4)
                out[k + "_sys_us_per_query"] = round(syst * per_q, 4)
        # hot-path shape over the window (absent from older balancers)
        d = {k: st1[k] - st0[k] for k in
             ("udp_queries", "udp_replies", "reply_runs",
              "reply_run_segments", "reply_singles", "backend_reads",
              "udp_rx_msgs", "shm_doorbells", "shm_drains")
             if k in st1 and k in st0}
        if "reply_runs" in d:
            out.update(d)
            if d.get("shm_drains"):
                out["doorbells_per_drain"] = round(
                    d["shm_doorbells"] / d["shm_drains"], 4)
            out["transports"] = sorted(
                {b.get("transport", "stream") for b in st1["backends"]})
            if d["reply_runs"]:
                out["mean_run_len"] = round(
                    d["reply_run_segments"] / d["reply_runs"], 2)
            if d["udp_replies"]:
                out["singles_share"] = round(
                    d["reply_singles"] / d["udp_replies"], 4)
            if d["backend_reads"]:
                out["replies_per_backend_read"] = round(
                    d["udp_replies"] / d["backend_reads"], 1)
            if d["udp_rx_msgs"]:
                out["queries_per_udp_msg"] = round(
                    d["udp_queries"] / d["udp_rx_msgs"], 2)
        try:
            q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            out["quota_cores"] = (int(q) // int(p)
                                  if q != "max" else None)
        except (OSError, ValueError):
            pass
        print(json.dumps(out), flush=True)
    finally:
        blast.kill()
        blast.wait()
        bal.terminate()
        for b in backends:
            b.stop()
        conn.close()
        zkd.stop()


if __name__ == "__main__":
    main()
