#!/usr/bin/env python3
"""Time the GPU batch resolver (binder_amd.gpuresolve) and record the
result in profiles/GPURESOLVE.md.

Workload: 1 000 000 queries, 90 % A and 10 % SRV, against the bench.py
tree's shape: 10 000 hosts plus 100 services of 8 members (each service
has its A and its SRV entry). Device events around resolve() and around
each kernel on buffers allocated beforehand; warm-up first; median and
min..max of the repeats. Bytes per query are the bytes the algorithm
has to move, computed from the shapes, not counters. Then the table's
upkeep: apply() of 1, 1 000 and 10 000 mixed ops and one compact(),
next to constructing a GpuAnswerTable from the whole image again. The
opt-in kernel pair (accept=3) is timed against the base pair on the same
batch, the two alternating repeat by repeat, and on that batch's EDNS +
mixed-case version. Last, the single-launch path for bursts
(table.burst(N).resolve) against resolve() on the first N queries of the
same batch, N = 64, 256, 4096 and all, alternating repeat by repeat:
device time between two events around the call, host wall time from
the call until the reply lengths can be read on the host (resolve()
reads the total back itself; the burst call is followed by a
synchronise), and both per call for 100 calls queued in a row.

The measurement runs in one child process under a time limit. Without a
GPU or the extension the file says "not measured".
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import struct
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
OUT = REPO / "profiles" / "GPURESOLVE.md"
HOSTS, SERVICES, MEMBERS = 10_000, 100, 8
BURSTS = (64, 256, 4096)


def labels(name: bytes) -> bytes:
    return b"".join(bytes([len(p)]) + p for p in name.split(b".")) + b"\0"


def query(name: bytes, qtype: int) -> bytes:
    return (struct.pack(">HHHHHH", 0x4242, 0x0100, 1, 0, 0, 0) +
            labels(name) + struct.pack(">HH", qtype, 1))


def query_ext(q: bytes) -> bytes:
    """A query() as a 0x20 resolver with EDNS sends it: every other
    letter of the name uppercase, ARCOUNT 1, an OPT record advertising
    1232 bytes."""
    name = bytes(c - 32 if i % 2 and 97 <= c <= 122 else c
                 for i, c in enumerate(q[12:-4]))
    return (q[:10] + b"\0\1" + name + q[-4:] +
            struct.pack(">BHHIH", 0, 41, 1232, 0, 0))


def header(name: bytes, qtype: int, an: int, ar: int) -> bytes:
    return (struct.pack(">HHHHHH", 0, 0x8400, 1, an, 0, ar) +
            labels(name) + struct.pack(">HH", qtype, 1))


def rr(owner: bytes, rtype: int, rdata: bytes) -> bytes:
    return owner + struct.pack(">HHIH", rtype, 1, 30, len(rdata)) + rdata


def build_image(native):
    """The table, the distinct queries, and (klen, body bytes read,
    reply bytes) per distinct query for the byte counts."""
    image, a_q, srv_q = native.AnswerImage(), [], []
    ptr = b"\xc0\x0c"
    for i in range(HOSTS):
        name = b"h%d.bench.foo.com" % i
        reply = header(name, 1, 1, 0) + rr(ptr, 1, bytes([10, 0, i >> 8,
                                                          i & 255]))
        image.add_reply(name, 1, reply)
        a_q.append((query(name, 1), len(name), 4 + len(reply), len(reply)))
    for s in range(SERVICES):
        dom = b"svc%d.bench.foo.com" % s
        srv = b"_http._tcp." + dom
        mem_a, mem_srv = [], []
        for m in range(MEMBERS):
            addr = bytes([10, 1, s, m])
            # short member names: the 8-member SRV reply must fit 512
            target = labels(b"m%d-s%d" % (m, s))
            mem_a.append((rr(ptr, 1, addr), b""))
            mem_srv.append((rr(ptr, 33, struct.pack(">HHH", 0, 10, 80) +
                               target), rr(target, 1, addr)))
        for name, qt, head, mem, qs in (
                (dom, 1, header(dom, 1, MEMBERS, 0), mem_a, a_q),
                (srv, 33, header(srv, 33, MEMBERS, MEMBERS), mem_srv,
                 srv_q)):
            image.add_service(name, qt, head, mem)
            total = len(head) + sum(len(a) + len(b) for a, b in mem)
            qs.append((query(name, qt), len(name), 6 + 8 * MEMBERS + total,
                       total))
    return image, a_q, srv_q


def worker(n: int, repeats: int) -> dict:
    import torch
    from binder_amd import _gpuresolve, _native, gpuresolve

    image, a_q, srv_q = build_image(_native)
    rng = random.Random(1)
    picks = [rng.choice(srv_q) if rng.random() < 0.1 else rng.choice(a_q)
             for _ in range(n)]
    ext = {q: query_ext(q) for q, *_ in a_q + srv_q}
    offs = [0]
    for p in picks:
        offs.append(offs[-1] + len(p[0]))
    # the bytes the two kernels must move, per query: query + its offset +
    # one slot + blob key and body head in; 8 bytes of result out; then
    # result, offsets and 3 query bytes + the body in; the reply out
    look_rd = sum(len(q) + 4 + 16 + 2 + klen + 4 for q, klen, _, _ in picks)
    emit_rd = sum(4 + 4 + 8 + 4 + 3 + body for _, _, body, _ in picks)
    emit_wr = sum(total for _, _, _, total in picks)
    qbuf_h = torch.frombuffer(bytearray(b"".join(p[0] for p in picks)),
                              dtype=torch.uint8).pin_memory()
    qoff_h = torch.tensor(offs, dtype=torch.int32).pin_memory()
    table = gpuresolve.GpuAnswerTable(image)

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]), out

    def series(fn):
        for _ in range(3):
            timed(fn)
        ms = sorted(timed(fn)[0] for _ in range(repeats))
        return {"median_ms": statistics.median(ms), "min_ms": ms[0],
                "max_ms": ms[-1]}

    res = {"n": n, "repeats": repeats, "tile": gpuresolve.TILE,
           "group": gpuresolve.GROUP, "device": torch.cuda.get_device_name(),
           "entries": len(image), "slots": table.cap}
    res["upload"] = series(lambda: (qbuf_h.to("cuda", non_blocking=True),
                                    qoff_h.to("cuda", non_blocking=True)))
    qbuf, qoff = qbuf_h.cuda(), qoff_h.cuda()
    res["resolve"] = series(lambda: table.resolve(qbuf, qoff, seed=7))
    rbuf, roff = table.resolve(qbuf, qoff, seed=7)
    assert int(roff[-1]) == emit_wr and bool((roff[1:] > roff[:-1]).all())
    res["download"] = series(lambda: rbuf.cpu())

    stream = torch.cuda.current_stream().cuda_stream
    body_off = torch.empty(n, dtype=torch.int32, device="cuda")
    rlen = torch.empty(n, dtype=torch.int32, device="cuda")
    batch = (qbuf.data_ptr(), qoff.data_ptr(), qbuf.numel(), n)
    res["lookup"] = series(lambda: _gpuresolve.lookup(
        *batch, table._slots.data_ptr(), table.cap, table._arena.data_ptr(),
        body_off.data_ptr(), rlen.data_ptr(), stream))
    res["emit"] = series(lambda: _gpuresolve.emit(
        *batch, table._arena.data_ptr(), body_off.data_ptr(),
        rlen.data_ptr(), roff.data_ptr(), rbuf.data_ptr(), 7, stream))
    # the opt-in pair: same batch, base and opt-in alternating; then the
    # same names asked in mixed case with an OPT record
    ebuf = torch.frombuffer(bytearray(b"".join(
        ext[p[0]] for p in picks)), dtype=torch.uint8).cuda()
    eoff = torch.tensor([0] + [len(ext[p[0]]) for p in picks]).cumsum(0).to(
        torch.int32).cuda()
    got, goff = table.resolve(ebuf, eoff, seed=7, accept=3)
    assert int(goff[-1]) == emit_wr + 11 * n
    assert torch.equal(table.resolve(qbuf, qoff, seed=7, accept=3)[0], rbuf)
    meta = torch.empty(n, dtype=torch.int32, device="cuda")
    ebatch = (ebuf.data_ptr(), eoff.data_ptr(), ebuf.numel(), n)

    def pair(bt, off, out):
        return (lambda: _gpuresolve.lookup_ext(
            *bt, table._slots.data_ptr(), table.cap, table._arena.data_ptr(),
            3, body_off.data_ptr(), rlen.data_ptr(), meta.data_ptr(),
            stream), lambda: _gpuresolve.emit_ext(
                *bt, table._arena.data_ptr(), body_off.data_ptr(),
                rlen.data_ptr(), meta.data_ptr(), off.data_ptr(),
                out.data_ptr(), 7, stream))
    runs = {"resolve0": lambda: table.resolve(qbuf, qoff, seed=7),
            "resolve3": lambda: table.resolve(qbuf, qoff, seed=7, accept=3),
            "resolve3_ext": lambda: table.resolve(ebuf, eoff, seed=7,
                                                  accept=3)}
    # each emit right behind its own lookup: they share body_off and rlen
    runs["lookup3"], runs["emit3"] = pair(batch, roff, rbuf)
    runs["lookup3_ext"], runs["emit3_ext"] = pair(ebatch, goff, got)
    ms = {k: [] for k in runs}
    for r in range(3 + repeats):
        for k, fn in runs.items():
            t = timed(fn)[0]
            if r >= 3:
                ms[k].append(t)
    for k, v in ms.items():
        v.sort()
        res[k] = {"median_ms": statistics.median(v), "min_ms": v[0],
                  "max_ms": v[-1]}
    kernel_s = (res["lookup"]["median_ms"] + res["emit"]["median_ms"]) / 1e3
    res["bytes_per_query"] = {"lookup_read": look_rd / n, "lookup_write": 8.0,
                              "emit_read": emit_rd / n,
                              "emit_write": emit_wr / n}
    res["kernel_qps"] = n / kernel_s
    res["kernel_gbps"] = (look_rd + 8 * n + emit_rd + emit_wr) / kernel_s / 1e9
    res["resolve_qps"] = n / (res["resolve"]["median_ms"] / 1e3)

    # bursts: resolve() and the fused launch on the first N queries
    def spread(v):
        v = sorted(v)
        return {"median_ms": statistics.median(v), "min_ms": v[0],
                "max_ms": v[-1]}

    def both(fn, sync):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev[0].record()
        fn()
        ev[1].record()
        if sync:
            torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]), wall

    def queued(fn, calls=100):
        """Per call, `calls` calls in a row with no wait between them:
        device time between two events around the run, and host time."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev[0].record()
        for _ in range(calls):
            fn()
        ev[1].record()
        host = (time.perf_counter() - t) * 1e3 / calls
        ev[1].synchronize()
        return {"device_ms": ev[0].elapsed_time(ev[1]) / calls,
                "host_ms": host}
    res["burst"] = {}
    for bn in sorted({b for b in BURSTS if b < n} | {n}):
        bq, bo = qbuf[:offs[bn]], qoff[:bn + 1]
        ws = table.burst(bn)
        want, woff = table.resolve(bq, bo, seed=7)
        got, gstart, glen = ws.resolve(bq, bo, seed=7)
        assert torch.equal(glen, (woff[1:] - woff[:-1]).int())
        assert ws.dropped() == 0
        if bn <= gpuresolve.FUSED_TILE:  # one tile: resolve()'s bytes
            assert torch.equal(got[:want.numel()], want)
            assert torch.equal(gstart, woff[:-1])
        runs = {"resolve": (lambda: table.resolve(bq, bo, seed=7), False),
                "burst": (lambda: ws.resolve(bq, bo, seed=7), True)}
        ms = {k: ([], []) for k in runs}
        for r in range(3 + repeats):
            for k, (fn, sync) in runs.items():
                dev, wall = both(fn, sync)
                if r >= 3:
                    ms[k][0].append(dev)
                    ms[k][1].append(wall)
        res["burst"][str(bn)] = {k: {"device": spread(d), "wall": spread(w),
                                     "queued": queued(runs[k][0])}
                                 for k, (d, w) in ms.items()}

    # keeping the device table current: apply() of a mixed delta (half
    # replacements, a quarter invalidations, a quarter new hosts) against
    # the only way there was before it, uploading the whole image again
    res["reupload"] = series(lambda: gpuresolve.GpuAnswerTable(image))
    live = gpuresolve.GpuAnswerTable(image, reserve_entries=4 * len(image),
                                     reserve_bytes=64 << 20)
    fresh = iter(range(HOSTS, 10 ** 9))

    def delta(ops):
        d = _native.AnswerDelta()
        for _ in range(ops):
            kind, i = rng.random(), rng.randrange(HOSTS)
            name = b"h%d.bench.foo.com" % i
            if kind < 0.25:
                d.invalidate(name)
                continue
            if kind < 0.5:
                i = next(fresh)
                name = b"h%d.bench.foo.com" % i
            d.upsert_reply(name, 1, header(name, 1, 1, 0) + rr(
                b"\xc0\x0c", 1, struct.pack(">I", 0x0A000000 + i % 2 ** 24)))
        return d
    for ops in (1, 1000, 10000):
        deltas = iter([delta(ops) for _ in range(3 + max(20, repeats))])
        res[f"apply{ops}"] = series(lambda: live.apply(next(deltas)))
    res["compact"] = series(live.compact)
    res["live"] = live.stats()
    return res


CONTEXT = """
Context only: the CPU hit path costs about 100-125 ns per query per core
(`profiles/SCALING.md`). That figure comes from a different box and
round; no ratio is claimed from it.
"""


def render(res) -> str:
    head = "# GPU batch resolver: timing\n\n"
    if res is None:
        return head + "not measured\n" + CONTEXT

    def row(name, key):
        s = res[key]
        return (f"| {name} | {s['median_ms']:.3f} | {s['min_ms']:.3f} .. "
                f"{s['max_ms']:.3f} |\n")
    b = res["bytes_per_query"]

    def burst_rows():
        out = ""
        for bn, r in res["burst"].items():
            for k, call in (("resolve", "resolve()"),
                            ("burst", "burst.resolve()")):
                d, w = r[k]["device"], r[k]["wall"]
                out += (f"| {bn} | {call} | {d['median_ms']:.4f} | "
                        f"{d['min_ms']:.4f} .. {d['max_ms']:.4f} | "
                        f"{w['median_ms']:.4f} | {w['min_ms']:.4f} .. "
                        f"{w['max_ms']:.4f} | "
                        f"{r[k]['queued']['device_ms']:.4f} | "
                        f"{r[k]['queued']['host_ms']:.4f} |\n")
        return out
    ratios = ", ".join(
        "N = %s device %.2f, wall %.2f, queued device %.2f, queued host "
        "%.2f" % (
            bn, r["burst"]["device"]["median_ms"] /
            r["resolve"]["device"]["median_ms"],
            r["burst"]["wall"]["median_ms"] /
            r["resolve"]["wall"]["median_ms"],
            r["burst"]["queued"]["device_ms"] /
            r["resolve"]["queued"]["device_ms"],
            r["burst"]["queued"]["host_ms"] /
            r["resolve"]["queued"]["host_ms"])
        for bn, r in res["burst"].items())
    return (head + f"`scripts/gpuresolve_bench.py` on {res['device']}: "
            f"{res['n']} queries (90 % A, 10 % SRV), {res['entries']} "
            f"entries in {res['slots']} slots, {res['repeats']} repeats "
            "after warm-up, device events.\n\n"
            f"Choices: T = {res['tile']} queries per lookup workgroup, "
            f"{res['group']} lanes per reply in emit.\n\n"
            "| step | median ms | min .. max ms |\n|---|---|---|\n" +
            row("upload qbuf + qoff (pinned)", "upload") +
            row("resolve() whole", "resolve") +
            row("bamd_resolve_lookup", "lookup") +
            row("bamd_resolve_emit", "emit") +
            row("download rbuf", "download") +
            row("new GpuAnswerTable(image), the whole upload", "reupload") +
            row("apply() of 1 op", "apply1") +
            row("apply() of 1 000 mixed ops", "apply1000") +
            row("apply() of 10 000 mixed ops", "apply10000") +
            row("compact()", "compact") +
            "\nThe opt-in pair (`accept=3`) against the base pair, the "
            "seven calls alternating repeat by repeat; `plain` is the batch "
            "above, `EDNS + mixed case` the same names with every other "
            "letter uppercase and an OPT record:\n\n"
            "| step | median ms | min .. max ms |\n|---|---|---|\n" +
            row("resolve() accept=0, plain", "resolve0") +
            row("resolve() accept=3, plain", "resolve3") +
            row("resolve() accept=3, EDNS + mixed case", "resolve3_ext") +
            row("bamd_resolve_lookup_ext, plain", "lookup3") +
            row("bamd_resolve_emit_ext, plain", "emit3") +
            row("bamd_resolve_lookup_ext, EDNS + mixed case",
                "lookup3_ext") +
            row("bamd_resolve_emit_ext, EDNS + mixed case", "emit3_ext") +
            f"\n- kernels: {res['kernel_qps'] / 1e6:.1f} M queries/s, "
            f"{res['kernel_gbps']:.1f} GB/s of needed bytes over kernel "
            "time\n"
            f"- resolve() whole: {res['resolve_qps'] / 1e6:.1f} M queries/s "
            "(adds the prefix sum, allocations and one synchronise)\n"
            f"- bytes per query from the shapes: lookup reads "
            f"{b['lookup_read']:.1f} and writes {b['lookup_write']:.0f}; "
            f"emit reads {b['emit_read']:.1f} and writes "
            f"{b['emit_write']:.1f}\n"
            "- opt-in over base on the plain batch, by the medians: "
            "resolve() %.2f, lookup %.2f, emit %.2f; resolve() on the EDNS "
            "+ mixed-case batch over the base pair on the plain one: %.2f "
            "(11 more bytes in and out per query)\n" % (
                res["resolve3"]["median_ms"] / res["resolve0"]["median_ms"],
                res["lookup3"]["median_ms"] / res["lookup"]["median_ms"],
                res["emit3"]["median_ms"] / res["emit"]["median_ms"],
                res["resolve3_ext"]["median_ms"] /
                res["resolve0"]["median_ms"]) +
            "- apply() and the upload are whole calls between two device "
            "events, host packing and copies included; a mixed delta is "
            "half replacements, a quarter invalidations, a quarter new "
            "hosts; an apply() that compacts first shows in its row's max\n"
            "- apply() over the whole upload, by the medians: " +
            ", ".join(
                f"{ops} ops " + "%.2f" % (res[f"apply{ops}"]["median_ms"] /
                                          res["reupload"]["median_ms"])
                for ops in (1, 1000, 10000)) +
            " (above 1 the delta costs more than uploading this "
            f"{res['entries']}-entry image again)\n"
            f"- the updated table at the end: {res['live']}\n"
            "\nBursts: `table.burst(N).resolve()`, one launch of "
            "`bamd_resolve_fused` into a buffer made beforehand and one "
            "reset of a cursor behind it, against `resolve()` on the first N queries of the "
            "batch above, inputs on the device, the two alternating repeat "
            "by repeat. `device` is the time between two events around the "
            "call; `wall` is host time from the call until the reply "
            "lengths can be read on the host: `resolve()` reads the total "
            "back itself, the burst call is followed by a synchronise. "
            "`queued` is 100 calls in a row with no wait between them, per "
            "call: device time between two events around the run, and the "
            "host's time. At 64 and 256 queries every column is launch and "
            "host overhead more than kernel time.\n\n"
            "| N | call | device median ms | min .. max | wall median ms | "
            "min .. max | queued device ms | queued host ms |\n"
            "|---|---|---|---|---|---|---|---|\n" + burst_rows() +
            f"\n- burst over resolve() by the medians: {ratios}\n"
            "- at 1 000 000 queries the fused kernel is the slower one: a "
            "workgroup of 1024 lanes looks up in one wave and one workgroup "
            "is resident per CU, which buys a burst's latency with a "
            "replay's throughput. Replay keeps `resolve()`; a serving loop "
            "uses `burst()`, whose call leaves the host after the launch "
            "and queues behind the one before it\n" + CONTEXT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out", type=Path, default=OUT)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(args.n, max(20, args.repeats))))
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
           __file__, "--worker", "--n", str(args.n), "--repeats",
           str(args.repeats)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    res = json.loads(p.stdout.splitlines()[-1]) if p.returncode == 0 else None
    if res is None:
        print(p.stderr[-2000:], file=sys.stderr)
    # the "## Oversize" section at the end of the file is
    # gpuresolve_oversize_bench.py's: keep it
    old = args.out.read_text() if args.out.exists() else ""
    _, mark, kept = old.partition("\n## Oversize\n")
    args.out.write_text(render(res) + mark + kept)
    print(render(res))
    return 0 if res is not None else 1


if __name__ == "__main__":
    sys.exit(main())
