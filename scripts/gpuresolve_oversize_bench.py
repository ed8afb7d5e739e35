#!/usr/bin/env python3
"""Time the GPU batch resolver's oversize pair (resolve(oversize=True),
native/gpu/resolvelarge.cpp) and record the result as the last section,
"## Oversize", of profiles/GPURESOLVE.md.

Small-reply batch: gpuresolve_bench.py's image and its 1 000 000
queries, plain and in their EDNS + mixed-case version. The opt-in pair
(accept=3) and the oversize pair (accept=3) run on the same buffers,
alternating repeat by repeat: what the switch costs when no reply is
large.

Large batch: an image with max_reply=4096, the same hosts and 100
services of 64 members whose SRV replies are above 3 KB. One query in
sixteen asks for such a service with an OPT record advertising 4096
bytes, the rest for hosts. After one lookup, three emits write the same
bytes (compared first), alternating repeat by repeat: emit_lim as it
ships, emit_lim with nothing listed (one 16-lane group per reply), and
the opt-in pair's emit_ext, which is that plain shape without the drain
loop and can serve this batch because nothing in it is truncated.

Bursts ("Oversize bursts"): table.burst(N, oversize=True), one launch of
bamd_resolve_fused_lim (native/gpu/resolvefusedlim.cpp), at N = 64, 256
and 4096. On the small-reply image against table.burst(N), same bytes;
on the large image against resolve(..., oversize=True), with the burst
table's columns (device time, wall time to readable lengths, 100 queued
calls); and the kernel's two thresholds tried one by one, on the large
batch and on one whose large replies are 4000-byte wire replies.

Device events around each launch on buffers allocated beforehand, three
warm-up rounds, median and min..max of the repeats. Fails without a GPU.
"""
from __future__ import annotations

import argparse
import random
import statistics
import struct
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from gpuresolve_bench import (HOSTS, OUT, build_image, header, labels,  # noqa
                              query, query_ext, rr)

MARK = "\n## Oversize\n"
SERVICES, MEMBERS = 100, 64


def large_image(native):
    image, hosts, srv = native.AnswerImage(max_reply=4096), [], []
    ptr = b"\xc0\x0c"
    for i in range(HOSTS):
        name = b"h%d.bench.foo.com" % i
        image.add_reply(name, 1, header(name, 1, 1, 0) +
                        rr(ptr, 1, bytes([10, 0, i >> 8, i & 255])))
        hosts.append(query(name, 1))
    for s in range(SERVICES):
        name = b"_http._tcp.svc%d.bench.foo.com" % s
        mem = []
        for m in range(MEMBERS):
            target, addr = labels(b"m%d-s%d" % (m, s)), bytes([10, 1, s, m])
            mem.append((rr(ptr, 33, struct.pack(">HHH", 0, 10, 80) + target),
                        rr(target, 1, addr)))
        image.add_service(name, 33, header(name, 33, MEMBERS, MEMBERS), mem)
        srv.append(query(name, 33)[:10] + b"\0\1" + query(name, 33)[12:] +
                   struct.pack(">BHHIH", 0, 41, 4096, 0, 0))
    return image, hosts, srv


def measure(n: int, repeats: int) -> dict:
    import torch
    from binder_amd import _gpuresolve as g, _native, gpuresolve

    stream = torch.cuda.current_stream().cuda_stream

    def device(queries):
        buf = torch.frombuffer(bytearray(b"".join(queries)),
                               dtype=torch.uint8).cuda()
        off = torch.tensor([0] + [len(q) for q in queries]).cumsum(0).to(
            torch.int32).cuda()
        return buf, off

    def alternate(runs):
        """{name: fn} -> {name: spread}; the calls in turn, each between
        two device events."""
        ms = {k: [] for k in runs}
        for r in range(3 + repeats):
            for k, fn in runs.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                fn()
                ev[1].record()
                ev[1].synchronize()
                if r >= 3:
                    ms[k].append(ev[0].elapsed_time(ev[1]))
        return {k: {"median_ms": statistics.median(v), "min_ms": min(v),
                    "max_ms": max(v)} for k, v in ms.items()}

    def emitter(emit, batch, arena, body, rlen, meta, roff, rbuf):
        return lambda **kw: emit(*batch, arena, body.data_ptr(),
                                 rlen.data_ptr(), meta.data_ptr(),
                                 roff.data_ptr(), rbuf.data_ptr(), 7, stream,
                                 **kw)

    def launches(table, buf, off, accept):
        """The two pairs' launches on one batch, each pair with buffers
        of its own, filled by one resolve() and one lookup. Returns the
        launches, and per pair what its emit takes."""
        batch = (buf.data_ptr(), off.data_ptr(), buf.numel(), n)
        tab = (table._slots.data_ptr(), table.cap, table._arena.data_ptr())
        runs, args = {}, {}
        for name, lookup, emit in (("ext", g.lookup_ext, g.emit_ext),
                                   ("lim", g.lookup_lim, g.emit_lim)):
            rbuf, roff = table.resolve(buf, off, 7, accept,
                                       oversize=name == "lim")
            body, rlen, meta = (torch.empty(n, dtype=torch.int32,
                                            device="cuda") for _ in range(3))
            look = (lambda lookup=lookup, body=body, rlen=rlen, meta=meta:
                    lookup(*batch, *tab, accept, body.data_ptr(),
                           rlen.data_ptr(), meta.data_ptr(), stream))
            look()
            args[name] = (batch, tab[2], body, rlen, meta, roff, rbuf)
            runs["lookup_" + name] = look
            runs["emit_" + name] = emitter(emit, *args[name])
        return runs, args

    res = {"n": n, "repeats": repeats,
           "device": torch.cuda.get_device_name()}
    # small replies: the timing script's own batch
    image, a_q, srv_q = build_image(_native)
    rng = random.Random(1)
    picks = [(rng.choice(srv_q) if rng.random() < 0.1
              else rng.choice(a_q))[0] for _ in range(n)]
    table = gpuresolve.GpuAnswerTable(image)
    for key, qs in (("plain", picks),
                    ("ext", [query_ext(q) for q in picks])):
        dev = device(qs)  # held here: the launches keep addresses only
        runs, args = launches(table, *dev, 3)
        assert torch.equal(args["ext"][-1], args["lim"][-1])  # rbuf
        assert torch.equal(args["ext"][-2], args["lim"][-2])  # roff
        res[key] = alternate(runs)
        del runs, args
    # large replies: one query in sixteen is a 64-member service
    image, hosts, srv = large_image(_native)
    qs = [rng.choice(srv) if i % 16 == 5 else rng.choice(hosts)
          for i in range(n)]
    table = gpuresolve.GpuAnswerTable(image)
    dev = device(qs)
    runs, args = launches(table, *dev, 1)
    roff, rbuf = args["lim"][-2:]
    lens = roff[1:] - roff[:-1]
    res["large_bytes"] = int(roff[-1])
    res["large_reply"] = int(lens.max())
    assert bool((lens > 0).all()) and res["large_reply"] > 3072
    # emit_ext behind lookup_lim's words: no reply here is truncated
    shapes = {"two_phase": runs["emit_lim"],
              "plain": lambda: runs["emit_lim"](list_above=2 ** 32 - 1),
              "emit_ext": emitter(g.emit_ext, *args["lim"])}
    want = rbuf.clone()
    for k, fn in shapes.items():  # the same bytes from every shape
        rbuf.zero_()
        fn()
        assert torch.equal(rbuf, want), k
    res["large"] = alternate({"lookup_lim": runs["lookup_lim"], **shapes})
    return res


BURSTS = (64, 256, 4096)
OFF = 2 ** 32 - 1  # a threshold nothing exceeds
CHUNKS = (64, 128, 256, 512, 1024)


def bursts(repeats: int) -> dict:
    """The fused burst path with and without `oversize`
    (native/gpu/resolvefusedlim.cpp); see "Oversize bursts" in render()."""
    import time
    from functools import partial

    import torch
    from binder_amd import _gpuresolve as g, _native, gpuresolve

    def device(queries):
        buf = torch.frombuffer(bytearray(b"".join(queries)),
                               dtype=torch.uint8).cuda()
        off = torch.tensor([0] + [len(q) for q in queries]).cumsum(0).to(
            torch.int32).cuda()
        return buf, off

    def spread(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v),
                "max_ms": max(v)}

    def once(fn, sync):
        """Device time between two events around the call, and host time
        until the reply lengths can be read."""
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

    def alternate(runs):
        """{name: (fn, sync)}: the calls in turn, three warm-up rounds."""
        ms = {k: ([], []) for k in runs}
        for r in range(3 + repeats):
            for k, (fn, sync) in runs.items():
                dev, wall = once(fn, sync)
                if r >= 3:
                    ms[k][0].append(dev)
                    ms[k][1].append(wall)
        return {k: {"device": spread(d), "wall": spread(w),
                    "queued": queued(runs[k][0])} for k, (d, w) in ms.items()}

    def packed(out):
        """A burst's replies gathered into query order, with offsets."""
        rbuf, rstart, rlen = out
        roff = torch.zeros(rlen.numel() + 1, dtype=torch.int64, device="cuda")
        roff[1:] = torch.cumsum(rlen, 0)
        at = torch.repeat_interleave(rstart - roff[:-1], rlen.long())
        return rbuf[at + torch.arange(int(roff[-1]), device="cuda")], roff

    def same(out, want, woff):
        got, goff = packed(out)
        assert torch.equal(goff, woff) and torch.equal(got, want)

    res, rng = {}, random.Random(1)
    # 1. the switch where it is not needed: small replies, the first
    # queries of gpuresolve_bench.py's batch (the same draws)
    image, a_q, srv_q = build_image(_native)
    table = gpuresolve.GpuAnswerTable(image)
    picks = [(rng.choice(srv_q) if rng.random() < 0.1
              else rng.choice(a_q))[0] for _ in range(max(BURSTS))]
    res["small"] = {}
    for n in BURSTS:
        buf, off = device(picks[:n])
        ws = {"burst0": (table.burst(n), 0), "burst3": (table.burst(n), 3),
              "lim3": (table.burst(n, oversize=True), 3)}
        for w, accept in ws.values():
            same(w.resolve(buf, off, 7, accept),
                 *table.resolve(buf, off, 7, accept))
        res["small"][str(n)] = alternate({
            k: (partial(w.resolve, buf, off, 7, accept), True)
            for k, (w, accept) in ws.items()})
    # 2. and 3. large replies: the script's large image, and 100 wire
    # replies of 4000 bytes for the copies that get cut
    image, hosts, srv = large_image(_native)
    wires = []
    for i in range(SERVICES):
        name = b"w%d.bench.foo.com" % i
        image.add_reply(name, 1, header(name, 1, 1, 0) + rr(
            b"\xc0\x0c", 16, bytes(4000 - len(name) - 30)))
        wires.append(query(name, 1)[:10] + b"\0\1" + query(name, 1)[12:] +
                     struct.pack(">BHHIH", 0, 41, 4096, 0, 0))
    table = gpuresolve.GpuAnswerTable(image)
    batches = {"services": [rng.choice(srv) if i % 16 == 5
                            else rng.choice(hosts)
                            for i in range(max(BURSTS))],
               "wires": [rng.choice(wires) if i % 16 == 5
                         else rng.choice(hosts) for i in range(max(BURSTS))]}
    shapes = {"plain": (OFF, OFF), "plan": (g.FUSED_LIST_ABOVE, OFF)}
    shapes.update({"chunk%d" % c: (g.FUSED_LIST_ABOVE, c) for c in CHUNKS})
    res["large"], res["deal"] = {}, {k: {} for k in batches}
    res["defaults"] = [g.FUSED_LIST_ABOVE, g.FUSED_CHUNK]
    for n in BURSTS:
        for key, qs in batches.items():
            buf, off = device(qs[:n])
            want, woff = table.resolve(buf, off, 7, 1, oversize=True)
            assert bool((woff[1:] > woff[:-1]).all())
            runs = {}
            for k, (above, chunk) in shapes.items():
                w = table.burst(n, oversize=True)
                w._launch = partial(g.fused_lim, list_above=above,
                                    chunk=chunk)
                same(w.resolve(buf, off, 7, 1), want, woff)
                runs[k] = (partial(w.resolve, buf, off, 7, 1), True)
            deal = alternate(runs)
            res["deal"][key][str(n)] = {k: v["device"]
                                        for k, v in deal.items()}
            if key != "services":
                continue
            ws = table.burst(n, oversize=True)
            same(ws.resolve(buf, off, 7, 1), want, woff)
            res["large"][str(n)] = alternate({
                "resolve": (partial(table.resolve, buf, off, 7, 1,
                                    oversize=True), False),
                "burst": (partial(ws.resolve, buf, off, 7, 1), True)})
            res["large"][str(n)]["bytes"] = int(woff[-1])
    return res


def render_bursts(res, before: str) -> str:
    import re
    parent = {m[1]: (float(m[2]), float(m[3]), float(m[4])) for m in re.finditer(
        r"^\| (\d+) \| burst\.resolve\(\) \| ([\d.]+) \| ([\d.]+) \.\. "
        r"([\d.]+) \|", before, re.M)}
    head = ("| N | call | device median ms | min .. max | wall median ms | "
            "min .. max | queued device ms | queued host ms |\n"
            "|---|---|---|---|---|---|---|---|\n")

    def rows(table, names):
        out = ""
        for n, r in table.items():
            for k, call in names:
                d, w = r[k]["device"], r[k]["wall"]
                out += (f"| {n} | {call} | {d['median_ms']:.4f} | "
                        f"{d['min_ms']:.4f} .. {d['max_ms']:.4f} | "
                        f"{w['median_ms']:.4f} | {w['min_ms']:.4f} .. "
                        f"{w['max_ms']:.4f} | "
                        f"{r[k]['queued']['device_ms']:.4f} | "
                        f"{r[k]['queued']['host_ms']:.4f} |\n")
        return out

    def over(table, a, b):
        return ", ".join(
            "N = %s device %.2f, wall %.2f, queued device %.2f, queued host "
            "%.2f" % (n, r[a]["device"]["median_ms"] /
                      r[b]["device"]["median_ms"],
                      r[a]["wall"]["median_ms"] / r[b]["wall"]["median_ms"],
                      r[a]["queued"]["device_ms"] /
                      r[b]["queued"]["device_ms"],
                      r[a]["queued"]["host_ms"] / r[b]["queued"]["host_ms"])
            for n, r in table.items())
    held = []
    for n, r in res["small"].items():
        med = r["burst0"]["device"]["median_ms"]
        if n not in parent:
            held.append(f"N = {n}: no row to hold {med:.4f} against")
            continue
        lo, hi = parent[n][1:]
        held.append(f"N = {n}: {med:.4f} is "
                    f"{'inside' if lo <= med <= hi else 'outside'} the "
                    f"table's {lo:.4f} .. {hi:.4f} (median {parent[n][0]:.4f})")
    above, chunk = res["defaults"]
    names = [("plain", "one group per reply (both thresholds 2^32 - 1)"),
             ("plan", f"plans above {above} jobs dealt out, no chunks")] + \
        [("chunk%d" % c, f"plans above {above} jobs, chunks of {c} bytes" +
          (" (ships)" if c == chunk else "")) for c in CHUNKS]
    deal = ""
    for key, label in (("services", "one query in sixteen a 64-member "
                        "service"), ("wires", "one query in sixteen a "
                                     "4000-byte wire reply")):
        deal += (f"\n{label[0].upper() + label[1:]}, device ms, median "
                 "(min .. max):\n\n| shape | " + " | ".join(
                     f"N = {n}" for n in res["deal"][key]) + " |\n|---|" +
                 "---|" * len(res["deal"][key]) + "\n")
        for k, name in names:
            deal += f"| {name} | " + " | ".join(
                f"{r[k]['median_ms']:.4f} ({r[k]['min_ms']:.4f} .. "
                f"{r[k]['max_ms']:.4f})"
                for r in res["deal"][key].values()) + " |\n"
    return (
        "\n### Oversize bursts\n\n`table.burst(N, oversize=True).resolve()`, "
        "one launch of `bamd_resolve_fused_lim`. Columns as in the burst "
        "table above; the calls of a table alternate repeat by repeat, "
        "three warm-up rounds, bytes compared with `resolve()`'s before "
        "timing.\n\nThe switch where it is not needed: the small-reply image, "
        "the first N queries of a plain batch. `burst(N)` with `accept=0` "
        "is the call of the burst table above; the other two have "
        "`accept=3` and write the same bytes:\n\n" + head +
        rows(res["small"], (("burst0", "burst(N), accept=0"),
                            ("burst3", "burst(N), accept=3"),
                            ("lim3", "burst(N, oversize=True), accept=3"))) +
        "\n- oversize over default at `accept=3` by the medians: " +
        over(res["small"], "lim3", "burst3") + "\n- `burst(N)` with "
        "`accept=0`, device median, against the burst table's "
        "`burst.resolve()` row: " + "; ".join(held) + "\n\nLarge replies: "
        "the large image above, one query in sixteen a 64-member service "
        "with a 4096-byte OPT record, `accept=1` (" + ", ".join(
            f"{r['bytes']} reply bytes at N = {n}"
            for n, r in res["large"].items()) + "):\n\n" + head +
        rows(res["large"], (("resolve", "resolve(oversize=True)"),
                            ("burst", "burst(N, oversize=True)"))) +
        "\n- burst over resolve() by the medians: " +
        over(res["large"], "burst", "resolve") + "\n\nThe dealing-out: the "
        "same kernel with its two thresholds as launch arguments, on that "
        "batch and on one where the sixteenth query asks for a 4000-byte "
        "wire reply instead (100 such hosts added to the image), every "
        "shape writing the same bytes.\n" + deal + READING)


# what the run recorded in profiles/GPURESOLVE.md showed; the figures in
# it are that run's
READING = "\n" + "\n".join((
    'What these show, in the run recorded here:',
    '',
    '- Where it is not needed the switch costs 2 to 3 % of device time '
    'at every N, less than the spread of either call (their min .. max '
    'overlap), and nothing on the host. `burst(N)` itself lies inside '
    "the burst table's min .. max at all three N: it is the same "
    'kernel.',
    '- On large replies the burst path takes 0.87 to 0.96 of '
    "`resolve(oversize=True)`'s device time, 0.89 to 0.99 when calls "
    "are queued, and a quarter of the host's time per call. It loses "
    'where a single call is waited for: 1.14 to 1.28 of the wall time. '
    "`resolve()`'s wall ends when its total is read, with its emit "
    "still in flight; the burst's ends at a synchronise behind the "
    'whole kernel.',
    '- Dealing out plans above 32 jobs is what pays: 0.52 to 0.53 of '
    'one group per reply on the services batch. Chunks change nothing '
    'there (no head in it is above 64 bytes) and the plan threshold '
    'changes nothing on the wire batch (no plan in it has more than 3 '
    'jobs).',
    '- Chunks pay on the wire batch, modestly: 256 bytes is 0.89 to '
    '0.90 of one group per reply, 512 the same within the spread, 64, '
    '128 and 1024 in between. A 4000-byte copy in one group is 63 '
    'rounds; four such replies per tile in 16 chunks each are one round'
    ' of 64 groups and four rounds of copying. The kernel ships with 32'
    ' jobs and 256 bytes.',
    '- Only the head of a plan is cut. A first version looked at all '
    'jobs of a plan, 131 reads by the one planning lane for a 64-member'
    ' service, and with any chunk size took 0.096 to 0.100 ms on the '
    'services batch against 0.083 to 0.088 with no chunks: more than '
    'chunks save on the wire batch. With the scan limited to the head '
    'the two rows are equal.',
)) + "\n"


def render(res) -> str:
    def rows(key, names):
        return "".join(
            f"| {label} | {res[key][k]['median_ms']:.3f} | "
            f"{res[key][k]['min_ms']:.3f} .. {res[key][k]['max_ms']:.3f} |\n"
            for k, label in names)
    head = "| step | median ms | min .. max ms |\n|---|---|---|\n"
    pair = (("lookup_ext", "bamd_resolve_lookup_ext"),
            ("lookup_lim", "bamd_resolve_lookup_lim"),
            ("emit_ext", "bamd_resolve_emit_ext"),
            ("emit_lim", "bamd_resolve_emit_lim"))

    def ratio(key, a, b):
        return res[key][a]["median_ms"] / res[key][b]["median_ms"]
    return (MARK + "\n`scripts/gpuresolve_oversize_bench.py` on "
            f"{res['device']}: {res['n']} queries, {res['repeats']} repeats "
            "after warm-up, device events around each launch, the launches "
            "of a table alternating repeat by repeat.\n\n"
            "Small replies: the batch and image of the first table above "
            "(no reply above 512 bytes), `accept=3`; the oversize pair "
            "writes the opt-in pair's bytes (compared before timing). "
            "Plain batch:\n\n" + head + rows("plain", pair) +
            "\nThe same names in mixed case with an OPT record:\n\n" + head +
            rows("ext", pair) +
            "\n- oversize over opt-in by the medians: lookup %.2f and emit "
            "%.2f on the plain batch, lookup %.2f and emit %.2f on the EDNS "
            "+ mixed-case batch\n" % (
                ratio("plain", "lookup_lim", "lookup_ext"),
                ratio("plain", "emit_lim", "emit_ext"),
                ratio("ext", "lookup_lim", "lookup_ext"),
                ratio("ext", "emit_lim", "emit_ext")) +
            "\nLarge replies: an image with `max_reply=4096`, 10000 hosts "
            "and 100 SRV services of 64 members; one query in sixteen asks "
            "for a service with a 4096-byte OPT record (the largest reply "
            f"is {res['large_reply']} bytes), the rest for hosts; "
            f"{res['large_bytes']} reply bytes in all. One lookup, then the "
            "emit in three shapes that write the same bytes (compared "
            "before timing): as it ships, with nothing listed (`list_above` "
            "= 2^32 - 1: one 16-lane group walks each reply), and the "
            "opt-in pair's `bamd_resolve_emit_ext`, the plain shape without "
            "the drain loop:\n\n" + head + rows("large", (
                ("lookup_lim", "bamd_resolve_lookup_lim"),
                ("two_phase", "bamd_resolve_emit_lim, two-phase (ships)"),
                ("plain", "bamd_resolve_emit_lim, nothing listed"),
                ("emit_ext", "bamd_resolve_emit_ext"))) +
            "\n- two-phase over plain by the medians: %.2f against the same "
            "kernel with nothing listed, %.2f against "
            "`bamd_resolve_emit_ext`\n" % (
                ratio("large", "two_phase", "plain"),
                ratio("large", "two_phase", "emit_ext")))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--out", type=Path, default=OUT)
    args = ap.parse_args()
    text = args.out.read_text() if args.out.exists() else ""
    before = text.split(MARK)[0]
    section = render(measure(args.n, args.repeats)) + render_bursts(
        bursts(max(25, args.repeats)), before)
    args.out.write_text(before.rstrip("\n") + "\n" + section)
    print(section)
    return 0


if __name__ == "__main__":
    sys.exit(main())
