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
    section = render(measure(args.n, args.repeats))
    text = args.out.read_text() if args.out.exists() else ""
    args.out.write_text(text.split(MARK)[0].rstrip("\n") + "\n" + section)
    print(section)
    return 0


if __name__ == "__main__":
    sys.exit(main())
