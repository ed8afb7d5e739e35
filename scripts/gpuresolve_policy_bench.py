#!/usr/bin/env python3
"""Time the GPU batch resolver's policy pair (resolve(oversize=True,
policy=ZonePolicy(b"foo.com")), native/gpu/resolvepolicy.cpp) and record
the result as the last section, "## Policy", of profiles/GPURESOLVE.md.

Cost of the switch: gpuresolve_bench.py's image and its 1 000 000
queries, none of which is a policy query. The oversize pair and the
policy pair run on the same buffers, alternating repeat by repeat, and
write the same bytes (compared first). The oversize pair is in the
rotation twice, so that its own run-to-run spread stands next to the
ratio; the policy lookup is there once more with a tally.

What it buys: the same batch with every second query turned into an
AAAA query for the same name, every query with an OPT record,
accept=ACCEPT_EDNS. Both pairs again; the share of the batch that is
served, and the device time of lookup + emit per query.

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
from gpuresolve_bench import OUT, build_image  # noqa: E402

MARK = "\n## Policy\n"
ZONE = b"foo.com"
OPT = struct.pack(">BHHIH", 0, 41, 1232, 0, 0)


def measure(n: int, repeats: int) -> dict:
    import torch
    from binder_amd import _gpuresolve as g, _native, gpuresolve

    stream = torch.cuda.current_stream().cuda_stream
    policy = gpuresolve.ZonePolicy(ZONE)
    zone = (policy._dev.data_ptr(), len(policy.wire))

    def alternate(runs):
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

    def launches(table, queries, accept):
        """Both pairs' launches on one batch, each pair with buffers of
        its own, filled by one resolve(); and the share each serves."""
        buf = torch.frombuffer(bytearray(b"".join(queries)),
                               dtype=torch.uint8).cuda()
        off = torch.tensor([0] + [len(q) for q in queries]).cumsum(0).to(
            torch.int32).cuda()
        batch = (buf.data_ptr(), off.data_ptr(), buf.numel(), n)
        tab = (table._slots.data_ptr(), table.cap, table._arena.data_ptr())
        tally = torch.zeros(g.TALLY_WORDS, dtype=torch.int64, device="cuda")
        runs, out, keep = {}, {}, [buf, off, tally]
        for name in ("lim", "pol"):
            rbuf, roff = table.resolve(buf, off, 7, accept, oversize=True,
                                       policy=policy if name == "pol"
                                       else None)
            body, rlen, meta = (torch.empty(n, dtype=torch.int32,
                                            device="cuda") for _ in range(3))
            cols = (body.data_ptr(), rlen.data_ptr(), meta.data_ptr())
            if name == "lim":
                look = (lambda cols=cols:
                        g.lookup_lim(*batch, *tab, accept, *cols, stream))
            else:
                look = (lambda cols=cols, t=0:
                        g.lookup_pol(*batch, *tab, accept, *zone, *cols, t,
                                     stream))
                runs["lookup_pol_tally"] = (lambda look=look:
                                            look(t=tally.data_ptr()))
            look()
            emit = g.emit_lim if name == "lim" else g.emit_pol
            runs["lookup_" + name] = look
            runs["emit_" + name] = (
                lambda emit=emit, cols=cols, roff=roff, rbuf=rbuf:
                emit(*batch, tab[2], *cols, roff.data_ptr(), rbuf.data_ptr(),
                     7, stream))
            out[name] = (rbuf, roff)
            keep += [body, rlen, meta]
        for k in ("lookup_lim", "emit_lim"):  # a second turn: the spread
            runs[k + "_again"] = runs[k]
        served = {k: float((roff[1:] > roff[:-1]).sum()) / n
                  for k, (_, roff) in out.items()}
        return runs, out, served, keep

    res = {"n": n, "repeats": repeats,
           "device": torch.cuda.get_device_name()}
    image, a_q, srv_q = build_image(_native)
    rng = random.Random(1)
    picks = [(rng.choice(srv_q) if rng.random() < 0.1
              else rng.choice(a_q))[0] for _ in range(n)]
    table = gpuresolve.GpuAnswerTable(image)
    # 1. no policy query in the batch: the same bytes from both pairs
    runs, out, served, keep = launches(table, picks, 0)
    assert torch.equal(out["lim"][0], out["pol"][0])
    assert torch.equal(out["lim"][1], out["pol"][1]) and served["pol"] == 1
    res["switch"] = alternate(runs)
    del runs, out, keep
    # 2. a dual-stack stub's capture: an AAAA for every other name
    mixed = [q[:10] + b"\0\1" + q[12:-4] +
             (b"\0\x1c" if i % 2 else q[-4:-2]) + q[-2:] + OPT
             for i, q in enumerate(picks)]
    runs, out, served, keep = launches(table, mixed, gpuresolve.ACCEPT_EDNS)
    res["served"] = served
    res["buys"] = alternate(runs)
    return res


def render(res) -> str:
    head = "| step | median ms | min .. max ms |\n|---|---|---|\n"
    names = (("lookup_lim", "bamd_resolve_lookup_lim"),
             ("lookup_lim_again", "bamd_resolve_lookup_lim, second turn"),
             ("lookup_pol", "bamd_resolve_lookup_pol"),
             ("lookup_pol_tally", "bamd_resolve_lookup_pol with a tally"),
             ("emit_lim", "bamd_resolve_emit_lim"),
             ("emit_lim_again", "bamd_resolve_emit_lim, second turn"),
             ("emit_pol", "bamd_resolve_emit_pol"))

    def rows(key):
        return "".join(
            f"| {label} | {res[key][k]['median_ms']:.3f} | "
            f"{res[key][k]['min_ms']:.3f} .. {res[key][k]['max_ms']:.3f} |\n"
            for k, label in names)

    def ratio(key, a, b):
        return res[key][a]["median_ms"] / res[key][b]["median_ms"]

    def against_spread(key, step):
        r, own = ratio(key, step + "_pol", step + "_lim"), \
            ratio(key, step + "_lim_again", step + "_lim")
        lim = res[key][step + "_lim"]
        lo, hi = lim["min_ms"] / lim["median_ms"], \
            lim["max_ms"] / lim["median_ms"]
        where = "inside" if lo <= r <= hi else "outside"
        return (f"{step} {r:.3f} (the oversize {step}'s second turn over "
                f"its first: {own:.3f}; its min .. max over its median: "
                f"{lo:.3f} .. {hi:.3f}, so the ratio is {where} its spread)")

    def per_query(key, pair):
        ms = res[key]["lookup_" + pair]["median_ms"] + \
            res[key]["emit_" + pair]["median_ms"]
        return ms * 1e6 / res["n"]

    s = res["served"]
    return (MARK + "\n`scripts/gpuresolve_policy_bench.py` on "
            f"{res['device']}: {res['n']} queries, {res['repeats']} repeats "
            "after warm-up, device events around each launch, the launches "
            "of a table alternating repeat by repeat. Zone `foo.com`.\n\n"
            "Cost of the switch: the batch and image of the first table "
            "above, `accept=0`. No query in it is a policy query, and the "
            "policy pair writes the oversize pair's bytes (compared before "
            "timing). The oversize pair is the parent's code and takes two "
            "turns per round:\n\n" + head + rows("switch") +
            "\n- policy over oversize by the medians: " +
            against_spread("switch", "lookup") + "; " +
            against_spread("switch", "emit") + "\n- the tally costs "
            "%.3f of the policy lookup without one\n" % ratio(
                "switch", "lookup_pol_tally", "lookup_pol") +
            "\nWhat it buys: the same batch with every second query turned "
            "into an AAAA query for the same name and an OPT record behind "
            "every query, `accept=ACCEPT_EDNS`. The oversize pair serves "
            f"{100 * s['lim']:.1f} % of it, the policy pair "
            f"{100 * s['pol']:.1f} %:\n\n" + head + rows("buys") +
            "\n- lookup + emit by the medians: %.2f ns per query of the "
            "batch with `policy`, %.2f ns without; per served query %.2f ns "
            "and %.2f ns\n" % (
                per_query("buys", "pol"), per_query("buys", "lim"),
                per_query("buys", "pol") / s["pol"],
                per_query("buys", "lim") / s["lim"]) + READING)


# what the run recorded in profiles/GPURESOLVE.md showed; the figures in
# it are that run's
READING = "\n" + "\n".join((
    'What these show, in the run recorded here:',
    '',
    '- The switch is not free in the lookup: 1.11 to 1.13 of the '
    'oversize lookup over three runs, against a spread of that lookup '
    'of about 1 % either way. The policy lookup hops over the labels to '
    'the type and holds the name against the zone before it hands a '
    'query for the table to `resolveOneExtT<true>`, which walks the '
    'same labels again byte by byte. Both walks are chains of dependent '
    'LDS byte reads, which is presumably what the lookup waits for more '
    'than for its probe; that was not profiled. Leaving out the hops '
    'that check the label boundary changed '
    'nothing (1.112 with them in one run, 1.126 without them in the '
    'next), so they stay for every zone. One walk '
    'that serves both would need the decisions inside '
    '`resolveOneExtT`, which the other kernels share; it is left as it '
    'is.',
    '- The emit is 1.01 of the oversize emit in all three runs, at the '
    "edge of that emit's spread: outside its min .. max in two runs, "
    'inside in the one recorded, where one repeat of the oversize emit '
    'ran 2.4 % long. It tests the metadata word once more per reply.',
    '- The tally adds 2 % to the policy lookup.',
    '- On the stub batch the policy pair serves all of it and the '
    'oversize pair half. Per query of the batch the policy pair takes '
    '1.14 of the time; per served query 0.57. A policy query is not '
    'cheaper than a hit in the lookup (0.34 ms for the half-and-half '
    'batch, 0.33 ms for a batch of hits): it takes no probe and no '
    'arena read, but walks its name twice. It is far cheaper in the '
    'emit: the half million policy replies add 0.02 ms to the 0.39 ms '
    'of the half million hits.',
)) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--out", type=Path, default=OUT)
    args = ap.parse_args()
    text = args.out.read_text() if args.out.exists() else ""
    section = render(measure(args.n, args.repeats))
    args.out.write_text(text.split(MARK)[0].rstrip("\n") + "\n" + section)
    print(section)
    return 0


if __name__ == "__main__":
    sys.exit(main())
