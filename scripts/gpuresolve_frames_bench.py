#!/usr/bin/env python3
"""Time the GPU batch resolver's frame bursts (GpuAnswerTable.frames,
native/gpu/resolveframes.cpp) and record the result as the last section,
"## Frames", of profiles/GPURESOLVE.md.

The traffic is the oversize test's image and its mixed_queries, wrapped
as UDP QUERY frames, N = 64, 512 and 4096. Two paths answer it and
alternate repeat by repeat:

  frames    FrameBurst.resolve on the frame run and its index
  burst     burst(N, oversize=True).resolve on the DNS messages already
            extracted, which is what the frame run costs without the
            new kernel; the host's share of that path, extracting the
            messages and framing the replies with numpy gathers, is
            timed beside it

Both write the same DNS bytes (compared first). Device events around
each call on buffers allocated beforehand, three warm-up rounds, median
and min..max of the repeats; host time per call over 100 queued calls.
Fails without a GPU.
"""
from __future__ import annotations

import argparse
import statistics
import struct
import sys
import time
from functools import partial
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]
OUT = REPO / "profiles" / "GPURESOLVE.md"
MARK = "\n## Frames\n"
SIZES = (64, 512, 4096)


def spread(v):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def measure(repeats: int) -> str:
    import numpy as np
    import torch
    from binder_amd import _native, gpuresolve
    from test_gpuresolve_oversize_box import LimRef, fill, mixed_queries

    def once(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), (time.perf_counter() - t) * 1e3

    def queued(fn, calls=100):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        host = (time.perf_counter() - t) * 1e3 / calls
        torch.cuda.synchronize()
        return host

    def gather(src, starts, lens):
        """src[starts[i]:starts[i] + lens[i]] end to end, and offsets."""
        off = np.concatenate(([0], np.cumsum(lens)))
        return src[np.repeat(starts - off[:-1], lens) +
                   np.arange(off[-1])], off

    table = gpuresolve.GpuAnswerTable(fill(LimRef(), True).image)
    rows, notes = [], []
    for n in SIZES:
        qs = mixed_queries(n)
        data = b"".join(
            struct.pack("<BBIIBBH16x", 0xB5, 1, 24 + len(q), i, 4, 0, 5353) + q
            for i, q in enumerate(qs))
        foff, consumed, _ = _native.frame_index(data, n)
        assert consumed == len(data)
        host = np.frombuffer(data, dtype=np.uint8)
        hoff = np.frombuffer(foff, dtype=np.int32).astype(np.int64)

        def extract():
            return gather(host, hoff[:-1] + 30, np.diff(hoff) - 30)

        def reframe(rbuf, rstart, rlen):
            """REPLY frames from a burst's read-back replies."""
            keep = rlen > 0
            out, off = gather(rbuf, rstart[keep] - 10, rlen[keep] + 10)
            head = np.zeros((int(keep.sum()), 10), dtype=np.uint8)
            head[:, 0], head[:, 1] = 0xB5, 2
            head[:, 2:6] = (rlen[keep] + 4).astype("<u4").view(
                np.uint8).reshape(-1, 4)
            head[:, 6:10] = host[(hoff[:-1][keep] + 6)[:, None] +
                                 np.arange(4)]
            out[off[:-1][:, None] + np.arange(10)] = head
            return out

        qbuf, qoff = extract()
        dev = [torch.from_numpy(a.copy()).cuda()
               for a in (host, hoff.astype(np.int32), qbuf,
                         qoff.astype(np.int32))]
        fw, bw = table.frames(n), table.burst(n, oversize=True)
        frames = partial(fw.resolve, dev[0], dev[1], 7, 3)
        burst = partial(bw.resolve, dev[2], dev[3], 7, 3)
        # the same DNS bytes, and the same REPLY frames once framed
        f_out, b_out = frames(), burst()
        b = [t.cpu().numpy() for t in b_out]
        f = [t.cpu().numpy() for t in f_out]
        assert (f[2] == np.where(b[2] > 0, b[2] + 10, 0)).all()
        padded = np.concatenate((np.zeros(10, np.uint8), b[0]))
        framed = reframe(padded, b[1] + 10, b[2])
        served = f[2] > 0
        mine, _ = gather(f[0], f[1][served], f[2][served])
        assert (mine == framed).all() and fw.end() == len(framed)
        ms = {"frames": ([], []), "burst": ([], [])}
        for r in range(3 + repeats):
            for k, fn in (("frames", frames), ("burst", burst)):
                d, w = once(fn)
                if r >= 3:
                    ms[k][0].append(d)
                    ms[k][1].append(w)
        hx, hf = [], []
        for _ in range(repeats):
            t = time.perf_counter()
            extract()
            hx.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            reframe(padded, b[1] + 10, b[2])
            hf.append((time.perf_counter() - t) * 1e3)
        for k, fn in (("frames", frames), ("burst", burst)):
            rows.append("| %d | %s | %s | %s | %.4f | %s |" % (
                n, k, spread(ms[k][0]), spread(ms[k][1]), queued(fn),
                "-" if k == "frames" else "%s + %s" % (spread(hx),
                                                       spread(hf))))
        notes.append("N = %d: device %.2f, wall %.2f (%d of %d frames "
                     "served, %d reply bytes)" % (
                         n, statistics.median(ms["frames"][0]) /
                         statistics.median(ms["burst"][0]),
                         statistics.median(ms["frames"][1]) /
                         statistics.median(ms["burst"][1]),
                         int(served.sum()), n, fw.end()))
    return (
        MARK + "\n`scripts/gpuresolve_frames_bench.py` on %s: "
        "`table.frames(N).resolve()`, one launch of `bamd_resolve_frames`, "
        "on N UDP QUERY frames of the oversize test's `mixed_queries` "
        "(`accept=3`), against `table.burst(N, oversize=True).resolve()` on "
        "the DNS messages already extracted. %d repeats after three "
        "warm-up rounds, the two calls alternating; ms, median (min .. "
        "max). Device: events around the call. Wall: one call and a "
        "synchronise. Host per call: 100 calls queued without a wait. "
        "Extract + frame: what the burst path leaves to the host, here "
        "as numpy gathers over the whole batch (one for the messages, one "
        "for the replies with their 10-byte headers), without the copies "
        "to and from the device.\n\n"
        "| N | call | device | wall | host per call | extract + frame |\n"
        "|---|---|---|---|---|---|\n" % (torch.cuda.get_device_name(0),
                                         repeats) +
        "\n".join(rows) + "\n\n- frames over burst by the medians: " +
        "; ".join(notes) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", type=Path, default=OUT)
    args = ap.parse_args()
    before = OUT.read_text().split(MARK)[0]
    section = measure(args.repeats)
    args.out.write_text(before.rstrip("\n") + "\n" + section)
    print(section)
    return 0


if __name__ == "__main__":
    sys.exit(main())
