"""burst(..., oversize=True) (native/gpu/resolvefusedlim.cpp) on an image
with a 4096-byte ceiling, against the oversize test's Python reference
LimRef.answer_lim, and for one tile against resolve(..., oversize=True).
Exact bytes; offsets by the burst path's layout contract."""
from itertools import accumulate

import pytest

from test_answer_image import wire
from test_gpuresolve_accept_box import ANYCASE, EDNS, edns, gr  # noqa: F401
from test_gpuresolve_box import dotted, rnd
from test_gpuresolve_burst_box import gather
from test_gpuresolve_oversize_box import (LimRef, fill, members,
                                          mixed_queries, tensors)

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEFCAFEF00D


@pytest.fixture(scope="module")
def big():
    return fill(LimRef(), True)


def burst(gr, ref, qs, accept, seed=SEED, rbuf=None):
    """One oversize burst. With the default buffer every reply is the
    reference's; one tile also has resolve()'s bytes and offsets."""
    table = gr.GpuAnswerTable(ref.image)
    ws = table.burst(len(qs), rbuf=rbuf, oversize=True)
    got, rstart, rlen = gather(ws.resolve(*tensors(qs), seed, accept))
    want = [ref.answer_lim(q, i, seed, accept) for i, q in enumerate(qs)]
    if rbuf is None:
        assert ws.rbuf.numel() == len(qs) * 4096
        assert rlen == [len(w) for w in want] and got == want
        assert ws.dropped() == 0
        if len(qs) <= gr.FUSED_TILE:
            data, roff = table.resolve(*tensors(qs), seed, accept,
                                       oversize=True)
            assert b"".join(got) == data.cpu().numpy().tobytes()
            assert all(s == o for s, o, n in zip(rstart, roff.tolist(), rlen)
                       if n)
    return want, got, rstart, rlen, ws


def test_size_edges(gr, big):
    stored, sizes = [512, 513, 4085, 4086, 4096], \
        [0, 512, 523, 524, 4095, 4096, 65535]
    qs, lens = [], []
    for t in stored:
        q = wire(b"t%d.foo.com" % t, qid=t)
        qs += [q] + [edns(q, size=s) for s in sizes]
        limits = [512] + [min(max(s, 512), 4096) for s in sizes]
        lens += [t + e if t + e <= lim else len(q) + e
                 for lim, e in zip(limits, [0] + [11] * 7)]
    assert len(qs) <= gr.FUSED_TILE
    assert [len(w) for w in burst(gr, big, qs, EDNS)[0]] == lens


@pytest.mark.parametrize("seed", [0, SEED])
@pytest.mark.parametrize("n", [9, 33, 64])
def test_services(gr, n, seed):
    """9 members stay with their group, 33 and 64 are dealt out; the
    same query twice draws two orders."""
    assert 2 * 9 + 3 <= gr._gpuresolve.FUSED_LIST_ABOVE < 2 * 33
    ref = LimRef()
    ref.service(b"_x._tcp.s.foo", 33, rnd(37, 7), members(n))
    ref.service(b"s.foo", 1, rnd(25, 8), [(a, b"") for a, _ in members(n)])
    ref.reply(b"w.foo", 1, rnd(45, 9))
    qs = [wire(b"_x._tcp.s.foo", 33, qid=1), wire(b"s.foo", qid=2, flags=0),
          wire(b"w.foo")]
    want = burst(gr, ref, ([edns(q, size=4096) for q in qs] + qs) * 2, EDNS,
                 seed)[0]
    assert all(want) and want[0] != want[6]
    assert sorted(want[0]) == sorted(want[6])


@pytest.mark.parametrize("tiles,plus", [(0, 1), (1, 1), (3, 5)])
@pytest.mark.parametrize("accept", [0, EDNS | ANYCASE])
def test_mixed_batch_and_layout(gr, big, accept, tiles, plus):
    T = gr.FUSED_TILE
    n = tiles * T + plus
    want, _, rstart, rlen, _ = burst(gr, big, mixed_queries(n), accept, 5)
    assert [bool(w) for w in want] == [
        (i % 10 in (0, 1, 8)) or (accept != 0 and i % 10 != 3)
        for i in range(n)]
    regions = []  # packed in query order in a tile; tiles disjoint, no gaps
    for t0 in range(0, n, T):
        served = [i for i in range(t0, min(t0 + T, n)) if rlen[i]]
        if not served:
            continue
        base = rstart[served[0]]
        assert [rstart[i] for i in served] == list(accumulate(
            (rlen[i] for i in served[:-1]), initial=base))
        regions.append((base, base + sum(rlen[i] for i in served)))
    ends = [0] + [b for _, b in sorted(regions)]
    assert [a for a, _ in sorted(regions)] == ends[:-1]
    assert ends[-1] == sum(rlen)


def test_pool_passes_with_listed_replies(gr, big):
    """More jobs than the pool holds and about 250 KiB in one tile: 64
    members in mixed case, and 4085 stored bytes that make a 4096-byte
    reply with the tail."""
    qs = [[edns(wire(b"_S._tcp.M64.foo.com", 33, qid=i), size=4096),
           edns(wire(b"t4085.foo.com", qid=i), size=4096),
           edns(wire(b"_s._TCP.m64.FOO.com", 33, qid=i), size=4096)][i % 3]
          for i in range(gr.FUSED_TILE + 1)]
    want = burst(gr, big, qs, EDNS | ANYCASE)[0]
    assert len(want[1]) == 4096 and all(len(w) > 3800 for w in want)
    assert sum(map(len, want[:gr.FUSED_TILE])) > 250_000


@pytest.mark.parametrize("staged", [True, False])
def test_truncated_longest_name(gr, staged):
    ref, key = LimRef(), dotted(253)
    ref.reply(key, 1, b"\0\0\x84\x03" + rnd(8, 1) + rnd(600, 2))
    asked = key[:100] + key[100:].upper()
    qs = [wire(asked, qid=0x1234, flags=0x0100),
          wire(asked, qid=0x4321, flags=0),
          edns(wire(asked, qid=7), size=600),
          wire(b"absent.foo") + bytes(0 if staged else 20000)]
    want = burst(gr, ref, qs, EDNS | ANYCASE)[0]
    assert [len(w) for w in want] == [271, 271, 282, 0]
    assert want[0][:12] == b"\x12\x34\x87\x03\0\1" + bytes(6)
    assert burst(gr, ref, qs, 0)[0] == [b""] * 4


def test_capacity(gr, big):
    import torch
    qs = mixed_queries(3 * gr.FUSED_TILE + 5)
    cap = sum(len(big.answer_lim(q, i, SEED, 3))
              for i, q in enumerate(qs)) // 2
    guard = torch.full((cap + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    want, got, rstart, rlen, ws = burst(gr, big, qs, 3, rbuf=guard[:cap])
    served = [i for i in range(len(qs)) if rlen[i]]
    assert served and all(got[i] == want[i] for i in served)
    assert all(0 <= rstart[i] and rstart[i] + rlen[i] <= cap for i in served)
    assert guard[cap:].tolist() == [0xAA] * 64
    assert ws.dropped() > 0
    assert len(served) + ws.dropped() == sum(map(bool, want))


def test_no_host_round_trip(gr, big):
    import torch
    qs = mixed_queries(gr.FUSED_TILE + 6)
    qbuf, qoff = (t.cuda() for t in tensors(qs))
    ws = gr.GpuAnswerTable(big.image).burst(len(qs), oversize=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ws.resolve(qbuf, qoff, SEED, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert gather(out)[0] == [big.answer_lim(q, i, SEED, 3)
                              for i, q in enumerate(qs)]
