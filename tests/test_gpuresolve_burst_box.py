"""The fused single-launch resolve (native/gpu/resolvefused.cpp,
GpuAnswerTable.burst) against the accept test's Python reference and
against resolve() on the same input. Exact bytes; offsets by the layout
contract: packed inside a tile, tiles in claim order."""
from itertools import accumulate

import pytest

from binder_amd import _native
from test_answer_image import wire
from test_gpuresolve_accept_box import (AcceptRef, edns, gr, mixed,  # noqa
                                        mixed_queries)
from test_gpuresolve_box import rnd

pytestmark = pytest.mark.gpu

SIZES = [(0, 1), (1, -1), (1, 0), (1, 1), (3, 5)]  # tiles, plus
SEED = 0xDEADBEEFCAFEF00D


def batch(n):
    """The accept test's mix, with the three replies at the size limit
    asked for under an advertised 522 in place of three misses."""
    qs = mixed_queries(n)
    for j, total in enumerate((501, 502, 512)):
        if 7 * j + 5 < n:
            qs[7 * j + 5] = edns(wire(b"t%d.foo.com" % total, qid=j),
                                 size=522)
    return qs


def tensors(qs, offs=None):
    import torch
    qbuf = torch.frombuffer(bytearray(b"".join(qs)), dtype=torch.uint8)
    offs = offs or list(accumulate(map(len, qs), initial=0))
    return qbuf.cuda(), torch.tensor(offs, dtype=torch.int32).cuda()


def gather(out):
    """(replies, rstart, rlen) as Python values."""
    data = out[0].cpu().numpy().tobytes()
    rstart, rlen = out[1].tolist(), out[2].tolist()
    return [data[s:s + l] if l else b"" for s, l in zip(rstart, rlen)], \
        rstart, rlen


@pytest.fixture(scope="module")
def cases(gr, mixed):
    """One launch per (n, accept), shared by the byte and layout tests."""
    table, done = gr.GpuAnswerTable(mixed.image), {}

    def get(tiles, plus, accept):
        n = tiles * gr.FUSED_TILE + plus
        if (n, accept) not in done:
            qs = batch(n)
            ws = table.burst(n)
            got = gather(ws.resolve(*tensors(qs), SEED, accept))
            done[n, accept] = (table, qs, ws, got)
        return done[n, accept]
    return get


@pytest.mark.parametrize("tiles,plus", SIZES)
@pytest.mark.parametrize("accept", [0, 1, 2, 3])
def test_bytes(gr, mixed, cases, tiles, plus, accept):
    _, qs, ws, (got, _, rlen) = cases(tiles, plus, accept)
    want = [mixed.answer_ext(q, i, SEED, accept) for i, q in enumerate(qs)]
    assert got == want and rlen == [len(w) for w in want]
    assert ws.dropped() == 0
    if len(qs) > 20 and accept & 1:  # 512 + 11 passes 522
        assert [bool(want[i]) for i in (5, 12, 19)] == [True, True, False]


@pytest.mark.parametrize("tiles,plus", SIZES)
@pytest.mark.parametrize("accept", [0, 1, 2, 3])
def test_layout(gr, cases, tiles, plus, accept):
    table, qs, _, (got, rstart, rlen) = cases(tiles, plus, accept)
    T, n, regions = gr.FUSED_TILE, len(qs), []
    for t0 in range(0, n, T):
        served = [i for i in range(t0, min(t0 + T, n)) if rlen[i]]
        if served:
            base = rstart[served[0]]
            assert [rstart[i] for i in served] == list(accumulate(
                (rlen[i] for i in served[:-1]), initial=base))
            regions.append((base, base + sum(rlen[i] for i in served)))
    ends = [0] + [b for _, b in sorted(regions)]
    assert [a for a, _ in sorted(regions)] == ends[:-1]
    assert ends[-1] == sum(rlen)
    if n <= T:
        rbuf, roff = table.resolve(*tensors(qs), SEED, accept)
        assert b"".join(got) == rbuf.cpu().numpy().tobytes()
        assert all(rstart[i] == roff[i] for i in range(n) if rlen[i])


def test_unstaged_tile_and_hostile_offsets(gr, mixed):
    T = gr.FUSED_TILE
    table = gr.GpuAnswerTable(mixed.image)
    ws = table.burst(T + 3)
    long = mixed_queries(T + 3)
    long[1] += b"\0" * (20000 - len(long[1]))  # tile 0 is read unstaged
    qs = mixed_queries(T + 3)
    offs = list(accumulate(map(len, qs), initial=0))
    offs[5] = offs[6] + 3        # a descending pair
    offs[T + 2] = offs[-1] + 100  # past qbuf
    for inp in (tensors(long), tensors(qs, offs)):
        got, _, rlen = gather(ws.resolve(*inp, SEED, 3))
        rbuf, roff = table.resolve(*inp, SEED, 3)
        data, roff = rbuf.cpu().numpy().tobytes(), roff.tolist()
        assert got == [data[a:b] for a, b in zip(roff, roff[1:])]
        assert 0 < sum(map(bool, rlen)) < T
    assert not rlen[5] and not rlen[T + 1] and not rlen[T + 2]


def test_job_pool_passes(gr):
    """A tile of 64-member services, 131 copy jobs each: more than the
    kernel's job pool holds at once, so the tile is written in passes."""
    ref, n = AcceptRef(), gr.FUSED_TILE + 1
    mem = [(rnd(2 + m % 3, m), rnd(1 + m % 2, 300 + m)) for m in range(64)]
    ref.service(b"_x._tcp.s.foo", 33, rnd(37, 7), mem)
    ref.service(b"s.foo", 1, rnd(25, 8), [(a, b"") for a, _ in mem])
    ref.reply(b"w.foo", 1, rnd(45, 9))
    qs = [[edns(wire(b"_X._tcp.s.foo", 33, qid=i)), wire(b"w.foo", qid=i),
           edns(wire(b"S.foo", qid=i))][i % 3] for i in range(n)]
    got = gather(gr.GpuAnswerTable(ref.image).burst(n).resolve(
        *tensors(qs), SEED, 3))[0]
    assert all(got) and got == [ref.answer_ext(q, i, SEED, 3)
                                for i, q in enumerate(qs)]


def test_capacity(gr, mixed):
    import torch
    table, qs = gr.GpuAnswerTable(mixed.image), batch(3 * gr.FUSED_TILE + 5)
    want = [mixed.answer_ext(q, i, SEED, 3) for i, q in enumerate(qs)]
    cap = sum(map(len, want)) // 2
    big = torch.full((cap + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    ws = table.burst(len(qs), rbuf=big[:cap])
    got, rstart, rlen = gather(ws.resolve(*tensors(qs), SEED, 3))
    served = [i for i in range(len(qs)) if rlen[i]]
    assert served and all(got[i] == want[i] for i in served)
    assert all(0 <= rstart[i] and rstart[i] + rlen[i] <= cap for i in served)
    assert big[cap:].tolist() == [0xAA] * 64
    assert ws.dropped() > 0
    assert len(served) + ws.dropped() == sum(map(bool, want))


def test_reuse_and_rebuild(gr):
    ref = AcceptRef()
    for i in range(40):
        ref.reply(b"old%d.foo.com" % i, 1, rnd(30 + i, i))
    table = gr.GpuAnswerTable(ref.image)
    ws = table.burst(700)
    for lo, hi in ((0, 40), (35, 50)):  # the second call starts at 0 again
        qs = [wire(b"old%d.foo.com" % i, qid=i) for i in range(lo, hi)]
        got, rstart, _ = gather(ws.resolve(*tensors(qs), 3))
        assert got == [ref.answer(q, i, 3) for i, q in enumerate(qs)]
        assert rstart[0] == 0
    delta = _native.AnswerDelta()
    for i in range(table.cap // 2 + 1):
        name, reply = b"new%d.foo.com" % i, rnd(20 + i % 50, 1000 + i)
        delta.upsert_reply(name, 1, reply)
        ref.table[name, 1] = (reply, None)
    table.apply(delta)
    assert table.compactions == 1
    qs = [wire(b"new%d.foo.com" % i, qid=i) for i in range(0, 513, 3)] + \
        [wire(b"old7.foo.com")]
    got = gather(ws.resolve(*tensors(qs), 3))[0]
    assert all(got) and got == [ref.answer(q, i, 3)
                                for i, q in enumerate(qs)]


def test_no_host_round_trip(gr, mixed):
    import torch
    table, qs = gr.GpuAnswerTable(mixed.image), batch(70)
    qbuf, qoff = tensors(qs)
    ws = table.burst(70)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ws.resolve(qbuf, qoff, SEED, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert gather(out)[0] == [mixed.answer_ext(q, i, SEED, 3)
                              for i, q in enumerate(qs)]
