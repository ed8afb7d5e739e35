"""Device table updates (native/gpu/update.cpp, GpuAnswerTable.apply)
against a plain dict updated serially: after every apply() one query
per key ever touched, and the untouched rest, must come back with the
exact reply bytes or None."""
import random
import struct

import pytest

from binder_amd import _native
from test_answer_delta import covers
from test_answer_image import wire
from test_gpuresolve_box import Ref, rnd

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED5EED


@pytest.fixture(scope="module")
def gr():
    from binder_amd import gpuresolve
    return gpuresolve


class Live:
    """A GpuAnswerTable and the dict that mirrors it (Ref.table)."""

    def __init__(self, gr, ref=None, **kw):
        self.ref = ref or Ref()
        self.t = gr.GpuAnswerTable(self.ref.image, **kw)
        self.keys = set(self.ref.table)

    def delta(self, ops):
        """(domain,) invalidates, (name, qtype, reply) and (name, qtype,
        head, members) upsert; the dict follows call by call."""
        d, tab = _native.AnswerDelta(), self.ref.table
        for op in ops:
            if len(op) == 1:
                d.invalidate(op[0])
                for k in [k for k in tab if covers(op[0], k)]:
                    del tab[k]
                self.keys.add((op[0], 1))
            else:
                (d.upsert_reply if len(op) == 3 else d.upsert_service)(*op)
                tab[op[:2]] = (op[2], op[3] if len(op) == 4 else None)
                self.keys.add(op[:2])
        return d

    def apply(self, ops):
        self.t.apply(self.delta(ops))
        self.check()

    def check(self):
        qs = [wire(name, qtype, qid=i & 0xFFFF)
              for i, (name, qtype) in enumerate(sorted(self.keys))]
        want = [self.ref.answer(q, i, SEED) or None
                for i, q in enumerate(qs)]
        assert self.t.resolve_list(qs, SEED) == want
        return want


def base():
    """Per i: a host, and a domain with an A entry and two SRV entries
    on its hash."""
    ref = Ref()
    for i in range(129):
        ref.reply(b"r%d.foo.com" % i, 1, rnd(40, i))
        ref.reply(b"d%d.svc.foo" % i, 1, rnd(30, 1000 + i))
        ref.reply(b"_a._tcp.d%d.svc.foo" % i, 33, rnd(50, 2000 + i))
        ref.service(b"_b._udp.d%d.svc.foo" % i, 33, rnd(20, 3000 + i),
                    [(rnd(5, i), rnd(3, i + 1)), (rnd(4, i + 2), b"")])
    return ref


@pytest.mark.parametrize("rot", range(5))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_apply_against_model(gr, n, rot):
    """n invalidations and n upserts in one delta, n around one
    workgroup of ops (64) and past two. Upsert i is, by (i + rot) % 5: a
    longer replacement, a shorter one, a new key, an invalidate and
    re-upsert of one key, a service body. Invalidation i is that
    re-upsert's, or a domain with an A and two SRV entries, or absent."""
    assert gr.OP_BLOCK + 1 == 65
    live = Live(gr, base(), reserve_bytes=1 << 17)
    inval, ups = [], []
    for i in range(n):
        kind, host = (i + rot) % 5, b"r%d.foo.com" % i
        if kind == 3:
            inval.append((host,))
        else:
            inval.append((b"d%d.svc.foo" % i,) if i % 2 == 0
                         else (b"absent%d.foo.com" % i,))
        if kind == 2:
            ups.append((b"new%d.foo.com" % i, 1, rnd(33 + i % 7, 4000 + i)))
        elif kind == 4:
            mem = [(rnd(3 + m, m + i), rnd(m % 3, 77 + m)) for m in range(5)]
            ups.append((b"_w._tcp." + host, 33, rnd(24, 5000 + i), mem))
        else:
            ups.append((host, 1, rnd(90 if kind == 0 else 20, 6000 + i)))
    before = live.t.stats()
    live.apply(inval + ups)
    after = live.t.stats()
    assert after["entries"] == len(live.ref.table)
    assert after["compactions"] == 0 and after["slots"] == before["slots"]
    assert after["tombstones"] == before["entries"] + sum(
        1 for i in range(n) if (i + rot) % 5 >= 2) - after["entries"]
    live.t.compact()
    live.check()
    assert live.t.stats()["tombstones"] == 0


@pytest.mark.parametrize("wrap", [False, True])
def test_chains(gr, wrap):
    """Five entries with one home (or homes in the last two of 1024
    slots, so the run wraps to slot 0): a tombstone in the middle keeps
    the later ones reachable, a new key of that home lands behind them,
    and the last one is replaced in place."""
    ref = Ref()
    ref.reply(b"seed", 1, rnd(12, 0))  # brings the 1024 slots
    homes = {}
    for i in range(5000):
        homes.setdefault(ref.image.home_slot(b"h%d" % i, 1), []).append(
            b"h%d" % i)
    if wrap:
        names = (homes.get(1022, []) + homes.get(1023, []))[:6]
    else:
        names = next(v for h, v in homes.items() if len(v) >= 6
                     and h < 1000)[:6]
    assert len(names) == 6
    for i, name in enumerate(names[:5]):
        ref.reply(name, 1, rnd(20 + i, i))
    live = Live(gr, ref, reserve_bytes=4096)
    live.keys.add((names[5], 1))
    assert live.check().count(None) == 1
    live.apply([(names[2],)])
    live.apply([(names[5], 1, rnd(31, 50))])
    live.apply([(names[4], 1, rnd(77, 51))])
    assert live.check().count(None) == 1  # only the invalidated name
    st = live.t.stats()
    assert (st["slots"], st["tombstones"], st["entries"]) == (1024, 1, 6)


@pytest.mark.parametrize("start", [0, 400])
def test_growth_and_churn(gr, start):
    ref = Ref()
    for i in range(start):
        ref.reply(b"k%d.foo.com" % i, 1, rnd(30 + i % 9, i))
    live = Live(gr, ref)
    slots0, n = live.t.stats()["slots"], start
    assert slots0 == (1024 if start else 0)
    while n <= 512:
        live.apply([(b"k%d.foo.com" % i, 1, rnd(30 + i % 9, i))
                    for i in range(n, n + 64)])
        n += 64
    st = live.t.stats()
    assert st["entries"] == n and st["slots"] > max(slots0, 2 * n - 1)
    rng, seen = random.Random(start), st["compactions"]
    for r in range(40):
        ops = []
        for i in rng.sample(range(128), 64):
            name = b"k%d.foo.com" % i
            ops.append((name,) if rng.random() < 0.4 else
                       (name, 1, rnd(rng.randrange(12, 200), r * 128 + i)))
        live.apply(ops)
        st = live.t.stats()
        assert 2 * (st["entries"] + st["tombstones"]) <= st["slots"]
    assert st["compactions"] > seen
    live.t.compact()
    st = live.t.stats()
    assert st["tombstones"] == 0 and st["dead_bytes"] == 0
    assert st["entries"] == len(live.ref.table)
    live.check()


def test_untrusted_offsets(gr):
    """The launchers with one descending uoff entry and one ioff entry
    beyond ibuf: the ops whose span or predecessor is that entry are
    left unapplied, the rest are applied, nothing else changes."""
    import torch
    from binder_amd import _gpuresolve
    live = Live(gr, base(), reserve_bytes=1 << 16)
    t, ent0 = live.t, live.t.stats()["entries"]
    inval = [(b"r%d.foo.com" % i,) for i in range(6)]
    ups = [(b"new%d.foo.com" % i, 1, rnd(40 + i, i)) for i in range(6)]
    p = live.delta(inval + ups).pack()
    ioff = list(struct.unpack("<7i", p["ioff"]))
    uoff = list(struct.unpack("<7i", p["uoff"]))
    ioff[3] = len(p["ibuf"]) + 5
    uoff[2] = uoff[1] - 3
    # the model takes back what the bad entries leave unapplied; the
    # delta packs domains and keys in sorted order, as these lists are
    for k in (2, 3, 4):
        live.ref.table[inval[k][0], 1] = (rnd(40, k), None)
    for k in (1, 2):
        del live.ref.table[ups[k][:2]]

    def dev(data, dtype):
        return torch.frombuffer(bytearray(data), dtype=dtype).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    ibuf, ubuf = dev(p["ibuf"], torch.uint8), dev(p["ubuf"], torch.uint8)
    ioff_d = dev(struct.pack("<7i", *ioff), torch.int32)
    uoff_d = dev(struct.pack("<7i", *uoff), torch.int32)
    ihash, uhash = dev(p["ihash"], torch.int64), dev(p["uhash"], torch.int64)
    _gpuresolve.invalidate(*t._table(), ibuf.data_ptr(), ioff_d.data_ptr(),
                           ibuf.numel(), ihash.data_ptr(), 6, stream)
    t._arena[t._used:t._used + ubuf.numel()].copy_(ubuf)
    _gpuresolve.insert(*t._table(), t._used, uoff_d.data_ptr(), ubuf.numel(),
                       uhash.data_ptr(), 6, stream)
    live.check()
    st = t.stats()
    assert (st["tombstones"], st["entries"]) == (3, ent0 - 3 + 4)
