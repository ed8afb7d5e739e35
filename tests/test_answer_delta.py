"""CPU tier of the device table updates: the normal form and the
refusals of _native.AnswerDelta (native/gpu/answerdelta.hpp). The packed
delta, applied as the device applies it - every invalidation, then every
upsert - must equal the calls applied one by one to a dict."""
import struct

import pytest

from binder_amd import _native
from test_answer_image import find

R = [bytes([65 + i]) * (12 + i) for i in range(6)]
MEM = [(b"s0", b"a0"), (b"s11", b"")]


def covers(domain, key):
    """applyInvalidate: (domain, A), and SRV keys hashed on domain."""
    name, qtype = key
    return name == domain if qtype == 1 else \
        name.split(b".", 2)[2:] == [domain]


def body_of(op):
    """What AnswerImage stores for the same call."""
    im = _native.AnswerImage()
    (im.add_reply if len(op) == 3 else im.add_service)(*op)
    return find(im, op[0], op[1])


def unpack(buf, off):
    off = struct.unpack("<%di" % (len(off) // 4), off)
    assert off[0] == 0 and off[-1] == len(buf)
    return [buf[a:b] for a, b in zip(off, off[1:])]


SEQUENCES = {
    "upsert-then-invalidate": [
        (b"a.foo.com", 1, R[0]), (b"_s._tcp.a.foo.com", 33, R[1]),
        (b"a.foo.com",)],
    "invalidate-then-upsert": [
        (b"a.foo.com",), (b"a.foo.com", 1, R[0]),
        (b"_s._tcp.a.foo.com", 33, R[1], MEM)],
    "same-key-twice": [
        (b"a.foo.com", 1, R[0]), (b"a.foo.com", 1, R[1]),
        (b"_s._tcp.a.foo.com", 33, R[2]),
        (b"_s._tcp.a.foo.com", 33, R[3], MEM)],
    "same-domain-twice": [
        (b"a.foo.com",), (b"a.foo.com", 1, R[0]), (b"a.foo.com",),
        (b"b.foo.com",)],
    "two-services-one-domain": [
        (b"_s._tcp.a.foo.com", 33, R[0]), (b"_t._udp.a.foo.com", 33, R[1]),
        (b"_s._tcp.b.foo.com", 33, R[2]), (b"a.foo.com",),
        (b"_t._udp.a.foo.com", 33, R[3])],
    "dotted-suffix": [
        (b"b.foo.com", 1, R[0]), (b"_s._tcp.b.foo.com", 33, R[1]),
        (b"foo.com", 1, R[2]), (b"_s._tcp.foo.com", 33, R[3]),
        (b"foo.com",)],
    "string-suffix": [
        (b"ab.foo.com", 1, R[0]), (b"_s._tcp.ab.foo.com", 33, R[1]),
        (b"b.foo.com", 1, R[2]), (b"_s._tcp.b.foo.com", 33, R[3]),
        (b"b.foo.com",)],
}


@pytest.mark.parametrize("name", SEQUENCES)
def test_normal_form_equals_serial(name):
    seq = SEQUENCES[name]
    # a table that already holds every key the sequence names
    start = {op[:2]: b"old" for op in seq if len(op) > 1}
    for op in seq:
        if len(op) == 1:
            start[op[0], 1] = start[b"_s._tcp." + op[0], 33] = b"old"
    serial, delta = dict(start), _native.AnswerDelta()
    im = _native.AnswerImage()
    im.add_reply(b"seed", 1, R[0])  # 1024 slots: hash & 1023 is the home
    for op in seq:
        if len(op) == 1:
            delta.invalidate(op[0])
            serial = {k: v for k, v in serial.items()
                      if not covers(op[0], k)}
        else:
            (delta.upsert_reply if len(op) == 3
             else delta.upsert_service)(*op)
            serial[op[:2]] = body_of(op)

    p = delta.pack()
    domains = unpack(p["ibuf"], p["ioff"])
    blobs = unpack(p["ubuf"], p["uoff"])
    ihash = struct.unpack("<%dQ" % (2 * len(domains)), p["ihash"])
    uhash = struct.unpack("<%dQ" % len(blobs), p["uhash"])
    assert len(delta) == len(domains) + len(blobs)
    assert len(set(domains)) == len(domains)
    phased = dict(start)
    for i, d in enumerate(domains):
        assert ihash[2 * i] & 1023 == im.home_slot(d, 1)
        assert ihash[2 * i + 1] & 1023 == im.home_slot(b"_x._y." + d, 33)
        phased = {k: v for k, v in phased.items() if not covers(d, k)}
    keys = set()
    for h, blob in zip(uhash, blobs):
        key = (blob[2:2 + blob[0]], blob[1])
        assert h & 1023 == im.home_slot(*key)
        keys.add(key)
        phased[key] = blob[2 + blob[0]:]
    assert len(keys) == len(blobs)
    assert phased == serial
    delta.clear()
    assert len(delta) == 0 and delta.pack()["uoff"] == bytes(4)


@pytest.mark.parametrize("call", [
    lambda d: d.upsert_reply(b"a", 1, b"x" * 513),
    lambda d: d.upsert_reply(b"a", 1, b"x" * 11),
    lambda d: d.upsert_reply(b"a" * 256, 1, b"x" * 12),
    lambda d: d.upsert_reply(b"a", 28, b"x" * 12),
    lambda d: d.upsert_reply(b"_s.d", 33, b"x" * 12),
    lambda d: d.upsert_service(b"a", 1, b"h" * 12, [(b"s", b"")] * 65),
    lambda d: d.upsert_service(b"a", 1, b"h" * 12,
                               [(b"s" * 250, b"t" * 251)]),
    lambda d: d.upsert_service(b"a", 1, b"h" * 11, []),
    lambda d: d.invalidate(b""),
    lambda d: d.invalidate(b"a" * 256),
])
def test_delta_refuses(call):
    d = _native.AnswerDelta()
    with pytest.raises(ValueError):
        call(d)
    assert len(d) == 0
    d.upsert_reply(b"a", 1, b"x" * 512)  # the limits themselves pass
    d.upsert_reply(b"a" * 255, 1, b"x" * 12)
    d.upsert_service(b"s", 1, b"h" * 12, [(b"s" * 4, b"t" * 3)] * 64)
    d.invalidate(b"a" * 255)
    assert len(d) == 3  # the invalidation covered one upsert
