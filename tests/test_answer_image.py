"""CPU tier of the GPU batch resolver: the bound fast-path parser and
the host image (native/gpu/answerimage.hpp) whose bytes the kernels
read. Needs neither a GPU nor hipcc."""
import struct

import pytest

from binder_amd import _native


def wire(name: bytes, qtype=1, qclass=1, flags=0x0100, counts=(1, 0, 0, 0),
         qid=0xBEEF, tail=b""):
    """A query for dotted `name`, labels encoded as they stand."""
    labels = b"".join(bytes([len(p)]) + p for p in name.split(b".") if p)
    return (struct.pack(">HH4H", qid, flags, *counts) + labels + b"\0" +
            struct.pack(">HH", qtype, qclass) + tail)


@pytest.mark.parametrize("w,want", [
    (wire(b"a.b"), (b"a.b", False, 0)),
    (wire(b"a.b", flags=0), (b"a.b", False, 0)),
    (wire(b""), (b"", False, 0)),
    (wire(b"a.b", tail=b"xyz"), (b"a.b", False, 0)),
    (wire(b"_s._tcp.d.e", 33), (b"_s._tcp.d.e", True, 8)),
    (wire(b"_s-1._t.d", 33), (b"_s-1._t.d", True, 8)),
    (wire(b"A.b"), None),
    (wire(b"a.b", 28), None),
    (wire(b"a.b", qclass=3), None),
    (wire(b"a.b", flags=0x8100), None),
    (wire(b"a.b", counts=(1, 0, 0, 1)), None),
    (wire(b"a.b")[:-1], None),
    (wire(b"a.b")[:12] + b"\xc0\x0c" + wire(b"a.b")[-4:] + b"pad", None),
    (wire(b"_s.d", 33), None),
    (wire(b"_s_x._tcp.d", 33), None),
    (wire(b"s._tcp.d", 33), None),
    (wire(b"a", tail=b"x" * 281), (b"a", False, 0)),   # 300 bytes
    (wire(b"a", tail=b"x" * 282), None),               # 301 bytes
])
def test_parse_fast(w, want):
    assert _native.parse_fast(w) == want


def find(im, qname, qtype):
    """AnswerTable::find over the image's exported bytes."""
    slots, arena = im.slots(), im.arena()
    cap = len(slots) // 16
    i = im.home_slot(qname, qtype)
    for _ in range(cap):
        _h, off, ln = struct.unpack_from("<QII", slots, 16 * i)
        if ln == 0:
            return None
        blob = arena[off:off + ln]
        if blob[:2] == bytes([len(qname), qtype]) and \
                blob[2:2 + len(qname)] == qname:
            return blob[2 + len(qname):]
        i = (i + 1) % cap
    return None


def test_image_walk_returns_every_body():
    im = _native.AnswerImage()
    assert len(im) == 0 and im.slots() == b"" and im.arena() == b""
    want = {}
    for i in range(700):  # past 512 entries: the slot array grows once
        name, reply = b"h%d.x" % i, bytes([i & 255]) * (12 + i % 50)
        im.add_reply(name, 1, reply)
        want[name, 1] = b"\0\0" + struct.pack("<H", len(reply)) + reply
    members = [(b"A" * 3, b"bb"), (b"C" * 5, b""), (b"", b"d" * 4)]
    im.add_service(b"_s._tcp.svc.x", 33, b"H" * 20, members)
    im.add_service(b"svc.x", 1, b"H" * 14, [(b"aa", b"")])
    assert len(im) == 702 and len(im.slots()) == 2048 * 16
    for key, body in want.items():
        assert find(im, *key) == body
    body = find(im, b"_s._tcp.svc.x", 33)
    assert body[:6] == bytes([1, 3]) + struct.pack("<HH", 34, 20)
    assert body[6:30] == struct.pack("<12H", 0, 3, 3, 2, 5, 5, 10, 0,
                                     10, 0, 10, 4)
    assert body[30:] == b"H" * 20 + b"AAAbbCCCCCdddd"
    assert find(im, b"svc.x", 1)[-16:] == b"H" * 14 + b"aa"
    assert find(im, b"_t._udp.svc.x", 33) is None
    assert find(im, b"nope", 1) is None
    # both SRV names of one domain share a home slot, the A name does not
    assert im.home_slot(b"_s._tcp.svc.x", 33) == \
        im.home_slot(b"_t._udp.svc.x", 33)


@pytest.mark.parametrize("call", [
    lambda im: im.add_reply(b"a", 1, b"x" * 513),
    lambda im: im.add_reply(b"a", 1, b"x" * 11),
    lambda im: im.add_reply(b"a" * 256, 1, b"x" * 12),
    lambda im: im.add_reply(b"a", 28, b"x" * 12),
    lambda im: im.add_reply(b"_s.d", 33, b"x" * 12),
    lambda im: im.add_service(b"a", 1, b"h" * 12, [(b"s", b"")] * 65),
    lambda im: im.add_service(b"a", 1, b"h" * 12, [(b"s" * 250, b"t" * 251)]),
    lambda im: im.add_service(b"a", 1, b"h" * 11, []),
    lambda im: im.home_slot(b"a", 2),
])
def test_image_refuses(call):
    im = _native.AnswerImage()
    with pytest.raises(ValueError):
        call(im)
    assert len(im) == 0
    im.add_reply(b"a", 1, b"x" * 512)  # the limits themselves pass
    im.add_reply(b"a" * 255, 1, b"x" * 12)
    im.add_service(b"s", 1, b"h" * 12, [(b"s" * 4, b"t" * 3)] * 64)
