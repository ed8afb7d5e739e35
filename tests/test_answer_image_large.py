"""The producer's reply ceiling (native/gpu/answerrules.hpp):
AnswerImage(max_reply=) and AnswerDelta(max_reply=). CPU only."""
import pytest

from binder_amd import _native
from test_answer_image import find

KINDS = [_native.AnswerImage, _native.AnswerDelta]


def put(obj, name, reply):
    add = obj.add_reply if hasattr(obj, "add_reply") else obj.upsert_reply
    add(name, 1, reply)


def put_service(obj, name, head, members):
    add = (obj.add_service if hasattr(obj, "add_service")
           else obj.upsert_service)
    add(name, 1, head, members)


@pytest.mark.parametrize("kind", KINDS)
def test_ceiling_range(kind):
    for bad in (0, 511, 4097, 65536):
        with pytest.raises(ValueError):
            kind(max_reply=bad)
    assert kind().max_reply == 512 and kind(max_reply=4096).max_reply == 4096
    with pytest.raises(AttributeError):
        kind().max_reply = 600
    small = kind(max_reply=512)  # the default, by name
    put(small, b"a", b"x" * 512)
    with pytest.raises(ValueError, match="reply longer than 512 bytes"):
        put(small, b"b", b"x" * 513)
    with pytest.raises(ValueError, match="reply longer than 512 bytes"):
        put_service(small, b"s", b"h" * 13, [(b"s" * 250, b"t" * 250)])
    assert len(small) == 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ceiling", [513, 4096])
def test_large_ceiling(kind, ceiling):
    obj = kind(max_reply=ceiling)
    put(obj, b"a", b"x" * ceiling)
    with pytest.raises(ValueError, match=f"longer than {ceiling} bytes"):
        put(obj, b"b", b"x" * (ceiling + 1))
    seg = (ceiling - 12) // 64
    mem = [(b"s" * (seg - 1), b"t")] * 63 + [(b"s" * (ceiling - 12 - 63 * seg),
                                              b"")]
    put_service(obj, b"s", b"h" * 12, mem)  # exactly the ceiling
    with pytest.raises(ValueError, match=f"longer than {ceiling} bytes"):
        put_service(obj, b"t", b"h" * 13, mem)
    with pytest.raises(ValueError, match="more than 64 members"):
        put_service(obj, b"t", b"h" * 12, [(b"s", b"")] * 65)
    assert len(obj) == 2


def test_large_image_exports_verified():
    """slots() and arena() walk the image against its own ceiling."""
    im = _native.AnswerImage(max_reply=4096)
    im.add_reply(b"w", 1, bytes(range(256)) * 16)
    mem = [(bytes([m]) * (20 + m), bytes([m]) * (m % 3)) for m in range(64)]
    im.add_service(b"_s._tcp.d", 33, b"H" * 30, mem)
    body = find(im, b"w", 1)
    assert body[:4] == b"\0\0\0\x10" and body[4:] == bytes(range(256)) * 16
    body = find(im, b"_s._tcp.d", 33)
    total = 30 + sum(len(a) + len(b) for a, b in mem)
    assert 2048 < total <= 4096
    assert body[:6] == bytes([1, 64, total & 255, total >> 8, 30, 0])
    assert body[6 + 8 * 64:] == b"H" * 30 + b"".join(a + b for a, b in mem)
