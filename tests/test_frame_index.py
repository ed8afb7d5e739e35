"""_native.frame_index (native/gpu/frameindex.hpp) against a plain walk
that makes bsock::nextFrame's decisions."""
import struct

import pytest

from binder_amd import _native

MAX_PAYLOAD = 1 << 20


def frame(ftype, payload=b"", magic=0xB5, plen=None):
    return struct.pack("<BBI", magic, ftype,
                       len(payload) if plen is None else plen) + payload


def walk(data, max_frames):
    offs, status = [0], _native.FRAME_INDEX_NEED_MORE
    while len(data) - offs[-1] >= 6:
        if len(offs) - 1 == max_frames:
            break
        magic, _, plen = struct.unpack_from("<BBI", data, offs[-1])
        if magic != 0xB5 or plen > MAX_PAYLOAD:
            status = _native.FRAME_INDEX_BAD
            break
        if len(data) - offs[-1] < 6 + plen:
            break
        offs.append(offs[-1] + 6 + plen)
    if len(offs) - 1 == max_frames:
        status = _native.FRAME_INDEX_FULL
    return offs, offs[-1], status


RUN = [frame(1, bytes(41)), frame(3), frame(9, b"x" * 300), frame(2, b"abcd"),
       frame(5, bytes(12)), frame(4)]


@pytest.mark.parametrize("data,max_frames,frames,status", [
    (b"", 8, 0, "NEED_MORE"),
    (RUN[0], 8, 1, "NEED_MORE"),
    (b"".join(RUN), 8, 6, "NEED_MORE"),
    (b"".join(RUN)[:-6 - 12 - 3], 8, 4, "NEED_MORE"),   # inside a header
    (b"".join(RUN)[:-6 - 5], 8, 4, "NEED_MORE"),        # inside a payload
    (frame(1, b"q", magic=0xB4) + RUN[1], 8, 0, "BAD"),
    (b"".join(RUN[:3]) + frame(3, magic=0) + RUN[4], 8, 3, "BAD"),
    (RUN[0] + frame(1, plen=MAX_PAYLOAD + 1), 8, 1, "BAD"),
    (RUN[0] + frame(1, plen=MAX_PAYLOAD), 8, 1, "NEED_MORE"),
    (b"".join(RUN), 4, 4, "FULL"),
    (b"".join(RUN), 6, 6, "FULL"),
    (b"".join(RUN), 0, 0, "FULL"),
])
def test_frame_index(data, max_frames, frames, status):
    foff, consumed, st = _native.frame_index(data, max_frames)
    offs = list(struct.unpack("<%di" % (len(foff) // 4), foff))
    assert (offs, consumed, st) == walk(data, max_frames)
    assert len(offs) == frames + 1 and consumed == offs[-1]
    assert st == getattr(_native, "FRAME_INDEX_" + status)
