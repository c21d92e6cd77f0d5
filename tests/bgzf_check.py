"""The BGZF checker of the bgzf tests: zlib is the oracle.

check(buf, parts=None) walks a buffer member by member and asserts the format; it returns the text.  parts: the byte offsets at which
parts of the buffer begin and end (part i is buf[parts[i]:parts[i + 1]]); a member's ISIZE may be short only where its part ends.
"""
import gzip
import struct
import zlib

PIECE = 65280
HEADER = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00])
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def members(buf):
    """[(offset, size, deflate bytes, text, stored)] of every member of buf"""
    buf = bytes(buf)
    out = []
    at = 0
    while at < len(buf):
        assert len(buf) - at >= 26, "a member of under 26 bytes at %d" % at
        assert buf[at:at + 16] == HEADER, "member header at %d: %s" % (at, buf[at:at + 16].hex())
        size = struct.unpack_from("<H", buf, at + 16)[0] + 1
        assert at + size <= len(buf), "BSIZE at %d leads past the buffer" % at
        d = zlib.decompressobj(-15)
        text = d.decompress(buf[at + 18:at + size])
        assert d.eof, "member at %d: the deflate stream does not end" % at
        assert len(d.unused_data) == 8, "member at %d: %d bytes behind the stream" % (at, len(d.unused_data))
        crc, isize = struct.unpack("<II", d.unused_data)
        assert isize == len(text) and isize <= PIECE, (at, isize, len(text))
        assert crc == zlib.crc32(text), "member at %d: CRC" % at
        out.append((at, size, size - 26, text, (buf[at + 18] & 7) == 1))
        at += size
    assert at == len(buf)
    return out


def check(buf, parts=None):
    buf = bytes(buf)
    ms = members(buf)
    ends = set(parts) if parts is not None else {len(buf)}
    for at, size, _, text, _ in ms:
        assert len(text) > 0 or buf[at:at + size] == EOF, "an empty member at %d that is not the end-of-file block" % at
        if at + size not in ends:
            assert len(text) == PIECE, "member at %d: %d bytes inside a part" % (at, len(text))
    if parts is not None:
        starts = {m[0] for m in ms} | {len(buf)}
        for p in parts:
            assert p in starts, "part bound %d is no member's start" % p
    text = b"".join(m[3] for m in ms)
    assert (gzip.decompress(buf) if buf else b"") == text
    return text
