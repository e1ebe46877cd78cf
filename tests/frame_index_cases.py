"""The frame index's candidate rule (include/flacmi.h, flacmi_frame_candidate) restated in
plain Python with the package's own crc.py, and the stream-decode fixture loader.

A byte offset p >= first_byte is a candidate iff the bytes at p pass every header check of
the reference's get_frame_header (decoder.py:133-185), the header with its CRC-8 byte lies
inside the stream, and the CRC-8 of the header equals that byte.
"""
import json
import os

from flac_amd.common import CRC8_POLYNOMIAL
from flac_amd.crc import crc8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_streams.json")
FIELDS = ("offset", "coded_number", "block_size", "header_bytes", "channel_code", "sample_size_code")


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def first_frame_byte(data: bytes) -> int:
    """Offset of the first frame: the magic and every metadata block skipped (decoder.py:36-44,
    90-96), for streams whose metadata the reference accepts."""
    p = 4
    while True:
        last, length = data[p] >> 7, int.from_bytes(data[p + 1:p + 4], "big")
        p += 4 + length
        if last:
            return p


def header_at(data: bytes, p: int, check_crc8: bool = True):
    """The candidate at p as a tuple in FIELDS order, or None."""
    n = len(data)
    if p + 6 > n or data[p] != 0xFF or (data[p + 1] & 0xFE) != 0xF8:
        return None
    bcode, rcode = data[p + 2] >> 4, data[p + 2] & 15
    ch, scode, reserved = data[p + 3] >> 4, (data[p + 3] >> 1) & 7, data[p + 3] & 1
    if bcode == 0 or bcode == 15 or rcode == 15 or ch > 10 or scode == 3 or reserved:
        return None
    b0 = data[p + 4]
    extra = next((k for k, lim in ((6, 0xFE), (5, 0xFC), (4, 0xF8), (3, 0xF0), (2, 0xE0), (1, 0xC0)) if b0 >= lim), 0)
    hb = 5 + extra + (1 if bcode == 6 else 2 if bcode == 7 else 0) + (1 if rcode == 12 else 2 if rcode >= 13 else 0)
    if p + hb + 1 > n:
        return None
    fno = b0 if extra == 0 else b0 & ((1 << (6 - extra)) - 1)
    for k in range(extra):
        fno = (fno << 6) | (data[p + 5 + k] & 0x3F)
    q = p + 5 + extra
    if bcode == 1:
        bs = 192
    elif bcode <= 5:
        bs = 144 << bcode
    elif bcode == 6:
        bs = data[q] + 1
    elif bcode == 7:
        bs = ((data[q] << 8) | data[q + 1]) + 1
    else:
        bs = 1 << bcode
    if check_crc8 and crc8(data[p:p + hb], CRC8_POLYNOMIAL) != data[p + hb]:
        return None
    return (p, fno, bs, hb + 1, ch, scode)


def candidates(data: bytes, first_byte: int = 0):
    """Every candidate of the stream, in offset order."""
    out = []
    p = data.find(b"\xff", first_byte)
    while p >= 0:
        h = header_at(data, p)
        if h is not None:
            out.append(h)
        p = data.find(b"\xff", p + 1)
    return out
