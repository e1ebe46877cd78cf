"""The device frame index (csrc/k_index.hip, flacmi_index_frames_device) against the plain
Python restatement of the candidate rule (tests/frame_index_cases.py): the tables must be
equal, order included."""
import numpy as np
import pytest

import frame_index_cases as FI
from flac_amd import abi
from flac_amd._lib import load

pytestmark = pytest.mark.gpu
CASES = FI.load_cases()


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def rows(table):
    return [tuple(int(r[f]) for f in FI.FIELDS) for r in table]


def header(bcode=1, rcode=0, ch=0, scode=4, number=b"\x07", extra=b""):
    h = bytes([0xFF, 0xF8, (bcode << 4) | rcode, (ch << 4) | (scode << 1)]) + number + extra
    return h + bytes([FI.crc8(h, FI.CRC8_POLYNOMIAL)])


def check(az, data, first=0, base_offset=0):
    table, n = az.index_frames(data, first, base_offset=base_offset)
    want = FI.candidates(bytes(data), first)
    assert n == len(want)
    assert rows(table) == want
    return want


@pytest.mark.parametrize("case", [c for c in CASES if not c["open_exception"]], ids=lambda c: c["name"])
def test_fixture_streams(az, case):
    data = bytes.fromhex(case["hex"])
    first = FI.first_frame_byte(data)
    want = check(az, data, first)
    offs = {w[0] for w in want}
    expect = [o for i, o in enumerate(case["offsets"]) if i != case.get("damaged_frame", -1)]
    assert set(expect) <= offs
    check(az, data, 0)  # the metadata scanned too: first_byte only filters


def test_random_mib(az):
    rng = np.random.default_rng(20261019)
    data = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    check(az, data)


def test_random_mib_with_planted_headers(az):
    """Random bytes hold about one candidate per 10 MB; plant headers of every length (1..7-byte
    numbers, 8- and 16-bit block sizes and sample rates), some with a wrong CRC-8, some cut by
    the stream's end, some overlapping."""
    rng = np.random.default_rng(7)
    data = bytearray(rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes())
    numbers = [b"\x00", b"\x7f", b"\xc2\x80", b"\xe0\xa0\x80", b"\xf0\x90\x80\x80", b"\xf8\x88\x80\x80\x80",
               b"\xfc\x84\x80\x80\x80\x80", b"\xfe\x82\x80\x80\x80\x80\x80", b"\xff\x01\x02\x03\x04\x05\x06"]
    planted = 0
    for k in range(3000):
        bcode = int(rng.integers(1, 15))
        rcode = int(rng.integers(0, 15))
        ex = bytes(rng.integers(0, 256, (1 if bcode == 6 else 2 if bcode == 7 else 0) +
                                (1 if rcode == 12 else 2 if rcode >= 13 else 0), dtype=np.uint8))
        h = bytearray(header(bcode, rcode, int(rng.integers(0, 11)), int(rng.choice([0, 1, 2, 4, 5, 6, 7])),
                             numbers[k % len(numbers)], ex))
        if k % 7 == 0:
            h[-1] ^= 1 + int(rng.integers(0, 255))
        p = int(rng.integers(0, len(data) - 4)) if k % 50 else len(data) - int(rng.integers(1, len(h) + 1))
        data[p:p + len(h)] = h[:len(data) - p]
        planted += 1
    want = check(az, bytes(data))
    assert len(want) > 2000
    check(az, bytes(data), first=len(data) // 2 + 1)


def test_sync_pairs_and_capacity_contract(az):
    # FF F8 pairs: a sync code at every even byte, none a header (block-size code 15)
    check(az, b"\xff\xf8" * 5000)
    # the densest real table here: 6-byte headers back to back, far more than the capacity
    data = header() * 3000 + b"\xff"
    want = FI.candidates(data)
    assert len(want) == 3000
    table, n = az.index_frames(data, 0, capacity=100)
    assert n == 3000 and rows(table) == want[:100]          # true count, first `capacity` entries
    table, n = az.index_frames(data, 0, capacity=n)         # the retry
    assert n == 3000 and rows(table) == want
    table, n = az.index_frames(data, 6 * 2990, capacity=4)
    assert n == 10 and rows(table) == want[2990:2994]


def test_headers_across_tile_and_lane_edges(az):
    T = load().flacmi_index_tile_bytes()
    h = header(number=b"\xc2\x80")  # 7 bytes
    places = [T - 16, T - 1, T, T + 1, T - len(h) + 1, 15, 16, 17, 1023, 1024, 1025, 2 * T - 1, 3 * T - 3, 0]
    for p in places:
        data = bytearray(4 * T)
        data[p:p + len(h)] = h
        want = check(az, bytes(data))
        assert [w[0] for w in want] == [p]
    data = bytearray(4 * T)
    for p in sorted(places):
        data[p:p + len(h)] = h
    data[4 * T - len(h):] = h                # ends with the stream
    data += h[:-1]                           # cut by the stream's end: no candidate
    want = check(az, bytes(data))
    assert 4 * T - len(h) in [w[0] for w in want] and 4 * T not in [w[0] for w in want]
    # a base that is 4-byte but not 16-byte aligned, sizes that end inside a 16-byte group
    for base_offset in (4, 8, 12):
        for cut in (0, 1, 5, 17):
            check(az, bytes(data[:len(data) - cut]), base_offset=base_offset)


def test_empty_and_tiny_streams(az):
    for n in (0, 1, 5, 6, 7, 15, 16, 17):
        data = (header() * 3)[:n]
        check(az, data)
