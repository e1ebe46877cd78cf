"""Burst inputs for the frame writer's ring-overrun path and the decoder's long Rice codes,
and the host model of a writer tile.

A unit is a quiet background plus a few loud events.  With one Rice partition for the whole
block (rice_max = 0) the parameter follows the block's mean, so every loud value costs a long
unary run: a 512-value tile of k_packw (csrc/k_frame.hip) then holds more bits than its LDS
ring (512 words for samples of <= 16 bits, 1024 for wider ones) and takes the redo path, and
the decoder meets Rice codes longer than its look-ahead.

The recipe is pure integer arithmetic on splitmix64 (tests/golden/make_golden.py restates it
without numpy for the streams of tests/golden/bursts.json).  Sample i of a unit, with
r = splitmix64(seed ^ (unit << 32) ^ i), lo = -(1 << (bits - 1)):
  background  "silence" 0 | "alt1" 1 - 2 (i & 1) | "noise3" r % 7 - 3 |
              "sine" round(3000 sin(2 pi i / 2048)) + (r >> 8) % 5 - 2
  ("burst", start, length)  start <= i < start + length: +-(-lo - 1 - (r >> 8) % (1 << (bits - 4))),
                            the sign from r & 1 (full-scale noise)
  ("spike", i[, value])     lo, or the value given
"""
import math

import numpy as np

M64 = (1 << 64) - 1
BACKGROUNDS = ("silence", "alt1", "noise3", "sine")


def splitmix64(x: np.ndarray) -> np.ndarray:
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


_SINE = [round(3000 * math.sin(2 * math.pi * k / 2048)) for k in range(2048)]


def unit(n: int, bits: int, seed: int, index: int, background: str, events=()) -> np.ndarray:
    """Samples of one unit (int64)."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = splitmix64(np.uint64(seed) ^ np.uint64((index << 32) & M64) ^ i)
    ii = i.astype(np.int64)
    if background == "silence":
        x = np.zeros(n, dtype=np.int64)
    elif background == "alt1":
        x = 1 - 2 * (ii & 1)
    elif background == "noise3":
        x = (r % np.uint64(7)).astype(np.int64) - 3
    elif background == "sine":
        x = np.asarray(_SINE, dtype=np.int64)[ii & 2047] + ((r >> np.uint64(8)) % np.uint64(5)).astype(np.int64) - 2
    else:
        raise ValueError(background)
    lo = -(1 << (bits - 1))
    for ev in events:
        if ev[0] == "burst":
            s, ln = ev[1], ev[2]
            assert 0 <= s and s + ln <= n, ev
            mag = -lo - 1 - ((r[s:s + ln] >> np.uint64(8)) % np.uint64(1 << (bits - 4))).astype(np.int64)
            x[s:s + ln] = np.where((r[s:s + ln] & np.uint64(1)) != 0, -mag, mag)
        elif ev[0] == "spike":
            x[ev[1]] = ev[2] if len(ev) > 2 else lo
        else:
            raise ValueError(ev)
    return x


def rows(units, n: int, bits: int, seed: int, n_tail: int = 0, tail: int = 0) -> np.ndarray:
    """Batch rows from [(background, events), ...]; the last n_tail rows hold tail samples
    (their events lie below tail) and zeros behind."""
    out = np.zeros((len(units), n), dtype=np.int16 if bits <= 16 else np.int32)
    for u, (bg, ev) in enumerate(units):
        ln = tail if u >= len(units) - n_tail else n
        out[u, :ln] = unit(ln, bits, seed, u, bg, ev)
    return out


def _values(m, rice_params, residual, n: int):
    """(zig-zag values, their Rice parameters) of samples order .. n - 1 of a unit."""
    order, po = int(m["order"]), int(m["part_order"])
    off, ln = int(m["res_offset"]), int(m["res_len"])
    assert ln == n - order
    z = np.asarray(residual[off:off + ln], dtype=np.uint64)
    p = np.asarray(rice_params[: 1 << po], dtype=np.int64)[np.arange(order, n) // (n >> po)]
    return z, p


def code_bits(m, rice_params, residual, n: int) -> np.ndarray:
    """Bits the writer spends at each sample index of a unit of n samples, from the oracle's
    analysis row (meta m, Rice parameters, zig-zag residual row): 0 below the predictor order,
    (z >> p) + 1 + p for a value, plus the 4- or 5-bit parameter field at a partition's first
    value.  The host restatement of tsum in packw_frame."""
    order, method, ps = int(m["order"]), int(m["coding_method"]), n >> int(m["part_order"])
    assert method in (4, 5)
    z, p = _values(m, rice_params, residual, n)
    bits = np.zeros(n, dtype=np.int64)
    bits[order:] = (z >> p.astype(np.uint64)).astype(np.int64) + 1 + p
    bits[order] += method
    bits[ps::ps] += method
    return bits


def tile_bits(m, rice_params, residual, n: int, tile: int = 512) -> np.ndarray:
    """Bit count of every tile [tile * t, tile * t + tile) of a unit's residual."""
    b = code_bits(m, rice_params, residual, n)
    pad = np.zeros(-(-n // tile) * tile, dtype=np.int64)
    pad[:n] = b
    return pad.reshape(-1, tile).sum(axis=1)


def ring_words(sample_size: int) -> int:
    """RW of the packw_frame instantiation that ships for a sample width."""
    return 512 if sample_size <= 16 else 1024


def longest_unary(m, rice_params, residual, n: int) -> int:
    """Largest z >> p of a unit: the zero run of its longest Rice code."""
    z, p = _values(m, rice_params, residual, n)
    return int((z >> p.astype(np.uint64)).max())


# A case: channels C, block n, tail (length of the short last frame, 0: none), sample bits (=
# sample_size), L, q, rice range, mode (1: fixed-only), first frame number, seed, upb (frames a
# sub-batch in the pipeline test) and one (background, events, expectations) per unit row, frame
# after frame.  Expectations, asserted from the oracle's analysis alone with RW = ring_words():
#   "redo"    a tile of >= 32 RW bits (at least one redo of the ring)
#   "two"     a tile of >= 64 RW bits (two or more passes)
#   "lone"    one code with z >> p >= 64 RW
#   "order1"  a predictor order >= 1 chosen
#   "parts2"  partition order 1 chosen
def _case(C, n, tail, bits, L, q, rmax, mode, first, seed, upb, units):
    return dict(C=C, n=n, tail=tail, bits=bits, L=L, q=q, rmin=0, rmax=rmax, mode=mode, first=first, seed=seed,
                upb=upb, units=units)


_B16 = [("noise3", [("burst", 4096, 512)], ("two",)),          # tile-aligned
        ("noise3", [("burst", 6000, 512)], ()),                # straddles tiles 11 and 12
        ("noise3", [("burst", 16384 - 300, 300)], ("redo",)),  # the last 300 samples
        ("sine", [("burst", 9216, 512)], ("redo", "order1"))]
CASES = {
    "burst16": _case(1, 16384, 0, 16, 8, 12, 0, 0, 0, 41, 3, _B16),
    # rice_max = 1: two partitions chosen; the second unit's overrunning tile starts partition 1
    "burst16_r01": _case(1, 16384, 0, 16, 8, 12, 1, 0, 7, 41, 1, [
        ("noise3", [("burst", 4096, 512)], ("redo", "parts2")),
        ("noise3", [("burst", 8192, 512)], ("redo", "parts2"))]),
    "burst16_stereo_tail": _case(2, 16384, 5000, 16, 8, 12, 0, 0, 126, 42, 2, [
        ("noise3", [], ()), ("noise3", [("burst", 8192, 512)], ("two",)),                    # channel 1 only
        ("noise3", [("burst", 1024, 512)], ("two",)), ("alt1", [("burst", 12288, 512)], ("two",)),
        ("noise3", [("burst", 5000 - 150, 150)], ()), ("noise3", [], ())]),                  # ends at the last sample
    "burst16_odd": _case(1, 16381, 0, 16, 8, 12, 0, 0, 3, 43, 1, [
        ("noise3", [("burst", 16381 - 200, 200)], ("redo",)),
        ("alt1", [("burst", 15872, 509)], ("two",))]),
    # fixed-only, digital silence: the reference's LPC path and rice_max >= 3 raise on it
    "lone16": _case(1, 16384, 0, 16, 0, 5, 0, 1, 0, 44, 2, [
        ("silence", [("spike", 8000)], ("two",)),
        ("silence", [("spike", 100), ("spike", 16000)], ()),
        ("alt1", [("spike", 5000)], ())]),
    # 16384 samples cannot hold a lone code of 64 * 512 bits (p = 0 needs a mean below 2, so
    # z < 32768); 40000 samples can (and the frame header carries the block size in 16 bits)
    "lone16_40k": _case(1, 40000, 0, 16, 0, 5, 0, 1, 0, 45, 1, [
        ("silence", [("spike", 20000)], ("two", "lone")),
        ("silence", [("spike", 0)], ("two", "lone"))]),
    "burst12": _case(1, 16384, 0, 12, 8, 12, 0, 0, 0, 46, 1, [
        ("noise3", [("burst", 2048, 512)], ("redo",)),
        ("noise3", [("burst", 16384 - 300, 300)], ("redo",))]),
    "burst24": _case(1, 16384, 0, 24, 8, 12, 0, 0, 0, 50, 1, [
        ("noise3", [("burst", 4096, 512)], ("redo",)),
        ("sine", [("burst", 16384 - 512, 512)], ("redo",))]),
    "burst24_32k": _case(1, 32768, 0, 24, 8, 12, 0, 0, 0, 47, 1, [
        ("noise3", [("burst", 16384, 512)], ("redo",)),
        ("sine", [("burst", 32768 - 512, 512)], ("redo",))]),
    "burst24_64k": _case(1, 65535, 0, 24, 8, 12, 0, 0, 0, 48, 1, [
        ("noise3", [("burst", 32768, 512)], ("two",)),
        ("noise3", [("burst", 65535 - 300, 300)], ("redo",))]),
    # -(1 << 23) in 65535 zeros: p = 8 and a code of 65535 zeros; 1 << 22 (z = 1 << 23): p = 7 and
    # 65536 zeros, the lone-code bound of the 1024-word ring
    "lone24_64k": _case(1, 65535, 0, 24, 0, 5, 0, 1, 0, 49, 1, [
        ("silence", [("spike", 30000)], ("two",)),
        ("silence", [("spike", 40000, 1 << 22)], ("two", "lone"))]),
}

# Blocks the analysis kernels cannot stage in LDS (flacmi_encode_host and flacmi_encode_pipeline
# answer FLACMI_E_UNSUPPORTED): the device writer runs on the oracle's analysis of these
# (flacmi_frame_sizes_device + flacmi_pack_frames_device), the decoder on the oracle writer's frames.
WRITER_ONLY = ("burst24_32k", "burst24_64k", "lone16_40k", "lone24_64k")
# The reference's decoder asserts a block-size code below 15 (decoder.py:194), so it refuses the
# 32768-sample frames its encoder writes, and the device decoder with it: writer tests only.
NO_DECODE = ("burst24_32k",)
assert all(w in CASES for w in WRITER_ONLY)


def case_rows(name: str):
    """(rows, n_tail_units) of a case."""
    c = CASES[name]
    n_tail = c["C"] if c["tail"] else 0
    return rows([(bg, ev) for bg, ev, _ in c["units"]], c["n"], c["bits"], c["seed"], n_tail, c["tail"]), n_tail


def largest_tiles(name: str, ora: dict) -> list:
    """[(largest tile in bits, longest zero run)] per unit of a case, from its oracle analysis."""
    c = CASES[name]
    out = []
    for u in range(len(c["units"])):
        ln = c["tail"] if c["tail"] and u >= len(c["units"]) - c["C"] else c["n"]
        a = (ora["meta"][u], ora["rice_params"][u], ora["residual"][u], ln)
        out.append((int(tile_bits(*a).max()), longest_unary(*a)))
    return out


def check_expectations(name: str, ora: dict) -> None:
    """The overrun conditions of a case, from the oracle's analysis alone: every unit analysed
    (status 0) and each expectation met.  They are conditions on the input: a unit that misses
    one needs another seed or burst, never another threshold."""
    c = CASES[name]
    RW = ring_words(c["bits"])
    for u, ((_, _, exp), (tile, run)) in enumerate(zip(c["units"], largest_tiles(name, ora))):
        m = ora["meta"][u]
        assert int(m["status"]) == 0, f"{name} unit {u}: the reference does not write this frame"
        for e in exp:
            ok = {"redo": tile >= 32 * RW, "two": tile >= 64 * RW, "lone": run >= 64 * RW,
                  "order1": int(m["order"]) >= 1, "parts2": int(m["part_order"]) == 1}[e]
            assert ok, f"{name} unit {u}: '{e}' not met (largest tile {tile} bits, longest run {run}, RW {RW})"
