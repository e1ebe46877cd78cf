"""Inputs of the fallback-subframe tests (FLACMI_FRAME_FALLBACK, include/flacmi.h): blocks the
reference cannot write (digital silence, constant and linear blocks, sparse noise, 4..7-sample
blocks) or writes larger than raw (full-scale white noise), beside ordinary ones.

Shared by tests/golden/make_fallback_golden.py (the reference's own verdicts and bytes, in
tests/golden/fallback_streams.json), tests/fallback_model.py's CPU test and the device test.
Every unit is a recipe over splitmix64 (tests/bursts.py), so the fixture holds no samples.

A unit recipe, for unit u of ln samples, r = splitmix64(seed ^ (u << 32) ^ i), full = 1 << (ss - 1):
  ("zero",)            digital silence
  ("const", v)         v
  ("ramp", a, b)       a + b i
  ("sine", amp)        round(amp sin(2 pi i / 97)) + r % 9 - 4
  ("sparse", lo, hi)   r % 7 - 3, but inside [lo, hi): (r >> 8) % 3 - 1 where r % 8 == 0, else 0
  ("noise", amp)       r % (2 amp + 1) - amp
  ("white",)           r % (2 full) - full (full scale)
  ("widespike", at)    32-bit only: 2^31 - 1000 + r % 200 - 100, and -2^31 at sample `at` (the
                       order-1 residual there needs 33 bits: FLACMI_STATUS_RESIDUAL_WIDE on 32-bit rows)
"""
import hashlib
import math
import os

import numpy as np

import bursts

CONSTANT, VERBATIM = 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fallback_streams.json")


def same_frame(data: bytes, want) -> bool:
    """A fixture frame is hex, or {len, sha256} above 4 KB."""
    if isinstance(want, str):
        return data == bytes.fromhex(want)
    return len(data) == want["len"] and hashlib.sha256(data).hexdigest() == want["sha256"]


def unit(recipe, ln: int, ss: int, seed: int, u: int) -> np.ndarray:
    i = np.arange(ln, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = bursts.splitmix64(np.uint64(seed) ^ np.uint64((u << 32) & bursts.M64) ^ i)
    ii = i.astype(np.int64)
    full = 1 << (ss - 1)
    kind = recipe[0]
    if kind == "zero":
        return np.zeros(ln, dtype=np.int64)
    if kind == "const":
        return np.full(ln, recipe[1], dtype=np.int64)
    if kind == "ramp":
        return recipe[1] + recipe[2] * ii
    if kind == "sine":
        s = np.asarray([round(recipe[1] * math.sin(2 * math.pi * k / 97)) for k in range(97)], dtype=np.int64)
        return s[ii % 97] + (r % np.uint64(9)).astype(np.int64) - 4
    if kind == "sparse":
        v = np.where(r % np.uint64(8) == 0, ((r >> np.uint64(8)) % np.uint64(3)).astype(np.int64) - 1, 0)
        return np.where((ii >= recipe[1]) & (ii < recipe[2]), v, (r % np.uint64(7)).astype(np.int64) - 3)
    if kind == "noise":
        return (r % np.uint64(2 * recipe[1] + 1)).astype(np.int64) - recipe[1]
    if kind == "white":
        return (r % np.uint64(2 * full)).astype(np.int64) - full
    if kind == "widespike":
        assert ss == 32
        x = (1 << 31) - 1000 + (r % np.uint64(200)).astype(np.int64) - 100
        x[recipe[1]] = -(1 << 31)
        return x
    raise ValueError(recipe)


def _case(C, n, tail, frames, ss, units, expect, L=8, q=12, rmin=0, rmax=3, first=0, seed=1):
    """units: one recipe per channel (every frame alike) or one per unit; expect likewise: the
    sub-kind each unit must get (0 as analysed, 1 CONSTANT, 2 VERBATIM), asserted by the fixture
    generator from the reference's own run."""
    k = frames * C
    units = list(units) * (k // len(units))
    expect = list(expect) * (k // len(expect))
    assert len(units) == k and len(expect) == k
    return dict(C=C, n=n, tail=tail, frames=frames, ss=ss, L=L, q=q, rmin=rmin, rmax=rmax, first=first, seed=seed,
                units=units, expect=expect)


Z, S, W = ("zero",), ("sine", 3000), ("white",)
CASES = {
    # 1. silence, 3 frames and a 7-sample tail: all CONSTANT
    "silence2": _case(2, 192, 7, 4, 16, [Z, Z], [1, 1], first=126, seed=1),
    # 2. constant -3 in 24-bit (int32 rows): the sign in ss bits
    "const24": _case(1, 64, 0, 2, 24, [("const", -3)], [1], rmax=2, seed=2),
    # 3. escaped first / escaped last in the frame
    "mix_ab": _case(2, 576, 0, 2, 16, [Z, S], [1, 0], rmax=4, seed=3),
    "mix_ba": _case(2, 576, 0, 2, 16, [S, Z], [0, 1], rmax=4, seed=4),
    # 4. linear ramps: the order-2 residual is all zeros, log2(0)
    "ramp": _case(1, 256, 0, 2, 16, [("ramp", -1000, 7), ("ramp", 900, -3)], [2, 2], seed=5),
    # 5. small noise with one finest partition (64 samples at order 4) of sparse {-1, 0, 1}: its
    # mean zig-zag value is below 1, so rice_size takes 1 << negative (ValueError)
    "sparse": _case(1, 1024, 0, 2, 16, [("sparse", 512, 576), ("sparse", 0, 64)], [2, 2], rmax=4, seed=6),
    # 6. full-scale white noise costs more than raw (the strictly-greater branch); the 24-bit
    # stereo frames (27.7 KB) exceed the writer's 16 KB LDS window
    "white16": _case(1, 4608, 0, 2, 16, [W], [2], rmax=5, first=5, seed=7),
    "white24s": _case(2, 4608, 0, 2, 24, [W, W], [2, 2], rmax=5, first=1000, seed=8),
    # 7. exactly at equality: stays Rice (found by search over seeds, make_fallback_golden.py
    # asserts that the reference writes 8 + n ss bits for it)
    "equal": _case(1, 32, 0, 1, 8, [("noise", 90)], [0], rmax=0, seed=2755),
    # 8. ss = 12 and 20 with odd n: subframes start unaligned.  4..7-sample blocks raise in tukey
    "odd12_7": _case(2, 7, 3, 4, 12, [("noise", 900), ("const", -2048)], [2, 1], rmax=0, seed=9),
    "odd12_191": _case(3, 191, 100, 3, 12, [Z, ("sine", 700), W], [1, 0, 2], seed=10),
    "odd20_7": _case(2, 7, 0, 3, 20, [("const", 524287), ("noise", 70000)], [1, 2], rmax=0, seed=11),
    "odd20_191": _case(3, 191, 0, 2, 20, [W, Z, ("sine", 90000)], [2, 1, 0], seed=12),
    # 9. one- and two-sample blocks
    "n1": _case(2, 1, 0, 3, 16, [Z, ("const", 5), Z, Z, ("const", -7), Z], [1] * 6, rmax=0, seed=13),
    "n2": _case(2, 2, 0, 3, 16, [Z, ("ramp", 5, 3), ("const", 9), Z, ("ramp", -1, 1), Z], [1, 2, 1, 1, 2, 1],
                rmax=0, seed=14),
    # 10. 8 channels, escaped and analysed alternating
    "ch8": _case(8, 192, 0, 2, 16, [Z, S, ("ramp", 0, 5), S, W, S, ("const", 77), S], [1, 0, 2, 0, 2, 0, 1, 0],
                 seed=15),
    # 11. a unit whose chosen residual needs 64-bit rows beside a silent channel: the 8-byte
    # redo still happens and the 64-bit general writer writes the CONSTANT
    "wide_const": _case(2, 1024, 0, 2, 32, [("widespike", 300), Z, Z, ("widespike", 700)], [0, 1, 1, 0], rmax=4,
                        seed=16),
    # the writer's LPC precision assertion (q = 16, encoder.py:619): the LPC subframes become
    # VERBATIM (moderate white noise: LPC wins narrowly on five of the six units)
    "q16": _case(2, 576, 0, 3, 16, [("noise", 2000)], [2, 2, 2, 2, 0, 2], q=16, rmax=4, seed=18),
}


def case_rows(name: str):
    """(rows [frames * C][n] int16 or int32, n_tail_units) of a case."""
    c = CASES[name]
    k, C, n = c["frames"] * c["C"], c["C"], c["n"]
    rows = np.zeros((k, n), dtype=np.int16 if c["ss"] <= 16 else np.int32)
    for u in range(k):
        ln = c["tail"] if c["tail"] and u >= k - C else n
        rows[u, :ln] = unit(c["units"][u], ln, c["ss"], c["seed"], u)
    return rows, (C if c["tail"] else 0)


def unit_lens(name: str):
    c = CASES[name]
    k = c["frames"] * c["C"]
    return [c["tail"] if c["tail"] and u >= k - c["C"] else c["n"] for u in range(k)]
