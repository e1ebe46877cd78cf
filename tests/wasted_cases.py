"""Inputs of the wasted-bits tests (FLACMI_DECODE_WASTED_SPEC and flacmi_wasted_rows_device,
include/flacmi.h): units whose samples are a signal of ss - w bits shifted left by w, so that the
unit has exactly w wasted bits, with a different w per channel and per frame.

Shared by tests/golden/make_wasted_golden.py (streams written by the reference's own writers with
the wasted-bits code in the subframe header, read back by the reference decoder with and without
its two corrections: tests/golden/wasted_streams.json), the CPU model test and the device tests.
Every unit is a recipe of tests/fallback_cases.py over splitmix64, so the fixture holds no samples.

A unit is (recipe, w): fallback_cases.unit(recipe, ln, ss - w, seed, u) << w, with two recipes more:
  ("bit",)        r % 2 - 1: the two values of a 1-bit sample, -1 and 0
  ("lone", at)    zeros and -1 at sample `at`: with w = ss - 1 the unit's only nonzero sample is
                  -2^(ss - 1)
`fallback` marks the cases whose subframes may be CONSTANT / VERBATIM (the rule of
FLACMI_FRAME_FALLBACK at the unit's own width ss - w); in every other case the reference alone
writes every subframe without raising.
"""
import hashlib
import os

import numpy as np

import bursts
import fallback_cases as FC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wasted_streams.json")
same_frame = FC.same_frame


def unit(recipe, w: int, ln: int, ss: int, seed: int, u: int) -> np.ndarray:
    if recipe[0] == "bit":
        i = np.arange(ln, dtype=np.uint64)
        with np.errstate(over="ignore"):
            r = bursts.splitmix64(np.uint64(seed) ^ np.uint64((u << 32) & bursts.M64) ^ i)
        x = (r % np.uint64(2)).astype(np.int64) - 1
    elif recipe[0] == "lone":
        x = np.zeros(ln, dtype=np.int64)
        x[recipe[1]] = -1
    else:
        x = FC.unit(recipe, ln, ss - w, seed, u)
    lo, hi = -(1 << (ss - w - 1)), (1 << (ss - w - 1)) - 1
    assert lo <= int(x.min()) and int(x.max()) <= hi, (recipe, w, ss)
    return x << w


def _case(C, n, tail, frames, ss, units, fallback=False, L=8, q=12, rmin=0, rmax=3, first=0, seed=1, twin=0):
    """units: one (recipe, w) per unit, or per frame's channels (every frame alike).  twin: every
    unit has w = twin, and the fixture also records the subframes the reference writes for the
    unshifted samples at ss - twin bits."""
    k = frames * C
    units = list(units) * (k // len(units))
    assert len(units) == k
    return dict(C=C, n=n, tail=tail, frames=frames, ss=ss, L=L, q=q, rmin=rmin, rmax=rmax, first=first, seed=seed,
                units=units, fallback=fallback, twin=twin)


def S(bits):
    """noise + sine filling about 60 % of `bits` bits (at most the 3000 of the other fixtures)"""
    return ("sine", min(3000, int(0.6 * (1 << (bits - 1))) - 4))


Z = ("zero",)
CASES = {
    # w = 0, 1, 2, 8 at ss 16 (int16 rows), one per frame, the last frame shorter
    "mono16": _case(1, 192, 100, 5, 16, [(S(16), 0), (S(15), 1), (S(14), 2), (S(8), 8), (S(15), 1)], first=7, seed=21),
    # two channels at ss 24: only the last channel has w > 0, all do, only the first, all (swapped)
    "stereo24": _case(2, 1152, 500, 4, 24, [(S(24), 0), (S(16), 8), (S(20), 4), (S(8), 16),
                                            (S(16), 8), (S(24), 0), (S(8), 16), (S(20), 4)], rmax=4, seed=22),
    # 8 channels of 16-sample blocks, a different w per channel and per frame
    "ch8_16": _case(8, 16, 9, 2, 16, [(S(16), 0), (S(15), 1), (S(14), 2), (S(8), 8), (S(16), 0), (S(16), 0), (S(16), 0),
                                      (S(13), 3), (S(15), 1), (S(15), 1), (S(14), 2), (S(14), 2), (S(8), 8), (S(8), 8),
                                      (S(15), 1), (S(12), 4)], rmax=0, seed=23),
    # the common 24-bit file: 16-bit samples << 8, blocks of 4608 (a quiet signal: frames below 4 KB)
    "big24": _case(1, 4608, 1000, 2, 24, [(("sine", 40), 8)], rmax=5, first=1000, seed=24, twin=8),
    "twin24": _case(2, 192, 77, 3, 24, [(S(16), 8), (("noise", 2000), 8)], seed=30, twin=8),
    "ss32": _case(1, 192, 0, 2, 32, [(S(24), 8)], seed=25),
    # a unit whose chosen residual needs 64-bit rows (fallback_cases' widespike, w = 0) beside a unit with
    # w = 8: the encoder redoes the batch with 8-byte residual rows and must shift the rows once
    "wide32": _case(2, 1024, 0, 2, 32, [(("widespike", 300), 0), (S(24), 8), (S(24), 8), (("widespike", 700), 0)],
                    rmax=4, seed=31),
    # moderate white noise: the reference's LPC candidates win narrowly on some units
    "lpc24": _case(2, 576, 0, 3, 24, [(("noise", 2000), 8), (("noise", 2000), 4)], rmax=4, seed=26),
    # width 1 (w = ss - 1), and the fallback subframes: a silent channel (w = 0, CONSTANT), an all-equal
    # block of 256 (w = 8, CONSTANT of 1), full-scale white noise of 8 bits << 8 (VERBATIM at ss - w) and a
    # unit whose only nonzero sample is -2^(ss - 1) (w = ss - 1, width 1)
    "w15": _case(1, 16, 5, 2, 16, [(("bit",), 15)], fallback=True, rmax=0, seed=27),
    "w23": _case(1, 192, 0, 1, 24, [(("bit",), 23)], fallback=True, seed=28),
    "fb16": _case(4, 192, 0, 2, 16, [(Z, 0), (("const", 1), 8), (("white",), 8), (("lone", 191), 15),
                                     (("lone", 0), 15), (("white",), 8), (Z, 0), (("const", -3), 4)],
                  fallback=True, seed=29),
}


def unit_lens(name: str):
    c = CASES[name]
    k = c["frames"] * c["C"]
    return [c["tail"] if c["tail"] and u >= k - c["C"] else c["n"] for u in range(k)]


def case_rows(name: str):
    """(rows [frames * C][n] int16 or int32, n_tail_units) of a case."""
    c = CASES[name]
    k, n = c["frames"] * c["C"], c["n"]
    rows = np.zeros((k, n), dtype=np.int16 if c["ss"] <= 16 else np.int32)
    for u, ln in enumerate(unit_lens(name)):
        recipe, w = c["units"][u]
        rows[u, :ln] = unit(recipe, w, ln, c["ss"], c["seed"], u)
    return rows, (c["C"] if c["tail"] else 0)


def wasted(name: str):
    """the w of every unit"""
    return [w for _, w in CASES[name]["units"]]


def samples_sha256(name: str) -> str:
    rows, _ = case_rows(name)
    return hashlib.sha256(rows.astype("<i8").tobytes()).hexdigest()


def stream(name: str, golden_case) -> bytes:
    """The whole .flac stream of a case: fLaC, a last-block STREAMINFO, the fixture's frames."""
    import info_cases as IC
    c = CASES[name]
    samples = c["n"] * (c["frames"] - 1) + (c["tail"] or c["n"])
    return IC.stream_header(c["C"], c["ss"], c["n"], c["n"], samples) + \
        b"".join(bytes.fromhex(h) for h in golden_case["frames"])
