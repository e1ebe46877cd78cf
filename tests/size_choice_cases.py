"""The tiny streams of tests/golden/size_choice_streams.json (the subframe choice by exact written
size, FLACMI_FLAG_SIZE_CHOICE) and the units of the GPU analysis tests, rebuilt from seeds:
make_size_choice_golden.py writes every candidate subframe of every unit with the reference's own
writers, the tests feed the same samples to the model and to the device.

Signals, one per block of a channel: "ar" an AR(2) with poles of radius 0.9, "tone" a
0.013-cycle/sample tone plus +-2 of dither, "noise" white noise of +-200, "zero" digital silence,
"const" a constant, "full" full-scale white noise, "tie" 16 samples of +-amp from the pinned seed.
"""
import hashlib

import numpy as np

_MIX = ("ar", "tone", "noise", "ar", "tone", "noise")
CASES = {
    # 16-bit mono with the corrected sign: the size rule and the sum |r| rule part ways
    "mix16": dict(C=1, ss=16, n=192, tail=0, L=8, q=12, rmin=0, rmax=3, rate=44100, seed=21, sign=True, fixed_only=False,
                  plan=[_MIX]),
    # the same blocks with the reference's sign
    "nosign16": dict(C=1, ss=16, n=192, tail=0, L=8, q=12, rmin=0, rmax=3, rate=44100, seed=21, sign=False,
                     fixed_only=False, plan=[_MIX]),
    # fixed candidates only
    "fixed16": dict(C=1, ss=16, n=192, tail=0, L=8, q=12, rmin=0, rmax=3, rate=44100, seed=21, sign=False,
                    fixed_only=True, plan=[_MIX]),
    # stereo (the right channel is the left plus a little noise) with a short last block of odd length
    "st16": dict(C=2, ss=16, n=192, tail=77, L=8, q=12, rmin=0, rmax=3, rate=44100, seed=22, sign=True, fixed_only=False,
                 plan=[("ar", "tone", "noise", "ar"), ("+0", "+0", "+0", "+0")]),
    # 24-bit, three channels, rice_min > 0
    "tri24": dict(C=3, ss=24, n=256, tail=0, L=6, q=14, rmin=1, rmax=4, rate=48000, seed=23, sign=True, fixed_only=False,
                  plan=[("ar", "noise"), ("tone", "ar"), ("noise", "tone")]),
    # blocks of 16: two candidates tie at the minimum, the first wins (seeds pinned by the generator's search)
    "tie16": dict(C=1, ss=16, n=16, tail=0, L=4, q=12, rmin=0, rmax=2, rate=44100, seed=0, sign=True, fixed_only=False,
                  plan=[("tie:4:208", "tie:40:9", "tie:40:337")]),
    # units only the fallback mode writes: silence fails the LPC stage (CONSTANT), full-scale noise is larger than raw (VERBATIM)
    "fb16": dict(C=1, ss=16, n=192, tail=0, L=8, q=12, rmin=0, rmax=3, rate=44100, seed=24, sign=True, fixed_only=False,
                 plan=[("zero", "ar", "full", "noise")], fallback=True),
}


def signal(kind: str, n: int, rng, scale: int = 1) -> np.ndarray:
    """n samples of one block; scale multiplies the 16-bit amplitudes (256 for 24-bit streams)."""
    if kind == "ar":
        e = rng.normal(0.0, 300.0 * scale, n + 64)
        x = np.zeros(n + 64)
        for i in range(n + 64):
            x[i] = e[i] + (1.7 * x[i - 1] if i >= 1 else 0.0) - (0.81 * x[i - 2] if i >= 2 else 0.0)
        lim = 32767 * scale
        return np.clip(np.rint(x[64:]), -lim, lim).astype(np.int64)
    if kind == "tone":
        ph = rng.uniform(0, 2 * np.pi)
        return np.rint(8000.0 * scale * np.sin(2 * np.pi * 0.013 * np.arange(n) + ph)).astype(np.int64) + \
            rng.integers(-2, 3, n)
    if kind == "noise":
        return rng.integers(-200, 201, n).astype(np.int64)
    if kind == "zero":
        return np.zeros(n, dtype=np.int64)
    if kind == "const":
        return np.full(n, 5, dtype=np.int64)
    if kind == "full":
        return rng.integers(-32768 * scale, 32768 * scale, n).astype(np.int64)
    if kind.startswith("tie:"):
        _, amp, seed = kind.split(":")
        return np.random.default_rng(int(seed)).integers(-int(amp), int(amp) + 1, n).astype(np.int64)
    raise ValueError(kind)


def total_frames(name: str) -> int:
    c = CASES[name]
    return c["n"] * len(c["plan"][0]) - (c["n"] - c["tail"] if c["tail"] else 0)


def channels(name: str) -> np.ndarray:
    """int64 [C][frames]"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    n, scale = c["n"], 256 if c["ss"] == 24 else 1
    rows = []
    for plan in c["plan"]:
        blocks = []
        for b, kind in enumerate(plan):
            if kind.startswith("+"):
                blocks.append(rows[int(kind[1:])][b * n:(b + 1) * n] + rng.integers(-3, 4, n))
            else:
                blocks.append(signal(kind, n, rng, scale))
        rows.append(np.concatenate(blocks))
    return np.stack(rows)[:, :total_frames(name)]


def samples_sha256(name: str) -> str:
    return hashlib.sha256(channels(name).astype("<i8").tobytes()).hexdigest()


def n_blocks(name: str) -> int:
    return len(CASES[name]["plan"][0])


def unit_rows(name: str):
    """(rows [n_blocks * C][n] of int16 / int32, zero padded; unit lengths): row f * C + k is
    channel k of block f, the batch layout of the analysis."""
    c = CASES[name]
    x = channels(name)
    nb, C, n = n_blocks(name), c["C"], c["n"]
    rows = np.zeros((nb * C, n), dtype=np.int16 if c["ss"] <= 16 else np.int32)
    lens = []
    for f in range(nb):
        ln = min(n, x.shape[1] - f * n)
        for k in range(C):
            rows[f * C + k, :ln] = x[k, f * n:f * n + ln]
            lens.append(ln)
    return rows, lens


def analysis_units(n: int = 192, seed: int = 31) -> np.ndarray:
    """The 12 units of the GPU analysis test: 4 AR, 3 tone, 3 noise, digital silence, full scale."""
    rng = np.random.default_rng(seed)
    kinds = ["ar"] * 4 + ["tone"] * 3 + ["noise"] * 3 + ["zero", "full"]
    return np.stack([signal(k, n, rng) for k in kinds]).astype(np.int16)


def narrow_units(n: int = 192, seed: int = 1) -> np.ndarray:
    """6 int32 units of a 24-bit stream whose data fits 12 bits (a faint AR(2) in +-30 of noise): the
    choice at the written width 24 differs from the choice at the measured width 12 on some."""
    rng = np.random.default_rng(seed)
    rows = np.stack([signal("ar", n, rng) // 64 + rng.integers(-30, 31, n) for _ in range(6)]).astype(np.int32)
    assert np.abs(rows).max() < 2048
    return rows
