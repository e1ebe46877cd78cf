"""The tiny streams of tests/golden/rice_search_streams.json (the exact Rice search,
FLACMI_FLAG_RICE_SEARCH), rebuilt from seeds: make_rice_search_golden.py feeds them to the
reference's encode() with its rice_partitions replaced by the rule, the tests feed them to the
model and to the device.

Gated signals: AR(2) noise x[i] = 1.6 x[i-1] - 0.8 x[i-2] + N(0, sigma), with a stretch of every
block set to digital silence (even blocks) or to sparse +-1 (odd blocks), never a whole block: the
reference's find_rice_parameter then has no value (a partition sum of 0, site 12) or a negative one
(a mean below 1, site 13) in some partition of some candidate order, and fails the unit.
"""
import hashlib

import numpy as np

CASES = {
    # 16-bit mono, every candidate order of 192 in range
    "gate16m": dict(C=1, ss=16, n=192, frames=5 * 192, L=8, q=5, rmin=0, rmax=4, rate=44100, seed=11, kind="gated"),
    # 16-bit stereo, rice_min > 0
    "gate16s": dict(C=2, ss=16, n=192, frames=4 * 192, L=8, q=5, rmin=1, rmax=3, rate=44100, seed=12, kind="gated"),
    # 24-bit, loud in the first half of every block only: parameters above 14 in some partitions (method 5)
    "loud24": dict(C=1, ss=24, n=256, frames=3 * 256, L=4, q=5, rmin=0, rmax=5, rate=44100, seed=13, kind="loud"),
    # a short last block of odd length (order 0 only there)
    "tail16": dict(C=1, ss=16, n=192, frames=2 * 192 + 77, L=8, q=5, rmin=0, rmax=4, rate=44100, seed=14, kind="gated"),
    # an odd block length: order 0 only in every block
    "odd16": dict(C=2, ss=16, n=255, frames=3 * 255, L=6, q=5, rmin=0, rmax=3, rate=44100, seed=15, kind="gated"),
}


def ar2(rng, total: int, sigma: float) -> np.ndarray:
    e = rng.normal(0.0, sigma, total)
    x = np.zeros(total)
    for i in range(total):
        x[i] = e[i] + (1.6 * x[i - 1] if i >= 1 else 0.0) - (0.8 * x[i - 2] if i >= 2 else 0.0)
    return np.rint(x).astype(np.int64)


def gated(rng, total: int, n: int, sigma: float = 400.0) -> np.ndarray:
    x = ar2(rng, total, sigma)
    for b, b0 in enumerate(range(0, total, n)):
        ln = min(n, total - b0)
        g0 = b0 + ln // 4 + int(rng.integers(0, ln // 8))
        g1 = min(b0 + ln - ln // 8, g0 + ln // 3 + int(rng.integers(0, ln // 8)))
        x[g0:g1] = 0
        if b % 2:
            idx = g0 + rng.choice(g1 - g0, size=max(1, (g1 - g0) // 12), replace=False)
            x[idx] = rng.choice([-1, 1], size=len(idx))
    return np.clip(x, -32768, 32767)


def loud(rng, total: int, n: int) -> np.ndarray:
    x = rng.integers(-100, 101, total)
    for b0 in range(0, total, n):
        x[b0:b0 + n // 2] = rng.integers(-(1 << 22), 1 << 22, n // 2)
    return x.astype(np.int64)


def channels(name: str) -> np.ndarray:
    """int64 [C][frames]"""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    rows = []
    for _ in range(c["C"]):
        rows.append(gated(rng, c["frames"], c["n"]) if c["kind"] == "gated" else loud(rng, c["frames"], c["n"]))
    return np.stack(rows)


def samples_sha256(name: str) -> str:
    return hashlib.sha256(channels(name).astype("<i8").tobytes()).hexdigest()


def n_blocks(name: str) -> int:
    c = CASES[name]
    return (c["frames"] + c["n"] - 1) // c["n"]


def tail_len(name: str) -> int:
    c = CASES[name]
    return c["frames"] % c["n"]


def unit_rows(name: str):
    """(rows [n_blocks * C][n] of int16 / int32, zero padded; unit lengths): row f * C + k is
    channel k of block f, the batch layout of the analysis."""
    c = CASES[name]
    x = channels(name)
    nb, C, n = n_blocks(name), c["C"], c["n"]
    rows = np.zeros((nb * C, n), dtype=np.int16 if c["ss"] <= 16 else np.int32)
    lens = []
    for f in range(nb):
        ln = min(n, c["frames"] - f * n)
        for k in range(C):
            rows[f * C + k, :ln] = x[k, f * n:f * n + ln]
            lens.append(ln)
    return rows, lens
