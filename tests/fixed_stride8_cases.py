"""Inputs of tests/test_gpu_fixed_stride8.py (k_resid_stream's fixed group at row stride 8), made
once per block length, and the numpy fixed sums that state what the inputs must be.  Test
infrastructure only; importing it needs no GPU.

Per block length n:
  (a) five units in which fixed order 0, 1, 2, 3, 4 has the smallest fixed sum in turn: a polynomial
      of that degree plus +-1 noise (order 0: the noise alone, its sign flipping three times in four, so
      that its first difference costs more than itself).  Where no polynomial inside 16 bits does it (a long
      block: its high differences vanish against the noise's), the unit is a sine arc of period 63,
      locally a polynomial, with the amplitude that puts its order - 1 difference above the noise
      and its order difference below.  winners() states the property, without the device;
  (b) +-1 noise with one +-30000 sample at position j, j = 0..8, 63, 64, 65, 127, 128, 129, n - 2, n - 1
      (those inside the block): the warm-up mask, the phase map, the step and wave seams;
  (c) full-scale alternation, both phases;
  (d) 16 units of the bench generator (oracle.synth_batch)."""
import functools

import numpy as np

import oracle

# n -> (rice_min, rice_max) as tests/stream_shape_cases.py picks them: the largest order whose
# finest partitions are whole 8-sample chunks
LENGTHS = {64: (0, 3), 128: (0, 4), 192: (0, 3), 320: (0, 2), 2880: (0, 3), 4608: (0, 5), 10240: (0, 5)}
SPIKES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 127, 128, 129, -2, -1)
Q = 5


def fixed_sums(x):
    """The five fixed sums of one unit (warm-up samples excluded), as the reference defines them."""
    r = np.asarray(x, dtype=np.int64)
    out = [int(np.abs(r).sum())]
    for _ in range(4):
        r = np.diff(r)
        out.append(int(np.abs(r).sum()))
    return out


def winner_unit(n, d, rng):
    """-> (unit, 'poly' or 'arc') whose smallest fixed sum is order d's (first minimum)."""
    t = np.arange(n, dtype=np.float64)
    noise = 2 * rng.integers(0, 2, n) - 1
    if d == 0:
        flips = rng.integers(0, 4, n) < 3
        return np.where(np.cumsum(flips) & 1, -1, 1).astype(np.int16), "poly"
    amp = 32000.0
    while amp >= 1.0:
        x = np.rint(amp * (2.0 * t / n - 1.0) ** d).astype(np.int64) + noise
        if int(np.argmin(fixed_sums(x))) == d:
            return x.astype(np.int16), "poly"
        amp /= 2.0
    w = 2.0 * np.pi / 63.0
    x = np.rint(min(20.0 / w ** (d - 1), 32000.0) * np.sin(w * t)).astype(np.int64) + noise
    return x.astype(np.int16), "arc"


@functools.lru_cache(maxsize=None)
def units(n):
    """-> (read-only int16 array [units][n], labels)."""
    rng = np.random.default_rng(8000 + n)
    rows, labels = [], []
    for d in range(5):
        x, kind = winner_unit(n, d, rng)
        rows.append(x)
        labels.append(f"order{d}-{kind}")
    for k, j in enumerate(sorted({j % n for j in SPIKES if -n <= j < n})):
        x = (2 * rng.integers(0, 2, n) - 1).astype(np.int16)
        x[j] = 30000 if k % 2 == 0 else -30000
        rows.append(x)
        labels.append(f"spike{j}")
    alt = np.where(np.arange(n) & 1, -32768, 32767).astype(np.int16)
    rows += [alt, np.roll(alt, 1)]
    labels += ["alt+", "alt-"]
    for x in oracle.synth_batch(0, 16, n, 16, 4242 + n, dtype=np.int16):
        rows.append(np.array(x[:n]))
        labels.append("bench")
    a = np.stack(rows)
    a.setflags(write=False)
    return a, tuple(labels)


def winners(n):
    """The (a) units' orders of smallest fixed sum: must be [0, 1, 2, 3, 4]."""
    a, _ = units(n)
    return [int(np.argmin(fixed_sums(a[d]))) for d in range(5)]


@functools.lru_cache(maxsize=None)
def reference(n, L):
    """The oracle's results for units(n): reference mode at L, or fixed-only mode (L = 0)."""
    from flac_amd import abi
    a, _ = units(n)
    rmin, rmax = LENGTHS[n]
    mode = abi.MODE_REFERENCE if L else abi.MODE_FIXED_ONLY
    ora = oracle.analyze_batch(a, oracle.make_params(L, Q, rmin, rmax, mode), n, sample_bits=16, threads=16)
    for v in ora.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ora
