"""The wasted-bits rule of include/flacmi.h (flacmi_wasted_rows_device) restated in numpy, for the
tests of k_wasted_rows: with m the bitwise OR of a unit's samples in two's complement, w = 0 when
m == 0, otherwise the number of trailing zero bits of m, clamped to sample_bits - 1; the unit is
then x >> w (arithmetic, exact) at sample_bits - w bits.  Also the sizes that follow from the
subframe header alone: its 8 + w bits (w - 1 zeros and a one behind the set flag bit; 8 for
w == 0), and the CONSTANT and VERBATIM subframes at the unit's own width."""
import numpy as np


def wasted_of(samples: np.ndarray, sample_bits: int) -> int:
    """w of one unit (a 1-D integer array of its samples, nothing behind its length)."""
    m = int(np.bitwise_or.reduce(np.asarray(samples, dtype=np.int64))) & ((1 << 64) - 1)
    if m == 0:
        return 0
    return min((m & -m).bit_length() - 1, sample_bits - 1)


def wasted_of_loop(samples, sample_bits: int) -> int:
    """The same by the definition, sample by sample: the largest k <= sample_bits - 1 such that
    2^k divides every sample; 0 for digital silence."""
    xs = [int(x) for x in samples]
    if not any(xs):
        return 0
    k = 0
    while k < sample_bits - 1 and all(x % (1 << (k + 1)) == 0 for x in xs):
        k += 1
    return k


def header_bits(w: int) -> int:
    """0 tttttt 0 for w == 0; 0 tttttt 1, w - 1 zeros and a one otherwise"""
    return 8 + w


def constant_bits(w: int, sample_bits: int) -> int:
    return header_bits(w) + (sample_bits - w)


def verbatim_bits(n: int, w: int, sample_bits: int) -> int:
    return header_bits(w) + n * (sample_bits - w)


def shifted(samples: np.ndarray, w: int) -> np.ndarray:
    """The unit the subframe is analysed and written from, in the input's element type."""
    return np.asarray(samples) >> w


def unit_with(n: int, sample_bits: int, w: int, at: int, dtype, rng) -> np.ndarray:
    """n random samples of sample_bits bits whose wasted bits are exactly w because of the one
    sample at index `at`: every other sample is a multiple of 2^(w + 1).  w = sample_bits - 1
    leaves -2^(sample_bits - 1) at `at` and zeros elsewhere."""
    lo, hi = -(1 << (sample_bits - 1)), (1 << (sample_bits - 1)) - 1
    if w == sample_bits - 1:
        x = np.zeros(n, dtype=np.int64)
        x[at] = lo
        return x.astype(dtype)
    x = rng.integers(lo, hi + 1, size=n, dtype=np.int64) & ~((1 << (w + 1)) - 1)
    x[at] |= 1 << w
    return x.astype(dtype)
