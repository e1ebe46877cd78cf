"""k_resid_stream's fixed group at row stride 8 (flac-py_amd/csrc/k_stream.hip, kFixB8a/kFixB8b and
fixed8), restated in numpy: no device.

A step is 128 samples.  MFMA row m (0..15) holds the 16-sample window 8m - 8 .. 8m + 7 of biased
samples u = x + 32768 split into bytes, as f16 values 1024 + byte: K index 8 kb + j is the high
byte (j < 4) or the low byte (j >= 4) of sample 8m - 8 + 4 kb + (j & 3).  Two B operands take the
same A: table t holds orders 2t + 1 and 2t + 2, column = 8 (order index) + phase rho, and its K
entry is 256 T[ia - j] (high bytes) or T[ia - (j - 4)] (low bytes) with ia = 8 + rho - 4 kb and T
the predictor's taps (T[0] = -1 for x[i] itself).  With the accumulator at C = 1.5 * 2^23 the
result is C - r for the fixed residual r of sample 8m + rho: the taps sum to zero, so the raw
operand's offset (256 * 1152 + 1024 per sample) cancels.  Exactness needs every partial sum inside
[2^23, 2^24) whatever the accumulation order: |partial - C| < 2^23, checked here for several
orders and for the worst one (every positive product first)."""
import math

import numpy as np
import pytest

C = 3 << 22  # 1.5 * 2^23


def fixed_tap(p, j):
    """k_stream.hip fixed_tap: T[0] = -1, T[j] = (-1)^(j-1) C(p, j) for 1 <= j <= p, else 0."""
    if j == 0:
        return -1
    if j < 0 or j > p:
        return 0
    return math.comb(p, j) * (1 if j & 1 else -1)


def b_table(t):
    """[32 K][16 columns] of table t, as the device lays it out (lane = 16 kb + column holds K
    entries 8 kb .. 8 kb + 7)."""
    b = np.zeros((32, 16), dtype=np.int64)
    for col in range(16):
        p, rho = 2 * t + (col >> 3) + 1, col & 7
        for kb in range(4):
            ia = 8 + rho - 4 * kb
            for j in range(4):
                b[8 * kb + j, col] = 256 * fixed_tap(p, ia - j)
                b[8 * kb + 4 + j, col] = fixed_tap(p, ia - j)
    return b


def a_rows(x, step):
    """[16 rows][32 K] of one step: raw operand values 1024 + byte of the biased samples behind a
    16-sample pad of biased zeros."""
    u = np.concatenate([np.full(16, 0x8000, dtype=np.int64), x.astype(np.int64) + 32768])
    a = np.zeros((16, 32), dtype=np.int64)
    for m in range(16):
        for kb in range(4):
            for j in range(4):
                s = u[16 + 128 * step + 8 * m - 8 + 4 * kb + j]
                a[m, 8 * kb + j] = 1024 + (s >> 8)
                a[m, 8 * kb + 4 + j] = 1024 + (s & 255)
    return a


def fixed_residual(x, p):
    """Order p residual at every position, zeros in front of the unit (the device masks i < p)."""
    r = np.concatenate([np.zeros(p, dtype=np.int64), x.astype(np.int64)])
    for _ in range(p):
        r = np.diff(r)
    return r


def k_orders(rng):
    """Accumulation orders over the 32 K entries: ascending, descending, the four 8-blocks
    interleaved, low bytes first, and random ones."""
    asc = np.arange(32)
    yield asc
    yield asc[::-1]
    yield asc.reshape(4, 8).T.ravel()
    yield np.concatenate([asc.reshape(4, 8)[:, 4:].ravel(), asc.reshape(4, 8)[:, :4].ravel()])
    for _ in range(4):
        yield rng.permutation(32)


def check_unit(x, rng):
    """-> the largest |partial sum - C| seen."""
    assert len(x) % 128 == 0
    tables = [b_table(0), b_table(1)]
    res = {p: fixed_residual(x, p) for p in range(1, 5)}
    worst = 0
    for step in range(len(x) // 128):
        a = a_rows(x, step)
        for t in range(2):
            prod = a[:, :, None] * tables[t][None, :, :]  # [row][K][column]
            d = prod.sum(axis=1)
            for col in range(16):
                p, rho = 2 * t + (col >> 3) + 1, col & 7
                want = -res[p][128 * step + 8 * np.arange(16) + rho]
                assert np.array_equal(d[:, col], want), (step, t, col)
            for order in k_orders(rng):
                worst = max(worst, int(np.abs(np.cumsum(prod[:, order, :], axis=1)).max()))
            # the worst order: every positive product, then every negative one (and the reverse)
            worst = max(worst, int(np.where(prod > 0, prod, 0).sum(axis=1).max()),
                        int(-np.where(prod < 0, prod, 0).sum(axis=1).min()))
    return worst


def units():
    rng = np.random.default_rng(8)
    yield "random", rng.integers(-32768, 32768, 256).astype(np.int16)
    alt = np.where(np.arange(256) & 1, -32768, 32767).astype(np.int16)
    yield "alternating", alt
    yield "alternating-", (-1 - alt.astype(np.int32)).astype(np.int16)
    for j in range(9):
        for big in (30000, -30000, 32767, -32768):
            x = rng.integers(-1, 2, 128).astype(np.int16)
            x[j] = big
            yield f"spike{j}:{big}", x


@pytest.mark.parametrize("name,x", list(units()), ids=[n for n, _ in units()])
def test_stride8_operands_give_the_fixed_residuals(name, x):
    worst = check_unit(x, np.random.default_rng(len(name)))
    assert worst < 2 ** 23, (name, worst)


def test_tables_hold_every_tap_once_per_phase():
    """Column (order, rho) of a table holds exactly the taps T[0..order], each once, as the pair
    (256 T, T), and the window never needs a tap index above 15."""
    for t in range(2):
        b = b_table(t)
        for col in range(16):
            p = 2 * t + (col >> 3) + 1
            hi = sorted(int(v) // 256 for v in b[:, col].reshape(4, 8)[:, :4].ravel() if v)
            lo = sorted(int(v) for v in b[:, col].reshape(4, 8)[:, 4:].ravel() if v)
            taps = sorted(fixed_tap(p, j) for j in range(p + 1))
            assert hi == taps and lo == taps, (t, col)
            assert b[:, col].sum() == 0  # the raw operand's offset cancels
    assert max(8 + 7 - 4 * 0, 0) <= 15 and 7 + 4 <= 11
