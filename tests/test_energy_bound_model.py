"""The energy bound (tests/energy_bound_model.py) against the CPU oracle's exact LPC
sums, no device: for every unit and every order the bound stays at or below the exact sum, so a
unit it decides loses in the oracle; and it decides most of the headline workload's units."""
import functools

import numpy as np
import pytest

import energy_bound_model as M
import oracle
from flac_amd import abi
from test_gpu_parity import _prune_signals

LENGTHS = (64, 128, 192, 1024, 4096, 4608, 10240)


def rmax_for(n):
    """The largest -r 0,rmax (<= 5) the stream kernel takes at n: whole 8-sample chunks per finest partition."""
    return max(o for o in range(6) if n % (1 << o) == 0 and ((n >> o) & 7) == 0)


def special_units(n):
    """Full-scale alternation, silence plus one spike, DC, a quiet and a loud pure tone (long
    predictors: large coefficients, negative shifts), silence; and -1 and -2 over the window's
    rectangle alone, zero in the tapers: the whole signal counts at full weight, the properly
    signed predictor leaves almost nothing and floor() rounds every residual towards zero, so
    the bound comes within n of the exact sums (it fails without its "- n" term)."""
    t = np.arange(n)
    mid = (t >= n // 4) & (t < 3 * n // 4)
    rows = [np.where(t % 2 == 0, 32767, -32768), np.where(t == n // 2, 30000, 0), np.full(n, 1234),
            np.round(300 * np.sin(2 * np.pi * t / 97.0)), np.round(30000 * np.sin(2 * np.pi * t / 61.0)), np.zeros(n),
            np.where(mid, -1, 0), np.where(mid, -2, 0)]
    return np.array(rows).astype(np.int16)


def check_units(a, n, L, q):
    """bound <= exact for every (unit, order) -> (usable units, decided units, worst bound / exact)."""
    ora = oracle.analyze_batch(a, oracle.make_params(L, q, 0, rmax_for(n)), n, sample_bits=16, threads=8)
    usable = decided = 0
    worst = 0.0
    for u in range(len(a)):
        st, site = int(ora["meta"]["status"][u]), int(ora["meta"]["site"][u])
        rec = ora["lpc_records"][u]
        if int(rec[0]) != 0:
            assert M.lower_bound(a[u][:n], ora["acf"][u], rec, L) is None, (n, L, q, u)
            continue
        if st != 0 and site != abi.SITE_CHOICE_TIE and not ora["lpc_sums"][u][:L].any():
            continue  # raised before the candidate sums
        b = M.lower_bound(a[u][:n], ora["acf"][u], rec, L)
        if b is None:
            assert int(rec[1]) != 0, (n, L, q, u)
            continue
        usable += 1
        exact = int(ora["lpc_sums"][u][:L].min())
        assert b <= 256 * exact, (n, L, q, u, b / 256.0, exact)
        worst = max(worst, b / 256.0 / max(exact, 1))
        dec = M.decides(a[u][:n], ora["acf"][u], rec, L, ora["fixed_sums"][u])
        if dec:
            assert exact > int(ora["fixed_sums"][u].min()), (n, L, q, u)
        decided += dec
    return usable, decided, worst


@functools.lru_cache(maxsize=None)
def c2_units():
    a = oracle.synth_batch(0, 200, 4608, 16, 2024, dtype=np.int16)
    a.setflags(write=False)
    return a


def test_headline_units_bound_holds_and_decides_most():
    usable, decided, worst = check_units(c2_units(), 4608, 12, 5)
    print("config-2 units: usable", usable, "decided", decided, "worst bound / exact %.3f" % worst)
    assert usable == 200 and decided >= 0.75 * 200, (usable, decided)


def test_open_mix_units():
    a = oracle.synth_batch(0, 100, 4608, 16, 2024, dtype=np.int16, open_eighths=5)
    usable, decided, worst = check_units(a, 4608, 12, 5)
    print("open 5/8 units: usable", usable, "decided", decided, "worst bound / exact %.3f" % worst)
    assert usable >= 90 and decided >= 10, (usable, decided)


@pytest.mark.parametrize("q", [5, 6, 9])
def test_near_ties_and_special_units(q):
    n = 4608
    a = np.concatenate([_prune_signals(n, 50 + q), special_units(n)])
    usable, decided, worst = check_units(a, n, 12, q)
    print("q", q, "usable", usable, "decided", decided, "worst bound / exact %.3f" % worst)
    assert usable >= 40 and worst <= 1.0


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_orders_precisions(n):
    a = np.concatenate([oracle.synth_batch(0, 10, n, 16, 300 + n, dtype=np.int16),
                        oracle.synth_batch(0, 10, n, 16, 400 + n, dtype=np.int16, open_eighths=5), special_units(n)])
    seen = 0
    for L in (3, 4, 8, 12):
        for q in (5, 6):
            usable, decided, worst = check_units(a, n, L, q)
            seen += usable
    assert seen >= 8 * 15, (n, seen)


def test_window_tables():
    """Chunks 0, 1 and the last one weigh nothing; inside the rectangle a chunk weighs 256; kappa
    grows with the lag and stays below the taper's steepest k-sample step."""
    for n in LENGTHS:
        kappa, cw = M.tables(n)
        _, w = oracle.tukey(n)
        assert w[0] == 0.0 and w[n - 1] == 0.0
        assert cw[0] == 0 and cw[1] == 0 and cw[-1] == 0 and cw.max() <= 256
        if n >= 256:
            assert cw[n // 16] == 256
        nr = n // 4 - 1
        assert all(0.0 < kappa[k] <= kappa[k + 1] for k in range(M.LAGS - 1))
        assert all(kappa[k - 1] <= min(1.0, 0.5 * np.pi * k / nr) * (1 + 1e-9) for k in range(1, M.LAGS + 1))
