"""The order-1 closed form and the energy bound over orders 2 .. L (tests/order1_bound_model.py,
DESIGN §4) against the CPU oracle's exact LPC sums, no device: neither bound exceeds the exact
sum of an order it speaks for, a unit the second test decides is one the quarter tiers decide
too (min exact - 2 n - 1024 > best fixed sum), and the two tests together decide nearly every
unit of the headline workload.  (**mut: the model's mutation switches, passed on to
order1_bound_model when the mutations DESIGN §4 records are run by hand; pytest passes none.)"""
import numpy as np
import pytest

import energy_bound_model as M
import oracle
import order1_bound_model as O
from flac_amd import abi
from test_energy_bound_model import c2_units, rmax_for, special_units
from test_gpu_parity import _prune_signals

LENGTHS = (64, 128, 192, 576, 4096, 10240)


def check_units(a, n, L, q, **mut):
    """Both bounds against every order's exact sum, and the tiers' verdict on every unit the
    second test decides -> (usable units, decided by the first test, added by the second)."""
    ora = oracle.analyze_batch(a, oracle.make_params(L, q, 0, rmax_for(n)), n, sample_bits=16, threads=8)
    usable = first = added = 0
    for u in range(len(a)):
        st, site = int(ora["meta"]["status"][u]), int(ora["meta"]["site"][u])
        rec, fs = ora["lpc_records"][u], ora["fixed_sums"][u]
        if int(rec[0]) != 0:
            assert O.bounds(a[u][:n], ora["acf"][u], rec, L, fs) is None, (n, L, q, u)
            continue
        if st != 0 and site != abi.SITE_CHOICE_TIE and not ora["lpc_sums"][u][:L].any():
            continue  # raised before the candidate sums
        b = O.bounds(a[u][:n], ora["acf"][u], rec, L, fs, **mut)
        if b is None:
            assert int(rec[1]) != 0, (n, L, q, u)
            continue
        usable += 1
        exact = [int(v) for v in ora["lpc_sums"][u][:L]]
        b1, s, br = b
        assert b1 <= exact[0] << s, (n, L, q, u, "order 1", b1 / float(1 << s), exact[0])
        assert (br is None) == (L == 1), (n, L, q, u)
        for p in range(2, L + 1):
            assert br <= 256 * exact[p - 1], (n, L, q, u, "order", p, br / 256.0, exact[p - 1])
        fmin = int(fs.min())
        if M.decides(a[u][:n], ora["acf"][u], rec, L, fs):
            first += 1
        elif O.decides(a[u][:n], ora["acf"][u], rec, L, fs, **mut):
            assert min(exact) - 2 * n - 1024 > fmin, (n, L, q, u, min(exact), fmin)
            added += 1
    return usable, first, added


def test_headline_units_bounds_hold_and_decide_nearly_all(**mut):
    usable, first, added = check_units(c2_units(), 4608, 12, 5, **mut)
    print("config-2 units: usable", usable, "first test", first, "second test adds", added)
    assert usable == 200 and first + added >= 190, (usable, first, added)


def test_open_mix_units(**mut):
    a = oracle.synth_batch(0, 100, 4608, 16, 2024, dtype=np.int16, open_eighths=5)
    usable, first, added = check_units(a, 4608, 12, 5, **mut)
    print("open 5/8 units: usable", usable, "first test", first, "second test adds", added)
    assert usable >= 90, usable


@pytest.mark.parametrize("q", [5, 6, 9])
def test_near_ties_and_special_units(q, **mut):
    n = 4608
    a = np.concatenate([_prune_signals(n, 50 + q), special_units(n)])
    usable, first, added = check_units(a, n, 12, q, **mut)
    print("q", q, "usable", usable, "first test", first, "second test adds", added)
    assert usable >= 40, usable


def floor_units(n):
    """-1 (and -2) with a zero every k samples: order 1's coefficient stays off -2^shift, so
    floor(c x / 2^s) rounds most residuals towards zero and the closed form comes within n of the
    exact sum (it fails without its "- 2^s n" term, which the other units do not show)."""
    t = np.arange(n)
    rows = [np.where(t % k == 0, 0, -1) for k in (5, 8, 12)] + [np.where(t % 7 == 0, 0, -2)]
    return np.array(rows).astype(np.int16)


@pytest.mark.parametrize("n", [192, 4608])
def test_floor_term_units(n, **mut):
    seen = 0
    for L in (1, 12):
        seen += check_units(floor_units(n), n, L, 5, **mut)[0]
    assert seen >= 4, seen


def test_closed_form_any_coefficient(**mut):
    """The closed form holds for any coefficient and shift, not only those the quantiser gives
    the unit at hand: against sum |x_i - floor(c x_{i-1} / 2^s)| computed here.  On 16-bit units of
    these lengths the quantiser's own c_1 is -2^s wherever the closed form comes near the exact
    sum (a constant: floor() then rounds nothing), so only this check needs the "- 2^s n" term:
    a constant -32753 under c = -15, s = 4 leaves 15/16 to floor() at every sample."""
    rng = np.random.default_rng(5)
    for n in (64, 576, 4608):
        units = list(floor_units(n)) + list(special_units(n)) + [np.full(n, -32753), np.full(n, 32753), np.full(n, -32768),
                                                                 rng.integers(-32768, 32768, n), np.cumsum(rng.integers(-40, 41, n))]
        for x in units:
            x = np.asarray(x, dtype=np.int64)
            f0, f1 = int(np.abs(x).sum()), int(np.abs(np.diff(x)).sum())
            for s in (0, 4, 9, 15):
                for c in {-(1 << s), -(1 << s) + 1, -15, -1, 0, 1, 7, (1 << s) - 1, -32768, 32767}:
                    exact = int(np.abs(x[1:] - ((c * x[:-1]) >> s)).sum())
                    b, s2 = O.order1_bound((c & 0xFFFF) | (s << 16), n, f0, f1, **mut)
                    assert s2 == s and b <= exact << s, (n, int(x[0]), int(x[1]), c, s, b / float(1 << s), exact)


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_orders(n, **mut):
    a = np.concatenate([oracle.synth_batch(0, 10, n, 16, 300 + n, dtype=np.int16),
                        oracle.synth_batch(0, 10, n, 16, 400 + n, dtype=np.int16, open_eighths=5), special_units(n)])
    seen = 0
    for L in (1, 2, 8, 12):
        for q in (5, 6):
            seen += check_units(a, n, L, q, **mut)[0]
    assert seen >= 8 * 15, (n, seen)


def test_new_words():
    """L = 1 leaves no order for the second pair: (0, 0), which passes whatever the sums; the
    order-1 word gives back a negative coefficient and its shift."""
    n = 4608
    a = c2_units()[:4]
    ora = oracle.analyze_batch(a, oracle.make_params(1, 5, 0, 5), n, sample_bits=16, threads=8)
    kappa, _ = M.tables(n)
    for u in range(len(a)):
        w = O.words(ora["acf"][u], ora["lpc_records"][u], 1, n, kappa)
        assert w is not None and w[:2] == (0, 0), (u, w)
        assert O.rest_bound(a[u], 0, 0, int(ora["fixed_sums"][u][0])) is None
        m = O.margins(a[u], ora["acf"][u], ora["lpc_records"][u], 1, ora["fixed_sums"][u])
        assert m[0] is None
        assert O.unpack_order1(w[2]) == (int(ora["lpc_records"][u][2 + 32]), int(ora["lpc_records"][u][2]))
    for c in (-32768, -15, -1, 0, 1, 15, 32767):
        for s in (0, 4, 15):
            assert O.unpack_order1((c & 0xFFFF) | (s << 16)) == (c, s)
    # a unit whose first pair is unusable (a status, a negative-shift order) has no new words
    sp = special_units(n)
    ob = oracle.analyze_batch(sp, oracle.make_params(12, 5, 0, 5), n, sample_bits=16, threads=8)
    unusable = [u for u in range(len(sp)) if int(ob["lpc_records"][u][0]) != 0 or int(ob["lpc_records"][u][1]) != 0]
    assert len(unusable) >= 1, unusable
    for u in unusable:
        assert O.words(ob["acf"][u], ob["lpc_records"][u], 12, n, kappa) is None, u
