"""k_resid_stream's energy-bound pre-test (k_lpc writes two words per unit from its
autocorrelation, the stream kernel proves from them, the order-0 sum and a window-weighted sum
gathered in staging that every LPC order loses, and runs no LPC group at all) against the CPU
oracle and the CPU model of the bound (tests/energy_bound_model.py), at the smallest shapes at
which it can go wrong: one nearly empty chunk slot (n = 64), the taper's end inside a chunk
(576), the runtime-shape and the constant-shape builds (4096 L 8, 4608 L 12), four waves
(10240), L off a multiple of 4, units whose words are unusable (a status, a negative-shift
order), near-tie tones that must reach the exact pass, and a tail class.

Every call runs under FLACMI_ENERGY_BOUND 0 (the tiers alone), 1 (pre-test, then the tiers) and
2 (pre-test, then the exact pass); under 2 meta.lpc_tiers says which units the pre-test decided
(1/4, pruned) and which it did not (5/4), and the model must agree wherever its bound is not
within 2% of the best fixed sum."""
import functools

import numpy as np
import pytest

import energy_bound_model as M
import oracle
import stream_shape_cases as S
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params
from test_energy_bound_model import special_units
from test_gpu_parity import _prune_signals, compare_with_oracle

pytestmark = pytest.mark.gpu

KNOB = "FLACMI_ENERGY_BOUND"
# (n, L, q, rmin, rmax)
CASES = [(64, 12, 5, 0, 3), (128, 4, 5, 0, 4), (192, 7, 5, 0, 3), (576, 10, 5, 0, 3), (4096, 8, 5, 0, 5),
         (4608, 12, 5, 0, 5), (4608, 11, 6, 0, 5), (10240, 12, 5, 0, 5)]
TAIL = (4608, 3328, 8, 6, 6)  # block, tail, L, q, units cut to the tail


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def make_units(n, seed):
    """80 units: 24 config-2 units (mostly decided), AR(1) and white noise and noisy tones
    (near ties: the exact pass), 24 of the bench's open mix, and the special units."""
    a = np.concatenate([_prune_signals(n, seed), oracle.synth_batch(0, 24, n, 16, seed + 1, dtype=np.int16, open_eighths=5),
                        special_units(n)])
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case_reference(case):
    n, L, q, rmin, rmax = case
    assert S.stream_shape(n, L, rmin, rmax, False) is not None and S.narrow_path(n, L, q, False), case
    a = make_units(n, 900 + n + L)
    ora = oracle.analyze_batch(a, oracle.make_params(L, q, rmin, rmax), n, sample_bits=16, threads=16)
    for v in ora.values():
        v.setflags(write=False)
    return a, ora


def model_verdicts(a, ora, L, lens):
    """Per unit: None (not the batch kernel's, or it raised before the choice), else (the model's
    bound times 256 or None where the words are unusable, 256 times the best fixed sum)."""
    out = []
    for u, k in enumerate(S.classify(a, ora, L, lens)):
        if k != "batch":
            out.append(None)
            continue
        n = lens[u]
        out.append((M.lower_bound(a[u][:n], ora["acf"][u], ora["lpc_records"][u], L), 256 * int(ora["fixed_sums"][u].min())))
    return out


def check_knob2_marks(meta, verdicts):
    """Under knob 2 the batch kernel's units are marked 1/4 (decided, pruned) or 5/4 (exact pass)."""
    t = meta["lpc_tiers"].astype(np.int64)
    decided = undecided = 0
    for u, v in enumerate(verdicts):
        if v is None:
            continue
        b, f = v
        low, pruned = int(t[u]) & 0xff, int(meta["lpc_order"][u]) == abi.LPC_PRUNED
        assert int(t[u]) >> 8 == 4 and low in (1, 5) and pruned == (low == 1), (u, int(t[u]), pruned)
        if b is not None and b > 1.02 * f:
            assert low == 1, (u, "the model decides with margin, the device did not", b / 256.0, f / 256.0)
        if b is None or b < 0.98 * f:
            assert low == 5, (u, "the device decided a unit the model does not", b, f / 256.0)
        decided += low == 1
        undecided += low == 5
    return decided, undecided


def assert_same_results(x, y, lens):
    for f in abi.META_DTYPE.names:
        if f != "lpc_tiers":
            assert np.array_equal(x["meta"][f], y["meta"][f]), f
    assert np.array_equal(x["rice_params"], y["rice_params"])
    for u, n in enumerate(lens):
        assert np.array_equal(x["residual"][u][:n], y["residual"][u][:n]), u


def run_knobs(az, a, ora, params, block, lens, L, tail=(0, 0)):
    """Production calls under knob 0, 1, 2 and the debug call against the oracle; the marks
    against the model -> (decided, undecided) under knob 2."""
    verdicts = model_verdicts(a, ora, L, lens)
    outs = {}
    for k in (0, 1, 2):
        with knob(KNOB, k):
            outs[k] = az.analyze(a, params, block, tail[0], tail[1], sample_bits=16, extras=("acf", "lpc_records"))
        compare_with_oracle({f: outs[k][f] for f in ("meta", "rice_params", "residual")}, ora, lens)
        # k_lpc's autocorrelation and records: the same bits with and without the bound words
        ok = ora["meta"]["status"] == 0
        assert np.array_equal(outs[k]["acf"][ok].view(np.uint64), ora["acf"][ok].view(np.uint64)), k
        assert np.array_equal(outs[k]["lpc_records"][ok], ora["lpc_records"][ok]), k
        if k:
            assert np.array_equal(outs[k]["acf"].view(np.uint64), outs[0]["acf"].view(np.uint64)), k
            assert np.array_equal(outs[k]["lpc_records"], outs[0]["lpc_records"]), k
    compare_with_oracle(az.analyze(a, params, block, tail[0], tail[1], sample_bits=16, debug=True), ora, lens)
    assert_same_results(outs[0], outs[1], lens)
    t1 = outs[1]["meta"]["lpc_tiers"].astype(np.int64)
    for u, v in enumerate(verdicts):
        if v is None:
            continue
        assert int(t1[u]) >> 8 == 4 and 1 <= (int(t1[u]) & 0xff) <= 5, (u, int(t1[u]))
        if v[0] is not None and v[0] > 1.02 * v[1]:
            assert int(t1[u]) == 1 | 4 << 8, (u, int(t1[u]))
    # the units of the list kernels carry their marks whatever the knob
    other = np.array([k is not None and k != "batch" for k in S.classify(a, ora, L, lens)])
    for k in (1, 2):
        assert np.array_equal(outs[k]["meta"]["lpc_tiers"][other], outs[0]["meta"]["lpc_tiers"][other]), k
    return check_knob2_marks(outs[2]["meta"], verdicts)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-l%d-q%d-r%d%d" % c)
def test_pre_test_vs_oracle_and_model(az, case):
    n, L, q, rmin, rmax = case
    a, ora = case_reference(case)
    decided, undecided = run_knobs(az, a, ora, make_params(L, q, rmin, rmax), n, [n] * len(a), L)
    print(case, "knob 2: decided", decided, "exact pass", undecided)
    assert undecided >= 4, "no near tie reached the exact pass"
    if n >= 576:  # (short blocks: the window's tapers and kappa leave the bound little to decide)
        assert decided >= 12, (decided, undecided)


def test_unusable_words_never_decide(az):
    """A unit that raises in Levinson-Durbin or the quantiser (k_lpc's record holds a status)
    keeps that status, and a unit with a negative-shift order (no coefficients: the candidate's
    sum runs from sample 0, outside the proof) carries the unusable marker: the model has no
    bound for it and under knob 2 the device sends it to the exact pass."""
    case = (4608, 12, 5, 0, 5)
    a, ora = case_reference(case)
    om, rec = ora["meta"], ora["lpc_records"]
    raised = np.flatnonzero((om["status"] != 0) & (om["site"] != abi.SITE_CHOICE_TIE) & ~ora["lpc_sums"].any(axis=1))
    negshift = np.flatnonzero(rec[:, 1] != 0)
    verdicts = model_verdicts(a, ora, 12, [4608] * len(a))
    negshift = [u for u in negshift if verdicts[u] is not None]
    assert len(raised) >= 2 and len(negshift) >= 1, (len(raised), len(negshift))
    assert all(verdicts[u][0] is None for u in negshift)
    with knob(KNOB, 2):
        out = az.analyze(a, make_params(12, 5, 0, 5), 4608, sample_bits=16)
    for u in raised:
        assert (int(out["meta"]["status"][u]), int(out["meta"]["site"][u])) == (int(om["status"][u]), int(om["site"][u])), u
    for u in negshift:
        assert int(out["meta"]["lpc_tiers"][u]) == 5 | 4 << 8, (u, int(out["meta"]["lpc_tiers"][u]))


def test_tail_class(az):
    block, tail, L, q, cut = TAIL
    a = np.array(make_units(block, 77))
    a[-cut:] = a[:cut]  # config-2 units (mostly decided at full length) as the tail's
    a[-cut:, tail:] = 0
    ora = oracle.analyze_batch(a, oracle.make_params(L, q, 0, 5), block, tail, cut, sample_bits=16, threads=16)
    lens = [block] * (len(a) - cut) + [tail] * cut
    decided, undecided = run_knobs(az, a, ora, make_params(L, q, 0, 5), block, lens, L, (tail, cut))
    print("tail class: decided", decided, "exact pass", undecided)
    t2 = None
    with knob(KNOB, 2):
        t2 = az.analyze(a, make_params(L, q, 0, 5), block, tail, cut, sample_bits=16)["meta"]["lpc_tiers"][-cut:]
    assert (t2.astype(np.int64) == (1 | 4 << 8)).any(), ("no tail unit decided by the pre-test", t2)
