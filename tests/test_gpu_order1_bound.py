"""k_resid_stream's second test (where the energy bound's pre-test fails on usable
words, orders 2 .. L by the energy bound on their own maxima and order 1 by a closed form on the
fixed sums of orders 0 and 1, from three more words of k_lpc's) against the CPU oracle and the
CPU model (tests/order1_bound_model.py), on the units of tests/test_gpu_energy_bound.py at the
shapes at which it can go wrong: one nearly empty chunk slot (n = 64), L = 1 (no orders 2 .. L)
and L = 2 (one), the taper's end inside a chunk (576), the runtime-shape and the constant-shape
builds (4096 L 8, 4608 L 12), listed units (4608 L 11 q 6), four waves (10240) and a tail class.

Every call runs under FLACMI_ENERGY_BOUND 0 (the tiers alone), 1 (both tests, then the tiers),
2 (the first test, then the exact pass), 3 (both tests, then the exact pass) and 4 (the first
test, then the tiers).  Under 3 meta.lpc_tiers says which units the two tests decided (1/4) and
which they did not (5/4); the models must agree wherever their margins are not within 2% of
zero.  Knobs 0, 1 and 4 (the tiers last) must agree field for field but for lpc_tiers.  Knobs 2
and 3 send an undecided unit to the exact pass, which reports its exact LPC order and sum where
the tiers prune it (FLACMI_LPC_PRUNED in both fields), so against knob 0 those two fields are
compared wherever both calls pruned or both did not, every other field everywhere, and no unit
may be pruned under 2 or 3 that the tiers alone do not prune."""
import numpy as np
import pytest

import energy_bound_model as M
import oracle
import order1_bound_model as O
import stream_shape_cases as S
import test_gpu_energy_bound as E
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params
from test_gpu_parity import compare_with_oracle

pytestmark = pytest.mark.gpu

KNOBS = (0, 1, 2, 3, 4)
# (n, L, q, rmin, rmax)
CASES = [(64, 12, 5, 0, 3), (192, 1, 5, 0, 3), (192, 2, 5, 0, 3), (576, 10, 5, 0, 3), (4096, 8, 5, 0, 5),
         (4608, 12, 5, 0, 5), (4608, 11, 6, 0, 5), (10240, 12, 5, 0, 5)]
DECIDED = 1 | 4 << 8
EXACT = 5 | 4 << 8


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def model_verdicts(a, ora, L, lens):
    """Per unit: None (not the batch kernel's, or it raised before the choice), else +1 (a test
    passes with margin), -1 (both fail with margin, or the words are unusable), 0 (too close)."""
    out = []
    for u, k in enumerate(S.classify(a, ora, L, lens)):
        if k != "batch":
            out.append(None)
            continue
        x, acf, rec, fs = a[u][:lens[u]], ora["acf"][u], ora["lpc_records"][u], ora["fixed_sums"][u]
        b, f = M.lower_bound(x, acf, rec, L), 256 * int(fs.min())
        if b is None:
            out.append(-1)
            continue
        mr, m1 = O.margins(x, acf, rec, L, fs)
        if b > 1.02 * f or ((mr is None or mr > 0.02) and m1 > 0.02):
            out.append(1)
        elif b < 0.98 * f and ((mr is not None and mr < -0.02) or m1 < -0.02):
            out.append(-1)
        else:
            out.append(0)
    return out


def assert_same_but_pruning(x, y, lens):
    """Field for field but lpc_tiers; lpc_order and lpc_sum wherever both calls pruned the unit or
    both did not (a knob that sends undecided units to the exact pass reports their exact LPC
    sums, where the tiers prune most of them: FLACMI_LPC_PRUNED in both fields)."""
    same = (x["meta"]["lpc_order"] == abi.LPC_PRUNED) == (y["meta"]["lpc_order"] == abi.LPC_PRUNED)
    for f in abi.META_DTYPE.names:
        if f in ("lpc_order", "lpc_sum"):
            assert np.array_equal(x["meta"][f][same], y["meta"][f][same]), f
        elif f != "lpc_tiers":
            assert np.array_equal(x["meta"][f], y["meta"][f]), f
    assert np.array_equal(x["rice_params"], y["rice_params"])
    for u, n in enumerate(lens):
        assert np.array_equal(x["residual"][u][:n], y["residual"][u][:n]), u


def run_knobs(az, a, ora, params, block, lens, L, tail=(0, 0)):
    """Production calls under every knob value against the oracle and against each other; the
    marks under knob 3 against the models -> (decided by the second test alone, exact passes)."""
    verdicts = model_verdicts(a, ora, L, lens)
    outs = {}
    for k in KNOBS:
        with knob(E.KNOB, k):
            outs[k] = az.analyze(a, params, block, tail[0], tail[1], sample_bits=16, extras=("acf", "lpc_records"))
        compare_with_oracle({f: outs[k][f] for f in ("meta", "rice_params", "residual")}, ora, lens)
        if k in (1, 4):  # the tiers behind the pre-tests: what the tiers alone give, pruning included
            E.assert_same_results(outs[0], outs[k], lens)
        elif k:
            assert_same_but_pruning(outs[0], outs[k], lens)
            assert not ((outs[k]["meta"]["lpc_order"] == abi.LPC_PRUNED) & (outs[0]["meta"]["lpc_order"] != abi.LPC_PRUNED)).any(), k
        if k:
            assert np.array_equal(outs[k]["acf"].view(np.uint64), outs[0]["acf"].view(np.uint64)), k
            assert np.array_equal(outs[k]["lpc_records"], outs[0]["lpc_records"]), k
    ok = ora["meta"]["status"] == 0
    assert np.array_equal(outs[0]["acf"][ok].view(np.uint64), ora["acf"][ok].view(np.uint64))
    assert np.array_equal(outs[0]["lpc_records"][ok], ora["lpc_records"][ok])
    tiers = {k: outs[k]["meta"]["lpc_tiers"].astype(np.int64) for k in KNOBS}
    om = ora["meta"]
    kinds = S.classify(a, ora, L, lens)
    alone = exact = 0
    for u, v in enumerate(verdicts):
        if int(om["status"][u]) != 0:  # a status keeps its site under every knob
            for k in KNOBS:
                gm = outs[k]["meta"]
                assert (int(gm["status"][u]), int(gm["site"][u])) == (int(om["status"][u]), int(om["site"][u])), (k, u)
        if kinds[u] is not None and kinds[u] != "batch":  # the list kernels' marks, whatever the knob
            for k in KNOBS[1:]:
                assert int(tiers[k][u]) == int(tiers[0][u]), (k, u, int(tiers[k][u]), int(tiers[0][u]))
        if v is None:
            continue
        t2, t3 = int(tiers[2][u]), int(tiers[3][u])
        pruned = int(outs[3]["meta"]["lpc_order"][u]) == abi.LPC_PRUNED
        assert t3 in (DECIDED, EXACT) and pruned == (t3 == DECIDED), (u, t3, pruned)
        assert t2 in (DECIDED, EXACT), (u, t2)
        if t2 == DECIDED:
            assert t3 == DECIDED, (u, "decided under knob 2 but not under knob 3")
        if v > 0:
            assert t3 == DECIDED, (u, "the models decide with margin, the device did not")
        if v < 0:
            assert t3 == EXACT, (u, "the device decided a unit the models do not")
        for k in (1, 4):  # the tiers' marks: 1/4 .. 5/4, and 1/4 wherever the pre-tests decided
            assert int(tiers[k][u]) >> 8 == 4 and 1 <= (int(tiers[k][u]) & 0xff) <= 5, (k, u, int(tiers[k][u]))
        assert t2 != DECIDED or int(tiers[4][u]) == DECIDED, (u, int(tiers[4][u]), t2)
        assert t3 != DECIDED or int(tiers[1][u]) == DECIDED, (u, int(tiers[1][u]), t3)
        alone += t3 == DECIDED and t2 == EXACT
        exact += t3 == EXACT
    return alone, exact


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-l%d-q%d-r%d%d" % c)
def test_second_test_vs_oracle_and_models(az, case):
    n, L, q, rmin, rmax = case
    a, ora = E.case_reference(case)
    alone, exact = run_knobs(az, a, ora, make_params(L, q, rmin, rmax), n, [n] * len(a), L)
    print(case, "knob 3: decided by the second test alone", alone, "exact pass", exact)
    if case == (4608, 12, 5, 0, 5):
        assert alone >= 1, "no unit decided by the second test alone"
        assert exact >= 4, "no near tie reached the exact pass"
    if case == (4608, 11, 6, 0, 5):
        kinds = S.classify(a, ora, L, [n] * len(a))
        assert any(k is not None and k != "batch" for k in kinds), "no listed unit"


def test_tail_class(az):
    block, tail, L, q, cut = E.TAIL
    a = np.array(E.make_units(block, 77))
    a[-cut:] = a[:cut]  # config-2 units as the tail's
    a[-cut:, tail:] = 0
    ora = oracle.analyze_batch(a, oracle.make_params(L, q, 0, 5), block, tail, cut, sample_bits=16, threads=16)
    lens = [block] * (len(a) - cut) + [tail] * cut
    alone, exact = run_knobs(az, a, ora, make_params(L, q, 0, 5), block, lens, L, (tail, cut))
    print("tail class: decided by the second test alone", alone, "exact pass", exact)
