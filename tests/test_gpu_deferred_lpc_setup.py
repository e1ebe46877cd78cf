"""k_resid_stream's energy-bound build reads nothing of the LPC record but its status word
before the pre-test: only a unit the pre-test leaves undecided builds the tap table
in LDS, waits at one barrier, forms the LPC operands and takes the MFMA exactness test.  k_lpc
therefore gives every unit that test lists (sum|taps| > 127 for some order) unusable bound
words, so a listed unit is never decided first.  What could go wrong, at the smallest shapes
that reach it:

  - a listed unit decided by the pre-test: it would report FLACMI_LPC_PRUNED and the mark 1/4
    instead of the list kernel's exact values and mark (the q 6 case holds such units: outside
    the bound, and the model's bound decides them with margin);
  - the late table read before it is whole (a missing barrier): wrong exact sums on the
    undecided units;
  - status and negative-shift units, which never had usable words.

Listed units that k_resid's list variant takes (sum|c| > 127) may still come back pruned by that
kernel's own sign bound, which this change does not touch: for those the check is that marks and
LPC fields are the same under every knob (knob 0 runs the earlier code); every other listed unit
must also carry the oracle's exact values.

The inputs and the oracle's results are test_gpu_energy_bound's (made once, shared)."""
import functools

import numpy as np
import pytest

import energy_bound_model as M
import oracle
import stream_shape_cases as S
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params
from test_gpu_energy_bound import assert_same_results, case_reference, make_units, model_verdicts
from test_gpu_parity import compare_with_oracle

pytestmark = pytest.mark.gpu

KNOB = "FLACMI_ENERGY_BOUND"
# (n, L, q, rmin, rmax): one wave and a nearly empty chunk slot; NG = 2 with L off a multiple of
# 4; 576; the runtime-shape and the constant-shape builds; q 6 (many units outside the MFMA
# bound); four waves and the second tap-table slot
CASES = [(64, 12, 5, 0, 3), (192, 7, 5, 0, 3), (576, 10, 5, 0, 3), (4096, 8, 5, 0, 5), (4608, 12, 5, 0, 5),
         (4608, 11, 6, 0, 5), (10240, 12, 5, 0, 5)]
Q6_CASE = (4608, 11, 6, 0, 5)
TAIL = (4608, 3328, 8, 6, 6)  # block, tail, L, q, units cut to the tail
DECIDED, EXACT = 1 | 4 << 8, 5 | 4 << 8


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def tail_reference():
    block, tail, L, q, cut = TAIL
    a = np.array(make_units(block, 77))
    a[-cut:] = a[:cut]
    a[-cut:, tail:] = 0
    a.setflags(write=False)
    ora = oracle.analyze_batch(a, oracle.make_params(L, q, 0, 5), block, tail, cut, sample_bits=16, threads=16)
    for v in ora.values():
        v.setflags(write=False)
    return a, ora


def listed_and_decidable(a, ora, L, lens):
    """(the units outside the MFMA bound; those of them that report exact LPC values: the list
    kernel's, and the units of k_resid's list variant that its own sign bound, which this build
    does not touch, leaves undecided; those of the second set whose record gives the model a
    bound at least 2% above the best fixed sum: the pre-test would decide them if it saw them)."""
    listed, exact, decidable = [], [], []
    for u, k in enumerate(S.classify(a, ora, L, lens)):
        if k is None or k == "batch":
            continue
        listed.append(u)
        if k != "list" and k[1]:
            continue
        exact.append(u)
        n = lens[u]
        b = M.lower_bound(a[u][:n], ora["acf"][u], ora["lpc_records"][u], L)
        if b is not None and b > 1.02 * 256 * int(ora["fixed_sums"][u].min()):
            decidable.append(u)
    return listed, exact, decidable


def run_case(az, a, ora, params, block, lens, L, tail=(0, 0)):
    """Every check of one call -> (listed, listed and decidable, batch units the model decides
    with margin, batch units the device left undecided under knob 2)."""
    om = ora["meta"]
    verdicts = model_verdicts(a, ora, L, lens)
    listed, exact, decidable = listed_and_decidable(a, ora, L, lens)
    outs = {}
    for k in (0, 1, 2):
        with knob(KNOB, k):
            outs[k] = az.analyze(a, params, block, tail[0], tail[1], sample_bits=16, extras=("acf", "lpc_records"))
        compare_with_oracle({f: outs[k][f] for f in ("meta", "rice_params", "residual")}, ora, lens)
        if k:  # k_lpc's outputs but the bound words: the same bits whatever the knob
            assert np.array_equal(outs[k]["acf"].view(np.uint64), outs[0]["acf"].view(np.uint64)), k
            assert np.array_equal(outs[k]["lpc_records"], outs[0]["lpc_records"]), k
    assert_same_results(outs[0], outs[1], lens)
    for k in (0, 1, 2):
        gm = outs[k]["meta"]
        # listed units: the list kernels' marks and LPC fields whatever the knob, and the oracle's
        # exact values
        for f in ("lpc_tiers", "lpc_order", "lpc_sum"):
            assert np.array_equal(gm[f][listed], outs[0]["meta"][f][listed]), (k, f)
        for u in exact:
            if int(om["status"][u]) != 0:
                continue
            assert int(gm["lpc_order"][u]) != abi.LPC_PRUNED and int(gm["lpc_sum"][u]) != abi.LPC_PRUNED, (k, u, "listed, pruned")
            assert int(gm["lpc_order"][u]) == int(om["lpc_order"][u]), (k, u, "lpc_order")
            assert int(gm["lpc_sum"][u]) == int(om["lpc_sum"][u]), (k, u, "lpc_sum")
        # units with a status keep it, and its site
        st = om["status"] != 0
        assert np.array_equal(gm["status"][st], om["status"][st]) and np.array_equal(gm["site"][st], om["site"][st]), k
    decided = undecided = 0
    t1, t2 = (outs[k]["meta"]["lpc_tiers"].astype(np.int64) for k in (1, 2))
    m2 = outs[2]["meta"]
    for u, v in enumerate(verdicts):
        if v is None:
            continue
        b, f = v
        assert int(t2[u]) in (DECIDED, EXACT), (u, int(t2[u]))
        if b is not None and b > 1.02 * f:  # the model decides with margin: 1/4 under both knobs
            assert int(t1[u]) == DECIDED and int(t2[u]) == DECIDED, (u, int(t1[u]), int(t2[u]))
            decided += 1
        if int(ora["lpc_records"][u][1]) != 0:  # a negative-shift order: never decided
            assert int(t2[u]) == EXACT, (u, "negative shift", int(t2[u]))
        if int(t2[u]) == EXACT and int(om["status"][u]) == 0:
            # undecided: operands built late, from the late table; the exact pass's values
            assert int(m2["lpc_order"][u]) == int(om["lpc_order"][u]), (u, "lpc_order (late setup)")
            assert int(m2["lpc_sum"][u]) == int(om["lpc_sum"][u]), (u, "lpc_sum (late setup)")
            undecided += 1
    return len(listed), len(decidable), decided, undecided


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-l%d-q%d-r%d%d" % c)
def test_deferred_setup(az, case):
    n, L, q, rmin, rmax = case
    a, ora = case_reference(case)
    listed, decidable, decided, undecided = run_case(az, a, ora, make_params(L, q, rmin, rmax), n, [n] * len(a), L)
    print(case, "listed", listed, "of them decidable by the model", decidable, "batch: decided with margin", decided,
          "undecided under knob 2", undecided)
    assert undecided >= 4, "too few units reach the late setup"
    if case == Q6_CASE:
        assert decidable >= 4, "too few listed units the pre-test would decide"


def test_deferred_setup_tail_class(az):
    block, tail, L, q, cut = TAIL
    a, ora = tail_reference()
    lens = [block] * (len(a) - cut) + [tail] * cut
    listed, decidable, decided, undecided = run_case(az, a, ora, make_params(L, q, 0, 5), block, lens, L, (tail, cut))
    print("tail class: listed", listed, "decidable", decidable, "decided", decided, "undecided", undecided)
    assert undecided >= 4
