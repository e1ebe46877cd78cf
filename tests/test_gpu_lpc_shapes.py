"""The k_lpc kernels (flac-py_amd/csrc/k_lpc.hip) over block lengths, against the CPU oracle, bit
for bit: k_lpc_tile<4/8/12>, k_lpc<LMAX,int16_t> and k_lpc<LMAX,int32_t> at lengths 1..4410 that
end inside a tile / ring cycle / load block, make the tile's segment clamp act, are too short for a
rectangle tile, sit on the Tukey division site, or read the window's zero pad to its end; 24, 26
(the widest fused) and 27-bit (the first unfused) full-scale samples; tail classes whose rows keep
noise past tail_len.  The table, its inputs and the conditions on them live in
tests/lpc_shape_cases.py (tests/test_lpc_shape_cases.py runs those without a device).

Every case goes through the production call and the debug call (compare_with_oracle); from the
debug call acf and lpc_records are then compared for EVERY unit, whatever its status (most units
of a short block raise somewhere after the LPC analysis, and compare_with_oracle stops there)."""
import numpy as np
import pytest

import lpc_shape_cases as S
import oracle
from flac_amd.analysis import Analyzer, make_params
from test_gpu_parity import compare_with_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def assert_lpc_outputs_of_every_unit(out, ora):
    """acf (as uint64) and lpc_records of a debug call against the oracle's, for every unit.
    At the Tukey site (n in 4..7) the device writes a zero acf row and the oracle returns before it
    touches its own, which oracle.analyze_batch allocated as zeros: those rows compare too.
    A unit that raises inside the LPC analysis has no record in the oracle (zeros); the device's has
    status | site << 16 in word 0, nothing after word 1, and in word 1 the negative-shift mask of
    the orders before the one that raised, which the oracle does not keep: word 1 is skipped for
    exactly those units."""
    om = ora["meta"]
    got, want = out["acf"].view(np.uint64), ora["acf"].view(np.uint64)
    for u in np.flatnonzero((got != want).any(axis=1)):
        raise AssertionError((int(u), "acf", out["acf"][u].tolist(), ora["acf"][u].tolist()))
    for u in range(len(om)):
        rec, ref = out["lpc_records"][u], ora["lpc_records"][u]
        if S.lpc_stage_failed(om, u):
            assert int(rec[0]) == int(om["status"][u]) | int(om["site"][u]) << 16, (u, "record status", int(rec[0]))
            assert not ref.any() and not rec[2:].any(), (u, "record of a unit that raised")
        else:
            assert np.array_equal(rec, ref), (u, "lpc_records", np.flatnonzero(rec != ref)[:8])


def run_both(az, a, ora, params, block, lens, bits, tail=(0, 0)):
    """The production call and the debug call, each against the oracle -> the debug output."""
    for debug in (False, True):
        out = az.analyze(a, params, block, tail[0], tail[1], sample_bits=bits, debug=debug)
        compare_with_oracle(out, ora, lens)
    assert_lpc_outputs_of_every_unit(out, ora)
    return out


def assert_rows_equal(part, whole, k, lens):
    """The first k rows of `whole` against the k-row call `part`, field for field: what k_lpc writes
    (status, site, acf, LPC records) for every unit, everything else wherever the unit has a
    result (an exception's row carries no other field)."""
    for name in ("acf", "lpc_records"):
        assert np.array_equal(part[name].view(np.uint64 if name == "acf" else np.int32),
                              whole[name][:k].view(np.uint64 if name == "acf" else np.int32)), name
    pm, wm = part["meta"], whole["meta"][:k]
    assert np.array_equal(pm["status"], wm["status"]) and np.array_equal(pm["site"], wm["site"])
    for u in np.flatnonzero(pm["status"] == 0):
        bad = oracle.meta_mismatches(pm[u], wm[u])
        assert not bad, (u, "meta", bad)
        npart, off, ln = int(pm["n_parts"][u]), int(pm["res_offset"][u]), int(pm["res_len"][u])
        assert off + ln == lens[u]
        assert np.array_equal(part["rice_params"][u][:npart], whole["rice_params"][u][:npart]), (u, "params")
        assert np.array_equal(part["residual"][u][off:off + ln], whole["residual"][u][off:off + ln]), (u, "residual")
        for name in ("fixed_sums", "lpc_sums"):
            assert np.array_equal(part[name][u], whole[name][u]), (u, name)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_block_lengths(az, case):
    builds = S.check_dispatch(case)
    facts = S.check_case_oracle(case)
    a, ora = S.case_reference(case)
    lens = [case.n] * len(a)
    p = make_params(case.L, case.q, S.RMIN, S.RMAX)
    whole = run_both(az, a, ora, p, case.n, lens, case.bits)
    print(S.case_id(case), [b[:2] + b[3:] for b in builds], facts)
    if case.group == "A":
        # the same units once through k_lpc<LMAX,int16_t> (a call below 64 units) and once through
        # the tile kernel
        k = S.A_PREFIX
        part = run_both(az, np.ascontiguousarray(a[:k]), S.prefix(ora, k), p, case.n, lens[:k], case.bits)
        assert_rows_equal(part, whole, k, lens)


@pytest.mark.parametrize("t", S.TAIL_CALLS, ids=S.tail_id)
def test_tail_class_rows_keep_noise_past_tail_len(az, t):
    """A short last block among longer rows: the tail class runs at the body's row pitch, and the
    samples at and past tail_len (full-scale noise here) must not enter its products."""
    S.check_tail_dispatch(t)
    facts = S.check_tail_oracle(t)
    a, ora = S.tail_reference(t)
    lens = [t.block] * S.TAIL_BODY + [t.tail] * S.TAIL_CUT
    run_both(az, a, ora, make_params(t.L, t.q, S.RMIN, S.RMAX), t.block, lens, t.bits, (t.tail, S.TAIL_CUT))
    print(S.tail_id(t), facts)
