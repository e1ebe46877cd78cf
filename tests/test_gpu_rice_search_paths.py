"""FLACMI_FLAG_RICE_SEARCH behind every analysis path: gated signals (tests/rice_search_cases.py's
recipe, one unit each) whose units fail in the reference's Rice step at sites 12 and 13 inside each
kernel, at the smallest shape each kernel accepts (tests/stream_shape_cases.py, sb_shape_ok and the
dispatch in csrc/k_resid.h).

Each case is analysed twice, with the flag clear and set.  The run with the flag clear is what the
analysis kernels leave (checked against the oracle where the oracle has the mode); the model
(tests/rice_search_model.py) applied to it is what the run with the flag set must give, field by
field: every field of every meta record, the first n_parts Rice parameters and every residual row."""
import functools

import numpy as np
import pytest

import oracle
import rice_search_cases as RC
import rice_search_model as RM
import stream_shape_cases as SC
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def gated_units(n, units, bits, seed, open_mix=0):
    """units rows of n samples: unit u has a stretch of digital silence (u % 3 == 0), of sparse +-1
    (u % 3 == 1) or no gap (u % 3 == 2), the signal itself scaled to `bits` bits; the first open_mix units are the bench's open mix (the units
    k_resid_stream lists), gated in the same way."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((units, n), dtype=np.int64)
    for u in range(units):
        x = oracle.synth_unit(u, n, 16, seed, 5).astype(np.int64) if u < open_mix else RC.ar2(rng, n, 400.0)
        x = np.clip(x, -32768, 32767) << (bits - 16)
        g0 = n // 4 + int(rng.integers(0, max(n // 8, 1)))
        g1 = g0 + n // 3 + int(rng.integers(0, max(n // 8, 1)))
        if u % 3 != 2:
            x[g0:g1] = 0
        if u % 3 == 1:
            idx = g0 + rng.choice(g1 - g0, size=max(1, (g1 - g0) // 12), replace=False)
            x[idx] = rng.choice([-1, 1], size=len(idx))
        rows[u] = x
    a = rows.astype(np.int16 if bits <= 16 else np.int32)
    a.setflags(write=False)
    return a


def run(az, a, n, bits, L, q, rmin, rmax, mode=abi.MODE_REFERENCE, lpc_sign=False, tail=(0, 0), check_oracle=True,
        both_sites=True):
    lens = [tail[0] if u >= a.shape[0] - tail[1] else n for u in range(a.shape[0])]
    base = az.analyze(a, make_params(L, q, rmin, rmax, mode, lpc_sign=lpc_sign), n, tail[0], tail[1], sample_bits=bits)
    got = az.analyze(a, make_params(L, q, rmin, rmax, mode, lpc_sign=lpc_sign, rice_search=True), n, tail[0], tail[1],
                     sample_bits=bits)
    sites = {(int(s), int(t)) for s, t in zip(base["meta"]["status"], base["meta"]["site"])}
    assert (0, 0) in sites and ((3, 12) in sites or (3, 13) in sites), sites
    if both_sites:  # both Rice sites and units the reference writes
        assert {(3, 12), (3, 13)} <= sites, sites
    if check_oracle:  # flag clear: the oracle's default results, the failures included
        ora = oracle.analyze_batch(np.ascontiguousarray(a), oracle.make_params(L, q, rmin, rmax, mode), n, tail[0], tail[1],
                                   sample_bits=bits, threads=16)
        for u in range(a.shape[0]):
            assert not RM.baseline_mismatches(base["meta"][u], ora["meta"][u]), (u, RM.baseline_mismatches(base["meta"][u], ora["meta"][u]))
    want = RM.apply(base, lens, rmin, rmax)
    assert len(want["rescued"]) >= 2
    for u in range(a.shape[0]):
        diff = RM.meta_fields_differ(got["meta"][u], want["meta"][u])
        assert not diff, (u, diff, got["meta"][u], want["meta"][u])
        k = int(want["meta"]["n_parts"][u])
        assert np.array_equal(got["rice_params"][u][:k], want["rice_params"][u][:k]), u
    assert np.array_equal(got["residual"], base["residual"])
    assert not (got["meta"]["status"] == abi.STATUS_VALUE_ERROR).any()
    return base, got, want


def test_stream_kernel_runtime_shape_and_listed_units(az):
    c = SC.CASES[0]
    assert SC.stream_shape(c.n, c.L, c.rmin, c.rmax, False)["NFIX"] == 0
    a = gated_units(c.n, 48, 16, 21, open_mix=24)
    ora = oracle.analyze_batch(np.ascontiguousarray(a), oracle.make_params(c.L, c.q, c.rmin, c.rmax), c.n, sample_bits=16)
    classes = SC.class_counts(SC.classify(a, ora, c.L, [c.n] * 48))
    assert classes["list"] + classes["list2"] >= 1 and classes["batch"] >= 1, classes
    run(az, a, c.n, 16, c.L, c.q, c.rmin, c.rmax)


def test_stream_kernel_constant_shape_and_listed_units(az):
    n, L = 4608, 12
    assert SC.stream_shape(n, L, 0, 5, False)["NFIX"] == 4608
    a = gated_units(n, 36, 16, 22, open_mix=18)
    ora = oracle.analyze_batch(np.ascontiguousarray(a), oracle.make_params(L, 5, 0, 5), n, sample_bits=16, threads=16)
    classes = SC.classify(a, ora, L, [n] * 36)
    counts = SC.class_counts(classes)
    assert counts["list"] + counts["list2"] >= 1 and counts["batch"] >= 1, counts
    base, got, want = run(az, a, n, 16, L, 5, 0, 5)
    listed = [u for u, k in enumerate(classes) if k is not None and k != "batch"]
    assert all(int(got["meta"]["status"][u]) == 0 for u in listed)


def test_general_kernel_int16(az):
    assert SC.stream_shape(192, 8, 0, 4, False) is None
    run(az, gated_units(192, 24, 16, 23), 192, 16, 8, 5, 0, 4)


def test_general_kernel_24_bit(az):
    run(az, gated_units(192, 24, 24, 24), 192, 24, 8, 5, 0, 4)


def test_int8_mfma_route(az):
    """24-bit rows, L >= 16, 8192 samples: k_resid's int8-MFMA kernel (Rice orders 0..5: not k_resid_sb's shape)."""
    run(az, gated_units(8192, 12, 24, 25), 8192, 24, 16, 12, 0, 5)


def test_sb_kernel(az):
    """The same with Rice orders up to 6: k_resid_sb (64 finest partitions of 128 samples)."""
    run(az, gated_units(8192, 12, 24, 26), 8192, 24, 16, 12, 0, 6)


def test_fixed_only(az):
    c = SC.FIXED_CASES[0]
    run(az, gated_units(c.n, 24, 16, 27), c.n, 16, 0, c.q, c.rmin, c.rmax, mode=abi.MODE_FIXED_ONLY)


def test_with_the_corrected_lpc_sign(az):
    base, got, want = run(az, gated_units(192, 24, 16, 28), 192, 16, 8, 5, 0, 4, lpc_sign=True, check_oracle=False,
                          both_sites=False)
    assert (got["meta"]["kind"] == 1).any()  # LPC subframes win with the corrected sign, and are searched


def test_overlap_split(az):
    """FLACMI_OVERLAP = -8: chunks of 8-unit rounds, k_lpc of the second beside k_resid of the first;
    the search runs once, behind the last chunk, over every unit (tail units included)."""
    a = np.array(gated_units(192, 27, 16, 29))
    a[24:, 77:] = 0
    c = SC.CASES[0]
    with knob("FLACMI_OVERLAP", -8):
        run(az, a, 192, 16, 8, 5, 0, 4, tail=(77, 3))
        run(az, gated_units(c.n, 48, 16, 21, open_mix=24), c.n, 16, c.L, c.q, c.rmin, c.rmax)
