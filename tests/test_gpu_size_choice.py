"""k_size_choice (FLACMI_FLAG_SIZE_CHOICE, csrc/k_size.hip) against tests/size_choice_model.py: the
whole record, the Rice parameters, the zig-zag row and, through outputs.fixed_sums / lpc_sums, every
candidate's bits, at the smallest shapes that reach each branch of the rule and of the kernel."""
import ctypes as C
import math

import numpy as np
import pytest

import lpc_sign_model as LS
import oracle
import size_choice_cases as SC
import size_choice_model as SZ
from flac_amd import abi
from flac_amd._lib import FlacmiError
from flac_amd.analysis import Analyzer, knob, make_params, unit_stride

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def base_analysis(rows, n, L, q, rmin, rmax, bits, sign, fixed_only, tail=0, n_tail=0):
    """The analysis with the flag clear, on the CPU: the records and the LPC-stage failures the model reads."""
    if fixed_only:
        return oracle.analyze_batch(rows, oracle.make_params(0, q, rmin, rmax, abi.MODE_FIXED_ONLY), n, tail, n_tail,
                                    sample_bits=bits)
    p = oracle.make_params(L, q, rmin, rmax)
    return (LS.analyze if sign else oracle.analyze_batch)(rows, p, n, tail, n_tail, sample_bits=bits)


def check(az, rows, n, L, q, rmin, rmax, bits, *, sign=False, fixed_only=False, tail=0, n_tail=0, sample_size=0,
          residual_bytes=4, sums=True):
    """One flacmi_analyze_host call with the flag against the model -> (device results, model results)."""
    rows = np.ascontiguousarray(rows)
    lens = [tail if (n_tail and u >= rows.shape[0] - n_tail) else n for u in range(rows.shape[0])]
    mode = abi.MODE_FIXED_ONLY if fixed_only else abi.MODE_REFERENCE
    p = make_params(L, q, rmin, rmax, mode, lpc_sign=sign, rice_search=True, size_choice=True, sample_size=sample_size)
    dev = az.analyze(rows, p, n, tail, n_tail, sample_bits=bits, residual_bytes=residual_bytes,
                     extras=("fixed_sums", "lpc_sums") if sums else ())
    base = base_analysis(rows, n, L, q, rmin, rmax, bits, sign, fixed_only, tail, n_tail)
    want = SZ.apply(base, rows, lens, L, q, rmin, rmax, sample_size or bits, fixed_only=fixed_only)
    bad = SZ.mismatches(dev, want, lens, sums)
    assert not bad, bad[:6]
    return dev, want


@pytest.mark.parametrize("sign,fixed_only", [(True, False), (False, False), (False, True)])
def test_16bit_units(az, sign, fixed_only):
    """AR, tone, noise, digital silence and full scale at n = 192, L 8, q 12, r 0..3."""
    rows = SC.analysis_units()
    dev, want = check(az, rows, 192, 8, 12, 0, 3, 16, sign=sign, fixed_only=fixed_only)
    m = dev["meta"]
    if fixed_only:
        assert not m["status"].any() and not m["lpc_order"].any() and not m["lpc_sum"].any() and not dev["lpc_sums"].any()
        assert int(m["order"][10]) == 0 and int(m["rice_bits"][10]) > 0  # silence is a FIXED subframe of zeros
    else:
        assert int(m["status"][10]) == abi.STATUS_ZERO_DIVISION and int(m["site"][10]) in SZ.LPC_STAGE_SITES  # silence
        assert not m["status"][:10].any() and int(m["status"][11]) == 0
        assert len({(int(k), int(o)) for k, o in zip(m["kind"][:10], m["order"][:10])}) >= 2
    if sign:
        assert int(m["kind"][:4].min()) == abi.KIND_LPC and int(m["order"][:4].max()) < 8  # AR: LPC below the top order
        assert all(int(k) == abi.KIND_FIXED for k in m["kind"][7:10])                        # noise: FIXED
    assert not m["lpc_tiers"].any()


@pytest.mark.parametrize("fixed_only", [True, False])
def test_tiny_blocks(az, fixed_only):
    """n = 1..8: order 0 alone up to 4 samples; in the reference mode 4..7 keep the Tukey site."""
    rng = np.random.default_rng(8)
    for n in range(1, 9):
        rows = rng.integers(-300, 301, (3, n)).astype(np.int16)
        dev, want = check(az, rows, n, 8, 12, 0, 2, 16, fixed_only=fixed_only)
        if fixed_only:
            assert not dev["meta"]["status"].any()
            if n <= 4:
                assert not dev["meta"]["order"].any() and (dev["fixed_sums"][:, 1:] == -1).all()
        elif 4 <= n <= 7:
            assert [(int(s), int(t)) for s, t in zip(dev["meta"]["status"], dev["meta"]["site"])] == [(abi.STATUS_ZERO_DIVISION, 1)] * 3


@pytest.mark.parametrize("rmin", [1, 2, 5])
def test_eligibility_by_partition_order(az, rmin):
    """n = 16, L 12: rice_min 1 bars the orders >= 8, rice_min 2 fixed order 4 too, rice_min 5 every candidate."""
    rows = np.random.default_rng(16).integers(-900, 901, (4, 16)).astype(np.int16)
    dev, want = check(az, rows, 16, 12, 12, rmin, 5, 16, sign=True)
    ok = dev["meta"]["status"] == 0
    if rmin == 5:
        assert [(int(s), int(t)) for s, t in zip(dev["meta"]["status"], dev["meta"]["site"])] == [(abi.STATUS_ASSERTION, 11)] * 4
        assert (dev["fixed_sums"] == -1).all() and (dev["lpc_sums"][:, :12] == -1).all()
        assert (dev["meta"]["fixed_order"] == -1).all() and (dev["meta"]["lpc_sum"] == -1).all()
    else:
        assert ok.all()
        limit = 16 >> rmin
        assert ((dev["lpc_sums"][:, :12] >= 0) == (np.arange(1, 13) < limit)[None, :]).all()
        assert ((dev["fixed_sums"] >= 0) == (np.arange(5) < limit)[None, :]).all()


def test_tail_class(az):
    """Body 192 with a tail of 77: an odd length has partition order 0 only."""
    rng = np.random.default_rng(77)
    rows = np.stack([SC.signal(k, 192, rng) for k in ("ar", "tone", "noise", "ar", "ar", "noise")]).astype(np.int16)
    rows[4:, 77:] = 0
    dev, want = check(az, rows, 192, 8, 12, 0, 3, 16, sign=True, tail=77, n_tail=2)
    assert [int(v) for v in dev["meta"]["part_order"][4:]] == [0, 0]
    assert [int(a) + int(b) for a, b in zip(dev["meta"]["res_offset"][4:], dev["meta"]["res_len"][4:])] == [77, 77]


def test_grid_loop(az):
    """300 units through a grid of 7 workgroups: every workgroup runs the unit loop more than once."""
    rng = np.random.default_rng(300)
    rows = rng.integers(-200, 201, (300, 64)).astype(np.int64) << rng.integers(0, 7, 300)[:, None]
    rows[::7] = np.cumsum(rows[::7], axis=1) >> 3
    rows = rows.astype(np.int16)
    with knob("FLACMI_RICE_GRID", 7):
        check(az, rows, 64, 4, 12, 0, 3, 16, sign=True)


def test_24bit_rows_order_32(az):
    """24-bit int32 rows, n = 322, L 32, q 15, with a full-scale alternating unit and full-scale noise,
    whose parameters above 14 give coding method 5; both row widths give the model's record.  (A
    candidate of 24-bit samples whose residual leaves int32 costs over 33 bits a sample and never
    wins by size, fixed order 0 costing at most 25: test_residual_wide reaches that status.)"""
    rng = np.random.default_rng(322)
    full = (1 << 23) - 1
    rows = np.stack([np.where(np.arange(322) % 2 == 0, full, -full - 1) + 0 * np.arange(322),
                     SC.signal("ar", 322, rng, 256), SC.signal("tone", 322, rng, 256),
                     rng.integers(-(1 << 23), 1 << 23, 322)]).astype(np.int32)
    for rb in (4, 8):
        dev, want = check(az, rows, 322, 32, 15, 0, 3, 24, sign=True, residual_bytes=rb)
        assert not dev["meta"]["status"].any()
        assert int(dev["meta"]["coding_method"][3]) == 5 and int(dev["rice_params"][3][:int(dev["meta"]["n_parts"][3])].max()) > 14
        assert 4 in [int(v) for v in dev["meta"]["coding_method"]]


def test_residual_wide(az):
    """32-bit samples with one step of almost 2^32: fixed order 1 is the smallest candidate and its
    residual needs 33 bits.  On 4-byte rows the unit reports FLACMI_STATUS_RESIDUAL_WIDE with the
    choice and every candidate's exact bits; the redo on 8-byte rows carries the flag."""
    n = 16
    x = np.zeros((3, n), dtype=np.int64)
    x[0] = np.arange(n) * 3 - (1 << 31) + 5
    x[0, 10:] += (1 << 32) - 64
    x[1] = np.random.default_rng(2).integers(-5000, 5000, n)
    x[2] = x[0][::-1]
    rows = x.astype(np.int32)
    base = base_analysis(rows, n, 0, 5, 3, 3, 32, False, True)
    want4 = SZ.apply(base, rows, [n] * 3, 0, 5, 3, 3, 32, fixed_only=True, residual_bytes=4)
    assert [int(v) for v in want4["meta"]["status"]] == [abi.STATUS_RESIDUAL_WIDE, 0, abi.STATUS_RESIDUAL_WIDE]
    dev, want = check(az, rows, n, 0, 5, 3, 3, 32, fixed_only=True)  # Analyzer.analyze redoes the wide units
    assert dev["residual"].dtype == np.uint64 and not dev["meta"]["status"].any() and int(dev["meta"]["order"][0]) == 1
    # the 4-byte call alone
    p4 = make_params(0, 5, 3, 3, abi.MODE_FIXED_ONLY, rice_search=True, size_choice=True)
    stride = unit_stride(n, 4)
    s = np.zeros((3, stride), dtype=np.int32)
    s[:, :n] = rows
    b = abi.Batch()
    b.samples, b.sample_bytes, b.sample_bits, b.unit_stride, b.n_units, b.block_len = s.ctypes.data, 4, 32, stride, 3, n
    meta = np.zeros(3, dtype=abi.META_DTYPE)
    rice = np.zeros((3, 9), dtype=np.int32)
    res = np.zeros((3, 16), dtype=np.uint32)
    fs = np.zeros((3, 5), dtype=np.int64)
    o = abi.Outputs()
    o.meta, o.rice_params, o.params_stride = meta.ctypes.data, rice.ctypes.data, 9
    o.residual, o.residual_bytes, o.residual_stride = res.ctypes.data, 4, 16
    o.fixed_sums = fs.ctypes.data
    assert az.lib.flacmi_analyze_host(az.ctx, C.byref(b), C.byref(p4), C.byref(o)) == 0
    for f in SZ.COMPARED:
        assert [int(v) for v in meta[f]] == [int(v) for v in want4["meta"][f]], f
    assert np.array_equal(fs, want4["fixed_sums"])


def test_q16_has_no_lpc_candidate(az):
    rows = SC.analysis_units()[:10]
    dev, want = check(az, rows, 192, 8, 16, 0, 3, 16, sign=True)
    assert (dev["lpc_sums"][:, :8] == -1).all() and (dev["meta"]["lpc_order"] == -1).all()
    assert not dev["meta"]["status"].any() and not dev["meta"]["kind"].any()


def test_negative_shift_orders_are_not_candidates(az):
    """The high-frequency multi-tone recipes of tests/golden/make_golden.py (n = 512, q 5): the
    quantiser's ([], 0) branch on some orders, which are then not eligible."""
    def multitone(freqs, amp, n):
        K = len(freqs)
        return [round(amp * sum(math.sin(2 * math.pi * f * i / 44100 + 0.5 * k) for k, f in enumerate(freqs)) / K)
                for i in range(n)]
    rows = np.asarray([multitone((19401.4, 17113.6, 10839.5), 30000, 512), multitone((8209.8, 3016.2), 30000, 512),
                       multitone((12316.6, 18965.5, 17232.8, 8024.8), 30000, 512)], dtype=np.int16)
    for sign in (False, True):
        dev, want = check(az, rows, 512, 24, 5, 0, 5, 16, sign=sign)
        base = base_analysis(rows, 512, 24, 5, 0, 5, 16, sign, False)
        masks = [int(r[1]) & 0xFFFFFFFF for r in base["lpc_records"]]
        if not sign:
            assert any(masks)
        for u, mask in enumerate(masks):
            if int(dev["meta"]["status"][u]) == 0:
                assert [int(v) == -1 for v in dev["lpc_sums"][u][:24]] == [bool(mask >> k & 1) for k in range(24)]


def test_tie_units_take_the_first_candidate(az):
    rows, lens = SC.unit_rows("tie16")
    c = SC.CASES["tie16"]
    dev, want = check(az, rows, 16, c["L"], c["q"], c["rmin"], c["rmax"], 16, sign=True)
    for u in range(len(lens)):
        sizes = list(dev["fixed_sums"][u]) + list(dev["lpc_sums"][u][:c["L"]])
        best = min(b for b in sizes if b >= 0)
        assert sizes.count(best) >= 2 and int(dev["meta"]["status"][u]) == 0
        assert int(dev["meta"]["order"][u]) + (4 if int(dev["meta"]["kind"][u]) else 0) == sizes.index(best)


def test_written_width_is_the_stream_s(az):
    """12-bit data in a 24-bit stream: reserved[2] = 24 and not batch.sample_bits decides; 0 falls
    back to batch.sample_bits."""
    rows = SC.narrow_units()
    d24, w24 = check(az, rows, 192, 8, 12, 0, 3, 12, sign=True, sample_size=24)
    d12, w12 = check(az, rows, 192, 8, 12, 0, 3, 12, sign=True)
    pick = lambda d: [(int(k), int(o)) for k, o in zip(d["meta"]["kind"], d["meta"]["order"])]  # noqa: E731
    assert pick(d24) != pick(d12)


def test_production_shape(az):
    """64 units of 4608, L 12, q 12, r 0..5, corrected sign."""
    rows = oracle.synth_batch(0, 64, 4608, 16, 2024, dtype=np.int16)
    dev, want = check(az, rows, 4608, 12, 12, 0, 5, 16, sign=True, sums=False)
    assert not dev["meta"]["status"].any()


def test_refused_combinations(az):
    a = np.zeros((1, 64), dtype=np.int16)
    a[0, ::3] = 100
    for p in (make_params(8, 12, 0, 3, size_choice=True),                                        # without the exact search
              make_params(8, 12, 0, 3, abi.MODE_LPC_ONLY, lpc_sign=True, size_choice=True),
              make_params(8, 12, 0, 3, abi.MODE_RICE_ONLY, rice_search=True, size_choice=True),
              make_params(8, 12, 0, 9, rice_search=True, size_choice=True),                      # rice_max > 8
              make_params(8, 12, 0, 3, rice_search=True, size_choice=True, sample_size=34),
              make_params(8, 12, 0, 3, rice_search=True, size_choice=True, sample_size=-1)):
        with pytest.raises(FlacmiError):
            az.analyze(np.zeros((1, 1024), dtype=np.int16) if p.rice_max == 9 else a, p, 1024 if p.rice_max == 9 else 64)
    # with the flag clear reserved[2] is not looked at, as before
    p = make_params(8, 12, 0, 3, sample_size=99)
    q = make_params(8, 12, 0, 3)
    r1, r2 = az.analyze(a, p, 64), az.analyze(a, q, 64)
    assert r1["meta"].tobytes() == r2["meta"].tobytes()
