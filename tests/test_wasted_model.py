"""tests/wasted_model.py against the definition of wasted bits, without a device: the OR / ctz
form the kernel uses agrees with a per-sample loop for every length 1..70 with the lowest set bit
at the first, the last and a middle sample, at the three sample widths the device tests use; the
corner cases of the rule (silence, the clamp, a lone most negative sample); the model against
tests/golden/wasted_streams.json, which the reference's own writers and its decoder with the two
corrections produced (every unit's w and width, the header's 8 + w bits in the exact CONSTANT and
VERBATIM sizes, subframes that follow each other without a gap, and for the 24-bit cases that are
16-bit samples << 8 every subframe exactly 8 bits longer than the one the reference writes for
the unshifted samples); and that the new entry point and flag are declared and bound."""
import os
import re

import numpy as np
import pytest

import golden_util as G
import wasted_cases as WC
import wasted_model as WM
from flac_amd import abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacmi.h")
WIDTHS = [(np.int16, 16), (np.int32, 24), (np.int32, 32)]


@pytest.mark.parametrize("dtype,ss", WIDTHS)
def test_or_ctz_agrees_with_a_per_sample_loop(dtype, ss):
    rng = np.random.default_rng(ss)
    for n in range(1, 71):
        for at in sorted({0, n // 2, n - 1}):
            for w in (0, 1, 2, 8, ss - 2, ss - 1):
                x = WM.unit_with(n, ss, w, at, dtype, rng)
                assert WM.wasted_of(x, ss) == w == WM.wasted_of_loop(x, ss), (n, at, w)
                y = WM.shifted(x, w)
                assert y.dtype == x.dtype and np.array_equal(y.astype(np.int64) << w, x.astype(np.int64))
                if w < ss - 1:  # the shifted unit has no wasted bits left and fits ss - w bits
                    assert WM.wasted_of(y, ss - w) == 0
                lo, hi = -(1 << (ss - w - 1)), (1 << (ss - w - 1)) - 1
                assert lo <= int(y.min()) and int(y.max()) <= hi


def test_rule_corner_cases():
    assert WM.wasted_of(np.zeros(192, np.int16), 16) == 0            # digital silence: no wasted bits
    assert WM.wasted_of(np.full(192, 256, np.int16), 16) == 8        # all equal 256: CONSTANT of 1 at 8 bits
    assert WM.wasted_of(np.array([0, -32768, 0], np.int16), 16) == 15
    assert WM.wasted_of(np.array([-(1 << 31)], np.int32), 32) == 31
    assert WM.wasted_of(np.array([1 << 20], np.int32), 16) == 15     # out-of-range samples: the clamp
    assert WM.wasted_of(np.array([-2, 4, 6], np.int32), 24) == 1
    assert np.array_equal(WM.shifted(np.array([-2, 4, 6], np.int32), 1), [-1, 2, 3])
    assert np.array_equal(WM.shifted(np.array([-32768, 0], np.int16), 15), [-1, 0])  # width 1: -1 and 0


def test_entry_point_is_declared_and_bound():
    text = open(HEADER).read()
    assert re.search(r"\bint flacmi_wasted_rows_device\(flacmi_ctx\* ctx, const flacmi_batch\* in, void\* out_rows, "
                     r"int64_t out_stride,\s+int32_t\* wasted, void\* stream\);", text)
    res, args = abi.SIGNATURES["flacmi_wasted_rows_device"]
    assert len(args) == 6
    from flac_amd.analysis import Analyzer
    assert callable(Analyzer.wasted_rows_device)


GOLD = G.load("wasted_streams.json")["cases"]


@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_model_reproduces_the_golden_wasted_bits_and_sizes(name):
    c, g = WC.CASES[name], GOLD[name]
    assert WC.samples_sha256(name) == g["samples_sha256"] and g["params"]["ss"] == c["ss"]
    rows, _ = WC.case_rows(name)
    lens = WC.unit_lens(name)
    for u, (ln, s) in enumerate(zip(lens, g["subframes"])):
        w = WM.wasted_of(rows[u, :ln], c["ss"])
        assert w == g["wasted"][u] == s["wasted_bits"] == WC.wasted(name)[u], f"unit {u}"
        assert s["sample_bits"] == c["ss"] - w
        y = WM.shifted(rows[u, :ln], w)
        if g["kinds"][u] == WC.FC.CONSTANT:
            assert s["type"] == "CONSTANT" and (y == y[0]).all() and s["bits"] == WM.constant_bits(w, c["ss"])
        elif g["kinds"][u] == WC.FC.VERBATIM:
            assert s["type"] == "VERBATIM" and s["bits"] == WM.verbatim_bits(ln, w, c["ss"])
        else:  # an analysed subframe is no larger than its VERBATIM form only where the fallback rule ran
            assert s["type"] in ("FIXED", "LPC") and s["bits"] > WM.header_bits(w) + s["order"] * (c["ss"] - w)
            if c["fallback"]:
                assert s["bits"] <= WM.verbatim_bits(ln, w, c["ss"])
    # frame lengths: header, the subframes back to back, padding to a byte, CRC-16
    for f, frame in enumerate(g["frames"]):
        subs = g["subframes"][f * c["C"]:(f + 1) * c["C"]]
        for a, b in zip(subs, subs[1:]):
            assert b["bit_offset"] == a["bit_offset"] + a["bits"]
        end = subs[-1]["bit_offset"] + subs[-1]["bits"]
        nbytes = len(frame) // 2 if isinstance(frame, str) else frame["len"]
        assert nbytes == (end + 7) // 8 + 2, f"frame {f}"


@pytest.mark.parametrize("name", sorted(n for n in WC.CASES if WC.CASES[n]["twin"]))
def test_shifted_24_bit_subframes_are_8_bits_longer_than_their_16_bit_twins(name):
    c, g = WC.CASES[name], GOLD[name]
    assert (c["ss"], c["twin"]) == (24, 8) and len(g["twin_subframes"]) == len(g["subframes"])
    for s, t in zip(g["subframes"], g["twin_subframes"]):
        assert (s["type"], s["order"]) == (t["type"], t["order"])
        assert (t["wasted_bits"], t["sample_bits"], s["sample_bits"]) == (0, 16, 16)
        assert s["bits"] == t["bits"] + 8


def test_default_reading_of_an_unflagged_frame_is_the_input():
    """The fixture's account of the unpatched reference: a frame without wasted bits reads alike
    in both modes; every frame with a flagged subframe raises or returns other samples."""
    for name, g in GOLD.items():
        C = WC.CASES[name]["C"]
        for f, d in enumerate(g["default"]):
            flagged = any(g["wasted"][f * C:(f + 1) * C])
            if not flagged:
                assert d["exception"] is None and d["subframes"] == g["subframes"][f * C:(f + 1) * C]
            else:
                assert d["exception"] is not None or d["subframes"] != g["subframes"][f * C:(f + 1) * C]


def test_decode_flag_is_declared():
    text = open(HEADER).read()
    assert re.search(r"FLACMI_DECODE_WASTED_SPEC = 1,", text) and abi.DECODE_WASTED_SPEC == 1
