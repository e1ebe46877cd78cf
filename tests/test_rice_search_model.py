"""tests/rice_search_model.py (the exact Rice search, FLACMI_FLAG_RICE_SEARCH) without a device:
the model on the oracle's analysis, through the frame-writer oracle, gives the bytes the reference's
own encode() wrote with its rice_partitions replaced by the rule
(tests/golden/rice_search_streams.json); the oracle leaves what a rescue needs on a Rice-site
failure; the bit-plane identity the kernel counts with; the search never writes more bits than the
reference where the reference succeeds; the numpy form of the model is the plain-integer one; the
rule's corner cases; and the flag is declared and bound."""
import os
import re

import numpy as np
import pytest

import frame_writer as FW
import golden_util as G
import oracle
import rice_search_cases as RC
import rice_search_model as RM
from flac_amd import abi
from flac_amd.analysis import make_params

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacmi.h")
GOLD = G.load("rice_search_streams.json")["cases"]
MESSAGE_SITE = {"math domain error": 12, "negative shift count": 13}


def _analysis(name):
    c = RC.CASES[name]
    rows, lens = RC.unit_rows(name)
    tail = RC.tail_len(name)
    out = oracle.analyze_batch(rows, oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], tail,
                               c["C"] if tail else 0, sample_bits=c["ss"], threads=4)
    return c, rows, lens, tail, out


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_model_and_frame_writer_give_the_fixture_bytes(name):
    c, rows, lens, tail, out = _analysis(name)
    g = GOLD[name]
    assert RC.samples_sha256(name) == g["samples_sha256"]
    # the oracle, which restates the unchanged reference, fails exactly the units the reference fails, where it does
    for u, before in enumerate(g["reference"]):
        st, site = int(out["meta"]["status"][u]), int(out["meta"]["site"][u])
        assert (st, site) == ((0, 0) if before == "ok" else (3, MESSAGE_SITE[before])), (u, before)
    new = RM.apply(out, lens, c["rmin"], c["rmax"], fast=False)
    assert new["rescued"] == {u for u, b in enumerate(g["reference"]) if b != "ok"}
    for u, want in enumerate(g["units"]):
        m = new["meta"][u]
        assert (int(m["status"]), int(m["site"])) == (0, 0)
        got = {"part_order": int(m["part_order"]), "coding_method": int(m["coding_method"]),
               "rice_params": [int(v) for v in new["rice_params"][u][: int(m["n_parts"])]]}
        assert got == {k: want[k] for k in got}, f"unit {u}"
        # rice_bits in the estimate convention: the written residual bits are the searched W (frame_bits.h)
        over = sum(k > 14 for k in got["rice_params"])
        np_ = int(m["n_parts"])
        written = int(m["rice_bits"]) - (4 * np_ if got["coding_method"] == 4 else 3 * np_ + over)
        assert written == want["bits"]
    frames = FW.frames_from_analysis(rows, new, c["C"], c["n"], tail, c["ss"], c["q"])
    assert [f.hex() if isinstance(f, bytes) else repr(f) for f in frames] == g["frames"]
    assert FW.stream_header(c["rate"], c["ss"], c["C"], c["frames"], c["n"]).hex() == g["header"]


@pytest.mark.parametrize("name", ["gate16m", "gate16s", "tail16"])
def test_oracle_leaves_the_residual_of_a_rice_site_failure(name):
    """A rescued unit's residual comes from the oracle: on sites 12 / 13 it has filled the choice,
    res_offset = order, res_len and the zig-zag row, which is the residual of that predictor."""
    c, rows, lens, tail, out = _analysis(name)
    failed = [u for u in range(len(lens)) if int(out["meta"]["status"][u]) == 3]
    assert failed
    for u in failed:
        m, n = out["meta"][u], lens[u]
        assert int(m["site"]) in RM.RICE_SITES
        assert int(m["res_offset"]) == int(m["order"]) and int(m["res_len"]) == n - int(m["order"])
        one = oracle.analyze_unit(rows[u, :n], oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]))
        assert np.array_equal(one["residual"], out["residual"][u][int(m["order"]):n])
        x = rows[u, :n].astype(np.int64)
        if int(m["kind"]) == 0:  # the fixed residual of that order, zig-zag (encoder.py:341-352, utils.py:91-94)
            r = x.copy()
            for _ in range(int(m["order"])):
                r = np.diff(r)
            zz = (r << 1) ^ (r >> 63)
            assert np.array_equal(one["residual"].astype(np.int64), zz)


def test_bit_plane_identity():
    rng = np.random.default_rng(5)
    for bits in (1, 7, 15, 16, 31, 33, 48):
        for ln in (1, 2, 17, 64):
            v = [int(x) for x in rng.integers(0, 1 << bits, ln, dtype=np.uint64)]
            for k in range(0, 31):
                assert RM.bit_plane_sum(v, k) == sum(x >> k for x in v)
    # the kernel's form: planes 0..29 counted, the rest as z >> 30; D(30) = sum (z >> 30), D(k) = cnt_k + 2 D(k + 1)
    v = [int(x) for x in rng.integers(0, 1 << 40, 50, dtype=np.uint64)] + [0, 1, (1 << 33) - 1]
    D = sum(x >> 30 for x in v)
    for k in range(29, -1, -1):
        D = sum((x >> k) & 1 for x in v) + 2 * D
        assert D == sum(x >> k for x in v)


def _reference_written_bits(m, params):
    over = sum(int(k) > 14 for k in params)
    np_ = int(m["n_parts"])
    return int(m["rice_bits"]) - (4 * np_ if int(m["coding_method"]) == 4 else 3 * np_ + over)


def test_search_never_writes_more_than_the_reference():
    rng = np.random.default_rng(9)
    n, checked, smaller = 192, 0, 0
    for trial in range(60):
        amp = int(rng.choice([3, 40, 900, 20000]))
        x = rng.integers(-amp, amp + 1, n)
        if trial % 3 == 0:
            x[: n // 2] //= 50
        if trial % 4 == 1:  # a few outliers carry the mean: floor(log2(mean)) overshoots the best parameter
            x = rng.integers(-2, 3, n)
            x[rng.choice(n, 6, replace=False)] = 5000
        p = oracle.make_params(0, 5, 0, 4, abi.MODE_RICE_ONLY)
        p.reserved[0] = int(rng.integers(0, 5))
        r = oracle.analyze_unit(x, p)
        if r["status"] != 0 or max(r["rice_params"]) > 30:
            continue
        P = p.reserved[0]
        s = RM.search(r["residual"], n, P, 0, 4)
        ref = _reference_written_bits(r, r["rice_params"])
        assert s["W"] <= ref
        checked += 1
        smaller += s["W"] < ref
    assert checked >= 20 and smaller >= 1


def test_numpy_form_is_the_plain_integer_model():
    rng = np.random.default_rng(3)
    for n, P, rmin, rmax in [(16, 0, 0, 4), (16, 3, 0, 4), (24, 0, 0, 5), (23, 2, 0, 5), (192, 4, 2, 2), (256, 1, 0, 8)]:
        for bits in (0, 1, 3, 14, 15, 16, 31, 33):
            z = [int(v) for v in rng.integers(0, 1 << bits, n - P, dtype=np.uint64)] if bits else [0] * (n - P)
            if bits == 3:
                z[len(z) // 2:] = [0] * (len(z) - len(z) // 2)
            assert RM.search_np(z, n, P, rmin, rmax) == RM.search(z, n, P, rmin, rmax), (n, P, bits)
    assert RM.search([1] * 22, 23, 1, 1, 5) is None and RM.search_np([1] * 22, 23, 1, 1, 5) is None


def test_rule_corner_cases():
    # all zero: k = 0 everywhere and the tie between the orders goes to rice_min
    s = RM.search([0] * 16, 16, 0, 1, 4)
    assert (s["part_order"], s["coding_method"], s["rice_params"], s["W"]) == (1, 4, [0, 0], 2 * 4 + 16)
    # a partition of one value 1: k = 0 and k = 1 both cost 2, the smaller wins
    assert RM.best_parameter([1], 14) == (2, 0)
    # the 14 / 15 boundary: a constant whose best parameter is 14 stays method 4, 15 needs method 5
    lo = RM.search([3 << 13] * 16, 16, 0, 0, 0)
    hi = RM.search([3 << 14] * 16, 16, 0, 0, 0)
    assert (lo["coding_method"], lo["rice_params"]) == (4, [14]) and (hi["coding_method"], hi["rice_params"]) == (5, [15])
    assert hi["rice_bits"] == hi["W"] + 3 + 1 and lo["rice_bits"] == lo["W"] + 4
    # method 5 only when it is strictly smaller: parameters 15 and up where the values need them, never 31
    big = RM.search([(1 << 33) - 1] * 16, 16, 0, 0, 0)
    assert (big["coding_method"], big["rice_params"]) == (5, [30])
    # a spike of 2^15 (zig-zag 2^16) in silence: the silent partitions take 0, the spike's partition of four
    # values 13 (k = 13 and k = 14 both cost 64)
    z = [0] * 64
    z[37] = 1 << 16
    s = RM.search(z, 64, 0, 0, 4)
    assert s["part_order"] == 4 and sorted(set(s["rice_params"])) == [0, 13] and s["coding_method"] == 4
    # no candidate order: nothing changes
    assert RM.candidate_orders(23, 0, 1, 5) == [] and RM.candidate_orders(16, 3, 0, 4) == [0, 1, 2]


def test_apply_leaves_other_failures_alone():
    rows = np.zeros((2, 192), dtype=np.int16)  # digital silence: ZeroDivisionError in Levinson (site 2)
    rows[1] = np.random.default_rng(1).integers(-500, 500, 192)
    out = oracle.analyze_batch(rows, oracle.make_params(8, 5, 0, 4), 192, sample_bits=16)
    assert int(out["meta"]["status"][0]) == 1
    new = RM.apply(out, [192, 192], 0, 4)
    assert not RM.meta_fields_differ(new["meta"][0], out["meta"][0]) and new["rescued"] == set()
    changed = RM.meta_fields_differ(new["meta"][1], out["meta"][1])
    assert set(changed) <= set(RM.SEARCHED)


def test_flag_is_declared_and_bound():
    text = open(HEADER).read()
    assert re.search(r"FLACMI_FLAG_RICE_SEARCH = 8,", text) and abi.FLAG_RICE_SEARCH == 8
    assert make_params(12, 5, 0, 5, rice_search=True).reserved[1] == 8
    assert make_params(12, 5, 0, 5, lpc_sign=True, rice_search=True).reserved[1] == 12
    assert make_params(12, 5, 0, 5).reserved[1] == 0
    from flac_amd.cli import make_argument_parser
    assert make_argument_parser().parse_args(["encode", "a.wav", "b.flac", "--rice-search"]).rice_search is True
    assert make_argument_parser().parse_args(["encode", "a.wav", "b.flac"]).rice_search is False
