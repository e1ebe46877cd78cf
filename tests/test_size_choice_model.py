"""The CPU model of FLACMI_FLAG_SIZE_CHOICE (tests/size_choice_model.py) against the fixture
written with the reference's own writers (tests/golden/size_choice_streams.json): every unit's
choice, every candidate's bits, the Rice fields and the frame bytes; every candidate's bits against
what tests/frame_assembler.py writes for it; and the refusals that need no device."""
import functools
import os

import numpy as np
import pytest

import fallback_model as FM
import frame_assembler as FA
import golden_util as G
import lpc_sign_model as LS
import oracle
import size_choice_cases as SC
import size_choice_model as SZ
from flac_amd import abi
from flac_amd import encoder as enc

GOLD = G.load("size_choice_streams.json")["cases"]


@functools.lru_cache(maxsize=None)
def modelled(name):
    """(rows, lens, the analysis with the flag clear, the model's results) of a case, computed once."""
    c = SC.CASES[name]
    rows, lens = SC.unit_rows(name)
    n_tail = c["C"] if c["tail"] else 0
    if c["fixed_only"]:
        base = oracle.analyze_batch(rows, oracle.make_params(0, c["q"], c["rmin"], c["rmax"], abi.MODE_FIXED_ONLY), c["n"],
                                    c["tail"], n_tail, sample_bits=c["ss"])
    else:
        p = oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"])
        analyse = LS.analyze if c["sign"] else oracle.analyze_batch
        base = analyse(rows, p, c["n"], c["tail"], n_tail, sample_bits=c["ss"])
    want = SZ.apply(base, rows, lens, c["L"], c["q"], c["rmin"], c["rmax"], c["ss"], fixed_only=c["fixed_only"])
    return rows, lens, base, want


def test_fixture_is_current():
    assert set(GOLD) == set(SC.CASES)
    for name, g in GOLD.items():
        assert g["samples_sha256"] == SC.samples_sha256(name), name
        assert g["params"] == {k: v for k, v in SC.CASES[name].items() if k != "plan"}, name
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "size_choice_streams.json")
    assert os.path.getsize(path) <= 250_000


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_model_is_the_fixture(name):
    c, g = SC.CASES[name], GOLD[name]
    rows, lens, base, want = modelled(name)
    assert len(g["units"]) == len(lens)
    for u, gu in enumerate(g["units"]):
        m = want["meta"][u]
        if gu["raised"] is not None:  # the LPC stage raises: the status of the analysis, nothing chosen
            assert int(m["status"]) != 0 and int(m["site"]) in SZ.LPC_STAGE_SITES and want["choices"][u] is None, u
            assert int(m["status"]) == {"ZeroDivisionError": 1, "AssertionError": 2, "ValueError": 3, "OverflowError": 4}[gu["raised"]]
            continue
        assert int(m["status"]) == 0, u
        assert list(want["fixed_sums"][u]) == gu["fixed"], u
        assert list(want["lpc_sums"][u][:len(gu["lpc"])]) == gu["lpc"] and not want["lpc_sums"][u][len(gu["lpc"]):].any(), u
        family, order = gu["choice"]
        assert (int(m["kind"]), int(m["order"])) == (abi.KIND_LPC if family == "lpc" else abi.KIND_FIXED, order), u
        assert want["choices"][u]["best"]["bits"] == gu["bits"], u
        assert (int(m["part_order"]), int(m["coding_method"])) == (gu["part_order"], gu["coding_method"]), u
        assert list(want["rice_params"][u][:int(m["n_parts"])]) == gu["rice_params"], u
        # fixed_order / lpc_order: the first smallest eligible candidate of each family
        fb = [b for b in gu["fixed"] if b >= 0]
        assert (int(m["fixed_order"]), int(m["fixed_sum"])) == (gu["fixed"].index(min(fb)), min(fb)), u
        if c["fixed_only"]:
            assert (int(m["lpc_order"]), int(m["lpc_sum"])) == (0, 0), u
        else:
            lb = [b for b in gu["lpc"] if b >= 0]
            assert (int(m["lpc_order"]), int(m["lpc_sum"])) == (gu["lpc"].index(min(lb)) + 1, min(lb)), u
        assert int(m["lpc_tiers"]) == 0


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_model_frames_are_the_fixture_frames(name):
    """The model's analysis through the frame writer's CPU model: the bytes of the fixture."""
    c, g = SC.CASES[name], GOLD[name]
    rows, lens, base, want = modelled(name)
    frames, kinds = FM.frames(rows, want, c["C"], c["n"], c["tail"], c["ss"], c["q"], fallback=bool(c.get("fallback")))
    assert kinds == [u["kind"] for u in g["units"]]
    assert [f.hex() for f in frames] == g["frames"]
    for f, data in enumerate(frames):  # and back to the samples, with a reader of the tests' own
        number, chans = LS.decode_frame(data, c["C"], c["ss"])
        assert number == f
        for k in range(c["C"]):
            u = f * c["C"] + k
            assert chans[k] == [int(v) for v in rows[u][:lens[u]]]


@pytest.mark.parametrize("name", ["mix16", "tri24", "tie16", "st16"])
def test_candidate_bits_are_what_the_assembler_writes(name):
    c = SC.CASES[name]
    rows, lens, base, want = modelled(name)
    seen = 0
    for u, r in enumerate(want["choices"]):
        x = [int(v) for v in rows[u][:lens[u]]]
        for lpc, bits_list in ((False, r["fixed"]), (True, r["lpc"])):
            for k, bits in enumerate(bits_list):
                if bits < 0:
                    continue
                P = k + 1 if lpc else k
                coefs, shift = (SZ.record_order(base["lpc_records"][u], P)[:2]) if lpc else (list(FA.FIXED[P]), 0)
                z = LS.zigzag(LS.lpc_residual(np.asarray(x, dtype=np.int64), coefs, shift))
                s = SZ.RM.search_np(z, len(x), P, c["rmin"], c["rmax"])
                b = FA.Bits()
                method = 0 if s["coding_method"] == 4 else 1
                if lpc:
                    FA.sub_lpc(b, x, coefs, c["q"], shift, c["ss"], s["part_order"], s["rice_params"], method, exact=True)
                else:
                    FA.sub_fixed(b, x, P, c["ss"], s["part_order"], s["rice_params"], method, exact=True)
                assert b.n == bits, (u, lpc, P)
                seen += 1
    assert seen >= 5 * len(lens)


def test_the_rules_part_ways_where_the_issue_says():
    """With the corrected sign: noise is FIXED by size and LPC by sum |r|; AR units are LPC at a lower
    order; the tone units agree.  Without it the rules disagree on noise.  The pinned 16-sample
    units tie at the minimum and the first candidate wins."""
    mix = GOLD["mix16"]["units"]
    kinds = SC.CASES["mix16"]["plan"][0]
    for u, kind in zip(mix, kinds):
        if kind == "noise":
            assert u["choice"][0] == "fixed" and u["sum_rule"][0] == "lpc"
        if kind == "ar":
            assert u["choice"][0] == u["sum_rule"][0] == "lpc" and u["choice"][1] < u["sum_rule"][1]
        if kind == "tone":
            assert u["choice"] == u["sum_rule"]
    assert any(u["choice"] != u["sum_rule"] for u in GOLD["nosign16"]["units"])
    _, _, _, want = modelled("tie16")
    for r in want["choices"]:
        sizes = r["fixed"] + r["lpc"]
        best = min(b for b in sizes if b >= 0)
        assert sizes.count(best) >= 2
        chosen = r["best"]["P"] + (4 if r["best"]["lpc"] else 0)
        assert chosen == sizes.index(best)


def test_eligibility():
    """n = 16, L 12: with rice_min 1 no candidate of order >= 8 is eligible, with rice_min 2 fixed order 4
    is not either, with rice_min 5 none is; q = 16 bars every LPC candidate; n <= 4 has fixed order 0 only."""
    x = np.random.default_rng(5).integers(-50, 51, (1, 16)).astype(np.int16)
    base = oracle.analyze_batch(x, oracle.make_params(12, 12, 0, 5), 16, sample_bits=16)
    assert int(base["meta"]["site"][0]) not in SZ.LPC_STAGE_SITES
    r1 = SZ.unit(x[0], base["lpc_records"][0], 12, 12, 1, 5, 16)
    assert all(b >= 0 for b in r1["fixed"]) and all((b >= 0) == (P < 8) for P, b in enumerate(r1["lpc"], 1))
    r2 = SZ.unit(x[0], base["lpc_records"][0], 12, 12, 2, 5, 16)
    assert [b >= 0 for b in r2["fixed"]] == [True] * 4 + [False] and all((b >= 0) == (P < 4) for P, b in enumerate(r2["lpc"], 1))
    r5 = SZ.unit(x[0], base["lpc_records"][0], 12, 12, 5, 5, 16)
    assert r5["best"] is None and set(r5["fixed"] + r5["lpc"]) == {-1}
    w = SZ.apply(base, x, [16], 12, 12, 5, 5, 16)
    assert (int(w["meta"]["status"][0]), int(w["meta"]["site"][0])) == (SZ.STATUS_ASSERTION, SZ.SITE_RICE_NO_ORDER)
    b16 = oracle.analyze_batch(x, oracle.make_params(8, 16, 0, 2), 16, sample_bits=16)
    r16 = SZ.unit(x[0], b16["lpc_records"][0], 8, 16, 0, 2, 16)
    assert set(r16["lpc"]) == {-1} and not r16["best"]["lpc"]
    r4 = SZ.unit(x[0][:4], None, 0, 12, 0, 2, 16, reference=False)
    assert [b >= 0 for b in r4["fixed"]] == [True, False, False, False, False] and r4["lpc_best"] == (0, 0)


def test_written_width_enters_the_choice():
    """The written width is the stream's, not the width the data fits: on 12-bit data in a 24-bit
    stream the two pick different candidates."""
    rows = SC.narrow_units()
    base = LS.analyze(rows, oracle.make_params(8, 12, 0, 3), 192, sample_bits=12)
    lens = [192] * len(rows)
    at24 = SZ.apply(base, rows, lens, 8, 12, 0, 3, 24)
    at12 = SZ.apply(base, rows, lens, 8, 12, 0, 3, 12)
    assert any((int(a["kind"]), int(a["order"])) != (int(b["kind"]), int(b["order"])) for a, b in zip(at24["meta"], at12["meta"]))


def test_refusals_need_no_device():
    pcm = np.zeros((1, 2048), dtype=np.int64)
    ok = enc.EncoderParameters(block_size=1024, rice_partition_order=range(0, 4), lpc_order=range(0, 9), qlp_precision=12)
    wide = enc.EncoderParameters(block_size=1024, rice_partition_order=range(0, 10), lpc_order=range(0, 9), qlp_precision=12)
    with pytest.raises(ValueError, match="size_choice needs rice_search"):
        next(enc.encode_planar(44100, 16, pcm, ok, size_choice=True))
    with pytest.raises(ValueError, match="size_choice needs rice_search"):
        next(enc.encode(44100, 16, 1, 2048, iter([]), ok, size_choice=True))
    with pytest.raises(ValueError, match="size_choice needs rice_search"):
        next(enc.encode_wav("no-such-file.wav", ok, size_choice=True))
    with pytest.raises(ValueError, match="wasted"):
        next(enc.encode_planar(44100, 16, pcm, ok, size_choice=True, rice_search=True, wasted=True))
    with pytest.raises(ValueError, match="stop <= 9"):
        next(enc.encode_planar(44100, 16, pcm, wide, size_choice=True, rice_search=True))
    with pytest.raises(ValueError, match="stop <= 9"):
        enc._check_size_choice(True, True, False, wide)
    from flac_amd.analysis import make_params
    p = make_params(8, 12, 0, 3, rice_search=True, size_choice=True, sample_size=24)
    assert p.reserved[1] == abi.FLAG_RICE_SEARCH | abi.FLAG_SIZE_CHOICE and abi.FLAG_SIZE_CHOICE == 16 and p.reserved[2] == 24
    assert make_params(8, 12, 0, 3).reserved[2] == 0
    from flac_amd import cli
    args = cli.make_argument_parser().parse_args(["encode", "a.wav", "b.flac", "--rice-search", "--size-choice"])
    assert args.size_choice and not cli.make_argument_parser().parse_args(["encode", "a.wav", "b.flac"]).size_choice
