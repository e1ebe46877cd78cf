"""The fallback-subframe rule (FLACMI_FRAME_FALLBACK, include/flacmi.h) on the CPU: the model
of tests/fallback_model.py over the oracle's analysis gives, for every case of
tests/fallback_cases.py, the sub-kinds and the frame bytes that the reference's own writers
gave (tests/golden/fallback_streams.json, made by tests/golden/make_fallback_golden.py and
read back there by the reference decoder).  No GPU."""
import hashlib
import json

import pytest

import fallback_cases as FC
import fallback_model as FM
import frame_writer as FW
import oracle

GOLDEN, same_frame = FC.GOLDEN, FC.same_frame
NAMES = sorted(FC.CASES)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


def analysis(name):
    c = FC.CASES[name]
    rows, n_tail = FC.case_rows(name)
    params = oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"])
    return c, rows, n_tail, oracle.analyze_batch(rows, params, c["n"], c["tail"], n_tail, sample_bits=c["ss"], threads=4)


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == NAMES
    for name in NAMES:
        c, g = FC.CASES[name], golden[name]
        assert g["params"] == {k: c[k] for k in g["params"]}, name
        rows, _ = FC.case_rows(name)
        assert hashlib.sha256(rows.astype("<i8").tobytes()).hexdigest() == g["samples_sha256"], name
        assert g["kinds"] == c["expect"], name
    kinds = [k for g in golden.values() for k in g["kinds"]]
    assert {0, FC.CONSTANT, FC.VERBATIM} <= set(kinds)
    # the size rule's strictly-greater branch and its equality edge are both present
    assert any(r is None and k == FC.VERBATIM and name != "q16"
               for name, g in golden.items() for r, k in zip(g["raised"], g["kinds"]))
    e = golden["equal"]
    assert e["kinds"] == [0] and e["bits"] == [8 + e["params"]["n"] * e["params"]["ss"]]


@pytest.mark.parametrize("name", NAMES)
def test_model_matches_the_reference_writers(golden, name):
    c, rows, n_tail, ora = analysis(name)
    frames, kinds = FM.frames(rows, ora, c["C"], c["n"], c["tail"], c["ss"], c["q"], c["first"])
    g = golden[name]
    assert kinds == g["kinds"]
    assert len(frames) == len(g["frames"]) == c["frames"]
    for f, (got, want) in enumerate(zip(frames, g["frames"])):
        assert isinstance(got, bytes), f"frame {f}: {got!r}"
        assert same_frame(got, want), f"frame {f}"
    # where the reference raised, the oracle has a reference exception (or the writer's
    # precision assertion), and nowhere else
    for u, r in enumerate(g["raised"]):
        m = ora["meta"][u]
        failing = int(m["status"]) in FM.REFERENCE_EXCEPTIONS or \
            (int(m["kind"]) == FW.KIND_LPC and (c["q"] - 1) & 15 == 15)
        assert failing == (r is not None), f"unit {u}: reference {r}, oracle status {int(m['status'])}"
        if r is not None and int(m["status"]):
            assert FW._EXC[int(m["status"])].__name__ == r, f"unit {u}"
        if r is None:
            assert FM.subframe_bits(rows[u], ora, u, FC.unit_lens(name)[u], c["ss"], c["q"]) == g["bits"][u]


@pytest.mark.parametrize("name", NAMES)
def test_a_constant_block_always_fails_in_the_reference(name):
    """The device scans only units with a nonzero status for all-equal samples."""
    c, rows, n_tail, ora = analysis(name)
    for u, ln in enumerate(FC.unit_lens(name)):
        if (rows[u, :ln] == rows[u, 0]).all():
            assert int(ora["meta"][u]["status"]) in FM.REFERENCE_EXCEPTIONS, f"{name} unit {u}"


@pytest.mark.parametrize("name", NAMES)
def test_rule_off_is_the_oracle_writer(name):
    c, rows, n_tail, ora = analysis(name)
    got, kinds = FM.frames(rows, ora, c["C"], c["n"], c["tail"], c["ss"], c["q"], c["first"], fallback=False)
    want = FW.frames_from_analysis(rows, ora, c["C"], c["n"], c["tail"], c["ss"], c["q"], first_frame=c["first"])
    assert not any(kinds)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        if isinstance(b, Exception):
            assert type(a) is type(b)
        else:
            assert a == b
