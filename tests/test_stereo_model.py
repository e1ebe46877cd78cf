"""The stereo-decorrelation rule (FLACMI_STEREO_BEST, include/flacmi.h) on the CPU: the model of
tests/stereo_model.py over the oracle's analysis of left, right, mid and side gives, for every
case of tests/stereo_cases.py with fallback off and on, the channel codes and the frame bytes
that the reference's own writers gave (tests/golden/stereo_streams.json, made by
tests/golden/make_stereo_golden.py and read back there by the reference decoder).  No GPU."""
import functools
import json

import pytest

import frame_writer as FW
import oracle
import stereo_cases as SC
import stereo_model as SM

RUNS = [(name, mode) for name, c in sorted(SC.CASES.items()) for mode in c["modes"]]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(SC.GOLDEN))["cases"]


@functools.lru_cache(maxsize=None)
def analysis(name):
    """The case's rows and the oracle's analysis of its candidates, computed once and shared."""
    c = SC.CASES[name]
    rows, _ = SC.case_rows(name)
    params = oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"])
    return rows, SM.analyse(rows, params, c["n"], c["tail"], c["ss"])


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == sorted(SC.CASES)
    for name, c in SC.CASES.items():
        g = golden[name]
        assert g["params"] == {k: c[k] for k in g["params"]}, name
        assert g["recipes"] == c["recipes"] and g["samples_sha256"] == SC.samples_sha256(name), name
        for mode in c["modes"]:
            assert g[mode]["codes"] == SC.EXPECT[(name, mode)], (name, mode)
    # every assignment is chosen somewhere, a frame fails without fallback, and the tie of the
    # `equal` pair (L_S = S_R = M_S with fallback) goes to the first in the rule's order
    codes = {code for g in golden.values() for mode in ("off", "on") if mode in g for code in g[mode]["codes"]}
    assert codes == {SC.L_R, SC.L_S, SC.S_R, SC.M_S, None}
    assert golden["st16"]["on"]["codes"][5] == SC.L_S


@pytest.mark.parametrize("name,mode", RUNS)
def test_model_matches_the_reference_writers(golden, name, mode):
    c = SC.CASES[name]
    rows, cands = analysis(name)
    frames, codes, sizes = SM.frames(rows, cands, c["n"], c["tail"], c["q"], c["first"], fallback=mode == "on")
    g = golden[name]
    assert codes == g[mode]["codes"]
    for f, (got, want) in enumerate(zip(frames, g[mode]["frames"])):
        if isinstance(want, dict) and "raises" in want:
            assert type(got).__name__ == want["raises"], f"frame {f}: {got!r}"
        else:
            assert isinstance(got, bytes), f"frame {f}: {got!r}"
            assert SC.same_frame(got, want), f"frame {f}"
    # the oracle fails exactly where the reference raised, with its exception, and counts the
    # reference's bits where it did not
    for f, (cand, dry) in enumerate(zip(cands, g["candidates"])):
        n = SC.frame_len(name, f)
        for k, ((samples, out, u, w), (raised, bits)) in enumerate(zip(cand, dry)):
            st = int(out["meta"][u]["status"])
            assert (st != 0) == (raised is not None), f"frame {f} candidate {k}: reference {raised}, status {st}"
            if raised is not None:
                assert FW._EXC[st].__name__ == raised, f"frame {f} candidate {k}"
            else:
                assert SM.FM.subframe_bits(samples, out, u, n, w, c["q"]) == bits, f"frame {f} candidate {k}"


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_a_constant_candidate_always_fails_in_the_reference(name):
    """The device scans only candidates with a nonzero status for all-equal samples; the mid of
    the `anti` pair and the side of the `equal` pair are such candidates."""
    _, cands = analysis(name)
    seen = 0
    for f, cand in enumerate(cands):
        n = SC.frame_len(name, f)
        for samples, out, u, _ in cand:
            if (samples[:n] == samples[0]).all():
                seen += 1
                assert int(out["meta"][u]["status"]) in SM.FM.REFERENCE_EXCEPTIONS, f"{name} frame {f}"
    assert seen or "anti" not in SC.CASES[name]["recipes"]


def test_mid_and_side_candidates():
    """floor of an odd negative sum, and the side's extra bit."""
    left, right, mid, side = SC.candidates([-1, 0, 32767, -32768, 3], [0, -1, -32768, 32767, 0])
    assert list(mid) == [-1, -1, -1, -1, 1] and list(side) == [-1, 1, 65535, -65535, 3]
