"""The corrected-LPC-sign mode (FLACMI_FLAG_LPC_SIGN, include/flacmi.h) on the CPU: the model of
tests/lpc_sign_model.py (oracle pieces, a Python negation) and the oracle frame writer give, for
every stream of tests/lpc_sign_cases.py, the bytes that the reference's own encode() gave with
its levinson_durbin's result negated (tests/golden/lpc_sign_streams.json, made by
tests/golden/make_lpc_sign_golden.py and read back there by the reference decoder).  No GPU."""
import functools
import json

import numpy as np
import pytest

import frame_writer as FW
import lpc_sign_cases as LC
import lpc_sign_model as LM
import oracle
from flac_amd import abi


@pytest.fixture(scope="module")
def golden():
    return json.load(open(LC.GOLDEN))["cases"]


@functools.lru_cache(maxsize=None)
def analysis(name):
    """The case's rows and the model's analysis, computed once and shared."""
    c = LC.CASES[name]
    rows = LC.case_rows(name)
    tail = LC.tail_len(name)
    out = LM.analyze(rows, oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], tail,
                     c["C"] if tail else 0, sample_bits=c["ss"])
    return rows, out


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == sorted(LC.CASES)
    for name, c in LC.CASES.items():
        assert golden[name]["params"] == c, name
        assert golden[name]["samples_sha256"] == LC.samples_sha256(name), name
    written = [v for g in golden.values() for u, v in enumerate(g["verdicts"])
               if u // g["params"]["C"] < len(g["frames"])]
    assert {v[0] for v in written} == {"fixed", "lpc"}
    assert sum(g["asymmetric"] for g in golden.values()) >= 1
    assert golden["silence"]["raises"] == "ZeroDivisionError"
    assert {g["params"]["C"] for g in golden.values()} >= {1, 2, 3}
    assert {g["params"]["q"] for g in golden.values()} >= {5, 6, 15}


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_model_matches_the_patched_reference(golden, name):
    c, g = LC.CASES[name], golden[name]
    rows, out = analysis(name)
    assert FW.stream_header(c["rate"], c["ss"], c["C"], c["frames"], c["n"]).hex() == g["header"]
    frames = FW.frames_from_analysis(rows, out, c["C"], c["n"], LC.tail_len(name), c["ss"], c["q"])
    assert len(frames) == LC.n_blocks(name)
    for f, want in enumerate(g["frames"]):
        assert isinstance(frames[f], bytes), f"frame {f}: {frames[f]!r}"
        assert LC.same_frame(frames[f], want), f"frame {f}"
    if g["raises"] is not None:
        assert type(frames[len(g["frames"])]).__name__ == g["raises"]
    # per unit: the reference's verdict
    for u, v in enumerate(g["verdicts"]):
        m = out["meta"][u]
        if isinstance(v, str):
            assert FW._EXC[int(m["status"])].__name__ == v, u
        else:
            assert int(m["status"]) == 0 and (["fixed", "lpc"][int(m["kind"])], int(m["order"])) == tuple(v), u
    assert out["asymmetric"] == g["asymmetric"]


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_frames_decode_to_the_input(name):
    c = LC.CASES[name]
    rows, out = analysis(name)
    frames = FW.frames_from_analysis(rows, out, c["C"], c["n"], LC.tail_len(name), c["ss"], c["q"])
    x = LC.channels(name)
    seen = 0
    for f, data in enumerate(frames):
        if not isinstance(data, bytes):
            continue
        number, chans = LM.decode_frame(data, c["C"], c["ss"])
        assert number == f
        assert np.array_equal(np.asarray(chans, dtype=np.int64), x[:, f * c["n"]:(f + 1) * c["n"]]), f
        seen += 1
    assert seen >= 2


def test_negation_is_not_a_negated_record():
    """quantise(-c) != -quantise(c) where a running error rounds to +2^(q-1): the clamp keeps
    -2^(q-1) and cuts +2^(q-1) to 2^(q-1) - 1, and the error feedback carries the difference on."""
    st, _, a, _ = oracle.quantize(np.array([1.99, 0.01]), 5)         # shift 3: 15.92 -> 16 clamps to 15
    st2, _, b, _ = oracle.quantize(np.array([-1.99, -0.01]), 5)      # -15.92 -> -16 stays
    assert a == [15, 1] and b == [-16, 0]


def test_mode_off_is_the_oracle():
    """The model's pieces with the negation left out are oracle.analyze_batch itself: what the
    model adds is the sign and nothing else."""
    c = LC.CASES["mono16"]
    rows = LC.case_rows("mono16")
    ora = oracle.analyze_batch(rows, oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"],
                               LC.tail_len("mono16"), 1, sample_bits=16)
    out = analysis("mono16")[1]
    # the reference's sign: the fixed predictor wins everywhere; the corrected one: LPC does
    assert (ora["meta"]["kind"] == abi.KIND_FIXED).all() and (out["meta"]["kind"] == abi.KIND_LPC).all()
    assert np.array_equal(ora["meta"]["fixed_sum"], out["meta"]["fixed_sum"])
    assert (out["meta"]["lpc_sum"] < ora["meta"]["lpc_sum"]).all()
