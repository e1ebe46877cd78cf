"""The stream kernel's shape table (tests/stream_shape_cases.py) without a device: the restated
host check against the kernel source's constants and against every case's expected build, and
every condition the GPU tests place on their inputs, on the CPU oracle alone."""
import os
import re

import pytest

import stream_shape_cases as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flac-py_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_match_the_source():
    """A retuned kSCPT / kCPT or a changed host check must change the restatement with it."""
    k = _source("k_stream.hip")
    assert int(re.search(r"#define FLACMI_STREAM_CPT (\d+)", k).group(1)) == S.K_SCPT
    assert "a.n % 64 != 0 || a.n < 64 || a.n > 8 * kSCPT * 256" in k
    assert "(1 << rmax_eff) > 32 || ((a.n >> rmax_eff) & 7) != 0" in k
    assert "a.rmin == 0 && rmax_eff == 5 && (a.n >> 5) > maxord" in k
    assert int(re.search(r"constexpr int kCPT = (\d+);", _source("device_common.h")).group(1)) == S.K_CPT


def test_restated_host_check():
    f = S.stream_shape
    assert S.stream_threads(2560) == 64 and S.stream_threads(2624) == 128 and S.stream_threads(10240) == 256
    # the BASELINE shapes: the constant-shape build at L = 4 NG only
    assert f(4608, 12, 0, 5, False) == {"nw": 2, "slots": 4.5, "P": 32, "R05": True, "NG": 3, "NFIX": 4608}
    assert f(4608, 11, 0, 5, False)["NFIX"] == 0 and f(4608, 0, 0, 5, True)["NFIX"] == 4608
    # refused: not a multiple of 64, too long, too many or ragged finest partitions, L, no order
    for args in ((3240, 8, 0, 5, False), (10304, 12, 0, 5, False), (1152, 12, 0, 6, False), (64, 12, 0, 5, False),
                 (1024, 13, 0, 5, False), (1024, 0, 0, 5, False), (1024, 12, 3, 2, False), (192, 12, 6, 6, False)):
        assert f(*args) is None, args
    assert f(1024, 0, 0, 5, True)["NG"] == 0
    # R05 needs n / 32 above every predictor order: L in reference mode, 4 in fixed-only mode
    assert not f(256, 12, 0, 5, False)["R05"] and f(256, 7, 0, 5, False)["R05"] and f(256, 0, 0, 5, True)["R05"]
    assert not f(128, 4, 0, 4, False)["R05"] and not f(4096, 12, 1, 5, False)["R05"] and not f(4096, 12, 0, 4, False)["R05"]
    assert not S.narrow_path(4608, 12, 9, False) and S.narrow_path(4608, 12, 8, False)


def test_table_covers_the_family():
    shapes = [S.check_dispatch(c) for c in S.CASES]
    assert {s["nw"] for s in shapes} == {1, 2, 3, 4}
    assert {s["NG"] for s in shapes} == {1, 2, 3} and {c.L % 4 != 0 for c in S.CASES} == {True, False}
    for nw in (2, 3, 4):  # a full last slot, and a ragged one, at every multi-wave size
        slots = [s["slots"] for s in shapes if s["nw"] == nw]
        assert S.K_SCPT in slots and any(v != int(v) for v in slots), (nw, slots)
    assert min(s["slots"] for s in shapes) < 1                       # fewer chunks than lanes
    assert {s["P"] for s in shapes} >= {4, 8, 16, 32}
    assert {(s["R05"], c.rmin > 0) for s, c in zip(shapes, S.CASES)} >= {(True, False), (False, False), (False, True)}
    assert len(S.FIXED_CASES) == 6
    for c in S.FIXED_CASES:
        assert S.check_dispatch(c, fixed_only=True)["NG"] == 0


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_reference_case_inputs(case):
    facts = S.check_case_oracle(case)
    print(S.case_id(case), facts)


@pytest.mark.parametrize("case", S.FIXED_CASES, ids=S.case_id)
def test_fixed_only_case_inputs(case):
    S.check_case_oracle(case, fixed_only=True)


@pytest.mark.parametrize("fixed_only", [True, False], ids=["fixed-only", "reference"])
def test_full_scale_inputs(fixed_only):
    S.check_full_scale_oracle(fixed_only)


@pytest.mark.parametrize("block,tail,L", S.TAIL_CALLS, ids=lambda v: str(v))
def test_tail_call_inputs(block, tail, L):
    facts = S.check_tail_oracle(block, tail, L)
    assert (facts["body"]["NFIX"] == 4608) == (block == 4608)
    assert S.stream_shape(64, L, 0, 5, False) is None  # 64 >> 5 = 2: not a tail to use here
