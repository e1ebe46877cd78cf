"""k_resid_stream (flac-py_amd/csrc/k_stream.hip) over every shape class its host check accepts,
against the CPU oracle, bit for bit, through the production call and the debug call: one to four
waves, full, ragged and nearly empty chunk slots, every number of MFMA groups with L on and off a
multiple of 4, the branch-free orders-0..5 build and the runtime-order one, finest partitions no
longer than the predictor order, candidate sums past 2^32, and a tail class that takes a second
stream build in the same call.  The table, its inputs and the conditions on them live in
tests/stream_shape_cases.py (tests/test_stream_shape_cases.py runs those without a device).

Which kernel took a unit is read off meta.lpc_tiers in reference mode (x/4: the batch kernel's
quarter tiers, 1/1: its list kernel, 0/1 or 1/1 after the sign bound: k_resid's list variant);
the debug call also pins acf, every fixed and LPC sum and the LPC records.  Only the 68-unit cases
(orders 0..5: n = 256, 2560, 2816, 4096, 5120, 5376, 7680, 7936, 10240) reach k_lpc_tile<4/8/12>
with them: the others hold 56 or 62 units, fewer than the tile kernel's whole wave of 64, and run
k_lpc<LMAX,int16_t>.  tests/test_gpu_lpc_shapes.py sweeps the k_lpc kernels over block lengths."""
import numpy as np
import pytest

import stream_shape_cases as S
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params
from test_gpu_parity import compare_with_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def run_both(az, a, ora, params, block, lens, tail=(0, 0)):
    """The production call and the debug call, each against the oracle -> the production output."""
    prod = None
    for debug in (False, True):
        out = az.analyze(a, params, block, tail[0], tail[1], sample_bits=16, debug=debug)
        compare_with_oracle(out, ora, lens)
        prod = prod or out
    return prod


def assert_dispatch_marks(prod, classes):
    """meta.lpc_tiers of a production run against the class restated on the oracle's record."""
    t = prod["meta"]["lpc_tiers"].astype(np.int64)
    for u, k in enumerate(classes):
        if k is None:
            continue
        if k == "batch":    # the only proof that the stream kernel took the launch
            assert int(t[u]) >> 8 == 4 and 1 <= (int(t[u]) & 0xff) <= 5, (u, k, int(t[u]))
        elif k == "list":
            assert int(t[u]) == 1 | 1 << 8, (u, k, int(t[u]))
        else:
            assert int(t[u]) == ((1 << 8) if k[1] else (1 | 1 << 8)), (u, k, int(t[u]))
    return S.class_counts(classes)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_reference_mode_shapes(az, case):
    S.check_dispatch(case)
    facts = S.check_case_oracle(case)
    a, ora = S.case_reference(case)
    lens = [case.n] * len(a)
    prod = run_both(az, a, ora, make_params(case.L, case.q, case.rmin, case.rmax), case.n, lens)
    seen = assert_dispatch_marks(prod, S.classify(a, ora, case.L, lens))
    print(S.case_id(case), "device classes", dict(seen), facts)
    assert seen["batch"] >= 1 and seen["list"] >= 1 and seen["list2"] >= case.min_list2, seen


@pytest.mark.parametrize("case", S.FIXED_CASES, ids=S.case_id)
def test_fixed_only_shapes(az, case):
    """MODE_FIXED_ONLY (NG 0) over the same inputs.  No lpc_tiers marker exists in this mode: the
    restated host check (check_dispatch) is the only evidence that k_resid_stream takes these."""
    S.check_dispatch(case, fixed_only=True)
    S.check_case_oracle(case, fixed_only=True)
    a, ora = S.case_reference(case, True)
    prod = run_both(az, a, ora, make_params(0, case.q, case.rmin, case.rmax, abi.MODE_FIXED_ONLY), case.n,
                    [case.n] * len(a))
    assert (prod["meta"]["lpc_tiers"] == 0).all()


@pytest.mark.parametrize("fixed_only", [True, False], ids=["fixed-only", "reference"])
def test_candidate_sums_past_2_pow_32(az, fixed_only):
    """Full-scale units of 10240 samples: the fixed order-4 sum of full-scale alternation is
    5 366 530 080, so a 32-bit slip in the cross-wave sums or in the argmin key (sum * 16 + order)
    shows; the constant units raise in the Rice search, on the device as in the oracle."""
    S.check_full_scale_oracle(fixed_only)
    a, ora = S.full_scale_reference(fixed_only)
    n = a.shape[1]
    p = make_params(0, 5, 0, 5, abi.MODE_FIXED_ONLY) if fixed_only else make_params(12, 5, 0, 5)
    prod = run_both(az, a, ora, p, n, [n] * len(a))
    for u in (0, 1):
        assert (int(prod["meta"]["status"][u]), int(prod["meta"]["site"][u])) == (3, 12), u


@pytest.mark.parametrize("block,tail,L", S.TAIL_CALLS, ids=lambda v: str(v))
def test_tail_class_on_the_stream_kernel(az, block, tail, L):
    """A short last block that is itself a stream shape: a second stream build in the same call,
    both launches through the same retry-list buffers.  The 4608 body takes the constant-shape
    build, so that call runs under both values of FLACMI_STREAM_GENERIC."""
    facts = S.check_tail_oracle(block, tail, L)
    a, ora = S.tail_reference(block, tail, L)
    lens = [block] * (S.TAIL_UNITS - S.TAIL_CUT) + [tail] * S.TAIL_CUT
    classes = S.classify(a, ora, L, lens)
    for generic in ((0, 1) if facts["body"]["NFIX"] else (0,)):
        with knob("FLACMI_STREAM_GENERIC", generic):
            prod = run_both(az, a, ora, make_params(L, S.TAIL_Q, 0, 5), block, lens, (tail, S.TAIL_CUT))
        nb = assert_dispatch_marks(prod, classes[:-S.TAIL_CUT])
        nt = assert_dispatch_marks({"meta": prod["meta"][-S.TAIL_CUT:]}, classes[-S.TAIL_CUT:])
        print((block, tail, L), "generic", generic, "device classes: body", dict(nb), "tail", dict(nt))
        assert nb["batch"] >= 1 and nb["list"] + nb["list2"] >= 1 and nt["list"] + nt["list2"] >= 1, (nb, nt)
