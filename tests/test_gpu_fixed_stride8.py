"""k_resid_stream's fixed group at row stride 8 (flac-py_amd/csrc/k_stream.hip, fixed8) against the
CPU oracle, bit for bit: the build that takes it is the energy bound's pre-test build (reference
mode, production call; fixed_sums requested, which does not turn pruning off).  The fixed-only build
runs over the same inputs; it keeps the 4-phase fixed group (stride 8 was measured there and gave
nothing: DESIGN §4), and must give the same five sums.  Per unit: all five fixed sums, meta field
for field, the zig-zag residual and the Rice parameters.

Block lengths (tests/fixed_stride8_cases.py holds the inputs and says what each is for):
    64     only the 4-phase tail block (masked)
    128    only the masked step 0
    192    step 0 plus the tail block
    320    one wave, 2.5 steps: the loop's single-step remainder
    2880   two waves, an odd number of 64-sample blocks (the tail on wave 0)
    4608   the constant-shape build, and the runtime-shape build under FLACMI_STREAM_GENERIC
    10240  four waves
each in reference mode at L = 12 and L = 4 and in fixed-only mode."""
import numpy as np
import pytest

import fixed_stride8_cases as F
import stream_shape_cases as S
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params
from test_gpu_parity import compare_with_oracle

pytestmark = pytest.mark.gpu

CASES = [(n, L) for n in F.LENGTHS for L in (12, 4, 0)]


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


@pytest.mark.parametrize("n,L", CASES, ids=lambda v: str(v))
def test_fixed_sums_and_results_match_the_oracle(az, n, L):
    rmin, rmax = F.LENGTHS[n]
    shape = S.stream_shape(n, L, rmin, rmax, L == 0)
    assert shape is not None and S.narrow_path(n, L, F.Q, L == 0), "not a k_resid_stream shape"
    assert shape["NG"] == (0 if L == 0 else 1 if L == 4 else 3)
    assert F.winners(n) == [0, 1, 2, 3, 4]
    a, labels = F.units(n)
    ora = F.reference(n, L)
    om = ora["meta"]
    params = make_params(L, F.Q, rmin, rmax, abi.MODE_REFERENCE if L else abi.MODE_FIXED_ONLY)
    builds = (0, 1) if shape["NFIX"] else (0,)
    assert (n == 4608) == (len(builds) == 2)
    for generic in builds:
        with knob("FLACMI_STREAM_GENERIC", generic):
            out = az.analyze(a, params, n, sample_bits=16, extras=("fixed_sums",))
        compare_with_oracle({k: out[k] for k in ("meta", "rice_params", "residual")}, ora, [n] * len(a))
        checked = 0
        for u, label in enumerate(labels):
            if int(om["status"][u]) != 0 and L:  # the reference raised inside the LPC analysis: no sums
                continue
            assert [int(v) for v in out["fixed_sums"][u]] == [int(v) for v in ora["fixed_sums"][u]], (generic, u, label)
            checked += 1
        assert checked >= len(labels) - 8, checked
        if L:  # the pre-test build took the batch: marks x/4 on the units no list kernel took
            t = out["meta"]["lpc_tiers"].astype(np.int64)
            assert int(((t >> 8) == 4).sum()) >= len(labels) // 2, list(t)
        else:
            assert (out["meta"]["lpc_tiers"] == 0).all()
    if L == 0:  # the (a) units: each fixed order is chosen once
        assert [int(v) for v in om["order"][:5]] == [0, 1, 2, 3, 4]
