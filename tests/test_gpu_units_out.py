"""k_units alone (csrc/k_units.hip, flacmi_units_out_device) against its numpy restatement
(tests/recompress_model.py, itself checked against a per-sample loop on the CPU): the decoder's
frames re-cut into the encoder's unit rows.

Every case runs between two guard regions, in a buffer whose every byte (the pitch padding
included) is garbage beforehand: the rows must equal the model's element for element up to the
pitch (zeros from each unit's length on), the guards must be untouched, the status word of every
frame and the measured width must be the model's."""
import numpy as np
import pytest

import recompress_model as rm

pytestmark = pytest.mark.gpu
CASES = rm.cases()


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def run(az, case, fill=0x5A):
    dt = np.int16 if case["sample_bytes"] == 2 else np.int32
    buf, g, stride, st, width = az.units_out(
        list(zip(case["frames"], case["pitches"])), case["channels"], case["s0"], case["block_len"], case["n_blocks"],
        case["tail_len"], case["sample_size"], case["sample_bytes"], stride=case["stride"], fill=fill,
        firsts=case.get("firsts"))
    n_units = (case["n_blocks"] + (1 if case["tail_len"] else 0)) * case["channels"]
    assert stride == case["stride"] and buf.dtype == dt
    guard_word = np.frombuffer(bytes([fill]) * dt().itemsize, dtype=dt)[0]
    assert (buf[:g] == guard_word).all(), "guard before the rows written"
    assert (buf[g + n_units * stride:] == guard_word).all(), "guard behind the rows written"
    return buf[g:g + n_units * stride].reshape(n_units, stride), st, width


@pytest.mark.parametrize("name", sorted(CASES))
def test_units_equal_the_model(az, name):
    case = CASES[name]
    want, status, width, mask = rm.units_out(*rm.model_args(case), firsts=case.get("firsts"))
    got, st, w = run(az, case)
    assert np.array_equal(st, status), (st, status)
    assert w == width
    assert rm.sample_bits(w, case["sample_size"]) == rm.sample_bits(width, case["sample_size"])
    bad = np.argwhere((got != want) & mask)
    assert bad.size == 0, f"first differing (unit, element): {bad[:5].tolist()}"
    if "bad_frames" in case:
        assert tuple(np.nonzero(st)[0]) == tuple(case["bad_frames"])


def test_zero_fill_does_not_depend_on_what_was_there(az):
    """the same call over two different garbage patterns: identical rows (nothing kept, nothing skipped)"""
    case = CASES["frame_5000_over_27_units"]
    a, _, _ = run(az, case, fill=0x5A)
    b, _, _ = run(az, case, fill=0xC3)
    assert np.array_equal(a, b)
    assert not a[-case["channels"]:, case["tail_len"]:].any()   # the tail units: zeros from tail_len, not from block_len


def test_status_and_width_are_reset_by_the_call(az):
    """az.units_out fills both with -1 first: a call without findings leaves 0 and the true width"""
    case = CASES["range16_fits"]
    _, st, w = run(az, case)
    assert not st.any() and w == 32767
    _, st, w = run(az, CASES["no_frames"])
    assert st.size == 0 and w == 0
