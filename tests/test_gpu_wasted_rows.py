"""flacmi_wasted_rows_device (k_wasted_rows, csrc/k_wasted.hip) against numpy (tests/wasted_model.py):
wasted[u] and the shifted rows, over block lengths around the 16-byte groups the kernel loads
(4 int32 or 8 int16 samples) up to the largest block, with a shorter tail unit, two input pitches,
in place and out of place.  One batch holds units of w = 0, 1, 8, sample_bits - 1 and an all-zero
one, with the one sample that decides w at index 0, at index n - 1 and in the last partial 16-byte
group.  Full-scale odd garbage lies from every unit's length to the pitch: it must not lower w and
must not be rewritten; nothing but the first `length` elements of each output row is written, in
place units with w == 0 stay bit-identical, and guard words behind the last row and behind
`wasted` stay intact."""
import ctypes as C

import numpy as np
import pytest

import wasted_model as WM
from flac_amd import abi
from flac_amd.analysis import device_batch

pytestmark = pytest.mark.gpu
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 192, 4609, 65535]
WIDTHS = [(np.int16, 16), (np.int32, 24), (np.int32, 32)]
GUARD = 64          # elements behind the last row, and behind wasted


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def _units(n, tail, dtype, ss, rng):
    """[(samples, w)]: the batch described above; the last unit is the shorter tail."""
    g = 16 // np.dtype(dtype).itemsize
    partial = (n - 1) // g * g          # first sample of the group the length falls into
    plan = [(0, 0), (1, n // 2), (8, 0), (ss - 1, n - 1), (None, 0), (8, n - 1), (8, partial), (1, n - 1),
            (0, n - 1), (ss - 1, 0)]
    units = []
    for w, at in plan:
        units.append((np.zeros(n, dtype), 0) if w is None else (WM.unit_with(n, ss, w, at, dtype, rng), w))
    units.append((WM.unit_with(tail, ss, 8, tail - 1, dtype, rng), 8))
    return units


def _rows(units, pitch, dtype):
    """rows [len(units)][pitch] + GUARD elements, the dtype's largest (odd) value wherever no
    sample lies."""
    flat = np.full(len(units) * pitch + GUARD, np.iinfo(dtype).max, dtype=dtype)
    for u, (x, _) in enumerate(units):
        flat[u * pitch:u * pitch + len(x)] = x
    return flat


@pytest.mark.parametrize("dtype,ss", WIDTHS)
@pytest.mark.parametrize("n", LENGTHS)
def test_wasted_rows_match_numpy(az, n, dtype, ss):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sb = np.dtype(dtype).itemsize
    tail = (n + 1) // 2
    base = ((n * sb + 15) // 16) * 16 // sb
    for pitch in (base, base + 128 // sb):
        units = _units(n, tail, dtype, ss, np.random.default_rng(1000 * n + ss + pitch))
        nu = len(units)
        for x, w in units:
            assert WM.wasted_of(x, ss) == w
        want_w = np.array([w for _, w in units], dtype=np.int32)
        rows = _rows(units, pitch, dtype)
        b = lambda t: device_batch(t.data_ptr(), sb, ss, pitch, nu, n, tail, 1)  # noqa: E731

        # out of place, at another pitch: only each unit's own samples are written
        out_pitch = pitch + 16 // sb
        fill = np.array(-21555 if sb == 2 else -1431655766).astype(dtype)
        d_in = torch.as_tensor(rows, device=dev)
        d_out = torch.as_tensor(np.full(nu * out_pitch + GUARD, fill, dtype=dtype), device=dev)
        d_w = torch.full((nu + GUARD,), -7, dtype=torch.int32, device=dev)
        az.wasted_rows_device(b(d_in), d_out.data_ptr(), out_pitch, d_w.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        want = np.full(nu * out_pitch + GUARD, fill, dtype=dtype)
        for u, (x, w) in enumerate(units):
            want[u * out_pitch:u * out_pitch + len(x)] = WM.shifted(x, w)
        got_w = d_w.cpu().numpy()
        assert np.array_equal(got_w[:nu], want_w), f"pitch {pitch}: wasted {got_w[:nu]} != {want_w}"
        assert (got_w[nu:] == -7).all(), "guard words behind wasted"
        assert np.array_equal(d_out.cpu().numpy(), want), f"pitch {pitch}: out-of-place rows"
        assert np.array_equal(d_in.cpu().numpy(), rows), f"pitch {pitch}: the input rows changed"

        # in place: garbage, guards and the units with w == 0 bit-identical
        d_w.fill_(-7)
        az.wasted_rows_device(b(d_in), d_in.data_ptr(), pitch, d_w.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        want = rows.copy()
        for u, (x, w) in enumerate(units):
            want[u * pitch:u * pitch + len(x)] = WM.shifted(x, w)
        got_w = d_w.cpu().numpy()
        assert np.array_equal(got_w[:nu], want_w) and (got_w[nu:] == -7).all(), f"pitch {pitch}: in place wasted"
        assert np.array_equal(d_in.cpu().numpy(), want), f"pitch {pitch}: in-place rows"


def test_wasted_rows_validation(az):
    """Pitches below the block length or off 16 bytes, misaligned or NULL pointers, a sample width
    the row type cannot hold and an in-place call at another pitch return FLACMI_E_INVALID before
    anything is launched; an empty batch is no error."""
    lib = az.lib

    def call(b, out=0x2000, out_stride=192, wasted=0x3000):
        return lib.flacmi_wasted_rows_device(az.ctx, C.byref(b), out, out_stride, wasted, None)

    ok = lambda **kw: device_batch(**{**dict(samples_ptr=0x1000, sample_bytes=2, sample_bits=16, unit_stride=192,  # noqa: E731
                                             n_units=4, block_len=192), **kw})
    assert call(ok(sample_bytes=3)) == abi.E_INVALID and b"sample_bytes" in lib.flacmi_last_error()
    assert call(ok(sample_bits=17)) == abi.E_INVALID
    assert call(ok(sample_bits=0)) == abi.E_INVALID
    assert call(ok(unit_stride=184)) == abi.E_INVALID
    assert call(ok(unit_stride=196)) == abi.E_INVALID      # 392 bytes: no multiple of 16
    assert call(ok(), out_stride=191) == abi.E_INVALID
    assert call(ok(), out_stride=194) == abi.E_INVALID
    assert call(ok(), out=0x2004) == abi.E_INVALID
    assert call(ok(samples_ptr=0x1008)) == abi.E_INVALID
    assert call(ok(), wasted=0x3002) == abi.E_INVALID
    assert call(ok(), out=0) == abi.E_INVALID
    assert call(ok(), wasted=0) == abi.E_INVALID
    assert call(ok(samples_ptr=0)) == abi.E_INVALID
    assert call(ok(block_len=0)) == abi.E_INVALID
    assert call(ok(block_len=65536, unit_stride=65536), out_stride=65536) == abi.E_INVALID
    assert call(ok(tail_len=193, n_tail_units=1)) == abi.E_INVALID
    assert call(ok(tail_len=0, n_tail_units=1)) == abi.E_INVALID
    assert call(ok(tail_len=100, n_tail_units=5)) == abi.E_INVALID
    assert call(ok(), out=0x1000, out_stride=200) == abi.E_INVALID and b"in place" in lib.flacmi_last_error()
    assert lib.flacmi_wasted_rows_device(None, None, 0, 0, 0, None) == abi.E_INVALID
    assert call(ok(n_units=0)) == 0  # an empty batch is no error
