"""flacmi_stereo_rows_device (k_stereo_rows, csrc/k_stereo.hip) against numpy: mid = (L + R) >> 1
in the input's element type and side = L - R in int32 for every frame's row pair, over block
lengths around the 16-byte groups the kernel loads (4 int32 or 8 int16 samples), with a shorter
last frame, two input pitches, the extremes of each sample width, zero fill from the frame's
length to the output pitch and guard words behind the last mid and side rows."""
import ctypes as C

import numpy as np
import pytest

from flac_amd import abi
from flac_amd.analysis import device_batch

pytestmark = pytest.mark.gpu
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 192, 4609]
WIDTHS = [(np.int16, 16), (np.int32, 24), (np.int32, 31)]
FRAMES = 4          # three full frames and a shorter tail
GUARD = 64          # elements behind the last row of each output


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def _inputs(n, tail, dtype, ss, pitch, seed):
    """rows [2 FRAMES][pitch]: random samples of ss bits with the width's extremes in the first
    positions, and garbage from each frame's length to the pitch (the kernel must not copy it)."""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (ss - 1)), (1 << (ss - 1)) - 1
    rows = rng.integers(lo, hi + 1, size=(2 * FRAMES, pitch), dtype=np.int64)
    extremes = [(hi, lo), (lo, hi), (-1, 0), (0, -1), (hi, hi), (lo, lo)]
    if ss == 31:  # the sums of (hi, hi) and (lo, lo) reach the ends of int32; first, so that n = 1 has them
        extremes = [(hi, lo), (lo, hi), (hi, hi), (lo, lo), (-1, 0), (0, -1)]
    for k, (left, right) in enumerate(extremes):
        f, pos = k % FRAMES, k // FRAMES
        if pos < (tail if f == FRAMES - 1 else n):
            rows[2 * f, pos], rows[2 * f + 1, pos] = left, right
    return rows.astype(dtype)


@pytest.mark.parametrize("dtype,ss", WIDTHS)
@pytest.mark.parametrize("n", LENGTHS)
def test_stereo_rows_match_numpy(az, n, dtype, ss):
    import torch
    dev = torch.device("cuda", 0)
    sb = np.dtype(dtype).itemsize
    tail = (n + 1) // 2
    base = ((n * sb + 15) // 16) * 16 // sb
    for pitch in (base, base + 128 // sb):
        rows = _inputs(n, tail, dtype, ss, pitch, seed=1000 * n + ss + pitch)
        mid_pitch = pitch                      # the input's pitch
        side_pitch = (n + 3) // 4 * 4 + (pitch - base)  # 16-byte rows of int32, the same slack in elements
        tdt = torch.int16 if sb == 2 else torch.int32
        d_rows = torch.as_tensor(rows, device=dev)
        d_mid = torch.full((FRAMES * mid_pitch + GUARD,), -21555, dtype=tdt, device=dev)
        d_side = torch.full((FRAMES * side_pitch + GUARD,), -1431655766, dtype=torch.int32, device=dev)
        b = device_batch(d_rows.data_ptr(), sb, ss, pitch, 2 * FRAMES, n, tail, 2)
        az.stereo_rows_device(b, d_mid.data_ptr(), mid_pitch, d_side.data_ptr(), side_pitch,
                              torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        mid, side = d_mid.cpu().numpy(), d_side.cpu().numpy()
        assert (mid[FRAMES * mid_pitch:] == -21555).all(), "guard words behind the mid rows"
        assert (side[FRAMES * side_pitch:] == -1431655766).all(), "guard words behind the side rows"
        mid, side = mid[: FRAMES * mid_pitch].reshape(FRAMES, mid_pitch), side[: FRAMES * side_pitch].reshape(FRAMES, side_pitch)
        for f in range(FRAMES):
            ln = tail if f == FRAMES - 1 else n
            left, right = rows[2 * f, :ln].astype(np.int64), rows[2 * f + 1, :ln].astype(np.int64)
            assert np.array_equal(mid[f, :ln].astype(np.int64), (left + right) >> 1), f"pitch {pitch} frame {f}: mid"
            assert np.array_equal(side[f, :ln].astype(np.int64), left - right), f"pitch {pitch} frame {f}: side"
            assert not mid[f, ln:].any() and not side[f, ln:].any(), f"pitch {pitch} frame {f}: zero fill"


def test_stereo_rows_extremes_are_present():
    """What the inputs above are for: a side of +-(2^ss - 1), the floor of an odd negative sum, and
    at ss = 31 sums and differences at the ends of int32."""
    rows = _inputs(192, 96, np.int16, 16, 192, 1).astype(np.int64)
    pairs = {(int(rows[2 * f, p]), int(rows[2 * f + 1, p])) for f in range(FRAMES) for p in range(2)}
    assert {(32767, -32768), (-32768, 32767), (-1, 0), (0, -1)} <= pairs
    rows = _inputs(1, 1, np.int32, 31, 4, 1).astype(np.int64)
    hi, lo = (1 << 30) - 1, -(1 << 30)
    assert {(int(rows[2 * f, 0]), int(rows[2 * f + 1, 0])) for f in range(FRAMES)} == {(hi, lo), (lo, hi), (hi, hi), (lo, lo)}


def test_stereo_rows_validation(az):
    """Odd unit counts, one tail unit, pitches below the block length or off 16 bytes and NULL
    pointers return FLACMI_E_INVALID before anything is launched."""
    lib = az.lib

    def call(b, mid=0x1000, mid_stride=192, side=0x2000, side_stride=192):
        return lib.flacmi_stereo_rows_device(az.ctx, C.byref(b), mid, mid_stride, side, side_stride, None)

    assert call(device_batch(0x1000, 2, 16, 192, 3, 192)) == abi.E_INVALID and b"even" in lib.flacmi_last_error()
    assert call(device_batch(0x1000, 2, 16, 192, 4, 192, 100, 1)) == abi.E_INVALID
    assert call(device_batch(0x1000, 2, 16, 192, 4, 192), mid_stride=191) == abi.E_INVALID
    assert call(device_batch(0x1000, 2, 16, 192, 4, 192), side_stride=194) == abi.E_INVALID
    assert call(device_batch(0x1000, 2, 16, 192, 4, 192), side=0x2004) == abi.E_INVALID
    assert call(device_batch(0x1000, 3, 16, 192, 4, 192)) == abi.E_INVALID
    assert call(device_batch(0x1000, 2, 16, 192, 4, 192), mid=0) == abi.E_INVALID
    assert call(device_batch(0x1000, 2, 16, 192, 4, 192), side=0) == abi.E_INVALID
    assert call(device_batch(0, 2, 16, 192, 4, 192)) == abi.E_INVALID
    assert lib.flacmi_stereo_rows_device(None, None, 0, 0, 0, 0, None) == abi.E_INVALID
    assert call(device_batch(0x1000, 2, 16, 192, 0, 192)) == 0  # an empty batch is no error
