"""The device PCM writer (csrc/k_index.hip k_pcm, flacmi_pcm_out_device) alone, against numpy:
planar int32 rows -> interleaved little-endian PCM of 1..4 bytes per sample, or raw int32.

The smallest shapes at which the stores could go wrong are all here: B = 3 and odd channel
counts (a sample straddles output dwords), block sizes 1, 3, 4, 5 (a frame smaller than,
equal to and just over one dword; frames that share a dword with both neighbours), 191 / 192
and 4608 (more than one step of the workgroup), and first output bytes at every offset mod 4."""
import numpy as np
import pytest

from flac_amd import abi

pytestmark = pytest.mark.gpu
BLOCKS = [1, 3, 4, 5, 191, 192, 4608]
STRIDE = 4608


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def expected(rows, blocks, channels, B, raw):
    out = []
    for f, bs in enumerate(blocks):
        fr = rows[f * channels:(f + 1) * channels, :bs].T.astype("<i4")  # [t][c]
        b = fr.reshape(-1).view(np.uint8).reshape(-1, 4)
        out.append(b[:, :4 if raw else B].reshape(-1))
    return np.concatenate(out)


def make_rows(rng, blocks, channels, B):
    lim = 1 << (8 * B - 1)
    rows = rng.integers(-lim, lim, (len(blocks) * channels, STRIDE), dtype=np.int64).astype(np.int32)
    rows[0, 0], rows[-1, 0] = lim - 1, -lim  # the exact ends of the range
    return rows


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_packed(az, B, channels):
    rng = np.random.default_rng(100 * B + channels)
    rows = make_rows(rng, BLOCKS, channels, B)
    unit = channels * B
    for lead in [k * unit for k in range(4)]:  # first bytes at several offsets mod 4 (all of them when unit is odd)
        out, st, total = az.pcm_out(rows, BLOCKS, channels, B, lead_bytes=lead)
        assert not st.any()
        assert np.array_equal(out[lead:total], expected(rows, BLOCKS, channels, B, False))
        assert (out[:lead] == 0xA5).all() and (out[total:] == 0xA5).all()  # nothing outside the frames


def test_first_byte_at_every_offset_mod_4(az):
    rng = np.random.default_rng(5)
    seen = set()
    for B, channels in ((1, 1), (3, 1), (1, 3), (3, 3), (2, 1)):
        rows = make_rows(rng, [5, 3, 1, 4], channels, B)
        for k in range(4):
            lead = k * B * channels
            out, st, total = az.pcm_out(rows, [5, 3, 1, 4], channels, B, lead_bytes=lead)
            assert not st.any()
            assert np.array_equal(out[lead:total], expected(rows, [5, 3, 1, 4], channels, B, False))
            assert (out[:lead] == 0xA5).all() and (out[total:] == 0xA5).all()
            first = lead
            for bs in [5, 3, 1, 4]:
                seen.add((B, first % 4))
                first += bs * B * channels
    assert {m for b, m in seen if b in (1, 3)} == {0, 1, 2, 3}


@pytest.mark.parametrize("B", [1, 2, 3])
def test_overflow_at_the_exact_boundaries(az, B):
    lim = 1 << (8 * B - 1)
    blocks = [5, 192, 3, 4, 191]
    rows = np.zeros((len(blocks) * 2, STRIDE), dtype=np.int32)
    rows[0 * 2 + 1, 4] = lim - 1      # frame 0: the largest value that fits
    rows[1 * 2 + 0, 191] = lim        # frame 1: one past it, in the last sample
    rows[2 * 2 + 1, 0] = -lim         # frame 2: the smallest that fits
    rows[3 * 2 + 1, 3] = -lim - 1     # frame 3: one below it
    rows[4 * 2 + 0, 200] = lim        # frame 4: past its block size, not a sample
    out, st, total = az.pcm_out(rows, blocks, 2, B)
    assert list(st) == [0, abi.STATUS_OVERFLOW, 0, abi.STATUS_OVERFLOW, 0]
    want = expected(rows, blocks, 2, B, False)
    lo = 0
    for f, bs in enumerate(blocks):
        hi = lo + bs * 2 * B
        if st[f] == 0:
            assert np.array_equal(out[lo:hi], want[lo:hi])
        lo = hi


def test_raw_mode(az):
    rng = np.random.default_rng(9)
    for channels in (1, 2, 3, 8):
        rows = rng.integers(-(1 << 31), 1 << 31, (len(BLOCKS) * channels, STRIDE), dtype=np.int64).astype(np.int32)
        out, st, total = az.pcm_out(rows, BLOCKS, channels, 2, raw=True)  # bytes_per_sample ignored
        assert not st.any() and total == sum(BLOCKS) * channels * 4
        assert np.array_equal(out[:total], expected(rows, BLOCKS, channels, 4, True))
        assert (out[total:] == 0xA5).all()


def test_frame_outside_the_buffer_is_refused(az):
    import torch
    rows = torch.zeros((2, 16), dtype=torch.int32, device="cuda")
    t = np.zeros(2, dtype=abi.PCM_FRAME_DTYPE)
    t[0] = (rows.data_ptr(), 16, 0, 8, 0)
    t[1] = (rows.data_ptr() + 64, 16, 8, 16, 0)   # ends at byte 48 of a 40-byte buffer
    tab = torch.from_numpy(t.view(np.uint8)).cuda()
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    from flac_amd._lib import check
    check(az.lib.flacmi_pcm_out_device(az.ctx, tab.data_ptr(), 2, 1, 2, 0, out.data_ptr(), 40, st.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, (17 << 16) | abi.STATUS_FRAME_TOO_LARGE]
    assert (out.cpu().numpy()[16:] == 0xA5).all()
