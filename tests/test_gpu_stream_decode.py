"""The stream decoder end to end (flac_amd.decoder over flacmi_decode_stream_host) against the
reference's own verdicts (tests/golden/decode_streams.json): the samples decode() yields, the
PCM decode_pcm() delivers, the exception class raised after them and how many samples came
first; the same with chunks so small that frames straddle them; round trips through this
project's encoder for the channel counts the reference decoder cannot read; CRC findings."""
import hashlib
import io

import numpy as np
import pytest

import frame_index_cases as FI
from flac_amd import abi, decoder
from flac_amd.analysis import knob

pytestmark = pytest.mark.gpu
CASES = [c for c in FI.load_cases() if not c["open_exception"]]
EXC = {"AssertionError": AssertionError, "ValueError": ValueError, "EOFError": EOFError,
       "OverflowError": OverflowError}


@pytest.fixture(scope="module", params=["fx", "generic"])
def path(request):
    with knob("FLACMI_DECODE_GENERIC", int(request.param == "generic")):
        yield request.param


def run_decode(data, **kw):
    """(samples as an int64 array [n][channels], exception or None)"""
    sr, ss, ch, n, it = decoder.decode(io.BytesIO(data), **kw)
    got, exc = [], None
    try:
        for s in it:
            got.append(s)
    except Exception as e:  # noqa: BLE001  -- the class is what the fixture records
        exc = e
    return (sr, ss, ch, n), np.array(got, dtype=np.int64).reshape(-1, ch), exc


def run_pcm(data, **kw):
    sr, ss, ch, n, it = decoder.decode_pcm(io.BytesIO(data), **kw)
    got, exc = b"", None
    try:
        for b in it:
            got += b
    except Exception as e:  # noqa: BLE001
        exc = e
    return got, exc


def delivered_frames(case):
    """Frames whose samples the reference yielded (a frame decode_frame raised on was read too)."""
    k = total = 0
    for bs in case["block_sizes"]:
        if total + bs > case["n_samples"]:
            break
        k, total = k + 1, total + bs
    assert total == case["n_samples"]
    return k


def check_samples(case, info, got, exc):
    assert info == (case["sample_rate"], case["sample_size"], case["channels"], case["samples"])
    assert len(got) == case["n_samples"]
    assert hashlib.sha256(got.astype("<i8").tobytes()).hexdigest() == case["samples_sha256"]
    if case["exception"] is None:
        assert exc is None, repr(exc)
    else:
        assert type(exc) is EXC[case["exception"]], repr(exc)
        assert f"frame {delivered_frames(case)}:" in str(exc)
        if "site" in case:
            assert case["site"] in str(exc)


def check_pcm(case, got, exc):
    assert len(got) == case["pcm_bytes"]
    assert hashlib.sha256(got).hexdigest() == case["pcm_sha256"]
    if case["wav_exception"] is None:
        assert exc is None and hashlib.sha256(got).hexdigest() == case["wav_sha256"]
    if case["pcm_exception"] is None:
        assert exc is None, repr(exc)
    else:
        assert type(exc) is EXC[case["pcm_exception"]], repr(exc)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_fixture_streams(path, case):
    data = bytes.fromhex(case["hex"])
    stats = []
    info, got, exc = run_decode(data, stats=stats)
    check_samples(case, info, got, exc)
    assert sum(s["frames"] for s in stats) == delivered_frames(case)
    if "damaged_frame" in case or "false_sync_at_frame" in case:
        assert stats[0]["pass2_frames"] >= 1
    if "damaged_frame" in case:
        assert stats[0]["probes"] >= 1
    if case["name"] == "f_maxbs_small":
        assert stats[0]["probes"] >= 1  # the 1152-sample block exceeds STREAMINFO's 192
    if case["sample_size"] % 8:
        with pytest.raises(AssertionError):
            decoder.decode_pcm(io.BytesIO(data))
    else:
        check_pcm(case, *run_pcm(data))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_fixture_streams_in_small_chunks(case):
    """400-byte chunks (doubled while a chunk holds no whole frame): every stream's frames
    straddle chunk ends, so the tail is carried over at least once."""
    data = bytes.fromhex(case["hex"])
    stats = []
    info, got, exc = run_decode(data, stats=stats, chunk_bytes=400)
    check_samples(case, info, got, exc)
    frames_bytes = len(data) - FI.first_frame_byte(data)
    if frames_bytes > 400:
        assert any(not s["final"] and s["consumed"] < s["bytes"] for s in stats), stats
    if case["sample_size"] % 8 == 0:
        check_pcm(case, *run_pcm(data, chunk_bytes=400))


def test_small_pcm_buffer_is_drained_in_parts_and_grows():
    """A PCM buffer that holds less than the chunk's frames: the call ends at the frame that
    does not fit (pcm_full) and the next call goes on from there; one too small for a single
    frame is replaced by a larger one."""
    case = next(c for c in CASES if c["name"] == "f_mixed")
    data = bytes.fromhex(case["hex"])
    stats = []
    info, got, exc = run_decode(data, stats=stats, pcm_buffer_bytes=40000)  # raw: 8 bytes per stereo sample
    check_samples(case, info, got, exc)
    assert [s["frames"] for s in stats] == [3, 1] and stats[0]["pcm_full"] and not stats[1]["pcm_full"]
    stats = []
    info, got, exc = run_decode(data, stats=stats, pcm_buffer_bytes=1000)   # not even the first 192-sample frame
    check_samples(case, info, got, exc)


@pytest.mark.parametrize("channels,bits,block", [(1, 16, 191), (3, 24, 191), (8, 16, 4608), (1, 16, 4608), (3, 24, 4608)])
def test_round_trip_with_this_encoder(path, channels, bits, block):
    """Mono and 3+ channel streams: the reference decoder cannot read them (encoder.py:95 writes
    L_R whatever the channel count), so the expected output is the source."""
    from flac_amd import encoder as enc
    rng = np.random.default_rng(channels * 100 + bits)
    n = 2 * block + 77
    t = np.arange(n)
    pcm = np.stack([np.round((1 << (bits - 2)) * np.sin(0.01 * (c + 1) * t) + rng.normal(0, 1 << (bits - 8), n))
                    for c in range(channels)]).astype(np.int64)
    p = enc.EncoderParameters(block_size=block, rice_partition_order=range(0, 4), lpc_order=range(0, 9), qlp_precision=10)
    data = b"".join(enc.encode_planar(44100, bits, pcm, p))
    info, got, exc = run_decode(data)
    assert exc is None and info == (44100, bits, channels, n)
    assert np.array_equal(got, pcm.T)
    raw, exc = run_pcm(data, chunk_bytes=3000)
    assert exc is None
    B = bits // 8
    want = pcm.T.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :B].reshape(-1)
    assert raw == want.tobytes()


def test_check_crc_finds_a_flipped_crc16_byte(path):
    case = next(c for c in CASES if c["name"] == "a_ref_192")
    data = bytearray.fromhex(case["hex"])
    k = 2
    data[case["offsets"][k + 1] - 1] ^= 0x40  # the last CRC-16 byte of frame k
    info, got, exc = run_decode(bytes(data))   # the reference reads the CRC unchecked
    check_samples(case, info, got, exc)
    info, got, exc = run_decode(bytes(data), check_crc=True)
    assert type(exc) is decoder.VerifyError and "frame 2" in str(exc) and "crc16" in str(exc)
    assert len(got) == sum(case["block_sizes"][:k])
    info, got, exc = run_decode(bytes.fromhex(case["hex"]), check_crc=True)
    check_samples(case, info, got, exc)
    # a false sync inside a frame must not hide a CRC-16 finding behind the frame-end one
    case = next(c for c in CASES if c["name"] == "b_false_sync")
    data = bytearray.fromhex(case["hex"])
    info, got, exc = run_decode(bytes(data), check_crc=True)
    check_samples(case, info, got, exc)
    data[case["offsets"][2] - 1] ^= 0x01
    info, got, exc = run_decode(bytes(data), check_crc=True)
    assert type(exc) is decoder.VerifyError and "frame 1" in str(exc) and "crc16" in str(exc)
    assert len(got) == case["block_sizes"][0]
