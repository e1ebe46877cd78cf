"""The stereo-decorrelation mode on the device (FLACMI_STEREO_BEST, include/flacmi.h;
k_stereo_rows and k_stereo_choose of csrc/k_stereo.hip, the _st builds of k_frame_sizes and the
general k_pack of csrc/k_frame.hip) against the bytes the reference's own writers gave under
Channels.L_R / L_S / S_R / M_S (tests/golden/stereo_streams.json): every case of
tests/stereo_cases.py with fallback off and on, byte for byte, through flacmi_encode_host and
flacmi_encode_pipeline (sub-batches of two frames, so the tail and the failing frame sit at
sub-batch edges); then decoded back to the input by flac_amd.decoder.decode.  With the mode off
the same inputs give the bytes the L_R writer gives (the oracle frame writer)."""
import ctypes as C
import functools
import json
import wave

import numpy as np
import pytest

import frame_writer as FW
import oracle
import stereo_cases as SC
import stereo_model as SM
from flac_amd import abi
from flac_amd.analysis import device_batch, frame_params

pytestmark = pytest.mark.gpu
RUNS = [(name, mode) for name, c in sorted(SC.CASES.items()) for mode in c["modes"]]
_STATUS = {"ZeroDivisionError": abi.STATUS_ZERO_DIVISION, "AssertionError": abi.STATUS_ASSERTION,
           "ValueError": abi.STATUS_VALUE_ERROR, "OverflowError": abi.STATUS_OVERFLOW}


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(SC.GOLDEN))["cases"]


def _params(c):
    return oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"])


@functools.lru_cache(maxsize=None)
def _lr_frames(name):
    """What the L_R writer gives for the case (the oracle's analysis and frame writer): bytes, or
    the exception instance of a frame the reference fails on.  Computed once."""
    c = SC.CASES[name]
    rows, n_tail = SC.case_rows(name)
    out = oracle.analyze_batch(rows, _params(c), c["n"], c["tail"], n_tail, sample_bits=c["ss"], threads=4)
    return FW.frames_from_analysis(rows, out, 2, c["n"], c["tail"], c["ss"], c["q"], first_frame=c["first"])


def _pcm(name, frames=None):
    c = SC.CASES[name]
    rows, _ = SC.case_rows(name)
    nf = c["frames"] if frames is None else frames
    return np.stack([np.concatenate([rows[2 * f + ch][: SC.frame_len(name, f)] for f in range(nf)])
                     for ch in range(2)]).astype(np.int64)


def _check(name, mode, golden, data, offsets, status, route):
    g = golden[name][mode]
    assert len(offsets) == len(g["frames"]) + 1 and offsets[0] == 0
    for f, want in enumerate(g["frames"]):
        got = bytes(data[int(offsets[f]):int(offsets[f + 1])])
        if isinstance(want, dict) and "raises" in want:  # the failing frame: no bytes, the reference's exception
            assert got == b"" and int(status[f]) & 0xFFFF == _STATUS[want["raises"]], \
                f"{name} {mode} {route}: frame {f} status {int(status[f]):#x}"
        else:
            assert int(status[f]) == 0, f"{name} {mode} {route}: frame {f} status {int(status[f]):#x}"
            assert SC.same_frame(got, want), f"{name} {mode} {route}: frame {f} ({len(got)} bytes) differs"
            assert got[3] >> 4 == g["codes"][f]


@pytest.mark.parametrize("name,mode", RUNS)
def test_stereo_frames_match_the_reference_writers(az, golden, name, mode):
    c = SC.CASES[name]
    rows, n_tail = SC.case_rows(name)
    kw = dict(sample_bits=c["ss"], channels=2, sample_size=c["ss"], first_frame=c["first"], fallback=mode == "on",
              stereo=True)
    data, offsets, status = az.encode_frames(rows, _params(c), c["n"], c["tail"], n_tail, **kw)
    _check(name, mode, golden, data, offsets, status, "encode_host")
    pdata, poff, pst, timing = az.encode_pipeline(rows, _params(c), c["n"], c["tail"], n_tail, units_per_batch=4, **kw)
    _check(name, mode, golden, pdata, poff, pst, "encode_pipeline")
    assert timing["sub_batches"] == (c["frames"] + 1) // 2
    assert np.array_equal(poff, offsets) and np.array_equal(pst, status)
    # the device decoder reads the frames before the first failing one back to the input
    from flac_amd.decoder import decode
    ok = next((f for f in range(c["frames"]) if int(status[f]) != 0), c["frames"])
    pcm = _pcm(name, ok)
    header = FW.stream_header(44100, c["ss"], 2, pcm.shape[1], c["n"])
    _, ss, ch, total, samples = decode(header + bytes(data[: int(offsets[ok])]), check_crc=True)
    assert (ss, ch, total) == (c["ss"], 2, pcm.shape[1])
    assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, 2).T, pcm)


@pytest.mark.parametrize("name", sorted(n for n, c in SC.CASES.items() if "off" in c["modes"]))
def test_with_the_mode_off_the_frames_are_the_l_r_frames(az, name):
    """stereo=False, and no keyword at all: the bytes and failures of the L_R writer."""
    c = SC.CASES[name]
    rows, n_tail = SC.case_rows(name)
    want = _lr_frames(name)
    kw = dict(sample_bits=c["ss"], channels=2, sample_size=c["ss"], first_frame=c["first"])
    results = [az.encode_frames(rows, _params(c), c["n"], c["tail"], n_tail, **kw),
               az.encode_frames(rows, _params(c), c["n"], c["tail"], n_tail, stereo=False, **kw),
               az.encode_pipeline(rows, _params(c), c["n"], c["tail"], n_tail, units_per_batch=4, stereo=False, **kw)[:3]]
    for data, offsets, status in results:
        for f, w in enumerate(want):
            got = bytes(data[int(offsets[f]):int(offsets[f + 1])])
            if isinstance(w, Exception):
                assert got == b"" and int(status[f]) & 0xFFFF == _STATUS[type(w).__name__], f"frame {f}"
            else:
                assert int(status[f]) == 0 and got == w and got[3] == 0x10, f"frame {f}"
    # and the stereo mode's failing frame has the same status word
    st = az.encode_frames(rows, _params(c), c["n"], c["tail"], n_tail, stereo=True, **kw)[2]
    for f in range(c["frames"]):
        if int(st[f]) != 0:
            assert int(st[f]) == int(results[0][2][f]), f"frame {f}"


def _encoder_parameters(c):
    from flac_amd import encoder as enc
    return enc.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                 lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])


def test_encode_with_stereo_writes_the_fixture_stream(golden):
    """encoder.encode(stereo=True): STREAMINFO as without the mode, then the fixture's frames; a
    channel count other than two is refused before any device work."""
    from flac_amd import encoder as enc
    name = "st16_tail"
    c, pcm = SC.CASES[name], _pcm(name)
    header = FW.stream_header(44100, c["ss"], 2, pcm.shape[1], c["n"])
    frames = iter([int(a), int(b)] for a, b in zip(*pcm))
    parts = list(enc.encode(44100, c["ss"], 2, pcm.shape[1], frames, _encoder_parameters(c), stereo=True))
    assert b"".join(parts[:3]) == header
    assert len(parts) == 3 + c["frames"]
    for f, want in enumerate(golden[name]["off"]["frames"]):
        assert SC.same_frame(parts[3 + f], want), f"frame {f}"
    plain = list(enc.encode_planar(44100, c["ss"], pcm, _encoder_parameters(c)))
    assert plain[:3] == parts[:3] and sum(map(len, parts)) < sum(map(len, plain))
    for channels in (1, 3):
        with pytest.raises(ValueError, match="2 channels"):
            next(enc.encode_planar(44100, 16, np.zeros((channels, 192), dtype=np.int64), _encoder_parameters(c),
                                   stereo=True))
        with pytest.raises(ValueError, match="2 channels"):
            next(enc.encode(44100, 16, channels, 192, iter([]), _encoder_parameters(c), stereo=True))


def test_cli_stereo_round_trip(golden, tmp_path):
    """`encode --stereo` on a WAV of the st16_tail case: the fixture's frames, decoded back to the input."""
    from flac_amd import cli
    from flac_amd.decoder import decode
    name = "st16_tail"
    c, pcm = SC.CASES[name], _pcm(name)
    wav, out = tmp_path / "in.wav", tmp_path / "out.flac"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(pcm.T).astype("<i2").tobytes())
    args = ["encode", str(wav), str(out), "-b", str(c["n"]), "-l", str(c["L"]), "-q", str(c["q"]), "-r", str(c["rmax"]),
            "--correct-reader"]
    assert cli.main(args + ["--stereo"]) == 0
    data = out.read_bytes()
    want = FW.stream_header(44100, 16, 2, pcm.shape[1], c["n"]) + b"".join(
        bytes.fromhex(f) for f in golden[name]["off"]["frames"])
    assert data == want
    sr, ss, ch, total, samples = decode(data, check_crc=True)
    assert (sr, ss, ch, total) == (44100, 16, 2, pcm.shape[1])
    assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, 2).T, pcm)
    assert cli.main(args) == 0  # without the flag: the L_R stream, larger
    assert len(out.read_bytes()) > len(data)


def test_mode_validation(az):
    """channels != 2, sample_size = 32, an unknown mode, and the mode at the two *_device frame
    entry points: FLACMI_E_INVALID before anything is launched."""
    lib = az.lib
    p = oracle.make_params(8, 12, 0, 3)
    off = np.zeros(4, dtype=np.int64)
    st = np.zeros(3, dtype=np.int32)
    out = np.zeros(4096, dtype=np.uint8)

    def host_calls(fp, rows, bits, units):
        hb = device_batch(rows.ctypes.data, rows.dtype.itemsize, bits, rows.shape[1], units, rows.shape[1])
        yield lib.flacmi_encode_host(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), off.ctypes.data, st.ctypes.data)
        yield lib.flacmi_encode_pipeline(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), units, out.ctypes.data, out.size,
                                         off.ctypes.data, st.ctypes.data, None)

    rows16 = np.zeros((6, 192), dtype=np.int16)
    rows32 = np.zeros((6, 192), dtype=np.int32)
    for channels, ss, mode, rows, text in ((1, 16, 1, rows16, b"channels == 2"), (3, 16, 1, rows16, b"channels == 2"),
                                           (2, 32, 1, rows32, b"sample_size <= 31"), (2, 16, 2, rows16, b"stereo mode"),
                                           (2, 16, -1, rows16, b"stereo mode")):
        fp = frame_params(channels, ss, 12)
        fp.reserved[1] = mode
        for rc in host_calls(fp, rows, ss, 6):
            assert rc == abi.E_INVALID and text in lib.flacmi_last_error(), (channels, ss, mode)
    b = device_batch(0x1000, 2, 16, 192, 2, 192)
    fp = frame_params(2, 16, 12, stereo=True)
    assert fp.reserved[1] == abi.STEREO_BEST and frame_params(2, 16, 12).reserved[1] == abi.STEREO_OFF
    assert lib.flacmi_frame_sizes_device(az.ctx, C.byref(b), C.byref(fp), 0x1000, 0x1000, 9, 0x1000, 0x1000,
                                         None) == abi.E_INVALID
    assert b"stereo mode" in lib.flacmi_last_error()
    assert lib.flacmi_pack_frames_device(az.ctx, C.byref(b), C.byref(fp), 0x1000, 0x1000, 9, 0x1000, 4, 192, 0x1000,
                                         0x1000, 0x1000, 64, None) == abi.E_INVALID
    assert b"stereo mode" in lib.flacmi_last_error()
