"""The fallback-subframe mode on the device (FLACMI_FRAME_FALLBACK, include/flacmi.h;
k_sub_kinds, k_frame_sizes and the general k_pack of csrc/k_frame.hip) against the bytes the
reference's own writers gave (tests/golden/fallback_streams.json): every case of
tests/fallback_cases.py, byte for byte, through flacmi_encode_host, flacmi_encode_pipeline
(sub-batches of two frames, so escaped frames sit at sub-batch edges) and the device entry
points with a caller-owned sub_kind array (its contents checked too), under the frame-writer
knob values 0, 1 and 2; then decoded back to the input by flac_amd.decoder.decode."""
import ctypes as C
import json
import os
import wave

import numpy as np
import pytest

import fallback_cases as FC
from fallback_cases import GOLDEN, same_frame
import frame_writer as FW
import oracle
from flac_amd import abi
from flac_amd.analysis import device_batch, frame_params, knob, params_stride_for, unit_stride

pytestmark = pytest.mark.gpu
NAMES = sorted(FC.CASES)


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


def _params(c):
    return oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"])


def _check(name, golden, data, offsets, status, route):
    g = golden[name]
    assert not np.asarray(status).any(), f"{name} {route}: status {[hex(int(s)) for s in status]}"
    assert len(offsets) == len(g["frames"]) + 1 and offsets[0] == 0
    for f, want in enumerate(g["frames"]):
        got = bytes(data[int(offsets[f]):int(offsets[f + 1])])
        assert same_frame(got, want), f"{name} {route}: frame {f} ({len(got)} bytes) differs from the fixture"


def _device_route(az, name, rbytes):
    """flacmi_analyze_device + flacmi_frame_sizes_device + flacmi_pack_frames_device with the
    caller's sub_kind array -> (frame bytes, offsets, status, sub_kind)."""
    import torch
    c = FC.CASES[name]
    rows, n_tail = FC.case_rows(name)
    Cn, n, ss = c["C"], c["n"], c["ss"]
    dev = torch.device("cuda", 0)
    units, frames = rows.shape[0], c["frames"]
    stride = unit_stride(n, rows.dtype.itemsize)
    padded = np.zeros((units, stride), dtype=rows.dtype)
    padded[:, :n] = rows
    s = torch.as_tensor(padded, device=dev)
    params = _params(c)
    pst = params_stride_for(c["rmax"])
    rstride = ((n * rbytes + 15) // 16) * 16 // rbytes
    meta = torch.zeros((units, abi.META_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    rp = torch.zeros((units, pst), dtype=torch.int32, device=dev)
    res = torch.zeros((units, rstride * rbytes // 4), dtype=torch.int32, device=dev)
    off = torch.zeros(frames + 1, dtype=torch.int64, device=dev)
    st = torch.zeros(frames, dtype=torch.int32, device=dev)
    kinds = torch.full((units + 2,), -1, dtype=torch.int32, device=dev)  # two guard words behind
    stream = torch.cuda.current_stream(dev).cuda_stream
    az.analyze_device(s.data_ptr(), rows.dtype.itemsize, ss, stride, units, n, params, meta.data_ptr(), rp.data_ptr(),
                      pst, res.data_ptr(), rstride, rbytes, stream, c["tail"], n_tail)
    b = device_batch(s.data_ptr(), rows.dtype.itemsize, ss, stride, units, n, c["tail"], n_tail)
    fp = frame_params(Cn, ss, c["q"], c["first"], fallback=True, sub_kind_ptr=kinds.data_ptr())
    az.frame_sizes_device(b, fp, meta.data_ptr(), rp.data_ptr(), pst, off.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    offsets = off.cpu().numpy()
    out = torch.zeros(int(offsets[-1]) + 64, dtype=torch.uint8, device=dev)
    az.pack_frames_device(b, fp, meta.data_ptr(), rp.data_ptr(), pst, res.data_ptr(), rbytes, rstride,
                          off.data_ptr(), st.data_ptr(), out.data_ptr(), int(offsets[-1]), stream)
    torch.cuda.synchronize(dev)
    host = out.cpu().numpy()
    assert not host[int(offsets[-1]):].any()  # nothing written behind the last frame
    k = kinds.cpu().numpy()
    assert (k[units:] == -1).all()
    return host[: int(offsets[-1])], offsets, st.cpu().numpy(), k[:units]


def _streaminfo_and_pcm(name):
    c = FC.CASES[name]
    rows, _ = FC.case_rows(name)
    lens = FC.unit_lens(name)
    pcm = np.stack([np.concatenate([rows[f * c["C"] + ch][: lens[f * c["C"] + ch]] for f in range(c["frames"])])
                    for ch in range(c["C"])]).astype(np.int64)
    return FW.stream_header(44100, c["ss"], c["C"], pcm.shape[1], c["n"]), pcm


@pytest.mark.parametrize("gen", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_fallback_frames_match_the_reference_writers(az, golden, name, gen):
    c = FC.CASES[name]
    rows, n_tail = FC.case_rows(name)
    kw = dict(sample_bits=c["ss"], channels=c["C"], sample_size=c["ss"], first_frame=c["first"], fallback=True)
    with knob("FLACMI_PACK_GENERIC", gen):
        data, offsets, status = az.encode_frames(rows, _params(c), c["n"], c["tail"], n_tail, **kw)
        _check(name, golden, data, offsets, status, "encode_host")
        pdata, poff, pst, timing = az.encode_pipeline(rows, _params(c), c["n"], c["tail"], n_tail,
                                                      units_per_batch=2 * c["C"], **kw)
        _check(name, golden, pdata, poff, pst, "encode_pipeline")
        assert timing["sub_batches"] == (c["frames"] + 1) // 2
        rbytes = 4
        if name == "wide_const":
            # on 32-bit rows the wide unit is not escaped: its frame keeps RESIDUAL_WIDE and the
            # caller redoes the batch with 64-bit rows, as flacmi_encode_host has done above
            _, _, st4, k4 = _device_route(az, name, 4)
            assert [int(s) & 0xFFFF for s in st4] == [abi.STATUS_RESIDUAL_WIDE] * 2
            assert list(k4) == golden[name]["kinds"]
            rbytes = 8
        ddata, doff, dst, kinds = _device_route(az, name, rbytes)
        _check(name, golden, ddata, doff, dst, "device entry points")
        assert list(kinds) == golden[name]["kinds"]
    if gen == 0:  # the device decoder reads the stream back to the input
        from flac_amd.decoder import decode
        header, pcm = _streaminfo_and_pcm(name)
        sr, ss, ch, total, samples = decode(header + data.tobytes(), check_crc=True)
        assert (ss, ch, total) == (c["ss"], c["C"], pcm.shape[1])
        assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, ch).T, pcm)


def test_big_verbatim_frames_exceed_the_lds_window(golden):
    """Case 6's 24-bit stereo frames advance k_pack's 16 KB window inside a VERBATIM subframe."""
    assert all(f["len"] > 4 * 4096 for f in golden["white24s"]["frames"])


def test_flag_and_pointer_validation(az):
    """Unknown flag bits, and the fallback bit with a null sub_kind pointer at the device entry
    points, return FLACMI_E_INVALID before anything is launched."""
    lib = az.lib
    b = device_batch(0x1000, 2, 16, 192, 2, 192)
    off = np.zeros(3, dtype=np.int64)
    st = np.zeros(2, dtype=np.int32)
    p = oracle.make_params(8, 12, 0, 3)
    for flags, text in ((abi.FRAME_FALLBACK, b"sub_kind"), (2, b"flag"), (abi.FRAME_FALLBACK | 4, b"flag")):
        fp = frame_params(1, 16, 12)
        fp.reserved0 = flags
        assert lib.flacmi_frame_sizes_device(az.ctx, C.byref(b), C.byref(fp), 0x1000, 0x1000, 9, 0x1000, 0x1000,
                                             None) == abi.E_INVALID
        assert text in lib.flacmi_last_error()
        assert lib.flacmi_pack_frames_device(az.ctx, C.byref(b), C.byref(fp), 0x1000, 0x1000, 9, 0x1000, 4, 192,
                                             0x1000, 0x1000, 0x1000, 64, None) == abi.E_INVALID
        assert text in lib.flacmi_last_error()
    fp = frame_params(1, 16, 12)
    fp.reserved0 = 2
    rows = np.zeros((2, 192), dtype=np.int16)
    hb = device_batch(rows.ctypes.data, 2, 16, 192, 2, 192)
    assert lib.flacmi_encode_host(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), off.ctypes.data,
                                  st.ctypes.data) == abi.E_INVALID
    out = np.zeros(4096, dtype=np.uint8)
    assert lib.flacmi_encode_pipeline(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), 2, out.ctypes.data, out.size,
                                      off.ctypes.data, st.ctypes.data, None) == abi.E_INVALID


def _encoder_parameters(c):
    from flac_amd import encoder as enc
    return enc.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                 lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])


@pytest.mark.parametrize("name,exc,msg", [("silence2", ZeroDivisionError, "float division by zero"),
                                          ("ramp", ValueError, "math domain error"),
                                          ("sparse", ValueError, "negative shift count")])
def test_without_fallback_the_reference_exception_is_raised(name, exc, msg):
    """fallback=False (and no keyword at all) raises what the encoder raised before the mode."""
    from flac_amd import encoder as enc
    c = FC.CASES[name]
    _, pcm = _streaminfo_and_pcm(name)
    for kw in ({}, {"fallback": False}):
        with pytest.raises(exc) as ei:
            b"".join(enc.encode_planar(44100, c["ss"], pcm, _encoder_parameters(c), **kw))
        assert type(ei.value) is exc and str(ei.value) == msg


@pytest.mark.parametrize("name", ["silence2", "ch8", "white24s"])
def test_encode_planar_with_fallback_writes_the_fixture_stream(golden, name):
    """encoder.encode_planar(fallback=True): STREAMINFO as without the mode, then the fixture's frames."""
    from flac_amd import encoder as enc
    c = FC.CASES[name]
    header, pcm = _streaminfo_and_pcm(name)
    it = enc.encode_planar(44100, c["ss"], pcm, _encoder_parameters(c), fallback=True)
    parts = list(it)
    assert b"".join(parts[:3]) == header
    # the stream's frame numbers start at 0: only cases with first = 0 compare with the fixture
    if c["first"] == 0:
        for f, want in enumerate(golden[name]["frames"]):
            assert same_frame(parts[3 + f], want), f"frame {f}"
    from flac_amd.decoder import decode
    _, ss, ch, total, samples = decode(b"".join(parts), check_crc=True)
    assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, ch).T, pcm)


def test_encode_wav_and_cli_with_fallback_round_trip(tmp_path):
    """A small WAV that ends in digital silence: without --fallback the encode stops at the first
    silent frame (ZeroDivisionError), with it the file round-trips through the decoder."""
    from flac_amd import cli
    from flac_amd import encoder as enc
    from flac_amd.decoder import decode
    n = 576
    t = np.arange(5 * n + 100)
    x = np.stack([np.round(9000 * np.sin(t / 7.0)) + t % 5, np.round(4000 * np.sin(t / 3.0)) - t % 3]).astype(np.int16)
    x[:, 3 * n:] = 0  # two silent frames and a silent 100-sample tail
    wav, out = tmp_path / "in.wav", tmp_path / "out.flac"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(x.T).astype("<i2").tobytes())
    args = ["encode", str(wav), str(out), "-b", str(n), "-l", "8", "-q", "12", "-r", "3", "--correct-reader"]
    with pytest.raises(ZeroDivisionError):
        cli.main(args)
    assert cli.main(args + ["--fallback"]) == 0
    data = out.read_bytes()
    p = enc.EncoderParameters(block_size=n, rice_partition_order=range(0, 4), lpc_order=range(0, 9), qlp_precision=12)
    assert b"".join(enc.encode_wav(str(wav), p, quirk=False, fallback=True)) == data
    sr, ss, ch, total, samples = decode(data, check_crc=True)
    assert (sr, ss, ch, total) == (44100, 16, 2, x.shape[1])
    assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, 2).T, x.astype(np.int64))
    assert os.path.getsize(out) < x.size * 2
