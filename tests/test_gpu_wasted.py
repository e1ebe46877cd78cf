"""The wasted-bits mode of the device encoder (FLACMI_FRAME_WASTED, include/flacmi.h; k_wasted_rows,
the _wb builds of k_sub_kinds, k_frame_sizes and k_pack in csrc/k_frame.hip) against the bytes the
reference's own writers gave with the wasted code in the subframe header
(tests/golden/wasted_streams.json): every case of tests/wasted_cases.py, byte for byte, through
flacmi_encode_host and flacmi_encode_pipeline (sub-batches of two frames, so sub-batch edges fall
between frames of different w) and encoder.encode / encode_planar; the mode off equal to the
encoder without the argument; the round trip through decode(..., spec_wasted_bits=True); the
compositions with fallback, fixed_only, lpc_sign and devices=[0, 0]; the single shift when the batch
is redone with 8-byte residual rows; and what is refused."""
import ctypes as C

import numpy as np
import pytest

import golden_util as G
import oracle
import wasted_cases as WC
from flac_amd import abi, info
from flac_amd import encoder as enc
from flac_amd.analysis import device_batch, frame_params
from flac_amd.decoder import decode

pytestmark = pytest.mark.gpu
NAMES = sorted(WC.CASES)
GOLD = G.load("wasted_streams.json")["cases"]


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def _params(c):
    return oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"])


def _encoder_parameters(c):
    return enc.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                 lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])


def _pcm(name):
    """planar int64 [channels][samples] of a case"""
    c = WC.CASES[name]
    rows, _ = WC.case_rows(name)
    lens = WC.unit_lens(name)
    return np.stack([np.concatenate([rows[f * c["C"] + ch][: lens[f * c["C"] + ch]] for f in range(c["frames"])])
                     for ch in range(c["C"])]).astype(np.int64)


def _check(name, data, offsets, status, route):
    g = GOLD[name]
    assert not np.asarray(status).any(), f"{name} {route}: status {[hex(int(s)) for s in status]}"
    assert len(offsets) == len(g["frames"]) + 1 and offsets[0] == 0
    for f, want in enumerate(g["frames"]):
        got = bytes(data[int(offsets[f]):int(offsets[f + 1])])
        assert WC.same_frame(got, want), f"{name} {route}: frame {f} ({len(got)} bytes) differs from the fixture"


@pytest.mark.parametrize("name", NAMES)
def test_wasted_frames_match_the_reference_writers(az, name):
    c = WC.CASES[name]
    rows, n_tail = WC.case_rows(name)
    kw = dict(sample_bits=c["ss"], channels=c["C"], sample_size=c["ss"], first_frame=c["first"],
              fallback=c["fallback"], wasted=True)
    before = rows.copy()
    data, offsets, status = az.encode_frames(rows, _params(c), c["n"], c["tail"], n_tail, **kw)
    _check(name, data, offsets, status, "encode_host")
    pdata, poff, pst, timing = az.encode_pipeline(rows, _params(c), c["n"], c["tail"], n_tail,
                                                  units_per_batch=2 * c["C"], **kw)
    _check(name, pdata, poff, pst, "encode_pipeline")
    assert timing["sub_batches"] == (c["frames"] + 1) // 2
    assert np.array_equal(rows, before), "the caller's rows are shifted on the device copy only"
    # the device decoder reads the frames back to the input, in the format's reading of the header
    stream = WC.stream(name, {"frames": [bytes(data[int(offsets[f]):int(offsets[f + 1])]).hex()
                                         for f in range(c["frames"])]})
    _, ss, ch, total, samples = decode(stream, check_crc=True, spec_wasted_bits=True)
    pcm = _pcm(name)
    assert (ss, ch, total) == (c["ss"], c["C"], pcm.shape[1])
    assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, ch).T, pcm)


def test_the_wide_case_needs_8_byte_rows():
    """wide32's premise, from the CPU oracle: analysed as the mode analyses them (x >> w), the chosen
    residuals of its two spike units do not fit 32 bits, so the host entry points in the test above
    went through their redo with 8-byte residual rows; the fixture's bytes say the second analysis
    saw rows shifted once (a second shift would have found w = 0 and written the samples >> 8)."""
    c = WC.CASES["wide32"]
    rows, _ = WC.case_rows("wide32")
    shifted = rows.copy()
    for u, w in enumerate(GOLD["wide32"]["wasted"]):
        shifted[u] >>= w
    ora = oracle.analyze_batch(shifted, _params(c), c["n"], sample_bits=c["ss"], threads=2)
    wide = [int(ora["residual"][u][int(m["res_offset"]):int(m["res_offset"]) + int(m["res_len"])].max()) >> 32
            for u, m in enumerate(ora["meta"])]
    assert [bool(x) for x in wide] == [True, False, False, True]


@pytest.mark.parametrize("name", ["stereo24", "ch8_16", "twin24"])
def test_encode_api_with_and_without_the_mode(name):
    """encoder.encode_planar / encode: wasted=True writes the fixture's frames behind the STREAMINFO of
    the mode off; wasted=False is the encoder called without the argument, and larger."""
    c = WC.CASES[name]
    assert c["first"] == 0 and not c["fallback"]
    pcm = _pcm(name)
    p = _encoder_parameters(c)
    plain = list(enc.encode_planar(44100, c["ss"], pcm, p))
    assert list(enc.encode_planar(44100, c["ss"], pcm, p, wasted=False)) == plain
    on = list(enc.encode_planar(44100, c["ss"], pcm, p, wasted=True))
    assert on[:3] == plain[:3], "STREAMINFO is unchanged"
    for f, want in enumerate(GOLD[name]["frames"]):
        assert WC.same_frame(on[3 + f], want), f"frame {f}"
    assert len(b"".join(on)) < len(b"".join(plain))
    per_sample = (list(int(v) for v in col) for col in pcm.T)
    assert list(enc.encode(44100, c["ss"], c["C"], pcm.shape[1], per_sample, p, wasted=True)) == on
    # several batches on two contexts of one device: the same bytes in block order
    assert list(enc.encode_planar(44100, c["ss"], pcm, p, wasted=True, blocks_per_batch=1, devices=[0, 0])) == on
    _, ss, ch, total, samples = decode(b"".join(on), check_crc=True, spec_wasted_bits=True)
    assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, ch).T, pcm)


@pytest.mark.parametrize("kw", [dict(fixed_only=True), dict(lpc_sign=True), dict(fallback=True),
                                dict(fallback=True, lpc_sign=True)], ids=lambda k: "+".join(sorted(k)))
@pytest.mark.parametrize("name", ["stereo24", "lpc24"])
def test_composition_round_trips_and_declares_the_wasted_bits(name, kw):
    """With fixed_only, lpc_sign and fallback the stream decodes to the input, every subframe
    declares its unit's w at sample_size - w bits, and the bytes equal those of two contexts."""
    c = WC.CASES[name]
    pcm = _pcm(name)
    p = _encoder_parameters(c)
    data = b"".join(enc.encode_planar(44100, c["ss"], pcm, p, wasted=True, **kw))
    assert b"".join(enc.encode_planar(44100, c["ss"], pcm, p, wasted=True, blocks_per_batch=1, devices=[0, 0],
                                      **kw)) == data
    _, ss, ch, total, samples = decode(data, check_crc=True, spec_wasted_bits=True)
    assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, ch).T, pcm)
    subs = [s for fr in info.analyze(data, spec_wasted_bits=True).frames for s in fr.subframes]
    assert [s.wasted_bits for s in subs] == GOLD[name]["wasted"]
    assert [s.sample_bits for s in subs] == [c["ss"] - w for w in GOLD[name]["wasted"]]
    if kw.get("fixed_only"):
        assert {s.type_name for s in subs} == {"FIXED"}
    if kw.get("lpc_sign"):
        assert "LPC" in {s.type_name for s in subs}


def test_stereo_with_wasted_is_refused(az):
    c = WC.CASES["stereo24"]
    pcm = _pcm("stereo24")
    with pytest.raises(ValueError, match="stereo"):
        next(enc.encode_planar(44100, c["ss"], pcm, _encoder_parameters(c), wasted=True, stereo=True))
    with pytest.raises(ValueError, match="stereo"):
        next(enc.encode(44100, c["ss"], 2, pcm.shape[1], iter(()), _encoder_parameters(c), wasted=True, stereo=True))
    lib = az.lib
    rows = np.zeros((2, 192), dtype=np.int16)
    hb = device_batch(rows.ctypes.data, 2, 16, 192, 2, 192)
    p = oracle.make_params(8, 12, 0, 3)
    fp = frame_params(2, 16, 12, wasted=True, stereo=True)
    off, st, out = np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(4096, dtype=np.uint8)
    assert lib.flacmi_encode_host(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), off.ctypes.data,
                                  st.ctypes.data) == abi.E_INVALID and b"stereo" in lib.flacmi_last_error()
    assert lib.flacmi_encode_pipeline(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), 2, out.ctypes.data, out.size,
                                      off.ctypes.data, st.ctypes.data, None) == abi.E_INVALID


def test_device_entry_points_refuse_the_flag_and_unknown_bits(az):
    """The *_device frame entry points have no slot for the wasted array: FLACMI_E_INVALID before
    anything is launched (the addresses are never read); so is every unknown bit, everywhere."""
    lib = az.lib
    b = device_batch(0x1000, 2, 16, 192, 2, 192)
    for flags, text in ((abi.FRAME_WASTED, b"FLACMI_FRAME_WASTED"), (abi.FRAME_WASTED | abi.FRAME_FALLBACK, b"sub_kind"),
                        (8, b"unknown"), (abi.FRAME_WASTED | 16, b"unknown")):
        fp = frame_params(1, 16, 12)
        fp.reserved0 = flags
        assert lib.flacmi_frame_sizes_device(az.ctx, C.byref(b), C.byref(fp), 0x1000, 0x1000, 9, 0x1000, 0x1000,
                                             None) == abi.E_INVALID
        if text != b"sub_kind":
            assert text in lib.flacmi_last_error()
        assert lib.flacmi_pack_frames_device(az.ctx, C.byref(b), C.byref(fp), 0x1000, 0x1000, 9, 0x1000, 4, 192,
                                             0x1000, 0x1000, 0x1000, 64, None) == abi.E_INVALID
    rows = np.zeros((2, 192), dtype=np.int16)
    hb = device_batch(rows.ctypes.data, 2, 16, 192, 2, 192)
    p = oracle.make_params(8, 12, 0, 3)
    off, st, out = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int32), np.zeros(4096, dtype=np.uint8)
    for flags in (8, abi.FRAME_WASTED | 16):
        fp = frame_params(1, 16, 12)
        fp.reserved0 = flags
        assert lib.flacmi_encode_host(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), off.ctypes.data,
                                      st.ctypes.data) == abi.E_INVALID
        assert lib.flacmi_encode_pipeline(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), 2, out.ctypes.data, out.size,
                                          off.ctypes.data, st.ctypes.data, None) == abi.E_INVALID
