"""FLACMI_FLAG_SIZE_CHOICE end to end: the streams of tests/golden/size_choice_streams.json (every
candidate written with the reference's own writers, the first smallest kept) through encode(),
encode_planar() and `encode --size-choice`, back through the device decoder; with the fallback and
stereo modes against their CPU models fed with the model's analysis; two contexts of one device;
and the refusals of the C interface."""
import wave

import numpy as np
import pytest

import golden_util as G
import lpc_sign_model as LS
import oracle
import size_choice_cases as SC
import size_choice_model as SZ
import stereo_model as SM
from flac_amd import abi, info
from flac_amd import encoder as enc
from flac_amd._lib import FlacmiError
from flac_amd.analysis import Analyzer, make_params
from flac_amd.decoder import decode

pytestmark = pytest.mark.gpu
GOLD = G.load("size_choice_streams.json")["cases"]


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def _encoder_parameters(c):
    return enc.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                 lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])


def _options(c):
    return dict(size_choice=True, rice_search=True, lpc_sign=c["sign"], fixed_only=c["fixed_only"],
                fallback=bool(c.get("fallback")))


def _stream(name):
    g = GOLD[name]
    return bytes.fromhex(g["header"]) + b"".join(bytes.fromhex(f) for f in g["frames"])


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_streams_are_the_fixture_streams(name):
    c = SC.CASES[name]
    x = SC.channels(name)
    want = _stream(name)
    assert b"".join(enc.encode_planar(c["rate"], c["ss"], x, _encoder_parameters(c), **_options(c))) == want
    sr, ss, ch, total, dec = decode(want, check_crc=True)
    assert (sr, ss, ch, total) == (c["rate"], c["ss"], c["C"], x.shape[1])
    assert np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, c["C"]).T, x)


def test_encode_cli_and_two_contexts(tmp_path):
    from flac_amd import cli
    name = "st16"
    c = SC.CASES[name]
    x = SC.channels(name)
    ep = _encoder_parameters(c)
    want = _stream(name)
    samples = iter([int(v) for v in x[:, i]] for i in range(x.shape[1]))
    assert b"".join(enc.encode(c["rate"], c["ss"], c["C"], x.shape[1], samples, ep, blocks_per_batch=2, **_options(c))) == want
    assert b"".join(enc.encode_planar(c["rate"], c["ss"], x, ep, devices=[0, 0], blocks_per_batch=1, **_options(c))) == want
    wav, out = tmp_path / "in.wav", tmp_path / "out.flac"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(c["C"])
        w.setsampwidth(2)
        w.setframerate(c["rate"])
        w.writeframes(np.ascontiguousarray(x.T).astype("<i2").tobytes())
    assert cli.main(["encode", str(wav), str(out), "-b", str(c["n"]), "-l", str(c["L"]), "-q", str(c["q"]),
                     "-r", f"{c['rmin']},{c['rmax']}", "--correct-reader", "--rice-search", "--lpc-sign", "--size-choice"]) == 0
    assert out.read_bytes() == want
    with pytest.raises(ValueError, match="size_choice needs rice_search"):
        cli.main(["encode", str(wav), str(out), "--size-choice"])


def test_smaller_than_the_sum_rule():
    """The same stream without the flag is larger: the sum |r| rule takes the top LPC order."""
    c = SC.CASES["mix16"]
    x = SC.channels("mix16")
    opts = _options(c)
    with_flag = b"".join(enc.encode_planar(c["rate"], c["ss"], x, _encoder_parameters(c), **opts))
    opts["size_choice"] = False
    without = b"".join(enc.encode_planar(c["rate"], c["ss"], x, _encoder_parameters(c), **opts))
    assert len(with_flag) < len(without)
    orders = [s.order for fr in info.analyze(without).frames for s in fr.subframes]
    assert orders.count(8) >= 3


@pytest.mark.parametrize("fallback", [False, True])
def test_stereo_candidates_are_sized_at_their_width(az, fallback):
    """The stereo mode's three analyses carry the flag, the side rows at ss + 1: device frames == the
    stereo model over the model's left, right, mid and side candidates."""
    name = "st16"
    c = SC.CASES[name]
    rows, lens = SC.unit_rows(name)
    n, tail, ss, L, q, rmin, rmax = c["n"], c["tail"], c["ss"], c["L"], c["q"], c["rmin"], c["rmax"]
    cands = LS.stereo_analyse(rows, oracle.make_params(L, q, rmin, rmax), n, tail, ss)
    done = {}
    for f in range(len(cands)):
        for k, (samples, out, u, w) in enumerate(cands[f]):
            if id(out) not in done:
                srows = rows if k < 2 else SM.candidate_rows(rows, n, tail)[k - 2]
                nu = len(out["meta"])
                nt = (2 if k < 2 else 1) if tail else 0
                done[id(out)] = SZ.apply(out, srows, [tail if u2 >= nu - nt else n for u2 in range(nu)], L, q, rmin, rmax, w)
            cands[f][k] = (samples, done[id(out)], u, w)
    want, codes = SM.frames(rows, cands, n, tail, q, 0, fallback)[:2]
    assert all(isinstance(f, bytes) for f in want) and set(codes) - {1}
    p = make_params(L, q, rmin, rmax, lpc_sign=True, rice_search=True, size_choice=True)
    data, offsets, status = az.encode_frames(rows, p, n, tail, 2 if tail else 0, sample_bits=ss, channels=2, sample_size=ss,
                                             fallback=fallback, stereo=True)
    assert not status.any() and data.tobytes() == b"".join(want)
    x = SC.channels(name)
    stream = b"".join(enc.encode_planar(c["rate"], ss, x, _encoder_parameters(c), stereo=True, fallback=fallback,
                                        lpc_sign=True, rice_search=True, size_choice=True))
    assert stream == bytes.fromhex(GOLD[name]["header"]) + b"".join(want)
    _, _, ch, _, dec = decode(stream, check_crc=True)
    assert np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, ch).T, x)


def test_written_width_comes_from_the_frame_parameters(az):
    """12-bit data in int32 rows declared as 12 bits, written into a 24-bit stream: flacmi_encode_host
    fills reserved[2] with sample_size, so the frames are the model's at 24 bits, not at 12."""
    import fallback_model as FM
    rows = SC.narrow_units()
    lens = [192] * len(rows)
    base = LS.analyze(rows, oracle.make_params(8, 12, 0, 3), 192, sample_bits=12)
    at24 = SZ.apply(base, rows, lens, 8, 12, 0, 3, 24)
    at12 = SZ.apply(base, rows, lens, 8, 12, 0, 3, 12)
    f24, _ = FM.frames(rows, at24, 1, 192, 0, 24, 12, fallback=False)
    f12, _ = FM.frames(rows, at12, 1, 192, 0, 24, 12, fallback=False)
    assert f24 != f12
    p = make_params(8, 12, 0, 3, lpc_sign=True, rice_search=True, size_choice=True)
    data, offsets, status = az.encode_frames(rows, p, 192, sample_bits=12, channels=1, sample_size=24)
    assert not status.any() and data.tobytes() == b"".join(f24)
    p.reserved[2] = 24  # stated and agreeing: the same
    data2, _, _ = az.encode_frames(rows, p, 192, sample_bits=12, channels=1, sample_size=24)
    assert data2.tobytes() == data.tobytes()


def test_refused_by_the_c_interface(az):
    rows = np.zeros((2, 1024), dtype=np.int16)
    rows[:, ::5] = 7
    p = make_params(8, 12, 0, 3, rice_search=True, size_choice=True)
    with pytest.raises(FlacmiError):  # the written width is per unit with wasted bits: a follow-up
        az.encode_frames(rows, p, 1024, channels=1, wasted=True)
    with pytest.raises(FlacmiError):
        az.encode_pipeline(rows, p, 1024, channels=1, wasted=True)
    p.reserved[2] = 24  # disagrees with the stream's 16
    with pytest.raises(FlacmiError):
        az.encode_frames(rows, p, 1024, channels=1, sample_size=16)
    with pytest.raises(FlacmiError):
        az.encode_pipeline(rows, p, 1024, channels=1, sample_size=16)
    with pytest.raises(FlacmiError):  # without the exact search
        az.encode_frames(rows, make_params(8, 12, 0, 3, size_choice=True), 1024, channels=1)
    # with the flag clear the wasted-bits mode is untouched
    data, _, status = az.encode_frames(rows, make_params(8, 12, 0, 3, rice_search=True), 1024, channels=1, wasted=True,
                                       fallback=True)
    assert not status.any() and len(data)
