"""recompress on the device (flac_amd.recompress over flacmi_recompress_host: the stream decoder's
passes, k_units, the encoder's analysis and frame writer) against

  - tests/golden/recompress_streams.json: the reference's decode feeding the reference's encode,
    byte for byte; where either raises, the frames before it and the same exception class;
  - the same cases at several chunk sizes: a frame cut by a chunk, a block assembled over three
    or more calls, a final call with no bytes left: equal bytes;
  - this project's own encode() over the decoded samples, for every opt-in mode alone and the
    four maximal combinations, on a 16-bit stereo stream and on a 24-bit stream of 16-bit audio;
  - decode(recompress(x)) == decode(x);
and the C entry points' state: restart, two contexts, the measured sample_bits, and the decoder
and the encoder called directly before and after a recompress on the same context."""
import io
import json
import os

import numpy as np
import pytest

import mode_matrix_cases as MC
import recompress_model as rm
from flac_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "recompress_streams.json")))["cases"]
SOURCES = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "decode_streams.json")))["cases"]}
EXC = {e.__name__: e for e in (AssertionError, ValueError, ZeroDivisionError, OverflowError, EOFError)}
MODES = ("fixed_only", "fallback", "stereo", "lpc_sign", "wasted", "rice_search", "size_choice")


def parameters(p):
    from flac_amd.encoder import EncoderParameters
    return EncoderParameters(block_size=p["block_size"], rice_partition_order=range(p["rice"][0], p["rice"][1]),
                             lpc_order=range(0, p["lpc_stop"]), qlp_precision=p["qlp"])


def input_of(case) -> bytes:
    return bytes.fromhex(SOURCES[case["source"]]["hex"] if "source" in case else case["hex"])


def drain(gen):
    """(the pieces yielded, the exception class raised after them or None)"""
    pieces, exc = [], None
    try:
        for piece in gen:
            pieces.append(bytes(piece))
    except Exception as e:  # noqa: BLE001
        exc = type(e)
    return pieces, exc


def frames_of(pieces, case=None):
    """the pieces behind the stream header (MAGIC, STREAMINFO's header and body, then kept metadata)"""
    k = 3 + 2 * (case.get("metadata_kept", 0) if case and case["keep_metadata"] else 0)
    return pieces[k:]


@pytest.mark.parametrize("chunk", [64, 257, 4096, 0], ids=["c64", "c257", "c4096", "whole"])
@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_fixture(case, chunk):
    from flac_amd.recompress import recompress
    kw = {"chunk_bytes": chunk} if chunk else {}
    stats = []
    pieces, exc = drain(recompress(input_of(case), parameters(case["parameters"]), keep_metadata=case["keep_metadata"],
                                   stats=stats, **kw))
    want_exc = EXC[case["exception"]] if case["exception"] else None
    assert exc is want_exc, (exc, case["exception"])
    assert len(frames_of(pieces, case)) == case["frames"]
    assert b"".join(pieces).hex() == case["out_hex"]
    if chunk == 64 and case["frames"] > 1 and want_exc is None:
        assert len(stats) > 2  # really in several calls


def test_fixture_covers_the_issue_list():
    names = {c["name"] for c in GOLD}
    for must in ("a_ref_192_to_256", "a_ref_192_to_100", "a_ref_576_to_192", "f_mixed_to_1152", "f_mixed_to_4608",
                 "f_maxbs_unknown_to_576", "g_8bit_to_192", "g_24bit_to_16", "g_32bit_to_192", "h_20bit_to_16",
                 "b_false_sync_to_128", "c_bad_crc8_to_128", "e_cut_5_to_100", "d_err_sync_to_100",
                 "d_err_coding_method_to_192", "i_wide_frame_to_128", "j_meta_3_to_128_keep", "j_meta_7_to_128_keep",
                 "j_meta_17_to_128_keep", "l_3ch_to_100", "l_8ch_to_100", "m_silent_block"):
        assert must in names
    assert {c["exception"] for c in GOLD} >= {None, "AssertionError", "ValueError", "OverflowError", "ZeroDivisionError"}


# ---- the identity against encode() -------------------------------------------------------------

def _pcm16():
    return np.concatenate([MC.pcm("general_a"), MC.pcm("general_c")], axis=1)  # [2][1037], 16-bit stereo


def _stream(pcm, ss, block=192, **modes):
    """a stream of this project's encoder that holds pcm (never fails: fallback + rice_search)"""
    from flac_amd.encoder import EncoderParameters, encode
    p = EncoderParameters(block_size=block, rice_partition_order=range(0, 4), lpc_order=range(0, 9), qlp_precision=8)
    modes = {"fallback": True, "rice_search": True} | modes
    return b"".join(encode(44100, ss, pcm.shape[0], pcm.shape[1], iter(pcm.T.tolist()), p, **modes))


@pytest.fixture(scope="module")
def inputs():
    from flac_amd.decoder import decode
    out = {}
    for name, pcm, ss, modes, spec in (("s16", _pcm16(), 16, {}, False), ("s24", _pcm16() << 8, 24, {}, False),
                                       ("s24_wasted", _pcm16() << 8, 24, {"wasted": True}, True)):
        x = _stream(pcm, ss, **modes)
        (_, _, _, _, it) = decode(x, spec_wasted_bits=spec)
        samples = list(it)
        assert np.array_equal(np.array(samples).T, pcm)  # the premise: decode(x) is pcm
        out[name] = (x, samples, ss, spec)
    return out


def _identity(inputs, which, modes, block=100, chunk=300):
    from flac_amd.encoder import EncoderParameters, encode
    from flac_amd.recompress import recompress
    x, samples, ss, spec = inputs[which]
    p = EncoderParameters(block_size=block, rice_partition_order=range(0, 3), lpc_order=range(0, 9), qlp_precision=8)
    want, want_exc = drain(encode(44100, ss, 2, len(samples), iter(samples), p, **modes))
    for kw in ({}, {"chunk_bytes": chunk}):
        got, exc = drain(recompress(x, p, spec_wasted_bits=spec, **modes, **kw))
        assert exc is want_exc, (exc, want_exc)
        assert len(got) == len(want)
        assert b"".join(got) == b"".join(want)
    return want, want_exc


@pytest.mark.parametrize("which", ["s16", "s24"])
@pytest.mark.parametrize("mode", ["default"] + [m for m in MODES])
def test_identity_each_mode_alone(inputs, which, mode):
    modes = {} if mode == "default" else {mode: True}
    if mode == "size_choice":
        modes["rice_search"] = True  # it is defined over the exact search
    _identity(inputs, which, modes)


@pytest.mark.parametrize("which", ["s16", "s24"])
@pytest.mark.parametrize("k", range(4))
def test_identity_maximal_sets(inputs, which, k):
    modes = {f: v for f, v in MC.MAXIMAL[k].items() if v}
    want, exc = _identity(inputs, which, modes, block=192, chunk=1000)
    assert exc is None and len(want) == 3 + 6  # fallback and rice_search: every block is written


def test_identity_wasted_in_wasted_out(inputs):
    want, exc = _identity(inputs, "s24_wasted", {"wasted": True, "fallback": True, "rice_search": True})
    assert exc is None
    x, samples, _, _ = inputs["s24_wasted"]
    assert len(b"".join(want)) < 0.8 * (len(samples) * 2 * 3)  # the 8 wasted bits are not written


@pytest.mark.parametrize("ss", [16, 24])
def test_full_scale_samples_are_no_range_finding(ss):
    """the two ends of the stream's range, in whole blocks and in the carry: no stop, encode()'s bytes"""
    from flac_amd.encoder import EncoderParameters, encode
    from flac_amd.recompress import recompress
    pcm = (_pcm16() << (ss - 16)).copy()
    hi, lo = (1 << (ss - 1)) - 1, -(1 << (ss - 1))
    pcm[0, 5], pcm[1, 7], pcm[0, 1030], pcm[1, 1036] = hi, lo, hi, lo
    x = _stream(pcm, ss)
    p = EncoderParameters(block_size=100, rice_partition_order=range(0, 3), lpc_order=range(0, 9), qlp_precision=8)
    modes = {"fallback": True, "rice_search": True}
    want = b"".join(encode(44100, ss, 2, pcm.shape[1], iter(pcm.T.tolist()), p, **modes))
    for chunk in (200, 1 << 20):
        stats = []
        assert b"".join(recompress(x, p, chunk_bytes=chunk, stats=stats, **modes)) == want
        assert not any(s["status"] for s in stats) and max(s["sample_bits"] for s in stats) == ss


@pytest.mark.parametrize("which,modes", [("s16", {}), ("s16", {"stereo": True, "fallback": True, "rice_search": True}),
                                         ("s24", {"fallback": True, "rice_search": True, "size_choice": True})])
def test_decode_of_recompress_is_decode(inputs, which, modes):
    from flac_amd.decoder import decode
    from flac_amd.encoder import EncoderParameters
    from flac_amd.recompress import recompress
    x, samples, ss, _ = inputs[which]
    p = EncoderParameters(block_size=256, rice_partition_order=range(0, 3), lpc_order=range(0, 9), qlp_precision=8)
    pieces, exc = drain(recompress(x, p, chunk_bytes=700, **modes))
    if exc is not None:  # the reference's encoder fails on some block: what was written still decodes to a prefix
        assert not modes
    (sr, ss2, ch, n, it) = decode(b"".join(pieces))
    got = list(it)
    assert (sr, ss2, ch, n) == (44100, ss, 2, len(samples))
    assert got == samples[:len(got)] and len(got) == (len(samples) if exc is None else 256 * len(frames_of(pieces)))


def test_python_refusals_before_device_work(inputs):
    from flac_amd.encoder import EncoderParameters
    from flac_amd.recompress import recompress
    x = inputs["s16"][0]
    p = EncoderParameters(block_size=256, rice_partition_order=range(0, 3), lpc_order=range(0, 9), qlp_precision=8)
    for kw in (dict(stereo=True, wasted=True), dict(size_choice=True), dict(lpc_sign=True, fixed_only=True),
               dict(size_choice=True, rice_search=True, wasted=True)):
        stats = []
        with pytest.raises(ValueError):
            list(recompress(x, p, stats=stats, **kw))
        assert stats == []
    mono = bytes.fromhex(SOURCES["b_false_sync"]["hex"])
    with pytest.raises(ValueError):
        list(recompress(mono, p, stereo=True))


# ---- the C entry points ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def _frames_at(x: bytes) -> int:
    from flac_amd.decoder import read_metadata
    b = io.BytesIO(x)
    read_metadata(b)
    return b.tell()


def _chunk(az, data: bytes, final, restart, block, ss=16, channels=2, first_byte=0, az_params=None, **fpkw):
    from flac_amd.analysis import frame_params, make_params
    buf = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, dtype=np.uint8)
    params = az_params or make_params(8, 8, 0, 2)
    fp = frame_params(channels, ss, params.qlp_precision, 0, **fpkw)
    return az.recompress_chunk(buf.ctypes.data, len(data), first_byte, channels, ss, False, 0, final, restart, block,
                               params, fp)


def test_c_calls_carry_restart_and_flush(az, inputs):
    x = inputs["s16"][0]
    body = x[_frames_at(x):]
    res, whole, off, st = _chunk(az, body, True, True, 100)
    assert (res.frames, res.samples, res.consumed, res.status, res.carry) == (6, 1037, len(body), 0, 0)
    assert res.blocks_out == 11 and len(st) == 11 and off[-1] == len(whole) == res.frame_bytes
    # the same in two calls cut inside a frame, then a final call with no bytes left
    cut = len(body) // 2
    r1, b1, _, s1 = _chunk(az, body[:cut], False, True, 100)
    assert 0 < r1.consumed <= cut and r1.carry == r1.samples % 100 and r1.blocks_out == r1.samples // 100
    r2, b2, _, s2 = _chunk(az, body[r1.consumed:], False, False, 100)
    assert r2.consumed == len(body) - r1.consumed and r2.carry == 37
    assert r1.blocks_out + r2.blocks_out == 10
    r3, b3, _, s3 = _chunk(az, b"", True, False, 100)
    assert (r3.frames, r3.consumed, r3.blocks_out, r3.carry) == (0, 0, 1, 0)
    assert b1.tobytes() + b2.tobytes() + b3.tobytes() == whole.tobytes()   # frame numbers run on across the calls
    # a final call with nothing left and no carry writes nothing
    r4, b4, o4, s4 = _chunk(az, b"", True, False, 100)
    assert (r4.blocks_out, r4.frame_bytes, len(b4), list(o4)) == (0, 0, 0, [0])
    # restart discards the carry and the block counter
    r1, b1, _, _ = _chunk(az, body[:cut], False, True, 100)
    assert r1.carry > 0
    res2, again, _, _ = _chunk(az, body, True, True, 100)
    assert again.tobytes() == whole.tobytes() and res2.blocks_out == 11
    # without it the carry opens the next call's first block
    r1, _, _, _ = _chunk(az, body[:cut], False, True, 100)
    res3, other, _, _ = _chunk(az, body, True, False, 100)
    assert res3.blocks_out == (r1.carry + 1037 + 99) // 100 and other.tobytes() != whole.tobytes()


def test_measured_sample_bits(az, inputs):
    from flac_amd.encoder import _sample_bits
    from flac_amd.recompress import recompress
    for which in ("s16", "s24"):
        x, samples, ss, _ = inputs[which]
        body = x[_frames_at(x):]
        res, _, _, _ = _chunk(az, body, True, True, 192, ss=ss)
        a = np.array(samples)
        w = int(np.where(a >= 0, a, ~a).max())
        assert res.sample_bits == rm.sample_bits(w, ss) <= _sample_bits(a)
    stats = []
    list(recompress(inputs["s24"][0], parameters({"block_size": 192, "rice": [0, 3], "lpc_stop": 9, "qlp": 8}),
                    fallback=True, rice_search=True, stats=stats))
    assert [s["sample_bits"] for s in stats] == [res.sample_bits] and stats[0]["final"] and stats[0]["blocks_out"] == 6


def test_range_stop_at_the_c_level(az):
    x = bytes.fromhex(SOURCES["i_wide_frame"]["hex"])
    body = x[_frames_at(x):]
    res, out, off, st = _chunk(az, body, True, True, 128, channels=1)
    assert (res.status, res.site) == (abi.STATUS_OVERFLOW, abi.DSITE["pcm_range"])
    assert (res.frames, res.samples, res.blocks_out, res.carry) == (1, 192, 1, 0)
    assert res.consumed == SOURCES["i_wide_frame"]["offsets"][1] - _frames_at(x)
    # two frames, 384 samples, blocks of 400: the wide frame's samples would only reach the carry, and
    # are range-checked by the call that decoded them all the same
    two = body[:SOURCES["i_wide_frame"]["offsets"][2] - _frames_at(x)]
    res, _, _, _ = _chunk(az, two, False, True, 400, channels=1)
    assert (res.status, res.site, res.blocks_out, res.carry) == (abi.STATUS_OVERFLOW, abi.DSITE["pcm_range"], 0, 0)
    assert (res.frames, res.samples) == (1, 192)
    # without the wide frame the same call keeps its samples
    one = body[:SOURCES["i_wide_frame"]["offsets"][1] - _frames_at(x)]
    res, _, _, _ = _chunk(az, one, False, True, 400, channels=1)
    assert (res.status, res.blocks_out, res.carry, res.frames) == (0, 0, 192, 1)


def test_two_contexts(inputs):
    from flac_amd.analysis import Analyzer
    x = inputs["s16"][0]
    body = x[_frames_at(x):]
    a, b = Analyzer(0), Analyzer(0)
    try:
        whole = _chunk(a, body, True, True, 100)[1].tobytes()
        cut = len(body) // 3
        ra = _chunk(a, body[:cut], False, True, 100)
        rb = _chunk(b, body[:2 * cut], False, True, 100)      # another stream position on the other context
        ra2 = _chunk(a, body[ra[0].consumed:], True, False, 100)
        rb2 = _chunk(b, body[rb[0].consumed:], True, False, 100)
        assert ra[1].tobytes() + ra2[1].tobytes() == whole
        assert rb[1].tobytes() + rb2[1].tobytes() == whole
    finally:
        a.close()
        b.close()


def test_direct_calls_before_and_after_share_no_state(inputs):
    """flacmi_decode_stream_host and flacmi_encode_host give, after a recompress on the same context
    (which grew and reused their buffers and left a carry), the bytes they give on a fresh one"""
    from flac_amd.analysis import Analyzer, make_params, unit_stride
    x, samples, _, _ = inputs["s16"]
    body = np.frombuffer(x[_frames_at(x):], dtype=np.uint8).copy()
    pcm = _pcm16()
    rows = np.zeros((10, unit_stride(192, 2)), dtype=np.int16)
    for b in range(5):
        rows[2 * b:2 * b + 2, :192] = pcm[:, b * 192:(b + 1) * 192]
    params = make_params(8, 8, 0, 2)

    def direct(az):
        out = np.zeros(1037 * 2 * 2 + 64, dtype=np.uint8)
        r = az.decode_stream(body.ctypes.data, len(body), 0, 2, 16, False, 192, True, out.ctypes.data, len(out), False, 2)
        enc = az.encode_frames(rows, params, 192, sample_bits=16, channels=2, sample_size=16, first_frame=3,
                               fallback=True)
        return (r.frames, r.samples, r.pcm_bytes, r.status, out[:r.pcm_bytes].tobytes(), enc[0].tobytes(),
                enc[1].tolist(), enc[2].tolist())

    fresh = Analyzer(0)
    az = Analyzer(0)
    try:
        want = direct(fresh)
        assert want[:4] == (6, 1037, 1037 * 4, 0) and want[4] == pcm.T.astype("<i2").tobytes()
        before = direct(az)
        r1 = _chunk(az, body.tobytes()[:len(body) // 2], False, True, 100, fallback=True)
        assert r1[0].carry > 0
        mid = direct(az)
        r2 = _chunk(az, body.tobytes()[r1[0].consumed:], True, False, 100, fallback=True)
        after = direct(az)
        assert before == want and mid == want and after == want
        # and the recompress itself was not disturbed by the calls in between
        ref = _chunk(fresh, body.tobytes(), True, True, 100, fallback=True)
        assert r1[1].tobytes() + r2[1].tobytes() == ref[1].tobytes()
    finally:
        fresh.close()
        az.close()
