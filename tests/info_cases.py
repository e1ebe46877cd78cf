"""Inputs of the stream-analysis tests (flac_amd.info over k_frame_info), assembled from the
fixtures the decoder tests already use, and the loader of tests/golden/frame_info.json, the
reference's own account of the same inputs (tests/golden/make_info_golden.py).

    single_frames()   every frame of decode.json: (name, bytes, channels, sample_size)
    streams()         name -> whole .flac bytes: the listed decode_streams.json cases, one stream
                      each of the fallback / stereo / lpc-sign fixtures, and `many_frames`
                      (decode.json's valid one-channel 16-bit frames repeated behind a
                      STREAMINFO until there are 130: the reference checks no frame number)

k_frame_info is also held, field by field, to the generated frames of tests/decode_fuzz_cases.py
(tests/test_gpu_decode_fuzz.py; the reference's verdicts on them are tests/golden/decode_fuzz.json,
made by tests/golden/make_decode_fuzz_golden.py); stream_header() below serves that test too.
"""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STREAM_CASES = (["a_ref_192", "b_false_sync", "c_bad_crc8", "e_cut_1", "e_cut_148", "f_mixed", "g_8bit", "g_24bit",
                 "g_32bit", "h_20bit", "i_wide_frame", "j_meta_0", "j_meta_19"])
MANY_FRAMES = 130
TEXT_STREAMS = ("a_ref_192", "f_mixed")  # the two streams of analyze_text.json


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def stream_header(channels, ss, max_bs=0, min_bs=0, samples=0, sr=44100) -> bytes:
    """fLaC and a last-block STREAMINFO (decoder.py:76-87's fields)."""
    v = (min_bs << 16) | max_bs
    v = (v << 48)  # min / max frame size: unknown
    v = (v << 20) | sr
    v = (v << 3) | (channels - 1)
    v = (v << 5) | (ss - 1)
    v = (v << 36) | samples
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + v.to_bytes(18, "big") + bytes(16)


def single_frames():
    return [(c["name"], bytes.fromhex(c["hex"]), c["channels"], c["sample_size"]) for c in _load("decode.json")["cases"]]


def decode_stream_cases():
    """The decode_streams.json cases analysed: the listed ones and every d_err_*."""
    return [c for c in _load("decode_streams.json")["cases"]
            if c["name"] in STREAM_CASES or c["name"].startswith("d_err_")]


def streams():
    out = {c["name"]: bytes.fromhex(c["hex"]) for c in decode_stream_cases()}
    fb = _load("fallback_streams.json")["cases"]["mix_ab"]
    p = fb["params"]
    out["fallback_mix_ab"] = stream_header(p["C"], p["ss"], p["n"], p["n"], p["n"] * p["frames"]) + \
        b"".join(bytes.fromhex(h) for h in fb["frames"])
    st = _load("stereo_streams.json")["cases"]["st16"]
    p = st["params"]
    out["stereo_st16"] = stream_header(2, p["ss"], p["n"], p["n"], p["n"] * p["frames"]) + \
        b"".join(bytes.fromhex(h) for h in st["on"]["frames"])
    ls = _load("lpc_sign_streams.json")["cases"]["stereo16_q6"]
    out["lpc_sign_stereo16_q6"] = bytes.fromhex(ls["header"]) + b"".join(bytes.fromhex(h) for h in ls["frames"])
    mono = [bytes.fromhex(c["hex"]) for c in _load("decode.json")["cases"]
            if c["exception"] is None and c["channels"] == 1 and c["sample_size"] == 16]
    out["many_frames"] = stream_header(1, 16) + b"".join(mono[k % len(mono)] for k in range(MANY_FRAMES))
    return out


def golden():
    """{"frames": {name: record}, "streams": {name: {...}}} (make_info_golden.py)."""
    return _load("frame_info.json")


def golden_text():
    return _load("analyze_text.json")
