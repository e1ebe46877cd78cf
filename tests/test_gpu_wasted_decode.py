"""FLACMI_DECODE_WASTED_SPEC (include/flacmi.h; decode_general of csrc/k_decode.hip, k_info.hip)
on the streams of tests/golden/wasted_streams.json, which the reference's own writers wrote with
the wasted-bits code in the subframe header (tests/golden/make_wasted_golden.py).

spec_wasted_bits=True must give what the reference decoder gives with its two corrections
(get_wasted_bits + 1, samples << wasted): the input samples of every case, with every CRC, frame
number and frame end clean, through the general decoder alone and through the default
k_decode_fx -> list path, frame by frame and as whole streams (index, both passes, chain walk,
PCM); the in-kernel comparison with `expect` sees the shifted samples; analyze reports each
subframe's w and width.  spec_wasted_bits=False must give what the unpatched reference gives for
each frame: its samples, or the class of its exception.
"""
import hashlib

import numpy as np
import pytest

import golden_util as G
import wasted_cases as WC
from flac_amd import abi, decoder, info
from flac_amd.analysis import knob

pytestmark = pytest.mark.gpu
GOLD = G.load("wasted_streams.json")["cases"]
CASES = sorted(n for n in WC.CASES if all(isinstance(f, str) for f in GOLD[n]["frames"]))


@pytest.fixture(scope="module", params=["fx", "generic"])
def az(request):
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    with knob("FLACMI_DECODE_GENERIC", int(request.param == "generic")):
        yield a
    a.close()


@pytest.fixture(scope="module")
def inputs():
    """name -> (rows, n_tail_units, frame bytes list): built once, never modified"""
    out = {}
    for name in CASES:
        rows, n_tail = WC.case_rows(name)
        assert WC.samples_sha256(name) == GOLD[name]["samples_sha256"]
        out[name] = (rows, n_tail, [bytes.fromhex(h) for h in GOLD[name]["frames"]])
    return out


def test_every_case_is_decodable_here():
    assert CASES == sorted(WC.CASES), "a frame above 4 KB is stored as a hash: the decoder tests could not read it"
    ws = {(WC.CASES[n]["ss"], w) for n in CASES for w in GOLD[n]["wasted"]}
    assert {(16, 0), (16, 1), (16, 2), (16, 8), (16, 15), (24, 0), (24, 4), (24, 8), (24, 16), (24, 23), (32, 8)} <= ws
    assert {s["type"] for n in CASES for s in GOLD[n]["subframes"]} == {"CONSTANT", "VERBATIM", "FIXED", "LPC"}


def _decode(az, name, inputs, rows=None, **kw):
    c = WC.CASES[name]
    src, n_tail, frames = inputs[name]
    data = np.frombuffer(b"".join(frames), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    return az.decode_frames(data, offsets, c["C"], c["ss"], first_frame=c["first"], expect=src if rows is None else rows,
                            block_len=c["n"], tail_len=c["tail"], n_tail_units=n_tail, check_crc=True, **kw)


@pytest.mark.parametrize("name", CASES)
def test_spec_reading_returns_the_corrected_references_samples(az, inputs, name):
    rows, _, _ = inputs[name]
    out, st, mm = _decode(az, name, inputs, spec_wasted_bits=True)
    assert not st.any(), f"frames with status: {[(i, hex(int(s))) for i, s in enumerate(st) if s]}"
    assert not mm.any()
    for u, ln in enumerate(WC.unit_lens(name)):
        assert np.array_equal(out[u, :ln], rows[u, :ln].astype(np.int32)), f"unit {u}"


@pytest.mark.parametrize("name", ["mono16", "stereo24", "fb16"])
def test_expect_is_compared_with_the_shifted_samples(az, inputs, name):
    """One low bit of a unit with w > 0 flipped in the source rows: exactly that frame reports one
    mismatching sample (the true source reports none: the test above)."""
    c = WC.CASES[name]
    rows = inputs[name][0].copy()
    u = next(k for k, w in enumerate(GOLD[name]["wasted"]) if w > 0)
    rows[u, 0] ^= 1
    _, st, mm = _decode(az, name, inputs, rows=rows, spec_wasted_bits=True)
    want = np.zeros(c["frames"], dtype=np.int64)
    want[u // c["C"]] = 1
    assert np.array_equal(mm, want)
    assert int(st[u // c["C"]]) == (abi.DSITE["samples"] << 16) | abi.STATUS_VERIFY
    assert not np.delete(st, u // c["C"]).any()


@pytest.mark.parametrize("name", CASES)
def test_default_reading_is_the_unpatched_references(az, inputs, name):
    """Each frame alone, as the fixture's generator read it: the unpatched reference's samples, or
    its exception class."""
    c = WC.CASES[name]
    _, _, frames = inputs[name]
    for f, (frame, want) in enumerate(zip(frames, GOLD[name]["default"])):
        data = np.frombuffer(frame, dtype=np.uint8)
        ln = WC.unit_lens(name)[f * c["C"]]
        out, st, _ = az.decode_frames(data, np.array([0, len(data)], dtype=np.int64), c["C"], c["ss"], first_frame=-1,
                                      block_len=c["n"], check_crc=False)
        st = int(st[0])
        if want["exception"] is not None:
            assert st != 0 and abi.STATUS_EXCEPTION[st & 0xFFFF].__name__ == want["exception"], f"frame {f}: {st:#x}"
            continue
        assert st == 0 or st & 0xFFFF == abi.STATUS_VERIFY, f"frame {f}: {st:#x}"
        dec = out[: c["C"], :ln].astype(np.int64)
        assert [list(r[:8]) for r in dec] == want["head"]
        assert hashlib.sha256(dec.astype("<i8").tobytes()).hexdigest() == want["sha256"]


@pytest.mark.parametrize("name", CASES)
def test_whole_stream_decodes_with_the_flag(az, inputs, name):
    """decode(): the frame index, the first pass with proposed ends, the chain walk, the PCM pass."""
    c = WC.CASES[name]
    rows, _, _ = inputs[name]
    data = WC.stream(name, GOLD[name])
    _, ss, ch, _, it = decoder.decode(data, check_crc=True, spec_wasted_bits=True)
    got = np.array(list(it), dtype=np.int64)
    lens = WC.unit_lens(name)
    want = np.concatenate([rows[f * c["C"]:(f + 1) * c["C"], :lens[f * c["C"]]].T for f in range(c["frames"])])
    assert (ss, ch) == (c["ss"], c["C"]) and np.array_equal(got, want.astype(np.int64))


def _account(subframes):
    return [{"type": s.type_name, "order": s.order, "wasted_bits": s.wasted_bits, "sample_bits": s.sample_bits,
             "bit_offset": s.bit_offset, "bits": s.bits} for s in subframes]


@pytest.mark.parametrize("name", CASES)
def test_analyze_reports_wasted_bits_and_widths(az, inputs, name):
    c = WC.CASES[name]
    rep = info.analyze(WC.stream(name, GOLD[name]), spec_wasted_bits=True)
    frames = list(rep.frames)
    assert len(frames) == c["frames"] and rep.trailing_bytes == 0
    got = [a for fr in frames for a in _account(fr.subframes)]
    assert got == GOLD[name]["subframes"]
    assert [a["wasted_bits"] for a in got] == GOLD[name]["wasted"]
    assert all(fr.crc8_ok and fr.crc16_ok for fr in frames)


@pytest.mark.parametrize("name", CASES)
def test_default_frame_info_is_the_unpatched_references_account(az, inputs, name):
    """k_frame_info on each frame alone, without the flag: the subframes the unpatched reference
    parsed, up to the statement where it raised."""
    c = WC.CASES[name]
    for f, (frame, want) in enumerate(zip(inputs[name][2], GOLD[name]["default"])):
        fi, si, _ = az.frame_info(frame, [0], c["C"], c["ss"])
        st = int(fi["status"][0])
        if want["parse_exception"] is None:
            assert st == 0 and int(fi["end"][0]) == want["end"], f"frame {f}: {st:#x}"
        else:
            assert abi.STATUS_EXCEPTION[st & 0xFFFF].__name__ == want["parse_exception"], f"frame {f}: {st:#x}"
        k = len(want["subframes"])
        assert int(fi["n_subframes"][0]) == k
        got = [{"type": abi.SUB_TYPE_NAMES[int(s["type"])], "order": int(s["order"]), "wasted_bits": int(s["wasted_bits"]),
                "sample_bits": int(s["sample_bits"]), "bit_offset": int(s["bit_offset"]), "bits": int(s["bits"])}
               for s in si[0][:k]]
        assert got == want["subframes"], f"frame {f}"


def test_unknown_decode_flag_bits_are_refused(az):
    """The made-up device addresses are never read: the flag check comes before any launch or copy
    (the stream argument is NULL; nothing is enqueued), as in the stereo rows' validation test."""
    import ctypes as C
    dp = abi.DecodeParams()
    dp.channels, dp.sample_size, dp.first_frame, dp.check_crc, dp.reserved0 = 1, 16, -1, 0, 2
    rc = az.lib.flacmi_decode_frames_device(az.ctx, 0x1000, 16, 0x2000, 1, C.byref(dp), None, None, 0, 0x3000, 0x4000, None)
    assert rc == abi.E_INVALID and b"reserved0" in az.lib.flacmi_last_error()
    rc = az.lib.flacmi_frame_info_device(az.ctx, 0x1000, 16, 0x2000, 1, C.byref(dp), 0x3000, 0x4000, None, 0, None)
    assert rc == abi.E_INVALID
    res, ires = abi.StreamResult(), abi.InfoResult()
    buf = (C.c_uint8 * 64)()
    assert az.lib.flacmi_decode_stream_host(az.ctx, buf, 64, 0, C.byref(dp), 0, 1, buf, 64, abi.PCM_RAW32, 4,
                                            C.byref(res)) == abi.E_INVALID
    assert az.lib.flacmi_info_stream_host(az.ctx, buf, 64, 0, C.byref(dp), 1, buf, buf, None, 0, 1,
                                          C.byref(ires)) == abi.E_INVALID
