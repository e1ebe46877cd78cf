"""The stream analysis on the device (csrc/k_info.hip behind flacmi_frame_info_device and
flacmi_info_stream_host, flac_amd.info, `python -m flac_amd analyze`) against the reference's
own account of the same bytes (tests/golden/frame_info.json, made by make_info_golden.py):
every field of every frame and subframe record, the partition bytes, the status words of the
malformed frames, the stream walk (false syncs, a damaged CRC-8, cut-off frames, chunks, a
small record capacity, a grid-stride loop), the CLI's text, and a stream of this project's own
encoder with every opt-in mode on."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import info_cases as IC
from flac_amd import abi, info
from flac_amd.analysis import knob

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = IC.golden()
SINGLE = IC.single_frames()
DECODE_CASES = {c["name"]: c for c in IC._load("decode.json")["cases"]}
STREAMS = IC.streams()
EXC = {"AssertionError": AssertionError, "ValueError": ValueError, "EOFError": EOFError}
STATUS = {"AssertionError": abi.STATUS_ASSERTION, "ValueError": abi.STATUS_VALUE_ERROR, "EOFError": abi.STATUS_EOF}
TYPE_CODE = {name: k for k, name in enumerate(abi.SUB_TYPE_NAMES)}
SENTINEL = 0xEE


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def part_byte(p):
    return (abi.PART_ESCAPE | p[1]) if isinstance(p, list) else p


def check_subframe(want, rec, parts, part_stride, where):
    """One flacmi_subframe_info record and its part_params row against the fixture's subframe."""
    got = {k: int(rec[k]) for k in ("bit_offset", "bits", "order", "wasted_bits", "sample_bits", "precision", "shift",
                                    "coding_method", "partition_order", "residual_bits", "abs_sum")}
    assert got == {k: want[k] for k in got}, where
    assert int(rec["type"]) == TYPE_CODE[want["type"]], where
    assert int(rec["constant_value"]) == want["constant"], where
    assert rec["coefficients"].tolist() == want["coefficients"] + [0] * (32 - len(want["coefficients"])), where
    assert int(rec["escaped_partitions"]) == sum(isinstance(p, list) for p in want["partitions"]), where
    stored = min(len(want["partitions"]), part_stride)
    assert int(rec["partitions_stored"]) == stored, where
    assert parts[:stored].tolist() == [part_byte(p) for p in want["partitions"][:stored]], where
    assert (parts[stored:] == SENTINEL).all(), where  # nothing written past what the subframe holds or the stride
    assert int(rec["reserved0"]) == 0 and int(rec["reserved1"]) == 0, where


def check_frame(want, fi, subs, parts, base, where, part_stride=64):
    """A flacmi_frame_info record (offsets relative to `base`) against a fixture frame that parsed."""
    got = {k: int(fi[k]) for k in ("block_size", "blocking_strategy", "sample_rate", "sample_size", "channel_code",
                                   "n_subframes", "header_bytes", "padding_bits")}
    assert got == {k: want[k] for k in got}, where
    assert int(fi["status"]) == 0, (where, hex(int(fi["status"])))
    assert (int(fi["offset"]) - base, int(fi["end"]) - base) == (want["offset"], want["end"]), where
    assert int(fi["coded_number"]) == want["number"], where
    assert (int(fi["crc8_stored"]), int(fi["crc8_computed"])) == (want["crc8"], want["crc8_computed"]), where
    assert (int(fi["crc16_stored"]), int(fi["crc16_computed"])) == (want["crc16"], want["crc16_computed"]), where
    for c, s in enumerate(want["subframes"]):
        check_subframe(s, subs[c], parts[c], part_stride, f"{where} subframe {c}")


def check_report(want, fr, where):
    """An info.FrameReport against a fixture frame."""
    assert (fr.offset, fr.end, fr.coded_number, fr.block_size, fr.n_subframes, fr.header_bytes, fr.padding_bits) == \
        (want["offset"], want["end"], want["number"], want["block_size"], want["n_subframes"], want["header_bytes"],
         want["padding_bits"]), where
    assert (fr.blocking_strategy, fr.sample_rate, fr.sample_size, fr.channel_code) == \
        (want["blocking_strategy"], want["sample_rate"], want["sample_size"], want["channel_code"]), where
    assert (fr.crc8_stored, fr.crc8_computed, fr.crc16_stored, fr.crc16_computed) == \
        (want["crc8"], want["crc8_computed"], want["crc16"], want["crc16_computed"]), where
    assert len(fr.subframes) == len(want["subframes"]), where
    for c, (s, w) in enumerate(zip(fr.subframes, want["subframes"])):
        got = {k: getattr(s, k) for k in ("bit_offset", "bits", "order", "wasted_bits", "sample_bits", "precision", "shift",
                                          "coefficients", "coding_method", "partition_order", "residual_bits", "abs_sum")}
        assert got == {k: w[k] for k in got}, (where, c)
        assert s.type_name == w["type"] and s.constant_value == w["constant"], (where, c)
        assert s.partitions == [("escape", p[1]) if isinstance(p, list) else ("rice", p) for p in w["partitions"]], (where, c)
        assert not s.truncated, (where, c)


# ---- single frames -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def single_results(az):
    """{(name, pad): (frame_info, subframe_info row, part_params row, offset)}: the frames of one
    (channels, sample size) in one launch, each frame once at every byte alignment; err_eof,
    which needs the stream's end, alone."""
    out = {}
    groups = {}
    for name, data, ch, ss in SINGLE:
        groups.setdefault((ch, ss), []).append((name, data))
    for (ch, ss), frames in groups.items():
        buf, offs, keys = bytearray(), [], []
        for pad in range(4):
            for name, data in frames:
                if name == "err_eof":
                    continue
                buf += bytes(-len(buf) % 4) + bytes(pad)
                offs.append(len(buf))
                keys.append((name, pad))
                buf += data
        fi, si, pp = az.frame_info(bytes(buf), offs, ch, ss, sentinel=SENTINEL)
        for k, key in enumerate(keys):
            out[key] = (fi[k], si[k], pp[k], offs[k])
    name, data, ch, ss = next(c for c in SINGLE if c[0] == "err_eof")
    for pad in range(4):
        fi, si, pp = az.frame_info(bytes(pad) + data, [pad], ch, ss, sentinel=SENTINEL)
        out[(name, pad)] = (fi[0], si[0], pp[0], pad)
    return out


@pytest.mark.parametrize("name", [c[0] for c in SINGLE if GOLD["frames"][c[0]]["exception"] is None])
def test_single_frame_fields_at_every_alignment(single_results, name):
    """Every field of the frame and its subframes, the frame's first byte at 4k, 4k + 1, 4k + 2
    and 4k + 3: the four alignments of the CRC-16's unaligned head and of the bit window."""
    want = GOLD["frames"][name]
    for pad in range(4):
        fi, si, pp, off = single_results[(name, pad)]
        check_frame(want, fi, si, pp, off, f"{name} pad {pad}")
    if name == "err_neg_shift":  # get_frame does not raise: _decode_prediction would
        assert int(single_results[(name, 0)][1][0]["shift"]) < 0
    if name == "bad_crc16":
        fi = single_results[(name, 0)][0]
        assert int(fi["crc16_stored"]) != int(fi["crc16_computed"]) and int(fi["crc8_stored"]) == int(fi["crc8_computed"])


@pytest.mark.parametrize("name", [c[0] for c in SINGLE if GOLD["frames"][c[0]]["exception"] is not None])
def test_malformed_frames_give_the_decoders_status_word(single_results, name):
    """The status word flacmi_decode_frames_device reports for the same frame (decode.json's
    site and exception class), end -1, and the subframes parsed before the stop."""
    case, want = DECODE_CASES[name], GOLD["frames"][name]
    assert want["exception"]["class"] == case["exception"]
    word = (abi.DSITE[case["site"]] << 16) | STATUS[case["exception"]]
    for pad in range(4):
        fi = single_results[(name, pad)][0]
        assert int(fi["status"]) == word, (pad, hex(int(fi["status"])))
        assert int(fi["end"]) == -1 and int(fi["n_subframes"]) == want["n_subframes"]
        assert int(fi["crc16_stored"]) == 0 and int(fi["crc16_computed"]) == 0


def test_every_err_frame_is_covered():
    errs = [c[0] for c in SINGLE if c[0].startswith("err_")]
    raised = [n for n in errs if GOLD["frames"][n]["exception"] is not None]
    assert len(errs) == 15 and sorted(set(errs) - set(raised)) == ["err_neg_shift"]


@pytest.mark.parametrize("name,channel,order", [("lpc8_p12", 0, 3), ("stereo_L_R_4608", 0, 5), ("fixed0_576", 0, 2)])
def test_partition_capacity(az, name, channel, order):
    """part_stride 1, 2^order - 1 and 2^order: every partition is parsed and counted, the first
    min(2^order, part_stride) parameters are stored, and neither the bytes past the stride (the
    next channel's and the next frame's rows) nor a frame without partitions get a byte."""
    _, data, ch, ss = next(c for c in SINGLE if c[0] == name)
    tail = next(c for c in SINGLE if c[0] == "constant_192")[1] if ch == 1 else data
    want = GOLD["frames"][name]
    assert want["subframes"][channel]["partition_order"] == order
    buf = data + bytes(-len(data) % 4) + tail
    for stride in (1, (1 << order) - 1, 1 << order):
        fi, si, pp = az.frame_info(buf, [0, len(data) + (-len(data) % 4)], ch, ss, part_stride=stride, sentinel=SENTINEL)
        check_frame(want, fi[0], si[0], pp[0], 0, f"{name} stride {stride}", part_stride=stride)
        assert int(si[0][channel]["partitions_stored"]) == stride
        assert int(fi[1]["status"]) == 0
        if ch == 1:
            assert (pp[1] == SENTINEL).all()  # CONSTANT: no partitions


# ---- streams ---------------------------------------------------------------------------------

def run_analyze(data, **kw):
    rep = info.analyze(data, **kw)
    frames, exc = [], None
    try:
        for fr in rep.frames:
            frames.append(fr)
    except Exception as e:  # noqa: BLE001  -- the class is what the fixture records
        exc = e
    return rep, frames, exc


def check_stream(name, rep, frames, exc):
    want = GOLD["streams"][name]
    assert [[t.value, ln, off, int(last)] for t, ln, off, last in rep.metadata] == want["metadata"]
    assert rep.first_frame_offset == want["first_frame_offset"]
    assert len(frames) == len(want["frames"]), name
    for k, (fr, w) in enumerate(zip(frames, want["frames"])):
        assert fr.index == k
        check_report(w, fr, f"{name} frame {k}")
    if want["exception"] is None:
        assert exc is None, repr(exc)
    else:
        assert type(exc) is EXC[want["exception"]["class"]], repr(exc)
        assert f"frame {want['exception']['frame']}:" in str(exc)
        assert rep.exception is exc
    assert rep.trailing_bytes == want["trailing_bytes"], name


@pytest.mark.parametrize("name", sorted(n for n in STREAMS if GOLD["streams"][n]["open_exception"] is None))
def test_fixture_streams(name):
    rep, frames, exc = run_analyze(STREAMS[name])
    check_stream(name, rep, frames, exc)
    if name == "b_false_sync":  # the header spelled inside VERBATIM samples is a candidate, not a frame
        assert rep.stats[0]["candidates"] > len(frames) == 3
    if name == "c_bad_crc8":
        assert rep.stats[0]["probes"] > 0 and not frames[1].crc8_ok and frames[0].crc8_ok
        assert "\tcrc8=BAD\t" in info.format_frame(frames[1], rep.streaminfo)[0]
    if name.startswith("e_cut_"):
        assert rep.trailing_bytes == int(name[6:]) and exc is None
    if name.startswith("d_err_") and GOLD["streams"][name]["exception"]:
        site = DECODE_CASES[name[2:]]["site"]
        assert site in str(exc)


@pytest.mark.parametrize("name", sorted(n for n in STREAMS if GOLD["streams"][n]["open_exception"] is None
                                        and n != "many_frames"))
def test_fixture_streams_in_small_chunks(name):
    """400-byte chunks (doubled while a chunk holds no whole frame): frames straddle chunk ends."""
    rep, frames, exc = run_analyze(STREAMS[name], chunk_bytes=400)
    check_stream(name, rep, frames, exc)
    if len(STREAMS[name]) - rep.first_frame_offset > 400:
        assert any(not s["final"] and s["consumed"] < s["bytes"] for s in rep.stats), rep.stats


def test_stream_with_unreadable_metadata_raises_on_open():
    assert GOLD["streams"]["j_meta_0"]["open_exception"]["class"] == "ValueError"
    with pytest.raises(ValueError):
        info.analyze(STREAMS["j_meta_0"])


@pytest.mark.parametrize("case", [c for c in IC.decode_stream_cases() if not c["open_exception"]], ids=lambda c: c["name"])
def test_frames_are_where_the_stream_decoder_finds_them(case):
    """The offsets and block sizes the stream-decode tests use (decode_streams.json: the frames
    the reference's get_frame read; j_meta_0, which it cannot open, is the test above)."""
    rep, frames, exc = run_analyze(bytes.fromhex(case["hex"]))
    assert [fr.offset for fr in frames] == case["offsets"]
    assert [fr.block_size for fr in frames] == case["block_sizes"]


@pytest.mark.parametrize("mode", ["whole", "chunks", "capacity7", "grid1"])
def test_many_frames(mode):
    """130 frames: a second wave of lanes; chunks that cut frames; a record capacity of 7 (the call
    reports `full` and is repeated from `consumed`); a grid of one workgroup (three strides)."""
    data = STREAMS["many_frames"]
    kw = {"chunks": {"chunk_bytes": 5000}, "capacity7": {"frame_capacity": 7}}.get(mode, {})
    with knob("FLACMI_INFO_GRID", 1 if mode == "grid1" else 0):
        rep, frames, exc = run_analyze(data, **kw)
    check_stream("many_frames", rep, frames, exc)
    assert rep.stats[0]["candidates"] > 64 if mode != "chunks" else len(rep.stats) > 10
    if mode == "capacity7":
        assert [s["frames"] for s in rep.stats[:-1]] == [7] * (IC.MANY_FRAMES // 7) and all(s["full"] for s in rep.stats[:-1])
        assert not rep.stats[-1]["full"]
    else:
        assert not any(s["full"] for s in rep.stats)
    s = info.summarize(rep, frames)
    assert s["frames"] == IC.MANY_FRAMES and s["crc_mismatches"] == {"crc8": 0, "crc16": 10}


# ---- command line ------------------------------------------------------------------------------

def run_cli(tmp_path, name, *flags):
    src = tmp_path / f"{name}.flac"
    src.write_bytes(STREAMS[name])
    r = subprocess.run([sys.executable, "-m", "flac_amd", "analyze", str(src), *flags], cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_prints_the_expected_text(tmp_path):
    texts = IC.golden_text()["streams"]
    assert run_cli(tmp_path, "a_ref_192") == texts["a_ref_192"]["plain"]
    assert run_cli(tmp_path, "f_mixed", "--partitions") == texts["f_mixed"]["partitions"]


def test_cli_json_lines_agree_with_the_report(tmp_path):
    out = run_cli(tmp_path, "f_mixed", "--json")
    objs = [json.loads(ln) for ln in out.splitlines()]
    rep, frames, exc = run_analyze(STREAMS["f_mixed"])
    assert exc is None
    assert objs[0]["first_frame_offset"] == rep.first_frame_offset
    assert objs[0]["streaminfo"]["channels"] == rep.streaminfo.channels
    meta = [o for o in objs if "metadata" in o]
    assert [(m["type"], m["length"], m["offset"]) for m in meta] == [(t.name.upper(), ln, off) for t, ln, off, _ in rep.metadata]
    got = [o["frame"] for o in objs if "frame" in o]
    assert got == [json.loads(json.dumps(info.frame_json(fr))) for fr in frames]
    assert got[1]["channel_assignment"] == "RIGHT_SIDE" and got[1]["subframes"][0]["type"] == "FIXED"
    assert objs[-1]["summary"] == json.loads(json.dumps(info.summary_json(info.summarize(rep, frames))))


# ---- this project's encoder, every opt-in mode on -------------------------------------------

def test_own_encoder_with_fallback_stereo_and_lpc_sign():
    """Two channels, blocks of 192: digital silence (CONSTANT), full-scale white noise
    (VERBATIM), and tones near a quarter of the sample rate that the fixed predictors cannot
    follow (LPC), the right channel close to the left (a side channel pays)."""
    from flac_amd import encoder as enc
    rng = np.random.default_rng(20261020)
    n = 192
    t = np.arange(4 * n)
    tone = np.round(9000 * np.sin(2 * np.pi * 0.23 * t) + 6000 * np.sin(2 * np.pi * 0.31 * t + 1.0)).astype(np.int64)
    left = np.concatenate([np.zeros(n, np.int64), rng.integers(-32768, 32768, n), tone])
    right = np.concatenate([np.zeros(n, np.int64), rng.integers(-32768, 32768, n), tone + rng.integers(-3, 4, 4 * n)])
    pcm = np.stack([left, right])
    p = enc.EncoderParameters(block_size=n, rice_partition_order=range(0, 3), lpc_order=range(0, 9), qlp_precision=12)
    data = b"".join(enc.encode_planar(44100, 16, pcm, p, fallback=True, stereo=True, lpc_sign=True))
    rep, frames, exc = run_analyze(io.BytesIO(data))
    assert exc is None and len(frames) == 6 and rep.trailing_bytes == 0
    s = info.summarize(rep, frames)
    assert s["samples"] == 6 * n and s["crc_mismatches"] == {"crc8": 0, "crc16": 0}
    assert s["subframes"]["CONSTANT"] + s["subframes"]["VERBATIM"] >= 1
    assert s["subframes"]["LPC"] >= 1
    assert s["frames"] - s["channel_assignments"]["INDEPENDENT"] >= 1
    assert s["streaminfo_disagreements"] == []
    for fr in frames:
        assert sum(x.bits for x in fr.subframes) == 8 * fr.bytes - 8 * fr.header_bytes - 16 - fr.padding_bits
        assert [x.bit_offset for x in fr.subframes] == [8 * fr.header_bytes, 8 * fr.header_bytes + fr.subframes[0].bits]
