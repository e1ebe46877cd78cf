"""The host side of the stream analysis (flac_amd.info, include/flacmi.h "stream analysis")
without a device: the metadata-block listing, summarize() and the text formatter over reports
built from the reference's records (tests/golden/frame_info.json, analyze_text.json), the two
new structs' layouts, and the ABI version."""
import ctypes
import io
import os
import re
import subprocess

import pytest

import info_cases as IC
from flac_amd import abi, info
from flac_amd.common import MetadataBlockType, Streaminfo

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacmi.h")
TYPE_CODE = {name: k for k, name in enumerate(abi.SUB_TYPE_NAMES)}


def report_from_fixture(g):
    """(StreamReport without frames, [FrameReport]) from a stream record of frame_info.json."""
    si = dict(g["streaminfo"])
    si["md5"] = bytes.fromhex(si["md5"])
    frames = []
    for k, f in enumerate(g["frames"]):
        subs = []
        for s in f["subframes"]:
            parts = [("escape", p[1]) if isinstance(p, list) else ("rice", p) for p in s["partitions"]]
            subs.append(info.SubframeReport(
                bit_offset=s["bit_offset"], bits=s["bits"], type=TYPE_CODE[s["type"]], order=s["order"],
                wasted_bits=s["wasted_bits"], sample_bits=s["sample_bits"], precision=s["precision"], shift=s["shift"],
                coefficients=s["coefficients"], coding_method=s["coding_method"], partition_order=s["partition_order"],
                escaped_partitions=sum(isinstance(p, list) for p in s["partitions"]), residual_bits=s["residual_bits"],
                abs_sum=s["abs_sum"], constant_value=s["constant"], partitions_stored=len(parts), partitions=parts))
        frames.append(info.FrameReport(
            index=k, offset=f["offset"], end=f["end"], coded_number=f["number"], status=0, block_size=f["block_size"],
            blocking_strategy=f["blocking_strategy"], sample_rate=f["sample_rate"], sample_size=f["sample_size"],
            channel_code=f["channel_code"], n_subframes=f["n_subframes"], header_bytes=f["header_bytes"],
            crc8_stored=f["crc8"], crc8_computed=f["crc8_computed"], crc16_stored=f["crc16"],
            crc16_computed=f["crc16_computed"], padding_bits=f["padding_bits"], subframes=subs))
    meta = [(MetadataBlockType(t), length, off, bool(last)) for t, length, off, last in g["metadata"]]
    rep = info.StreamReport(streaminfo=Streaminfo(**si), metadata=meta, first_frame_offset=g["first_frame_offset"],
                            frames=iter(()), trailing_bytes=g["trailing_bytes"])
    return rep, frames


def test_abi_version_is_6():
    assert abi.ABI_VERSION == 6
    assert re.search(r"#define FLACMI_ABI_VERSION 6\b", open(HEADER).read())


def test_info_struct_layouts_match_header(tmp_path):
    """sizeof and every offsetof of flacmi_frame_info / flacmi_subframe_info / flacmi_info_result,
    C compiler against ctypes (as test_abi.py does for the other structs), and the numpy views."""
    structs = {"flacmi_frame_info": abi.FrameInfo, "flacmi_subframe_info": abi.SubframeInfo,
               "flacmi_info_result": abi.InfoResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py) and ctypes.sizeof(py) % 8 == 0, cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, f"{cname}.{f}"
    for py, dt in ((abi.FrameInfo, abi.FRAME_INFO_DTYPE), (abi.SubframeInfo, abi.SUBFRAME_INFO_DTYPE)):
        assert dt.itemsize == ctypes.sizeof(py)
        for f, _ in py._fields_:
            assert dt.fields[f][1] == getattr(py, f).offset, f


@pytest.mark.parametrize("name", ["j_meta_19", "a_ref_192", "f_mixed"])
def test_metadata_blocks_are_listed_as_the_reference_reads_them(name):
    g = IC.golden()["streams"][name]
    buf = io.BytesIO(IC.streams()[name])
    si, blocks = info.read_blocks(buf)
    assert [[t.value, length, off, int(last)] for t, length, off, last in blocks] == g["metadata"]
    assert buf.tell() == g["first_frame_offset"]
    want = dict(g["streaminfo"])
    assert {k: (v.hex() if isinstance(v, bytes) else v) for k, v in vars(si).items()} == want
    if name == "j_meta_19":
        assert [b[0] for b in blocks] == [MetadataBlockType.Streaminfo, MetadataBlockType.Padding,
                                          MetadataBlockType.VorbisComment]
        assert info.format_metadata(blocks)[1] == f"metadata=1\ttype=PADDING\tlength=19\toffset={blocks[1][2]}\tlast=0"


def test_metadata_the_reference_cannot_read_raises_the_same():
    """j_meta_0: a zero-length PADDING block; skip_metadata's get.bytes(0) raises ValueError
    (binary.py:38) before any frame is read."""
    g = IC.golden()["streams"]["j_meta_0"]
    assert g["open_exception"] == {"class": "ValueError", "line": "binary.py:38"}
    with pytest.raises(ValueError):
        info.read_blocks(io.BytesIO(IC.streams()["j_meta_0"]))
    with pytest.raises(ValueError):
        info.analyze(IC.streams()["j_meta_0"])
    with pytest.raises(AssertionError):
        info.read_blocks(io.BytesIO(b"fLaX" + IC.streams()["a_ref_192"][4:]))


@pytest.mark.parametrize("name", ["a_ref_192", "f_mixed", "c_bad_crc8", "many_frames", "fallback_mix_ab", "stereo_st16",
                                  "lpc_sign_stereo16_q6", "g_32bit", "e_cut_148"])
def test_summarize_totals_equal_sums_over_the_fixture(name):
    g = IC.golden()["streams"][name]
    rep, frames = report_from_fixture(g)
    s = info.summarize(rep, frames)
    fs = g["frames"]
    subs = [x for f in fs for x in f["subframes"]]
    assert s["frames"] == len(fs) and s["samples"] == sum(f["block_size"] for f in fs)
    assert s["trailing_bytes"] == g["trailing_bytes"]
    for t in abi.SUB_TYPE_NAMES:
        assert s["subframes"][t] == sum(x["type"] == t for x in subs)
    coded = [x for x in subs if x["type"] in ("FIXED", "LPC")]
    assert sum(s["orders"].values()) == len(coded)
    for (t, o), n in s["orders"].items():
        assert n == sum(x["type"] == t and x["order"] == o for x in coded)
    codes = {"LEFT_SIDE": 8, "RIGHT_SIDE": 9, "MID_SIDE": 10}
    for a, n in s["channel_assignments"].items():
        assert n == sum((f["channel_code"] == codes[a]) if a in codes else f["channel_code"] <= 7 for f in fs)
    for o in range(16):
        assert s["partition_orders"].get(o, 0) == sum(x["partition_order"] == o for x in coded)
    assert s["residual_types"] == {"RICE": sum(x["coding_method"] == 4 for x in coded),
                                   "RICE2": sum(x["coding_method"] == 5 for x in coded)}
    assert s["escaped_partitions"] == sum(isinstance(p, list) for x in subs for p in x["partitions"])
    bits = s["bits"]
    assert bits["residual"] == sum(x["residual_bits"] for x in subs)
    assert bits["subframe"] == sum(x["bits"] - x["residual_bits"] for x in subs)
    assert bits["framing"] == sum(8 * f["header_bytes"] + 16 + f["padding_bits"] for f in fs)
    total = sum(f["end"] - f["offset"] for f in fs)
    assert sum(bits.values()) == 8 * total  # every bit of every frame is in exactly one class
    sizes = [f["end"] - f["offset"] for f in fs]
    assert s["frame_bytes"] == {"min": min(sizes), "max": max(sizes), "mean": total / len(fs)}
    si = g["streaminfo"]
    assert s["compression_ratio"] == 8 * total / (si["channels"] * si["sample_size"] * s["samples"])
    assert s["crc_mismatches"] == {"crc8": sum(f["crc8"] != f["crc8_computed"] for f in fs),
                                   "crc16": sum(f["crc16"] != f["crc16_computed"] for f in fs)}
    if name == "c_bad_crc8":  # the flipped CRC-8 byte lies inside the CRC-16's range
        assert s["crc_mismatches"] == {"crc8": 1, "crc16": 1}
    if name == "many_frames":  # decode.json's bad_crc16 frame, once per round of the 13 frames
        assert s["crc_mismatches"]["crc16"] == 10 and s["frames"] == IC.MANY_FRAMES


def test_summarize_lists_disagreements_with_streaminfo():
    g = IC.golden()["streams"]["a_ref_192"]
    rep, frames = report_from_fixture(g)
    assert info.summarize(rep, frames)["streaminfo_disagreements"] == []  # the reference encoder's own header
    si = vars(rep.streaminfo) | {"max_block_size": 100, "min_block_size": 193, "samples": 7,
                                 "max_frame_size": 10, "min_frame_size": 100000}
    rep.streaminfo = Streaminfo(**si)
    d = info.summarize(rep, frames)["streaminfo_disagreements"]
    assert len(d) == 5
    for word in ("max_block_size 100 < largest block 192", "min_block_size 193 > smallest block 192",
                 "max_frame_size 10 <", "min_frame_size 100000 >", "samples 7 != 818"):
        assert any(word in x for x in d), (word, d)


@pytest.mark.parametrize("name", IC.TEXT_STREAMS)
@pytest.mark.parametrize("partitions", [False, True])
def test_text_formatter_prints_the_generators_text(name, partitions):
    """format_metadata / format_frame / format_summary over the fixture's records against the
    text the generator's own formatter made from the reference's dataclasses."""
    rep, frames = report_from_fixture(IC.golden()["streams"][name])
    lines = info.format_metadata(rep.metadata)
    for fr in frames:
        lines += info.format_frame(fr, rep.streaminfo, partitions)
    lines += info.format_summary(info.summarize(rep, frames))
    want = IC.golden_text()["streams"][name]["partitions" if partitions else "plain"]
    assert "".join(ln + "\n" for ln in lines) == want
    if partitions:
        assert "\tpartitions=" in want


def test_fixture_holds_what_the_issue_lists():
    g = IC.golden()
    assert len(g["frames"]) == 36 and set(g["frames"]) == {c[0] for c in IC.single_frames()}
    errs = [c[0] for c in IC.single_frames() if c[0].startswith("err_")]
    assert len(errs) == 15 and {"d_" + n for n in errs} <= set(g["streams"])  # every err_* frame, alone and in a stream
    assert set(IC.STREAM_CASES) <= set(g["streams"])
    assert len(g["streams"]["many_frames"]["frames"]) >= 130
    assert g["frames"]["err_neg_shift"]["exception"] is None and g["frames"]["err_neg_shift"]["subframes"][0]["shift"] < 0
    golden_dir = os.path.join(os.path.dirname(__file__), "golden")
    largest = max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir)
                  if f not in ("frame_info.json", "analyze_text.json"))
    assert os.path.getsize(os.path.join(golden_dir, "frame_info.json")) <= largest
