"""The batch decoder's host logic that needs no device (flac_amd.batch, the argument checks of
flacmi_decode_batch_host, the bindings of the new entries)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import frame_index_cases as FI
from flac_amd import abi, batch
from flac_amd._lib import load

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacmi.h")
ALL = FI.load_cases()
CASES = [c for c in ALL if not c["open_exception"]]


def test_split_stream_strips_exactly_the_metadata():
    for c in CASES:
        data = bytes.fromhex(c["hex"])
        si, region = batch.split_stream(data)
        assert region == data[FI.first_frame_byte(data):], c["name"]
        assert (si.channels, si.sample_size, si.sample_rate, si.samples) == (c["channels"], c["sample_size"],
                                                                           c["sample_rate"], c["samples"])
        if c["offsets"]:
            assert len(data) - len(region) == c["offsets"][0]


def test_open_streams_records_the_reader_exception_and_goes_on(tmp_path):
    bad = next(c for c in ALL if c["name"] == "j_meta_0")
    good = CASES[0]
    p = tmp_path / "good.flac"
    p.write_bytes(bytes.fromhex(good["hex"]))
    infos, regions, errors = batch.open_streams([bytes.fromhex(bad["hex"]), p, b"RIFFnot a flac", b""])
    assert type(errors[0]) is ValueError and infos[0] is None and regions[0] == b""
    assert errors[1] is None and infos[1].channels == good["channels"] and len(regions[1]) > 0
    assert isinstance(errors[2], AssertionError) and isinstance(errors[3], Exception)
    assert batch.group_by_kind(infos) == {None: [0, 2, 3], (good["channels"], good["sample_size"]): [1]}


def test_seg_offsets_are_the_running_sizes():
    seg = batch.seg_offsets([b"abc", b"", b"de", b""])
    assert seg.dtype == np.int64 and seg.tolist() == [0, 3, 3, 5, 5]
    assert batch.seg_offsets([]).tolist() == [0]


def test_split_by_budget():
    assert batch.split_by_budget([], 10) == []
    assert batch.split_by_budget([3, 3, 3, 3], 6) == [(0, 2), (2, 4)]
    assert batch.split_by_budget([3, 3, 3, 3], 100) == [(0, 4)]
    assert batch.split_by_budget([30, 1, 1, 30, 30], 10) == [(0, 1), (1, 3), (3, 4), (4, 5)]  # one above the budget: alone
    assert batch.split_by_budget([0, 0, 5, 5, 1], 5) == [(0, 3), (3, 4), (4, 5)]
    rng = np.random.default_rng(3)
    sizes = rng.integers(0, 50, 200).tolist()
    parts = batch.split_by_budget(sizes, 64)
    assert [lo for lo, _ in parts] == [0] + [hi for _, hi in parts[:-1]] and parts[-1][1] == 200
    for lo, hi in parts:
        assert sum(sizes[lo:hi]) <= 64 or hi - lo == 1
        assert hi == 200 or sum(sizes[lo:hi + 1]) > 64  # greedy: the next one did not fit


def test_disagreeing_streams_raise_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the check")
    monkeypatch.setattr(batch, "_analyzer", no_device)
    mono = next(c for c in CASES if c["channels"] == 1)
    stereo = next(c for c in CASES if c["channels"] == 2 and c["sample_size"] == 16)
    wide = next(c for c in CASES if c["sample_size"] == 24)
    for pair in ((mono, stereo), (stereo, wide)):
        with pytest.raises(ValueError, match="agree"):
            batch.decode_batch([bytes.fromhex(c["hex"]) for c in pair])
    with pytest.raises(ValueError, match="dtype"):
        batch.decode_batch([bytes.fromhex(mono["hex"])], dtype="int8")
    with pytest.raises(ValueError, match="dtype"):
        batch.decode_files([bytes.fromhex(mono["hex"])], dtype="float64")
    assert batch.check_agreement([None, None]) == (1, 16)


def test_decode_files_groups_and_restores_the_input_order(monkeypatch):
    """the device call replaced by one that labels every row with its stream's size"""
    calls = []

    def fake(infos, regions, errors, channels, sample_size, dtype, *rest):
        assert all((si.channels, si.sample_size) == (channels, sample_size) for si in infos)
        calls.append((channels, sample_size, dtype, len(infos)))
        return batch.BatchResult(data=[("row", len(r)) for r in regions], lengths=[len(r) for r in regions],
                                 sample_rates=[si.sample_rate for si in infos], errors=[None] * len(infos),
                                 channels=channels, sample_size=sample_size)
    monkeypatch.setattr(batch, "_decode_opened", fake)
    names = ["a_ref_192", "j_meta_3", "g_24bit", "j_meta_0", "f_mixed", "e_cut_5", "g_8bit", "b_false_sync"]
    cases = [next(c for c in ALL if c["name"] == n) for n in names]
    streams = [bytes.fromhex(c["hex"]) for c in cases]
    res = batch.decode_files(streams)
    assert calls == [(2, 16, "int16", 2), (1, 16, "int16", 3), (2, 24, "int32", 1), (2, 8, "int32", 1)]
    for c, s, r in zip(cases, streams, res):
        if c["open_exception"]:
            assert r.data is None and type(r.error) is ValueError and r.length == 0
            continue
        n = len(batch.split_stream(s)[1])
        assert r.data == ("row", n) and r.length == n and r.error is None
        assert (r.channels, r.sample_size, r.sample_rate) == (c["channels"], c["sample_size"], c["sample_rate"])
    calls.clear()
    batch.decode_files(streams, dtype="float32")
    assert {c[2] for c in calls} == {"float32"}


def test_batch_host_refuses_bad_segment_tables_without_a_device():
    lib = load()
    dp = abi.DecodeParams()
    dp.channels, dp.sample_size, dp.first_frame = 1, 16, -1
    res = (abi.BatchStreamResult * 4)()
    summary = abi.BatchSummary()
    data = np.zeros(64, dtype=np.uint8)

    def call(seg, n=None, d=dp):
        seg = np.asarray(seg, dtype=np.int64)
        rc = lib.flacmi_decode_batch_host(None, data.ctypes.data, seg.ctypes.data, len(seg) - 1 if n is None else n,
                                          ctypes.byref(d), 0, ctypes.cast(res, ctypes.c_void_p), ctypes.byref(summary))
        return rc, lib.flacmi_last_error().decode()
    assert call([0], 0) == (abi.E_INVALID, "n_streams must be at least 1")
    assert call([0, 10, 5, 20])[1].startswith("seg_offsets descend at stream 1")
    assert call([4, 10])[1] == "seg_offsets must start at 0"
    bad = abi.DecodeParams()
    bad.channels, bad.sample_size = 9, 16
    assert "channels" in call([0, 10], d=bad)[1]
    assert call([0, 10, 10, 64]) == (abi.E_INVALID, "null context")  # a good table: only the context is missing
    assert lib.flacmi_decode_batch_fetch(None, None, 0, abi.PLANAR_INT32, 0, None, None) == abi.E_INVALID
    assert lib.flacmi_planar_out_device(None, None, 0, 0, 1, None, 16, abi.PLANAR_INT16, None, 0, None, None) == abi.E_INVALID


def test_new_entries_agree_with_the_header(tmp_path):
    """argument counts of the three prototypes, the enum values and the two result structs' layouts"""
    text = open(HEADER).read()
    for name in ("flacmi_planar_out_device", "flacmi_decode_batch_host", "flacmi_decode_batch_fetch"):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == len(abi.SIGNATURES[name][1]), name
        assert abi.SIGNATURES[name][0] is ctypes.c_int
    enum = re.search(r"enum flacmi_planar_elem \{([^}]*)\}", text).group(1)
    assert [int(v) for v in re.findall(r"= (\d+)", enum)] == [abi.PLANAR_INT16, abi.PLANAR_INT32, abi.PLANAR_FLOAT32]
    assert abi.PLANAR_ELEM == {"int16": 0, "int32": 1, "float32": 2}
    structs = {"flacmi_batch_stream_result": abi.BatchStreamResult, "flacmi_batch_summary": abi.BatchSummary,
               "flacmi_pcm_frame": abi.PcmFrame}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, f"{cname}.{f}"
    assert int(re.search(r"#define FLACMI_ABI_VERSION (\d+)", text).group(1)) == abi.ABI_VERSION == 6
    assert ctypes.sizeof(abi.PcmFrame) == 32  # the layout of flacmi_pcm_frame did not change


def test_cli_parses_decode_many():
    from flac_amd.cli import make_argument_parser
    a = make_argument_parser().parse_args(["decode-many", "--out-dir", "o", "x.flac", "y.flac", "--check-crc"])
    assert a.action == "decode-many" and [p.name for p in a.infiles] == ["x.flac", "y.flac"]
    assert a.check_crc and not a.spec_wasted_bits and str(a.out_dir) == "o"
    with pytest.raises(SystemExit):
        make_argument_parser().parse_args(["decode-many", "x.flac"])  # --out-dir is required
