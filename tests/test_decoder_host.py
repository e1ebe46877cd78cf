"""Host side of the stream decoder, no device: metadata parsing (flac_amd.decoder against
tests/golden/decode_streams.json, the reference's own verdicts), the candidate rule's
restatement against the frame offsets the reference read, flacmi_host_chain_walk on
hand-made tables, and argument validation of the new entry points."""
import ctypes as C
import io

import numpy as np
import pytest

import frame_index_cases as FI
from flac_amd import abi, decoder
from flac_amd._lib import load

CASES = FI.load_cases()
BY_NAME = {c["name"]: c for c in CASES}
EXC = {"AssertionError": AssertionError, "ValueError": ValueError, "EOFError": EOFError}


# ---- metadata ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_metadata_matches_reference(case):
    data = bytes.fromhex(case["hex"])
    f = io.BytesIO(data)
    if case["open_exception"]:
        with pytest.raises(EXC[case["open_exception"]]):
            decoder.read_metadata(f)
        return
    si = decoder.read_metadata(f)
    assert (si.sample_rate, si.sample_size, si.channels, si.samples) == \
        (case["sample_rate"], case["sample_size"], case["channels"], case["samples"])
    assert f.tell() == FI.first_frame_byte(data)
    if case["offsets"]:
        assert f.tell() == case["offsets"][0]


def test_metadata_assertion_sites():
    good = bytes.fromhex(BY_NAME["a_ref_192"]["hex"])
    with pytest.raises(AssertionError):
        decoder.read_metadata(io.BytesIO(b"fLaX" + good[4:]))          # the magic
    with pytest.raises(AssertionError):
        decoder.read_metadata(io.BytesIO(good[:4] + b"\x81" + good[5:]))  # first block is no STREAMINFO
    with pytest.raises(ValueError):
        decoder.read_metadata(io.BytesIO(good[:4] + b"\x7f" + good[5:]))  # MetadataBlockType(127)
    with pytest.raises(EOFError):
        decoder.read_metadata(io.BytesIO(good[:20]))
    with pytest.raises(AssertionError):  # decode_pcm: sample_size % 8, before any output
        decoder.decode_pcm(io.BytesIO(bytes.fromhex(BY_NAME["h_20bit"]["hex"])))


# ---- the candidate rule against the reference's frame offsets -------------------------------

@pytest.mark.parametrize("case", [c for c in CASES if not c["open_exception"]], ids=lambda c: c["name"])
def test_reference_frame_offsets_are_candidates(case):
    data = bytes.fromhex(case["hex"])
    first = FI.first_frame_byte(data)
    cand = FI.candidates(data, first)
    offs = [c[0] for c in cand]
    assert offs == sorted(set(offs)) and all(o >= first for o in offs)
    expect = list(case["offsets"])
    if "damaged_frame" in case:
        damaged = expect.pop(case["damaged_frame"])
        assert damaged not in offs
        assert FI.header_at(data, damaged, check_crc8=False) is not None
    assert set(expect) <= set(offs)
    by_off = {c[0]: c for c in cand}
    # block sizes the reference read (a frame whose decode_frame raised was read too)
    for o, bs in zip(case["offsets"], case["block_sizes"]):
        if o in by_off:
            assert by_off[o][2] == bs


def test_false_sync_fixture_has_more_candidates_than_frames():
    case = BY_NAME["b_false_sync"]
    data = bytes.fromhex(case["hex"])
    cand = FI.candidates(data, FI.first_frame_byte(data))
    assert len(cand) > len(case["offsets"])
    k = case["false_sync_at_frame"]
    inside = [c for c in cand if case["offsets"][k] < c[0] < case["offsets"][k + 1]]
    assert len(inside) == 1 and inside[0][2] == 576


# ---- flacmi_host_chain_walk -------------------------------------------------------------

EOF_ST = (abi.DSITE["eof"] << 16) | abi.STATUS_EOF
FRAME_END = (abi.DSITE["frame_end"] << 16) | abi.STATUS_VERIFY
BLOCK_SIZE = (abi.DSITE["block_size"] << 16) | abi.STATUS_VERIFY
PARTS = (abi.DSITE["partitions"] << 16) | abi.STATUS_ASSERTION


def walk(offsets, status, ends, stream_bytes, first=0, final=1, probes=(), capacity=16):
    """Run the walk; probes: {pos: (status, end)} answered when the walk asks.  Returns
    (state, pos, stop_status, chain as (offset, end, candidate, status), probed positions)."""
    lib = load()
    n = len(offsets)
    t = np.zeros(max(n, 1), dtype=abi.CANDIDATE_DTYPE)
    t["offset"][:n] = offsets
    st = np.array(list(status) + [0], dtype=np.int32)
    en = np.array(list(ends) + [0], dtype=np.int64)
    chain = (abi.ChainFrame * capacity)()
    w = abi.Walk()
    w.pos = first
    probes = dict(probes)
    asked = []
    for _ in range(64):
        rc = lib.flacmi_host_chain_walk(t.ctypes.data, n, st.ctypes.data, en.ctypes.data, stream_bytes, final,
                                        C.byref(w), chain, capacity)
        assert rc == 0, lib.flacmi_last_error()
        if w.state != abi.WALK_PROBE:
            break
        asked.append(w.pos)
        w.probe_status, w.probe_end = probes[w.pos]
    got = [(c.offset, c.end, c.candidate, c.status) for c in chain[:w.n_chain]]
    return w.state, w.pos, w.stop_status, got, asked


def test_walk_plain_chain():
    state, pos, _, chain, asked = walk([10, 50, 90], [0, 0, 0], [50, 90, 120], 120, first=10)
    assert (state, pos, asked) == (abi.WALK_DONE, 120, [])
    assert chain == [(10, 50, 0, 0), (50, 90, 1, 0), (90, 120, 2, 0)]


def test_walk_skips_false_candidate():
    # candidate 1 (offset 30) lies inside frame 0, which therefore did not end where proposed
    state, pos, _, chain, asked = walk([10, 30, 50], [FRAME_END, PARTS, 0], [50, -1, 80], 80, first=10)
    assert (state, pos, asked) == (abi.WALK_DONE, 80, [])
    assert chain == [(10, 50, 0, FRAME_END), (50, 80, 2, 0)]


def test_walk_inserts_start():
    # no candidate at 50 (its CRC-8 byte is wrong): probed, joins the chain, never final
    state, pos, _, chain, asked = walk([10, 90], [FRAME_END, 0], [50, 120], 120, first=10, probes={50: (0, 90)})
    assert (state, pos, asked) == (abi.WALK_DONE, 120, [50])
    assert chain == [(10, 50, 0, FRAME_END), (50, 90, -1, FRAME_END), (90, 120, 1, 0)]


def test_walk_probes_oversized_block():
    state, pos, _, chain, asked = walk([10, 50], [0, BLOCK_SIZE], [50, -1], 120, first=10, probes={50: (0, 120)})
    assert (state, asked) == (abi.WALK_DONE, [50])
    assert chain[1] == (50, 120, 1, FRAME_END)


@pytest.mark.parametrize("final", [1, 0])
def test_walk_eof_leaves_pos_at_the_cut_frame(final):
    # the final chunk's caller ends the stream silently there; any other carries [pos, ..) over
    state, pos, stop, chain, _ = walk([10, 50], [0, EOF_ST], [50, -1], 70, first=10, final=final)
    assert (state, pos, stop) == (abi.WALK_DONE, 50, 0)
    assert chain == [(10, 50, 0, 0)]
    state, pos, stop, chain, asked = walk([10], [FRAME_END], [50], 53, first=10, final=final, probes={50: (EOF_ST, -1)})
    assert (state, pos, stop, asked) == (abi.WALK_DONE, 50, 0, [50])


def test_walk_reference_error_stops_at_its_frame():
    state, pos, stop, chain, _ = walk([10, 50, 90], [0, PARTS, 0], [50, -1, 120], 120, first=10)
    assert (state, pos, stop) == (abi.WALK_STOPPED, 50, PARTS)
    assert chain == [(10, 50, 0, 0)]
    state, pos, stop, chain, asked = walk([10], [FRAME_END], [50], 120, first=10, probes={50: (PARTS, -1)})
    assert (state, pos, stop, asked, len(chain)) == (abi.WALK_STOPPED, 50, PARTS, [50], 1)


def test_walk_full_chain_resumes():
    lib = load()
    t = np.zeros(3, dtype=abi.CANDIDATE_DTYPE)
    t["offset"] = [0, 10, 20]
    st, en = np.zeros(3, np.int32), np.array([10, 20, 30], np.int64)
    chain = (abi.ChainFrame * 3)()
    w = abi.Walk()
    assert lib.flacmi_host_chain_walk(t.ctypes.data, 3, st.ctypes.data, en.ctypes.data, 30, 1, C.byref(w), chain, 2) == 0
    assert (w.state, w.n_chain, w.pos) == (abi.WALK_FULL, 2, 20)
    w.state = abi.WALK_RUN
    assert lib.flacmi_host_chain_walk(t.ctypes.data, 3, st.ctypes.data, en.ctypes.data, 30, 1, C.byref(w), chain, 3) == 0
    assert (w.state, w.n_chain, w.pos) == (abi.WALK_DONE, 3, 30)


# ---- argument validation (before any device call) ------------------------------------------

def test_new_entry_points_reject_bad_arguments():
    lib = load()
    E = abi.E_INVALID
    cnt = C.c_int64(0)
    buf = (C.c_uint8 * 64)()
    assert lib.flacmi_index_tile_bytes() > 0 and lib.flacmi_index_tile_bytes() % 16 == 0
    assert lib.flacmi_index_frames_device(None, buf, 64, 0, None, 0, C.byref(cnt), None) == E
    fake = C.c_void_p(1)  # never dereferenced: every check below fails first
    assert lib.flacmi_index_frames_device(fake, buf, -1, 0, None, 0, C.byref(cnt), None) == E
    assert lib.flacmi_index_frames_device(fake, C.addressof(buf) + 1, 8, 0, None, 0, C.byref(cnt), None) == E
    assert b"4-byte aligned" in lib.flacmi_last_error()
    assert lib.flacmi_index_frames_device(fake, buf, 8, 0, None, 4, C.byref(cnt), None) == E
    assert lib.flacmi_pcm_out_device(fake, buf, 1, 0, 2, 0, buf, 64, buf, None) == E      # channels
    assert lib.flacmi_pcm_out_device(fake, buf, 1, 2, 5, 0, buf, 64, buf, None) == E      # bytes_per_sample
    assert lib.flacmi_pcm_out_device(fake, buf, 1, 2, 2, 7, buf, 64, buf, None) == E      # mode
    assert lib.flacmi_pcm_out_device(fake, buf, 1, 2, 2, 0, None, 64, buf, None) == E     # null out
    dp = abi.DecodeParams()
    dp.channels, dp.sample_size = 2, 16
    res = abi.StreamResult()
    assert lib.flacmi_decode_stream_host(fake, buf, 64, 65, C.byref(dp), 0, 1, buf, 64, 0, 2, C.byref(res)) == E
    assert lib.flacmi_decode_stream_host(fake, buf, 64, 0, C.byref(dp), 0, 1, buf, 64, 0, 0, C.byref(res)) == E
    assert lib.flacmi_decode_stream_host(fake, buf, 64, 0, C.byref(dp), 70000, 1, buf, 64, 0, 2, C.byref(res)) == E
    dp.channels = 9
    assert lib.flacmi_decode_stream_host(fake, buf, 64, 0, C.byref(dp), 0, 1, buf, 64, 0, 2, C.byref(res)) == E
    w = abi.Walk()
    w.pos = -1
    assert lib.flacmi_host_chain_walk(None, 0, None, None, 10, 1, C.byref(w), None, 0) == E
    assert lib.flacmi_host_chain_walk(None, 0, None, None, 10, 1, None, None, 0) == E


def test_new_struct_layouts_match_header(tmp_path):
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacmi.h")
    structs = {"flacmi_frame_candidate": abi.FrameCandidate, "flacmi_pcm_frame": abi.PcmFrame,
               "flacmi_chain_frame": abi.ChainFrame, "flacmi_walk": abi.Walk,
               "flacmi_stream_result": abi.StreamResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, f"{cname}.{f}"
    assert abi.CANDIDATE_DTYPE.itemsize == C.sizeof(abi.FrameCandidate)
    assert lib_tile() == 4096


def lib_tile():
    return load().flacmi_index_tile_bytes()
