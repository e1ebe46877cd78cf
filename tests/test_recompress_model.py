"""CPU checks of the recompress path (no device):
(a) the numpy restatement of k_units (tests/recompress_model.py: placement, zero fill, range
    status, measured width) against the per-sample loop, over the shapes the GPU test runs;
(b) the stream header, with and without keep_metadata;
(c) the refusals that need no device;
(d) the row width does not change the bytes: the invariant the int32 unit rows of a 24-bit stream
    rest on."""
import ctypes
import os
import sys
from io import BytesIO

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recompress_model as rm  # noqa: E402

CASES = rm.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_units_model_equals_the_per_sample_loop(name):
    case = CASES[name]
    args = rm.model_args(case)
    units, status, width, mask = rm.units_out(*args, firsts=case.get("firsts"))
    lu, ls, lw = rm.units_out_loop(*args, firsts=case.get("firsts"))
    assert units.dtype == lu.dtype and units.shape == lu.shape
    assert np.array_equal(units, lu)
    assert np.array_equal(status, ls)
    assert width == lw
    if "bad_frames" in case:
        assert tuple(np.nonzero(status)[0]) == tuple(case["bad_frames"]), name
        assert mask.all() == (not case["bad_frames"])
    else:
        assert not status.any() and mask.all()
    # zero fill: from each unit's length to the pitch
    C, B = case["channels"], case["block_len"]
    for u in range(units.shape[0]):
        n = B if u // C < case["n_blocks"] else case["tail_len"]
        assert not units[u, n:].any()


def test_cases_cover_the_shapes():
    cs = list(CASES.values())
    assert {c["block_len"] for c in cs} >= set(rm.BLOCKS)
    assert {c["channels"] for c in cs} >= set(rm.CHANNELS)
    assert {c["sample_bytes"] for c in cs} == {2, 4}
    assert any(c["n_blocks"] == 0 and c["tail_len"] for c in cs)          # tail only: the carry extraction
    assert any(c["n_blocks"] and not c["tail_len"] for c in cs)           # whole blocks only
    assert any(c["n_blocks"] and c["tail_len"] for c in cs)
    assert any(c["s0"] == 1 for c in cs) and any(c["s0"] == c["block_len"] - 1 > 1 for c in cs)
    assert any(len(set(c["pitches"])) > 1 for c in cs)                    # two row pitches in one list
    assert any(c["frames"] and c["frames"][0].shape[1] == 0 for c in cs)  # an empty carry pseudo-frame
    assert any(c["frames"] and c["frames"][0].shape[1] == c["block_len"] - 1 > 1 for c in cs)
    for c in cs:  # the pitch: a multiple of 16 bytes that holds the block
        assert c["stride"] >= c["block_len"] and (c["stride"] * c["sample_bytes"]) % 16 == 0
    # frames that go on past the last unit (samples not read)
    assert any(sum(f.shape[1] for f in c["frames"]) > c["s0"] + c["n_blocks"] * c["block_len"] + c["tail_len"]
               for c in cs)


def test_measured_width_is_the_hosts_sample_bits():
    from flac_amd.encoder import _sample_bits
    rng = np.random.default_rng(5)
    for bits in (2, 3, 8, 12, 16, 17, 24, 32):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        for x in (np.array([lo]), np.array([hi]), np.array([0]), np.array([-1]), rng.integers(lo, hi + 1, 50)):
            x = x.astype(np.int64)
            w = int(np.where(x >= 0, x, ~x).max())
            got = rm.sample_bits(w, 32)
            assert got <= max(2, bits)
            assert got <= _sample_bits(x)            # never wider than what _planar measures
            assert x.min() >= -(1 << (got - 1)) and x.max() <= (1 << (got - 1)) - 1  # and it holds the data
            assert rm.sample_bits(w, 16) == min(16, got)


# ---- (b) the header -------------------------------------------------------------------------

def _parameters(block_size=192):
    from flac_amd.encoder import EncoderParameters
    return EncoderParameters(block_size=block_size, rice_partition_order=range(0, 4), lpc_order=range(0, 9),
                             qlp_precision=12)


def _input_header(blocks, md5=bytes(range(16)), channels=2, sample_size=16, samples=1234):
    from flac_amd.common import MAGIC, MetadataBlockHeader, MetadataBlockType, Streaminfo
    from flac_amd.encoder import put_metadata_block_header, put_metadata_block_streaminfo
    si = Streaminfo(min_block_size=100, max_block_size=4096, min_frame_size=11, max_frame_size=999, sample_rate=44100,
                    channels=channels, sample_size=sample_size, samples=samples, md5=md5)
    out = MAGIC + put_metadata_block_header(MetadataBlockHeader(not blocks, MetadataBlockType.Streaminfo, 34)).buffer
    out += put_metadata_block_streaminfo(si).buffer
    for k, (t, body) in enumerate(blocks):
        out += put_metadata_block_header(MetadataBlockHeader(k == len(blocks) - 1, MetadataBlockType(t), len(body))).buffer
        out += body
    return si, bytes(out)


def test_header_default_is_encodes():
    from flac_amd.encoder import _stream_header
    from flac_amd.recompress import read_metadata_blocks, stream_header
    blocks = [(4, b"vorbis comment"), (3, bytes(36)), (1, bytes(7))]
    si, raw = _input_header(blocks)
    buf = BytesIO(raw + b"\xff\xf8rest")
    got_si, got_blocks = read_metadata_blocks(buf)
    assert got_si == si and got_blocks == blocks
    assert buf.read() == b"\xff\xf8rest"  # left at the first frame
    p = _parameters()
    assert b"".join(stream_header(si, p)) == b"".join(_stream_header(44100, 16, 2, 1234, p))


def test_header_keep_metadata():
    from flac_amd.decoder import read_metadata
    from flac_amd.recompress import read_metadata_blocks, stream_header
    blocks = [(4, b"vorbis comment"), (3, bytes(36)), (2, b"appl" + bytes(5)), (1, bytes(7))]
    si, _ = _input_header(blocks)
    p = _parameters(256)
    out = b"".join(stream_header(si, p, blocks))
    buf = BytesIO(out + b"tail")
    si2, kept = read_metadata_blocks(buf)
    assert buf.read() == b"tail"
    assert kept == [b for b in blocks if b[0] != 3]            # byte for byte, in order, no SEEKTABLE
    assert si2.md5 == si.md5 and si2.samples == si.samples      # the signature stays
    assert (si2.min_block_size, si2.max_block_size, si2.min_frame_size, si2.max_frame_size) == (256, 256, 0, 0)
    assert read_metadata(BytesIO(out)) == si2                   # the `last` flags end the list where it ends
    # a SEEKTABLE alone: STREAMINFO becomes the last block
    out = b"".join(stream_header(si, p, [(3, bytes(18))]))
    assert len(out) == 4 + 4 + 34 and out[4] == 0x80
    # no block at all
    assert b"".join(stream_header(si, p, [])) == out


# ---- (c) refusals ---------------------------------------------------------------------------

def test_python_refusals_need_no_device(monkeypatch):
    import flac_amd.recompress as rc
    from flac_amd.encoder import EncoderParameters

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(rc, "_sessions", no_device)
    _, mono = _input_header([], channels=1)
    _, stereo = _input_header([])
    p = _parameters()
    wide = EncoderParameters(block_size=192, rice_partition_order=range(0, 11), lpc_order=range(0, 9), qlp_precision=12)
    for data, par, kw in ((mono, p, dict(stereo=True)), (stereo, p, dict(stereo=True, wasted=True)),
                          (stereo, p, dict(lpc_sign=True, fixed_only=True)), (stereo, wide, dict(rice_search=True)),
                          (stereo, p, dict(size_choice=True)),
                          (stereo, p, dict(size_choice=True, rice_search=True, wasted=True)),
                          (stereo, p, dict(chunk_bytes=0))):
        with pytest.raises(ValueError):
            list(rc.recompress(data, par, **kw))
    with pytest.raises(AssertionError):  # 44.1 kHz: the subset's LPC order bound, as encode()
        list(rc.recompress(stereo, EncoderParameters(192, range(0, 4), range(0, 20), 12)))
    with pytest.raises(AssertionError):  # not a FLAC stream
        list(rc.recompress(b"RIFF" + stereo[4:], p))


def test_c_refusals_need_no_device():
    from flac_amd import abi
    from flac_amd._lib import load
    from flac_amd.analysis import frame_params, make_params
    lib = load()
    fake = ctypes.c_void_p(1)  # never dereferenced: every refusal comes before any device work
    buf = (ctypes.c_uint8 * 64)()
    E = abi.E_INVALID

    def call(block_len=192, channels=2, ss=16, dch=None, dss=None, params=None, first_byte=0, nbytes=64, **fpkw):
        dp = abi.DecodeParams()
        dp.channels, dp.sample_size, dp.first_frame = dch or channels, dss or ss, -1
        fp = frame_params(channels, ss, 12, 0, **fpkw)
        res = abi.RecompressResult()
        return lib.flacmi_recompress_host(fake, buf, nbytes, first_byte, ctypes.byref(dp), 0, 0, 1, block_len,
                                          ctypes.byref(params or make_params(8, 12, 0, 3)), ctypes.byref(fp),
                                          ctypes.byref(res))
    assert call(block_len=0) == E and call(block_len=65536) == E and call(block_len=-5) == E
    assert call(stereo=True, wasted=True) == E                   # the pinned combinations of flacmi_encode_host
    assert call(channels=3, stereo=True) == E
    assert call(ss=32, stereo=True) == E
    assert call(params=make_params(8, 12, 0, 3, rice_search=True, size_choice=True), wasted=True) == E
    assert call(params=make_params(8, 12, 0, 3, size_choice=True)) == E
    assert call(params=make_params(8, 12, 0, 9, rice_search=True)) == E
    assert call(params=make_params(8, 12, 0, 3, abi.MODE_FIXED_ONLY, lpc_sign=True)) == E
    assert call(params=make_params(8, 12, 0, 3, rice_search=True, size_choice=True, sample_size=24)) == E
    assert call(params=make_params(33, 12, 0, 3)) == E
    assert call(dch=1) == E and call(dss=24) == E                # the two halves disagree
    assert call(first_byte=65) == E and call(nbytes=-1) == E
    fp = frame_params(2, 16, 12, 0)
    fp.reserved0 = 2
    dp = abi.DecodeParams()
    dp.channels, dp.sample_size = 2, 16
    res = abi.RecompressResult()
    assert lib.flacmi_recompress_host(fake, buf, 64, 0, ctypes.byref(dp), 0, 0, 1, 192,
                                      ctypes.byref(make_params(8, 12, 0, 3)), ctypes.byref(fp), ctypes.byref(res)) == E
    dp.reserved0 = 2  # an unknown decode flag
    fp.reserved0 = 0
    assert lib.flacmi_recompress_host(fake, buf, 64, 0, ctypes.byref(dp), 0, 0, 1, 192,
                                      ctypes.byref(make_params(8, 12, 0, 3)), ctypes.byref(fp), ctypes.byref(res)) == E
    # flacmi_units_out_device's own
    w = (ctypes.c_uint32 * 1)()

    def units(channels=2, s0=0, B=16, nb=1, tail=0, ss=16, sbytes=2, stride=16, units_ptr=buf, width=w):
        return lib.flacmi_units_out_device(fake, buf, 1, channels, s0, B, nb, tail, ss, units_ptr, sbytes, stride, buf,
                                           width, None)
    assert units(channels=0) == E and units(channels=9) == E
    assert units(B=0) == E and units(B=65536) == E
    assert units(tail=16) == E and units(tail=-1) == E and units(nb=-1) == E and units(s0=-1) == E
    assert units(ss=3) == E and units(ss=17) == E and units(ss=33, sbytes=4, stride=16) == E
    assert units(sbytes=3) == E
    assert units(stride=15) == E and units(stride=12) == E and units(stride=20) == E
    assert units(width=None) == E
    assert units(units_ptr=ctypes.byref(buf, 8)) == E            # rows must be 16-byte aligned


def test_struct_mirror_matches_header(tmp_path):
    import subprocess
    from flac_amd import abi
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacmi.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(flacmi_recompress_result));']
    for f, _ in abi.RecompressResult._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(flacmi_recompress_result, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.RecompressResult)
    for f, _ in abi.RecompressResult._fields_:
        assert int(got[f]) == getattr(abi.RecompressResult, f).offset, f


# ---- (d) row width ---------------------------------------------------------------------------

def test_row_width_does_not_change_the_bytes():
    """A 24-bit stream of 12-bit content: the analysis of int16 rows and of int32 rows (at the
    measured 12 bits and at the stream's 24, both upper bounds) and the frame writer give the same
    frames.  recompress keeps int32 unit rows for every stream wider than 16 bits."""
    import frame_writer as FW
    import oracle
    n, channels, blocks, tail = 192, 2, 3, 77
    a16 = oracle.synth_batch(0, blocks * channels, n, 12, 99, dtype=np.int16, stride=192)
    a16[-channels:, tail:] = 0
    assert a16.min() >= -2048 and a16.max() <= 2047 and (np.abs(a16.astype(np.int64)).max() >= 256)
    a32 = np.zeros((a16.shape[0], 200), dtype=np.int32)
    a32[:, :192] = a16
    p = oracle.make_params(8, 12, 0, 3)
    streams = []
    for rows, bits in ((a16, 12), (a32, 12), (a32, 24)):
        out = oracle.analyze_batch(rows, p, n, tail, channels, sample_bits=bits)
        frames = FW.frames_from_analysis(rows, out, channels, n, tail, 24, 12)
        assert all(isinstance(f, bytes) for f in frames)
        streams.append(b"".join(frames))
    assert streams[0] == streams[1] == streams[2] and len(streams[0]) > 100
