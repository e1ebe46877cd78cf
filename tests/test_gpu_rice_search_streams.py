"""FLACMI_FLAG_RICE_SEARCH end to end: the streams of tests/golden/rice_search_streams.json (the
reference's encode() with its rice_partitions replaced by the rule) through encode(),
encode_planar() and `encode --rice-search`, back through the device decoder; with the fallback,
stereo and wasted-bits modes against their CPU models fed with the searched analysis; the
refusals; and the same inputs with the flag clear, which fail where the reference fails."""
import wave

import numpy as np
import pytest

import fallback_model as FM
import frame_writer as FW
import golden_util as G
import oracle
import rice_search_cases as RC
import rice_search_model as RM
import stereo_model as SM
from flac_amd import abi, info
from flac_amd import encoder as enc
from flac_amd.analysis import Analyzer, make_params
from flac_amd.decoder import decode
from mode_matrix_model import _wasted_subframe

pytestmark = pytest.mark.gpu
GOLD = G.load("rice_search_streams.json")["cases"]


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def _encoder_parameters(c):
    return enc.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                 lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])


def _searched(rows, c, tail, n_tail, ss=None, threads=4):
    """The oracle's analysis of rows with the search applied: the dictionary the CPU models take."""
    ss = ss or c["ss"]
    out = oracle.analyze_batch(np.ascontiguousarray(rows), oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]),
                               c["n"], tail, n_tail, sample_bits=ss, threads=threads)
    lens = [tail if u >= rows.shape[0] - n_tail else c["n"] for u in range(rows.shape[0])]
    return RM.apply(out, lens, c["rmin"], c["rmax"])


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_streams_are_the_patched_reference_streams(name, tmp_path):
    from flac_amd import cli
    c, g = RC.CASES[name], GOLD[name]
    x = RC.channels(name)
    ep = _encoder_parameters(c)
    want = bytes.fromhex(g["header"]) + b"".join(bytes.fromhex(f) for f in g["frames"])
    samples = iter([int(v) for v in x[:, i]] for i in range(c["frames"]))
    data = b"".join(enc.encode(c["rate"], c["ss"], c["C"], c["frames"], samples, ep, rice_search=True, blocks_per_batch=2))
    assert data == want, "encode"
    assert b"".join(enc.encode_planar(c["rate"], c["ss"], x, ep, rice_search=True)) == want, "encode_planar"
    wav, out = tmp_path / "in.wav", tmp_path / "out.flac"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(c["C"])
        w.setsampwidth(c["ss"] // 8)
        w.setframerate(c["rate"])
        inter = np.ascontiguousarray(x.T).astype("<i4")
        w.writeframes(inter.view(np.uint8).reshape(-1, 4)[:, :c["ss"] // 8].tobytes())
    assert cli.main(["encode", str(wav), str(out), "-b", str(c["n"]), "-l", str(c["L"]), "-q", str(c["q"]),
                     "-r", f"{c['rmin']},{c['rmax']}", "--correct-reader", "--rice-search"]) == 0
    assert out.read_bytes() == want, "encode --rice-search"
    sr, ss, ch, total, dec = decode(want, check_crc=True)
    assert (sr, ss, ch, total) == (c["rate"], c["ss"], c["C"], c["frames"])
    assert np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, c["C"]).T, x)


@pytest.mark.parametrize("name", ["gate16m", "gate16s"])
def test_flag_clear_is_the_reference_with_its_failures(az, name):
    c, g = RC.CASES[name], GOLD[name]
    rows, lens = RC.unit_rows(name)
    out = az.analyze(rows, make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], sample_bits=c["ss"])
    ora = oracle.analyze_batch(rows, oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], sample_bits=c["ss"])
    for u in range(len(lens)):
        assert not RM.baseline_mismatches(out["meta"][u], ora["meta"][u]), u
        k = int(out["meta"]["n_parts"][u])
        assert np.array_equal(out["rice_params"][u][:k], ora["rice_params"][u][:k])
    assert {int(v) for v in out["meta"]["site"]} >= {12, 13}
    first = g["reference"][0]
    assert first != "ok"
    with pytest.raises(ValueError, match=first):  # encode() stops at the first frame, as the reference does
        list(enc.encode_planar(c["rate"], c["ss"], RC.channels(name), _encoder_parameters(c)))


@pytest.mark.parametrize("name", ["gate16m", "gate16s", "tail16"])
def test_with_fallback_the_gated_frames_are_fixed_or_lpc(az, name):
    """fallback alone writes the units the Rice step fails as VERBATIM; with the search they are the
    analysed FIXED / LPC subframes, smaller, and the bytes are the fallback model's on the searched
    analysis."""
    c, g = RC.CASES[name], GOLD[name]
    x = RC.channels(name)
    ep = _encoder_parameters(c)
    alone = b"".join(enc.encode_planar(c["rate"], c["ss"], x, ep, fallback=True))
    both = b"".join(enc.encode_planar(c["rate"], c["ss"], x, ep, fallback=True, rice_search=True))
    t_alone = [s.type_name for fr in info.analyze(alone).frames for s in fr.subframes]
    t_both = [s.type_name for fr in info.analyze(both).frames for s in fr.subframes]
    failed = [u for u, b in enumerate(g["reference"]) if b != "ok"]
    assert failed and all(t_alone[u] == "VERBATIM" for u in failed)
    assert all(t in ("FIXED", "LPC") for t in t_both) and len(both) < len(alone)
    rows, lens = RC.unit_rows(name)
    tail = RC.tail_len(name)
    n_tail = c["C"] if tail else 0
    frames, kinds = FM.frames(rows, _searched(rows, c, tail, n_tail), c["C"], c["n"], tail, c["ss"], c["q"], fallback=True)
    assert not any(kinds) and both == bytes.fromhex(g["header"]) + b"".join(frames)
    data, offsets, status = az.encode_frames(rows, make_params(c["L"], c["q"], c["rmin"], c["rmax"], rice_search=True),
                                             c["n"], tail, n_tail, sample_bits=c["ss"], channels=c["C"],
                                             sample_size=c["ss"], fallback=True)
    assert not status.any() and data.tobytes() == b"".join(frames)
    _, _, ch, _, dec = decode(both, check_crc=True)
    assert np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, ch).T, x)


@pytest.mark.parametrize("fallback", [False, True])
def test_stereo_candidates_are_searched(az, fallback):
    """The stereo mode's three analyses carry the flag: device frames == the stereo model over the
    searched left, right, mid and side candidates."""
    name = "gate16s"
    c = RC.CASES[name]
    rows, lens = RC.unit_rows(name)
    p = oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"])
    cands = SM.analyse(rows, p, c["n"], 0, c["ss"])
    done = {}
    for f in range(len(cands)):
        for k, (samples, out, u, w) in enumerate(cands[f]):
            if id(out) not in done:
                done[id(out)] = RM.apply(out, [c["n"]] * len(out["meta"]), c["rmin"], c["rmax"])
            cands[f][k] = (samples, done[id(out)], u, w)
    assert sum(len(d["rescued"]) for d in done.values()) >= 4
    want, codes = SM.frames(rows, cands, c["n"], 0, c["q"], 0, fallback)[:2]
    assert all(isinstance(f, bytes) for f in want)
    data, offsets, status = az.encode_frames(rows, make_params(c["L"], c["q"], c["rmin"], c["rmax"], rice_search=True),
                                             c["n"], sample_bits=c["ss"], channels=2, sample_size=c["ss"],
                                             fallback=fallback, stereo=True)
    assert not status.any() and data.tobytes() == b"".join(want)
    x = RC.channels(name)
    stream = b"".join(enc.encode_planar(c["rate"], c["ss"], x, _encoder_parameters(c), stereo=True, fallback=fallback,
                                        rice_search=True))
    assert stream == bytes.fromhex(GOLD[name]["header"]) + b"".join(want)
    _, _, ch, _, dec = decode(stream, check_crc=True)
    assert np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, ch).T, x)


def test_wasted_units_are_searched(az):
    """16-bit gated samples << 8 in a 24-bit stream with the wasted-bits mode: every unit is analysed
    and searched as x >> 8 and written at 16 bits behind a header declaring 8 wasted bits."""
    name = "gate16s"
    c = RC.CASES[name]
    rows, lens = RC.unit_rows(name)
    srch = _searched(rows, c, 0, 0)
    want = []
    for f in range(rows.shape[0] // 2):
        bits = FW.Bits()
        for b in FW.frame_header(f, c["n"]):
            bits.put(b, 8)
        for u in (2 * f, 2 * f + 1):
            m = srch["meta"][u]
            assert int(m["status"]) == 0
            off, ln = int(m["res_offset"]), int(m["res_len"])
            _wasted_subframe(bits, rows[u], m, srch["residual"][u][off:off + ln], srch["rice_params"][u][: int(m["n_parts"])],
                             c["n"], 16, c["q"], 8)
        bits.put(0, (8 - bits.n % 8) % 8)
        body = bits.to_bytes()
        want.append(body + FW.crc16(body).to_bytes(2, "big"))
    wide = rows.astype(np.int32) << 8
    data, offsets, status = az.encode_frames(wide, make_params(c["L"], c["q"], c["rmin"], c["rmax"], rice_search=True),
                                             c["n"], sample_bits=24, channels=2, sample_size=24, wasted=True)
    assert not status.any() and data.tobytes() == b"".join(want)
    x = RC.channels(name) << 8
    stream = b"".join(enc.encode_planar(c["rate"], 24, x, _encoder_parameters(c), wasted=True, rice_search=True))
    assert stream[42:] == b"".join(want)
    _, ss, ch, _, dec = decode(stream, check_crc=True, spec_wasted_bits=True)
    assert ss == 24 and np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, ch).T, x)


def test_refused_combinations(az):
    from flac_amd._lib import FlacmiError
    pcm = np.zeros((1, 2048), dtype=np.int64)
    wide = enc.EncoderParameters(block_size=1024, rice_partition_order=range(0, 10), lpc_order=range(0, 9), qlp_precision=5)
    with pytest.raises(ValueError, match="rice_search"):
        next(enc.encode_planar(44100, 16, pcm, wide, rice_search=True))
    with pytest.raises(ValueError, match="rice_search"):
        next(enc.encode(44100, 16, 1, 2048, iter([]), wide, rice_search=True))
    with pytest.raises(ValueError, match="rice_search"):
        enc.encode_residual([1] * 1024, 1024, 16, 0, range(0, 10), rice_search=True)
    rows = np.zeros((2, 1024), dtype=np.int16)
    with pytest.raises(FlacmiError):  # the C-ABI refuses it before any launch
        az.encode_frames(rows, make_params(8, 5, 0, 9, rice_search=True), 1024, channels=1)
    with pytest.raises(FlacmiError):
        az.encode_frames(rows, make_params(8, 5, 0, 3, abi.MODE_LPC_ONLY, rice_search=True), 1024, channels=1)


def test_encode_residual_keyword():
    """The function-level form: a residual with a silent partition raises in the reference and is
    written by the search; the partitions are the model's."""
    z = [5, -3, 8, 1] * 8 + [0] * 16 + [2, -2] * 8
    with pytest.raises(ValueError):
        enc.encode_residual(z, 64, 16, 0, range(0, 3))
    r = enc.encode_residual(z, 64, 16, 0, range(0, 3), rice_search=True)
    zz = [(v << 1) ^ (v >> 63) for v in z]
    want = RM.search(zz, 64, 0, 0, 2)
    assert r.coding_method.value == want["coding_method"]
    assert [p.parameter for p in r.partitions] == want["rice_params"]
    assert [v for p in r.partitions for v in p.residual] == zz
