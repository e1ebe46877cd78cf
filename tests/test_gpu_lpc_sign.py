"""The corrected-LPC-sign mode on the device (FLACMI_FLAG_LPC_SIGN, include/flacmi.h: the sign
of the quantiser's scale in lpc_finish of csrc/k_lpc.hip, and the exact-candidate dispatch of
csrc/flacmi_host.cpp) against the CPU model of tests/lpc_sign_model.py, unit by unit and field by
field, on the smallest shapes that reach each kernel; and against the bytes the reference's own
encode() gave with its levinson_durbin's result negated (tests/golden/lpc_sign_streams.json)
through encode(), encode_planar() and the command line.  With the flag clear the same calls give
what the oracle's default path gives, pruned sentinels included."""
import functools
import json
import wave

import numpy as np
import pytest

import fallback_model as FM
import frame_writer as FW
import golden_util as G
import lpc_shape_cases as LS
import lpc_sign_cases as LC
import lpc_sign_model as LM
import oracle
import stereo_model as SM
import stream_shape_cases as SS
from flac_amd import abi
from flac_amd.analysis import make_params

pytestmark = pytest.mark.gpu
SEED = 2024
LISTED = 0x101  # meta.lpc_tiers of a unit k_resid_stream's list kernel took, pruning or not
_STATUS = {"ZeroDivisionError": abi.STATUS_ZERO_DIVISION, "AssertionError": abi.STATUS_ASSERTION,
           "ValueError": abi.STATUS_VALUE_ERROR, "OverflowError": abi.STATUS_OVERFLOW}
META_FIELDS = [f for f in abi.META_DTYPE.names if f != "coefs"]


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(LC.GOLDEN))["cases"]


def compare_with_model(out, mod, lens, L, sums=False, listed=False):
    """Every unit: status and site.  Every unit with a result: every meta field (lpc_tiers is 0 and
    nothing is pruned in the mode), the coefficients, the Rice parameters and the residual row.
    Every unit whose LPC analysis completed: its whole LPC record but word 0 (the device's status
    word, which the oracle's layout leaves 0), and with sums its candidate sums."""
    gm, mm = out["meta"], mod["meta"]
    assert not (gm["lpc_order"] == abi.LPC_PRUNED).any()
    # no pruning tier runs; 0x101 (one exact pass) is the marker of k_resid_stream's list kernel
    assert np.isin(gm["lpc_tiers"], (0, LISTED) if listed else (0,)).all(), gm["lpc_tiers"]
    for u in range(len(lens)):
        assert (int(gm["status"][u]), int(gm["site"][u])) == (int(mm["status"][u]), int(mm["site"][u])), \
            (u, "status/site", int(gm["status"][u]), int(gm["site"][u]), int(mm["status"][u]), int(mm["site"][u]))
        if mod["record_ok"][u] and L > 0:
            assert np.array_equal(out["lpc_records"][u][1:], mod["lpc_records"][u][1:]), (u, "lpc_records")
            if sums:
                assert np.array_equal(out["lpc_sums"][u], mod["lpc_sums"][u]), (u, "lpc_sums")
        if int(mm["status"][u]) != 0:
            continue
        for f in META_FIELDS:
            if f == "lpc_tiers":
                continue
            assert int(gm[f][u]) == int(mm[f][u]), (u, f, int(gm[f][u]), int(mm[f][u]))
        k = int(mm["ncoefs"][u])
        assert list(gm["coefs"][u][:k]) == list(mm["coefs"][u][:k]), (u, "coefs")
        npart = int(mm["n_parts"][u])
        assert np.array_equal(out["rice_params"][u][:npart], mod["rice_params"][u][:npart]), (u, "params")
        off, ln = int(mm["res_offset"][u]), int(mm["res_len"][u])
        assert off + ln == lens[u]
        assert np.array_equal(out["residual"][u][off:off + ln].astype(np.uint64),
                              mod["residual"][u][off:off + ln]), (u, "residual")


def run_case(az, a, n, bits, L, q, rmin, rmax, tail=(0, 0), mode=abi.MODE_REFERENCE, listed=False):
    """The production call (no optional output but the records) and the call with lpc_sums, each
    against the model -> (the last device result, the model's)."""
    mod = LM.analyze(a, oracle.make_params(L, q, rmin, rmax, mode), n, tail[0], tail[1], sample_bits=bits)
    lens = [n] * (a.shape[0] - tail[1]) + [tail[0]] * tail[1]
    p = make_params(L, q, rmin, rmax, mode, lpc_sign=True)
    assert p.reserved[1] == abi.FLAG_LPC_SIGN
    for extras, sums in ((("lpc_records",), False), (("lpc_records", "lpc_sums"), True)):
        out = az.analyze(a, p, n, tail[0], tail[1], sample_bits=bits, extras=extras)
        compare_with_model(out, mod, lens, L, sums, listed)
    return out, mod


def kinds(mod):
    m = mod["meta"]
    ok = m["status"] == 0
    return int((ok & (m["kind"] == abi.KIND_FIXED)).sum()), int((ok & (m["kind"] == abi.KIND_LPC)).sum())


# ---------------------------------------------------------------------------------------
# analysis: one case per kernel path
# ---------------------------------------------------------------------------------------
def test_stream_kernel_runtime_shape_and_lpc_tile(az):
    """69 = 64 + 5 units of 256 samples: k_lpc_tile<12> and k_lpc<12, int16_t>, then the
    runtime-shape k_resid_stream in its exact mode."""
    a = oracle.synth_batch(0, 69, 256, 16, SEED)
    assert [(k, m, c) for k, m, _, c in LS.launch_split(69, 2, 12, 256)] == [("tile", 12, 64), ("gen16", 12, 5)]
    sh = SS.stream_shape(256, 12, 0, 5, False)
    assert sh and sh["NFIX"] == 0 and SS.narrow_path(256, 12, 5, False)
    _, mod = run_case(az, a, 256, 16, 12, 5, 0, 5)
    assert kinds(mod)[1] >= 60


def test_stream_kernel_constant_shape(az):
    a = oracle.synth_batch(0, 8, 4608, 16, SEED)
    assert SS.stream_shape(4608, 12, 0, 5, False)["NFIX"] == 4608
    _, mod = run_case(az, a, 4608, 16, 12, 5, 0, 5)
    assert kinds(mod) == (0, 8)


def test_q6_units_beyond_the_f16_and_int8_bounds(az):
    """q 6: coefficients up to 32 in magnitude.  Units whose taps leave the stream kernel's exact
    ranges (sum |c| <= 127, the f16 bound) go through both list kernels."""
    a = oracle.synth_batch(0, 30, 4608, 16, SEED)
    assert SS.stream_shape(4608, 12, 0, 5, False) and SS.narrow_path(4608, 12, 6, False)
    out, mod = run_case(az, a, 4608, 16, 12, 6, 0, 5, listed=True)
    m = mod["meta"]
    big = [u for u in range(30) if int(np.abs(m["coefs"][u][:int(m["ncoefs"][u])]).sum()) > 127]
    assert len(big) >= 1 and kinds(mod)[1] >= 25
    # k_resid_stream_list marks the units it computes (outside the f16 bound, sum |c| <= 127); a unit
    # whose taps leave the int8 range it hands on to k_resid's list variant, which marks nothing
    # without pruning: both list kernels ran
    tiers = out["meta"]["lpc_tiers"]
    assert (tiers == LISTED).any() and (tiers[big] == 0).all()


@pytest.mark.parametrize("n,L,units", [(200, 12, 6), (8, 4, 20)])
def test_general_kernel(az, n, L, units):
    """Lengths off every multiple of 64: the general k_resid.  8-sample blocks keep some FIXED
    winners."""
    assert SS.stream_shape(n, L, 0, 3, False) is None
    a = oracle.synth_batch(0, units, n, 16, SEED, stride=max(n, 8))
    _, mod = run_case(az, a, n, 16, L, 5, 0, 3)
    fixed, lpc = kinds(mod)
    assert lpc >= 1 and (n != 8 or fixed >= 1)


@pytest.mark.parametrize("n", [322, 1024])
def test_24_bit_l32_q15(az, n):
    """k_lpc<32, int32_t>; 1024 samples reach the int8-MFMA exact variant, 322 the int64 chains."""
    a = oracle.synth_batch(0, 3, n, 24, SEED, dtype=np.int32, stride=LS.row_pitch(n, 4))
    assert LS.launch_split(3, 4, 32, a.shape[1]) == [("ring", 32, 0, 3)]
    _, mod = run_case(az, a, n, 24, 32, 15, 0, 4)
    assert kinds(mod)[1] >= 1


def test_31_bit_samples(az):
    """The 64-bit chains (sample_bits + q = 43)."""
    a = oracle.synth_batch(0, 4, 256, 31, SEED, dtype=np.int32)
    assert int(np.abs(a.astype(np.int64)).max()) >= 1 << 28
    run_case(az, a, 256, 31, 8, 12, 0, 4)


@pytest.mark.parametrize("L", [16, 17])
def test_int16_high_orders(az, L):
    """k_lpc<16, int16_t> and k_lpc<32, int16_t>."""
    a = oracle.synth_batch(0, 3, 192, 16, SEED)
    assert LS.launch_split(3, 2, L, 192) == [("gen16", 16 if L == 16 else 32, 0, 3)]
    run_case(az, a, 192, 16, L, 12, 0, 3)


def test_tail_class(az):
    a = oracle.synth_batch(0, 6, 4410, 16, SEED, stride=LS.row_pitch(4410, 2))
    a[4:, 882:] = 0
    run_case(az, a, 4410, 16, 12, 5, 0, 3, tail=(882, 2))


def test_edge_units(az):
    """Every unit of tests/golden/edge.json the mode applies to (the failing and near-tie ones
    among them), in the mode, against the model."""
    seen = set()
    for e in G.load("edge.json")["units"]:
        if e["params"]["fixed_only"]:
            continue
        xs = G.samples_for(e, oracle.synth_unit)
        pr = e["params"]
        n = len(xs)
        a = np.zeros((1, max(8, LS.row_pitch(n, 2))), dtype=np.int16)
        a[0, :n] = xs
        _, mod = run_case(az, a, n, 16, pr["L"], pr["q"], pr["rmin"], pr["rmax"])
        seen.add((int(mod["meta"]["status"][0]), int(mod["meta"]["site"][0])))
    # the sign-independent sites are still reached, and units with a result exist
    assert {(0, 0), (1, 1), (1, 2), (3, 9)} <= seen, seen


def test_lpc_only_mode_and_the_python_subframe(az):
    a = oracle.synth_batch(0, 5, 200, 16, SEED)
    _, mod = run_case(az, a, 200, 16, 8, 5, 0, -1, mode=abi.MODE_LPC_ONLY)
    from flac_amd import encoder as enc
    xs = [int(v) for v in a[0]]
    header, sub = enc.encode_subframe_lpc(xs, range(0, 9), 5, lpc_sign=True)
    m = mod["meta"][0]
    k = int(m["ncoefs"])
    assert header.type_.order == int(m["order"]) and sub.shift == int(m["shift"])
    assert list(sub.coefficients) == [int(c) for c in m["coefs"][:k]] and list(sub.warmup) == xs[:k]
    zz = mod["residual"][0][k:200].astype(np.int64)
    assert list(sub.residual) == [int(v) for v in (zz >> 1) ^ -(zz & 1)]
    plain = enc.encode_subframe_lpc(xs, range(0, 9), 5)[1]
    assert sum(map(abs, sub.residual)) < sum(map(abs, plain.residual))


def test_flag_validation(az):
    """FIXED_ONLY and RICE_ONLY with the flag: FLACMI_E_INVALID; fixed_only with lpc_sign in
    Python: ValueError before any device work."""
    from flac_amd import encoder as enc
    from flac_amd._lib import FlacmiError
    a = oracle.synth_batch(0, 2, 64, 16, SEED)
    for mode in (abi.MODE_FIXED_ONLY, abi.MODE_RICE_ONLY):
        with pytest.raises(FlacmiError) as ei:
            az.analyze(a, make_params(0, 5, 0, 3, mode, lpc_sign=True), 64)
        assert ei.value.code == abi.E_INVALID and b"FLACMI_FLAG_LPC_SIGN" in az.lib.flacmi_last_error()
    fp = enc.EncoderParameters(block_size=64, rice_partition_order=range(0, 4), lpc_order=range(0, 9), qlp_precision=5)
    pcm = np.zeros((1, 64), dtype=np.int64)
    with pytest.raises(ValueError, match="lpc_sign"):
        next(enc.encode(44100, 16, 1, 64, iter([]), fp, fixed_only=True, lpc_sign=True))
    with pytest.raises(ValueError, match="lpc_sign"):
        next(enc.encode_planar(44100, 16, pcm, fp, fixed_only=True, lpc_sign=True))
    with pytest.raises(ValueError, match="lpc_sign"):
        next(enc.encode_wav("does-not-exist.wav", fp, fixed_only=True, lpc_sign=True))


# ---------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------
def _encoder_parameters(c):
    from flac_amd import encoder as enc
    return enc.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                 lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])


def _collect(gen):
    """-> (the chunks a generator yields, the exception that ended it or None)"""
    parts = []
    try:
        for p in gen:
            parts.append(p)
    except (ZeroDivisionError, AssertionError, ValueError, OverflowError) as e:
        return parts, e
    return parts, None


def _check_stream(parts, err, g, what):
    assert b"".join(parts[:3]).hex() == g["header"], what
    assert len(parts) == 3 + len(g["frames"]), (what, len(parts))
    for f, want in enumerate(g["frames"]):
        assert LC.same_frame(parts[3 + f], want), (what, f"frame {f}")
    assert (type(err).__name__ if err else None) == g["raises"], (what, err)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_streams_are_the_patched_reference_streams(golden, name, tmp_path):
    """encode(), encode_planar() and `encode --lpc-sign` write the fixture's bytes and stop where
    the reference stops, with its exception; the device decoder returns the input."""
    from flac_amd import cli
    from flac_amd import encoder as enc
    from flac_amd.decoder import decode
    c, g = LC.CASES[name], golden[name]
    x = LC.channels(name)
    ep = _encoder_parameters(c)
    samples = iter([int(v) for v in x[:, i]] for i in range(c["frames"]))
    parts, err = _collect(enc.encode(c["rate"], c["ss"], c["C"], c["frames"], samples, ep, lpc_sign=True,
                                     blocks_per_batch=2))
    _check_stream(parts, err, g, "encode")
    pparts, perr = _collect(enc.encode_planar(c["rate"], c["ss"], x, ep, lpc_sign=True))
    _check_stream(pparts, perr, g, "encode_planar")
    wav, out = tmp_path / "in.wav", tmp_path / "out.flac"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(c["C"])
        w.setsampwidth(c["ss"] // 8)
        w.setframerate(c["rate"])
        inter = np.ascontiguousarray(x.T).astype("<i4")
        w.writeframes(inter.view(np.uint8).reshape(-1, 4)[:, :c["ss"] // 8].tobytes())
    args = ["encode", str(wav), str(out), "-b", str(c["n"]), "-l", str(c["L"]), "-q", str(c["q"]),
            "-r", f"{c['rmin']},{c['rmax']}", "--correct-reader", "--lpc-sign"]
    if g["raises"]:
        with pytest.raises(_exc(g["raises"])):
            cli.main(args)
    else:
        assert cli.main(args) == 0
    assert out.read_bytes() == b"".join(parts)
    # the frames written, back to the input through the device decoder
    done = len(g["frames"])
    total = min(done * c["n"], c["frames"])
    header = FW.stream_header(c["rate"], c["ss"], c["C"], total, c["n"])
    sr, ss, ch, tot, dec = decode(header + b"".join(parts[3:]), check_crc=True)
    assert (sr, ss, ch, tot) == (c["rate"], c["ss"], c["C"], total)
    assert np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, c["C"]).T, x[:, :total])
    # without the keyword: the default stream, in which no LPC subframe wins; it is larger
    plain, plain_err = _collect(enc.encode_planar(c["rate"], c["ss"], x, ep))
    assert plain[:3] == parts[:3]
    if not g["raises"] and plain_err is None and c["n"] > 8:
        assert sum(map(len, parts)) < sum(map(len, plain))


def _exc(name):
    return {"ZeroDivisionError": ZeroDivisionError, "AssertionError": AssertionError, "ValueError": ValueError,
            "OverflowError": OverflowError}[name]


@functools.lru_cache(maxsize=None)
def _model(name):
    c = LC.CASES[name]
    rows = LC.case_rows(name)
    tail = LC.tail_len(name)
    return rows, LM.analyze(rows, oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], tail,
                            c["C"] if tail else 0, sample_bits=c["ss"])


def _check_frames(want, data, offsets, status, what):
    assert len(offsets) == len(want) + 1
    for f, w in enumerate(want):
        got = bytes(data[int(offsets[f]):int(offsets[f + 1])])
        if isinstance(w, Exception):
            assert got == b"" and int(status[f]) & 0xFFFF == _STATUS[type(w).__name__], (what, f)
        else:
            assert int(status[f]) == 0 and got == w, (what, f, int(status[f]))


@pytest.mark.parametrize("name", sorted(LC.CASES))
@pytest.mark.parametrize("fallback", [False, True])
def test_frames_with_and_without_fallback(az, name, fallback):
    """flacmi_encode_host and flacmi_encode_pipeline (sub-batches of two frames) in the mode,
    against the model under the oracle frame writer, and composed with the fallback model."""
    c = LC.CASES[name]
    rows, mod = _model(name)
    tail = LC.tail_len(name)
    n_tail = c["C"] if tail else 0
    want, sub_kinds = FM.frames(rows, mod, c["C"], c["n"], tail, c["ss"], c["q"], 0, fallback=fallback)
    p = make_params(c["L"], c["q"], c["rmin"], c["rmax"], lpc_sign=True)
    kw = dict(sample_bits=c["ss"], channels=c["C"], sample_size=c["ss"], fallback=fallback)
    data, offsets, status = az.encode_frames(rows, p, c["n"], tail, n_tail, **kw)
    _check_frames(want, data, offsets, status, "encode_host")
    pdata, poff, pst, _ = az.encode_pipeline(rows, p, c["n"], tail, n_tail, units_per_batch=2 * c["C"], **kw)
    _check_frames(want, pdata, poff, pst, "encode_pipeline")
    if name == "silence" and fallback:
        assert sub_kinds[2:] == [FM.CONSTANT, FM.CONSTANT] and all(isinstance(w, bytes) for w in want)


def _correlated(rows):
    """The case's independent channels made a correlated pair: right = left + right / 32 on the
    even frames, left = right + left / 32 on the odd ones."""
    r = rows.astype(np.int64)
    for f in range(rows.shape[0] // 2):
        a, b = (2 * f, 2 * f + 1) if f % 2 == 0 else (2 * f + 1, 2 * f)
        r[b] = np.clip(r[a] + (r[b] >> 5), -32768, 32767)
    return r.astype(rows.dtype)


@pytest.mark.parametrize("fallback", [False, True])
def test_frames_with_stereo(az, fallback):
    """The stereo mode over the mode: left/right, mid and side are each analysed with the flag."""
    from flac_amd.decoder import decode
    name = "stereo16_q6"
    c = LC.CASES[name]
    rows = _correlated(LC.case_rows(name))
    tail = LC.tail_len(name)
    cands = LM.stereo_analyse(rows, oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], tail, c["ss"])
    want, codes, _ = SM.frames(rows, cands, c["n"], tail, c["q"], 0, fallback=fallback)
    p = make_params(c["L"], c["q"], c["rmin"], c["rmax"], lpc_sign=True)
    kw = dict(sample_bits=c["ss"], channels=2, sample_size=c["ss"], fallback=fallback, stereo=True)
    data, offsets, status = az.encode_frames(rows, p, c["n"], tail, 2, **kw)
    _check_frames(want, data, offsets, status, "encode_host")
    pdata, poff, pst, _ = az.encode_pipeline(rows, p, c["n"], tail, 2, units_per_batch=4, **kw)
    _check_frames(want, pdata, poff, pst, "encode_pipeline")
    assert all(isinstance(w, bytes) for w in want) and len(set(codes) - {SM.SC.L_R}) >= 1, codes
    header = FW.stream_header(c["rate"], c["ss"], 2, c["frames"], c["n"])
    _, _, _, _, dec = decode(header + bytes(data), check_crc=True)
    pcm = np.stack([np.concatenate([rows[2 * f + ch][:LC.block_len(name, f)] for f in range(LC.n_blocks(name))])
                    for ch in range(2)]).astype(np.int64)
    assert np.array_equal(np.asarray(list(dec), dtype=np.int64).reshape(-1, 2).T, pcm)


# ---------------------------------------------------------------------------------------
# off means off
# ---------------------------------------------------------------------------------------
def test_with_the_flag_clear_nothing_changes(az):
    """No keyword, lpc_sign=False and reserved[1] = 0 by hand: the oracle's default analysis
    (oracle.meta_mismatches: a pruned unit is one whose LPC candidates lose in the oracle), with
    pruned sentinels and tier words present as before, and the default frames."""
    a = oracle.synth_batch(0, 69, 256, 16, SEED)
    ora = oracle.analyze_batch(a, oracle.make_params(12, 5, 0, 5), 256, sample_bits=16, threads=4)
    by_hand = make_params(12, 5, 0, 5)
    by_hand.reserved[1] = 0
    outs = [az.analyze(a, p, 256, sample_bits=16)
            for p in (make_params(12, 5, 0, 5), make_params(12, 5, 0, 5, lpc_sign=False), by_hand)]
    for out in outs:
        for u in range(69):
            bad = oracle.meta_mismatches(out["meta"][u], ora["meta"][u])
            assert not bad, (u, bad)
            off, ln, k = int(ora["meta"]["res_offset"][u]), int(ora["meta"]["res_len"][u]), int(ora["meta"]["n_parts"][u])
            assert np.array_equal(out["residual"][u][off:off + ln].astype(np.uint64), ora["residual"][u][off:off + ln])
            assert np.array_equal(out["rice_params"][u][:k], ora["rice_params"][u][:k])
        assert np.array_equal(out["meta"], outs[0]["meta"])
    m = outs[0]["meta"]
    assert (m["lpc_order"] == abi.LPC_PRUNED).any() and (m["lpc_sum"][m["lpc_order"] == abi.LPC_PRUNED] == -1).all()
    assert m["lpc_tiers"].any()
    on = az.analyze(a, make_params(12, 5, 0, 5, lpc_sign=True), 256, sample_bits=16)["meta"]
    assert not (on["lpc_order"] == abi.LPC_PRUNED).any() and np.isin(on["lpc_tiers"], (0, LISTED)).all()
    # the frames of a fixture stream without the mode: the oracle's default frames
    name = "mono16"
    c = LC.CASES[name]
    rows = LC.case_rows(name)
    tail = LC.tail_len(name)
    dflt = oracle.analyze_batch(rows, oracle.make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], tail, 1,
                                sample_bits=16)
    want = FW.frames_from_analysis(rows, dflt, 1, c["n"], tail, 16, c["q"])
    data, offsets, status = az.encode_frames(rows, make_params(c["L"], c["q"], c["rmin"], c["rmax"]), c["n"], tail, 1,
                                             sample_bits=16, channels=1, sample_size=16)
    _check_frames(want, data, offsets, status, "flag clear")
