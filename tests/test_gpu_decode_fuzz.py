"""The device frame parsers (k_decode_fx in its source-row and samples_out builds, k_decode,
k_frame_info) and the stream decoder over the seeded grammar fuzz of tests/decode_fuzz_cases.py:
frames no encoder of this project writes, features combined, packed back to back so that every
wave holds unlike frames at every byte alignment.

Expectations come from the plain model (tests/decode_model.py), which
tests/test_decode_fuzz_model.py ties to the reference decoder's recorded verdicts
(tests/golden/decode_fuzz.json, made by tests/golden/make_decode_fuzz_golden.py); the sample
hashes are compared with that fixture directly.  Nothing here reads the reference.

Every decoder test runs under the three settings of test_gpu_decode.py's fixture: k_decode_fx
first (the default), everything through k_decode, and k_decode_fx without its LPC pass.
"""
import functools
import hashlib

import numpy as np
import pytest

import decode_fuzz_cases as G
import decode_model as M
import info_cases as IC
from flac_amd import abi
from flac_amd.analysis import get_knob, knob
from test_decode_fuzz_model import NO_REFERENCE, PINNED_WIDE, load_fixture
from test_gpu_decode import az  # noqa: F401  (the module fixture: fx, generic, fx_nolpc)

pytestmark = pytest.mark.gpu
STATUS = {AssertionError: abi.STATUS_ASSERTION, ValueError: abi.STATUS_VALUE_ERROR, EOFError: abi.STATUS_EOF}
SENTINEL = 0xEE
TYPE_CODE = {name: k for k, name in enumerate(abi.SUB_TYPE_NAMES)}


def verify(site):
    return (abi.DSITE[site] << 16) | abi.STATUS_VERIFY


def up(n, m):
    return (max(n, 1) + m - 1) // m * m


@functools.lru_cache(maxsize=1)
def world():
    """The cases, the fixture rows by name, and for every valid frame the model's result."""
    cases = G.frames(G.SEED)
    fx = load_fixture()["by_name"]
    valid = [c for c in cases if c.truth is not None and c.name != PINNED_WIDE]
    model = {c.name: M.decode(c.data, c.channels, c.sample_size) for c in valid}
    assert all(isinstance(r, M.Decoded) for r in model.values())
    rows = {c.name: np.array(model[c.name].samples, dtype=np.int64) for c in valid}
    broken = [c for c in cases if c.truth is None]
    return cases, fx, valid, model, rows, broken


def groups(frames, seed):
    """{(channels, sample_size argument): frames in a seeded order}."""
    out = {}
    for c in frames:
        out.setdefault((c.channels, c.sample_size), []).append(c)
    rng = G.Rng(seed)
    for key in sorted(out):
        rng.shuffle(out[key])
    return {key: out[key] for key in sorted(out)}


def pack(frames, pad=0):
    """Frames back to back behind `pad` bytes: (stream as uint8, offsets with the end)."""
    buf, offs = bytearray(pad), []
    for c in frames:
        offs.append(len(buf))
        buf += c.data
    offs.append(len(buf))
    return np.frombuffer(bytes(buf), dtype=np.uint8), np.array(offs, dtype=np.int64)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return None if len(bad) == 0 else (tuple(int(v) for v in bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def device_hash(rows):
    return hashlib.sha256(rows.astype("<i8").tobytes()).hexdigest()


def check_decoded(name, out, f, channels, want_rows, fx):
    bs = want_rows.shape[1]
    got = out[f * channels:(f + 1) * channels, :bs].astype(np.int64)
    assert first_difference(got, want_rows) is None, (name, first_difference(got, want_rows))
    if name not in NO_REFERENCE and fx[name]["decoded_sha256"] is not None:
        assert device_hash(got) == fx[name]["decoded_sha256"], name


# ---- mixed batches ---------------------------------------------------------------------------

def test_mixed_batches_at_every_alignment(az):
    """Each (channels, sample size) group as one stream, its frames shuffled and back to back, with
    0 to 3 bytes in front: status 0, the model's samples element by element, the fixture's hash."""
    cases, fx, valid, model, rows, _ = world()
    for (ch, ss), frames in groups(valid, G.SEED + 2).items():
        stride = up(max(rows[c.name].shape[1] for c in frames), 4)
        for pad in range(4):
            data, offs = pack(frames, pad)
            out, st, mm = az.decode_frames(data, offs, ch, ss, first_frame=-1, out_stride=stride, check_crc=True)
            bad = [(frames[f].name, hex(int(s))) for f, s in enumerate(st) if s]
            assert not bad, (ch, ss, pad, bad[:5])
            for f, c in enumerate(frames):
                check_decoded(c.name, out, f, ch, rows[c.name], fx)


# ---- source rows -----------------------------------------------------------------------------

def source_batches(valid, rows, dtype, with_out):
    """Launches of frames that share (channels, sample size) and take one of two block sizes (the
    batch's block_len and tail_len): [(channels, ss, frames, block_len, tail_len, n_tail_units)]."""
    lim = np.iinfo(dtype)
    by = {}
    for c in valid:
        r = rows[c.name]
        code = c.truth["channel_code"]
        if r.min() < lim.min or r.max() > lim.max or (code >= 8 and not with_out):
            continue  # (decorrelated frames need samples_out: flacmi.h)
        if dtype == np.int16 and (code >= 8 or (c.truth["sample_size"] or c.sample_size) > 16):
            continue
        by.setdefault((c.channels, c.sample_size), {}).setdefault(r.shape[1], []).append(c)
    out = []
    for (ch, ss), sizes in sorted(by.items()):
        order = sorted(sizes, reverse=True)
        for k in range(0, len(order), 2):
            big, small = sizes[order[k]], sizes[order[k + 1]] if k + 1 < len(order) else []
            out.append((ch, ss, big + small, order[k], order[k + 1] if small else 0, len(small) * ch))
    return out


def expect_rows(frames, rows, ch, block_len, dtype):
    e = np.zeros((len(frames) * ch, up(block_len, 8)), dtype=dtype)  # 16-byte rows: the vector loads' condition
    for f, c in enumerate(frames):
        r = rows[c.name]
        e[f * ch:(f + 1) * ch, :r.shape[1]] = r
    return e


def pick_targets(batches, seed):
    """Eight frames by the seed, of different subframe types: {frame name: (channel, sample index)}."""
    kinds = {"CONSTANT": lambda s: s["type"] == "CONSTANT", "VERBATIM": lambda s: s["type"] == "VERBATIM",
             "FIXED0": lambda s: s["type"] == "FIXED" and s["order"] == 0,
             "FIXED2": lambda s: s["type"] == "FIXED" and s["order"] == 2,
             "FIXED4": lambda s: s["type"] == "FIXED" and s["order"] == 4,
             "LPC<=12": lambda s: s["type"] == "LPC" and s["order"] <= 12 and not s["wasted_flag"],
             "LPC>12": lambda s: s["type"] == "LPC" and s["order"] > 12,
             "wasted": lambda s: s["wasted_flag"] == 1}
    rng = G.Rng(seed)
    frames = [c for b in batches for c in b[2]]
    targets = {}
    for kind, test in kinds.items():
        pool = [(c, n) for c in frames if c.name not in targets for n, s in enumerate(c.truth["subframes"]) if test(s)]
        c, n = pool[rng.below(len(pool))]
        targets[c.name] = (n, rng.below(c.truth["block_size"]))
    assert len(targets) == 8
    return targets


@pytest.mark.parametrize("with_out", [True, False], ids=["samples_out", "compare_only"])
@pytest.mark.parametrize("dtype", [np.int32, np.int16], ids=["int32_rows", "int16_rows"])
def test_source_rows(az, dtype, with_out):
    """The builds that compare with source rows (int16 / int32, with and without samples_out):
    every frame reproduces its rows (status 0, no mismatch); with one expected sample changed
    in each of eight frames, exactly those report DSITE_SAMPLES and one mismatch."""
    cases, fx, valid, model, rows, _ = world()
    batches = source_batches(valid, rows, dtype, with_out)
    assert sum(len(b[2]) for b in batches) >= (150 if dtype == np.int16 else 300)
    targets = pick_targets(batches, G.SEED + 3 + int(with_out))
    hit = set()
    for ch, ss, frames, block_len, tail_len, n_tail in batches:
        data, offs = pack(frames, 1)
        e = expect_rows(frames, rows, ch, block_len, dtype)
        kw = dict(first_frame=-1, block_len=block_len, tail_len=tail_len, n_tail_units=n_tail,
                  out_stride=up(block_len, 4), samples_out=with_out)
        out, st, mm = az.decode_frames(data, offs, ch, ss, expect=e, **kw)
        assert not st.any() and not mm.any(), (ch, ss, block_len, [(frames[f].name, hex(int(s))) for f, s in enumerate(st) if s][:5])
        if with_out:
            for f, c in enumerate(frames):
                check_decoded(c.name, out, f, ch, rows[c.name], fx)
        changed = [f for f, c in enumerate(frames) if c.name in targets]
        if not changed:
            continue
        for f in changed:
            n, i = targets[frames[f].name]
            e[f * ch + n, i] ^= 1
            hit.add(frames[f].name)
        _, st, mm = az.decode_frames(data, offs, ch, ss, expect=e, **kw)
        for f, c in enumerate(frames):
            if f in changed:
                assert (int(st[f]), int(mm[f])) == (verify("samples"), 1), (c.name, hex(int(st[f])), int(mm[f]))
            else:
                assert (int(st[f]), int(mm[f])) == (0, 0), (c.name, hex(int(st[f])), int(mm[f]))
    assert hit == set(targets)


# ---- ends ------------------------------------------------------------------------------------

def test_frame_ends(az):
    """flacmi_decode_frames_end_device with every frame proposed to end at the stream's end:
    frame_end is where the reference's reader stands after get_frame, the status DSITE_FRAME_END
    and nothing else (0 for the stream's last frame, which does end there)."""
    cases, fx, valid, model, rows, _ = world()
    for (ch, ss), frames in groups(valid, G.SEED + 2).items():
        data, offs = pack(frames, 3)
        total = int(offs[-1])
        # frame 2k is frame k to the stream's end; the odd entries start at the end (nothing to read)
        inter = np.array([v for o in offs[:-1] for v in (int(o), total)], dtype=np.int64)
        stride = up(max(rows[c.name].shape[1] for c in frames), 4)
        out, st, mm, end = az.decode_frames(data, inter, ch, ss, first_frame=-1, out_stride=stride, frame_end=True)
        for k, c in enumerate(frames):
            want_end = int(offs[k]) + (fx[c.name]["end"] if c.name not in NO_REFERENCE else len(c.data))
            assert want_end == int(offs[k + 1])
            assert int(end[2 * k]) == want_end, (c.name, int(end[2 * k]), want_end)
            assert int(st[2 * k]) == (0 if want_end == total else verify("frame_end")), (c.name, hex(int(st[2 * k])))
            check_decoded(c.name, out, 2 * k, ch, rows[c.name], fx)


# ---- mutated and cut frames ------------------------------------------------------------------

def expected_word(res, channels, proposed_end):
    """(status word, frame_end, samples restored) the decoder owes for a model result: the first
    reference exception wins over any verifier finding, among findings the first found is kept."""
    rep = res.report
    found = []
    if "sample_size" in rep:  # the header parsed: its CRC-8, then the channel count, before any subframe
        if rep["crc8"] != rep["crc8_computed"]:
            found.append(verify("crc8"))
        code = rep["channel_code"]
        if (channels if code == 1 else code + 1 if code <= 7 else 2) != channels:
            return (found + [verify("channels")])[0], -1, False
    if isinstance(res, M.Failed):
        return (abi.DSITE[res.site] << 16) | STATUS[res.exception], -1, False
    if res.end != proposed_end:
        found.append(verify("frame_end"))
    if rep["crc16"] != rep["crc16_computed"]:
        found.append(verify("crc16"))
    return (found + [0])[0], res.end, True


def run_both(az, *args, **kw):
    """decode_frames through k_decode_fx first and through k_decode alone: they agree on every
    status word, mismatch count and frame end; returns the run of the fixture's own setting."""
    res = {}
    for gen in (0, 1):
        with knob("FLACMI_DECODE_GENERIC", gen):
            res[gen] = az.decode_frames(*args, **kw)
    assert np.array_equal(res[0][1], res[1][1]), "fx and generic disagree on a status word"
    assert np.array_equal(res[0][2], res[1][2]), "fx and generic disagree on a mismatch count"
    assert np.array_equal(res[0][3], res[1][3]), "fx and generic disagree on a frame end"
    return res[get_knob("FLACMI_DECODE_GENERIC")]


def check_broken(c, res, st, end, out, f, fx, proposed_end, alone):
    word, want_end, restored = expected_word(res, c.channels, proposed_end)
    assert int(st) == word, (c.name, hex(int(st)), hex(word), getattr(res, "site", None))
    assert int(end) == want_end, (c.name, int(end), want_end)
    # the reference reads an L_R frame as two subframes: its verdict is this reading's otherwise
    same_reading = c.channels == 2 or res.report.get("channel_code") != 1
    if alone and same_reading and isinstance(res, M.Failed) and int(st) & 0xFFFF != abi.STATUS_VERIFY:
        assert abi.STATUS_EXCEPTION[int(st) & 0xFFFF].__name__ == fx[c.name]["exception"], c.name
    if restored:
        got = out[f * c.channels:(f + 1) * c.channels, :res.report["block_size"]].astype(np.int64)
        want = np.array(res.samples, dtype=np.int64)
        assert first_difference(got, want) is None, (c.name, first_difference(got, want))
        if alone and same_reading and fx[c.name]["exception"] is None and fx[c.name]["decoded_sha256"]:
            assert device_hash(got) == fx[c.name]["decoded_sha256"], c.name
            assert int(end) == fx[c.name]["end"], c.name


def test_mutated_and_cut_frames_alone(az):
    """Each damaged frame in a buffer of its own: the reference's exception class at the model's
    statement, or the reference's samples and end; k_decode_fx and k_decode agree throughout."""
    cases, fx, valid, model, rows, broken = world()
    seen = 0
    for c in broken:
        try:
            res = M.decode(c.data, c.channels, c.sample_size)
        except M.OutOfDomain:
            continue
        data, offs = pack([c])
        stride = up(res.report["block_size"], 4)
        out, st, mm, end = run_both(az, data, offs, c.channels, c.sample_size, first_frame=-1, out_stride=stride,
                                    frame_end=True)
        check_broken(c, res, st[0], end[0], out, 0, fx, len(c.data), True)
        seen += 1
    assert seen >= 0.9 * len(broken)


def test_mutated_and_cut_frames_in_one_stream(az):
    """The damaged frames of a (channels, sample size) group back to back: a frame that runs off
    its own bytes reads on into the next one, as the model does at the same offset."""
    cases, fx, valid, model, rows, broken = world()
    for (ch, ss), frames in groups(broken, G.SEED + 4).items():
        data, offs = pack(frames, 2)
        stream = data.tobytes()
        results = []
        for k, c in enumerate(frames):
            try:
                results.append(M.decode(stream, ch, ss, offset=int(offs[k])))
            except M.OutOfDomain:
                results.append(None)
        stride = up(max([r.report["block_size"] for r in results if r is not None] + [4]), 4)
        out, st, mm, end = run_both(az, data, offs, ch, ss, first_frame=-1, out_stride=stride, frame_end=True)
        for k, (c, res) in enumerate(zip(frames, results)):
            if res is None:
                continue
            check_broken(c, res, st[k], end[k], out, k, fx, int(offs[k + 1]), False)


# ---- the two pinned divergences ---------------------------------------------------------------

def test_wide_side_channel_is_refused_not_miscoded(az):
    """L_S at 32 bits with a side channel that leaves int32 (the reference restores it with
    unbounded integers): the documented choice is a verifier status, DSITE_SIDE_RANGE, never
    status 0 with other samples than the reference's."""
    cases, fx, *_ = world()
    c = next(c for c in cases if c.name == PINNED_WIDE)
    data, offs = pack([c])
    out, st, mm = az.decode_frames(data, offs, 2, 32, first_frame=-1, out_stride=16)
    assert int(st[0]) == verify("side_range"), hex(int(st[0]))
    # the report is of the parse alone and reads the frame to its end
    fi, si, pp = az.frame_info(c.data, [0], 2, 32, sentinel=SENTINEL)
    assert (int(fi[0]["status"]), int(fi[0]["end"])) == (0, len(c.data)) and int(si[0][1]["sample_bits"]) == 33


def test_fixed_order_0_with_no_width_left(az):
    """A FIXED order-0 subframe whose wasted-bits count reaches the sample size reads no sample
    at the (non-positive) width: the reference decodes it, and so do both decoders."""
    cases, fx, valid, model, rows, _ = world()
    c = next(c for c in valid if c.name == "fixed0_wasted_ge_ss")
    assert c.truth["subframes"][0]["sample_bits"] <= 0 and fx[c.name]["exception"] is None
    data, offs = pack([c], 1)
    out, st, mm = az.decode_frames(data, offs, c.channels, c.sample_size, first_frame=-1, out_stride=32)
    assert int(st[0]) == 0, hex(int(st[0]))
    check_decoded(c.name, out, 0, 1, rows[c.name], fx)


# ---- k_frame_info ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def az_info():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def check_info_subframe(want, rec, parts, part_stride, where):
    for k in ("bit_offset", "bits", "order", "wasted_bits", "sample_bits", "precision", "shift", "coding_method",
              "partition_order", "residual_bits", "abs_sum"):
        assert int(rec[k]) == want[k], (where, k, int(rec[k]), want[k])
    assert int(rec["type"]) == TYPE_CODE[want["type"]], where
    assert int(rec["constant_value"]) == want["constant"], where
    assert rec["coefficients"].tolist() == want["coefficients"] + [0] * (32 - len(want["coefficients"])), where
    assert int(rec["escaped_partitions"]) == sum(k == "escape" for k, _ in want["partitions"]), where
    stored = min(len(want["partitions"]), part_stride)
    assert int(rec["partitions_stored"]) == stored, where
    assert parts[:stored].tolist() == [(abi.PART_ESCAPE | v) if k == "escape" else v for k, v in want["partitions"][:stored]], where
    assert (parts[stored:] == SENTINEL).all(), where  # counted, not stored: the sentinel stays
    assert int(rec["reserved0"]) == 0 and int(rec["reserved1"]) == 0, where


@pytest.mark.parametrize("part_stride,grid", [(64, 0), (4, 0), (64, 1)], ids=["stride64", "stride4", "grid1"])
def test_frame_info_on_mixed_streams(az_info, part_stride, grid):
    """Every field of every frame and subframe record and the part_params bytes against what the
    generator wrote; with part_stride 4 the partitions past the stride are counted, not stored;
    once with a grid of one workgroup (the grid-stride loop over unlike frames)."""
    cases, fx, valid, model, rows, _ = world()
    with knob("FLACMI_INFO_GRID", grid):
        for (ch, ss), frames in groups(valid, G.SEED + 5).items():
            data, offs = pack(frames, 1 + part_stride % 3)
            fi, si, pp = az_info.frame_info(data.tobytes(), offs[:-1], ch, ss, part_stride=part_stride, sentinel=SENTINEL)
            for f, c in enumerate(frames):
                t, rec, base = c.truth, fi[f], int(offs[f])
                for k in ("block_size", "blocking_strategy", "sample_rate", "sample_size", "channel_code", "n_subframes",
                          "header_bytes", "padding_bits"):
                    assert int(rec[k]) == t[k], (c.name, k, int(rec[k]), t[k])
                assert int(rec["status"]) == 0, (c.name, hex(int(rec["status"])))
                assert (int(rec["offset"]), int(rec["end"])) == (base, base + t["end"]), c.name
                assert int(rec["coded_number"]) == t["number"], c.name
                assert (int(rec["crc8_stored"]), int(rec["crc8_computed"])) == (t["crc8"], t["crc8_computed"]), c.name
                assert (int(rec["crc16_stored"]), int(rec["crc16_computed"])) == (t["crc16"], t["crc16_computed"]), c.name
                assert int(rec["reserved0"]) == 0, c.name
                for n, s in enumerate(t["subframes"]):
                    check_info_subframe(s, si[f][n], pp[f][n], part_stride, f"{c.name} subframe {n}")


def test_frame_info_on_damaged_frames(az_info):
    """The status word and the end of every mutated and cut frame in the mixed streams (a negative
    shift is no exception of get_frame: status 0 and the frame's end)."""
    cases, fx, valid, model, rows, broken = world()
    for (ch, ss), frames in groups(broken, G.SEED + 4).items():
        data, offs = pack(frames, 2)
        stream = data.tobytes()
        fi, si, pp = az_info.frame_info(stream, offs[:-1], ch, ss, sentinel=SENTINEL)
        for k, c in enumerate(frames):
            try:
                res = M.decode(stream, ch, ss, offset=int(offs[k]), domain=False)
            except M.OutOfDomain:
                continue
            if isinstance(res, M.Failed) and res.site != "neg_shift":
                want = ((abi.DSITE[res.site] << 16) | STATUS[res.exception], -1)
            else:
                want = (0, res.end)
            assert (int(fi[k]["status"]), int(fi[k]["end"])) == want, (c.name, hex(int(fi[k]["status"])), int(fi[k]["end"]), want)


# ---- stream decoder --------------------------------------------------------------------------

def test_stream_decoder_walks_the_fuzz(az):
    """The one-channel 16-bit group behind a STREAMINFO through flac_amd.decoder.decode, whole and
    in chunks that frames straddle: the model's samples in order.  The payloads hold false syncs
    (a whole header with a good CRC-8 inside a frame), which the walk must pass over."""
    from flac_amd import decoder
    cases, fx, valid, model, rows, _ = world()
    frames = groups(valid, G.SEED + 6)[(1, 16)]
    assert any(c.name == "verbatim_false_sync" for c in frames)
    head = IC.stream_header(1, 16, max_bs=max(c.truth["block_size"] for c in frames))
    stream = head + b"".join(c.data for c in frames)
    starts = set(np.cumsum([len(head)] + [len(c.data) for c in frames]).tolist())
    table, n = az.index_frames(stream, first_byte=len(head))
    inside = [int(o) for o in table["offset"] if int(o) not in starts]
    assert n == len(table) and inside, "no false sync inside a frame: the walk's skipping is not exercised"
    want = np.concatenate([rows[c.name][0] for c in frames])
    for chunk in (decoder.DEFAULT_CHUNK_BYTES, 1500):
        stats = []
        sr, ss, ch, _, it = decoder.decode(stream, chunk_bytes=chunk, stats=stats)
        got = np.array(list(it), dtype=np.int64).reshape(-1)
        assert (ss, ch) == (16, 1) and len(got) == len(want), (chunk, len(got), len(want))
        assert first_difference(got, want) is None, (chunk, first_difference(got, want))
        assert chunk >= len(stream) or len(stats) > 2
