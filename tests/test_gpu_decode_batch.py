"""The batch decoder end to end (flac_amd.batch over flacmi_decode_batch_host and k_planar)
against the reference's verdict on each stream alone: tests/golden/decode_streams.json, every
(channels, sample size) group in one device call each, in several orders, under both values of
the FLACMI_DECODE_GENERIC knob; and tests/golden/decode_batch_streams.json, pairs of streams that
spell one frame across the boundary between them."""
import hashlib
import io
import json
import os
import random

import numpy as np
import pytest
import torch

import frame_index_cases as FI
from flac_amd import batch, decoder
from flac_amd.analysis import knob

pytestmark = pytest.mark.gpu
ALL = FI.load_cases()
CASES = [c for c in ALL if not c["open_exception"]]
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault((_c["channels"], _c["sample_size"]), []).append(_c)
MONO = GROUPS[(1, 16)]
EXC = {"AssertionError": AssertionError, "ValueError": ValueError, "EOFError": EOFError,
       "OverflowError": OverflowError}
PATTERN = {"int16": 0x5A5A, "int32": 0x5A5A5A5A, "float32": 7.5}
PAIRS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_batch_streams.json")


@pytest.fixture(scope="module", params=["fx", "generic"])
def path(request):
    with knob("FLACMI_DECODE_GENERIC", int(request.param == "generic")):
        yield request.param


def delivered_frames(case):
    """Frames whose samples the reference yielded (a frame decode_frame raised on was read too)."""
    k = total = 0
    for bs in case["block_sizes"]:
        if total + bs > case["n_samples"]:
            break
        k, total = k + 1, total + bs
    assert total == case["n_samples"]
    return k


def run_batch(cases, dtype="int32", **kw):
    """decode_batch into a tensor preset to a pattern, one 16-byte group longer than the longest
    stream; checks the padding of every row; -> (result, rows as numpy [N][C][T])"""
    g = 8 if dtype == "int16" else 4
    ch = cases[0]["channels"]
    longest = max(c["n_samples"] for c in cases)
    pitch = (longest + g - 1) // g * g + g
    out = torch.full((len(cases), ch, pitch), PATTERN[dtype], dtype=getattr(torch, dtype), device="cuda")
    r = batch.decode_batch([bytes.fromhex(c["hex"]) for c in cases], dtype=dtype, out=out, **kw)
    assert r.data is out and len(r.stats) == 1
    rows = out.cpu().numpy()
    for s, n in enumerate(r.lengths):
        assert not rows[s, :, n:].any(), f"{cases[s]['name']}: padding from {n} to {pitch} is not 0"
    return r, rows


def check_stream(case, r, rows, s):
    name = case["name"]
    n = r.lengths[s]
    assert n == case["n_samples"], name
    got = rows[s, :, :n].T  # [n][channels], as decode() yields them
    assert hashlib.sha256(got.astype("<i8").tobytes()).hexdigest() == case["samples_sha256"], name
    assert r.sample_rates[s] == case["sample_rate"], name
    exc = r.errors[s]
    if case["exception"] is None:
        assert exc is None, (name, repr(exc))
    else:
        assert type(exc) is EXC[case["exception"]], (name, repr(exc))
        assert f"frame {delivered_frames(case)}:" in str(exc), (name, str(exc))
        if "site" in case:
            assert case["site"] in str(exc), (name, str(exc))


@pytest.mark.parametrize("kind", sorted(GROUPS), ids=lambda k: f"{k[0]}ch{k[1]}bit")
def test_every_group_in_one_call(path, kind):
    cases = GROUPS[kind]
    r, rows = run_batch(cases)
    assert (r.channels, r.sample_size) == kind
    for s, c in enumerate(cases):
        check_stream(c, r, rows, s)
    assert r.stats[0]["streams"] == len(cases)
    assert r.stats[0]["frames"] == sum(delivered_frames(c) for c in cases)


def test_mono_group_holds_every_site_cut_and_alignment():
    names = {c["name"] for c in MONO}
    assert len(CASES) == 63 and len(MONO) == 54
    assert {f"e_cut_{k}" for k in list(range(1, 17)) + [148]} <= names
    assert {f"j_meta_{k}" for k in range(1, 20)} <= names
    assert sum(n.startswith("d_err_") for n in names) >= 14


@pytest.mark.parametrize("order", ["fixture", "reverse", "shuffle1", "shuffle2"])
def test_mono_group_in_other_orders(path, order):
    """Every cut stream and every failing stream with other neighbours."""
    cases = list(MONO)
    if order == "reverse":
        cases.reverse()
    elif order != "fixture":
        random.Random({"shuffle1": 20261021, "shuffle2": 7}[order]).shuffle(cases)
    r, rows = run_batch(cases)
    for s, c in enumerate(cases):
        check_stream(c, r, rows, s)


@pytest.mark.parametrize("kind", [k for k in sorted(GROUPS) if k[1] == 16], ids=lambda k: f"{k[0]}ch")
def test_int16_rows_are_the_pcm(path, kind):
    cases = GROUPS[kind]
    r, rows = run_batch(cases, dtype="int16")
    for s, c in enumerate(cases):
        pcm = np.ascontiguousarray(rows[s, :, :r.lengths[s]].T).astype("<i2").tobytes()
        assert len(pcm) == c["pcm_bytes"], c["name"]
        assert hashlib.sha256(pcm).hexdigest() == c["pcm_sha256"], c["name"]
        if c["pcm_exception"] is None:
            assert r.errors[s] is None, (c["name"], repr(r.errors[s]))
        else:
            assert type(r.errors[s]) is EXC[c["pcm_exception"]], (c["name"], repr(r.errors[s]))
    wide = [s for s, c in enumerate(cases) if c["name"] == "i_wide_frame"]
    for s in wide:  # stopped by the range finding, at the frame that holds the wide samples
        assert "frame 1:" in str(r.errors[s]) and "pcm_range" in str(r.errors[s])


@pytest.mark.parametrize("name", ["g_8bit", "g_24bit", "g_32bit", "h_20bit", "a_ref_192"])
def test_float32_is_the_scaled_int32(name):
    case = next(c for c in CASES if c["name"] == name)
    r, rows = run_batch([case])
    check_stream(case, r, rows, 0)
    rf, rowsf = run_batch([case], dtype="float32")
    assert rf.lengths == r.lengths and rowsf.dtype == np.float32
    want = rows.astype(np.float32) * np.float32(2.0 ** -(case["sample_size"] - 1))
    assert np.array_equal(rowsf.view(np.uint32), want.view(np.uint32))
    assert np.abs(rowsf).max() <= 1.0 and np.abs(rowsf).max() > 0


def test_batch_and_stream_calls_interleave_on_one_context():
    """A batch of one stream, the stream decoder on the same stream, the batch again: the batch
    leaves the context's buffers usable, and the other way round."""
    case = next(c for c in CASES if c["name"] == "b_false_sync")
    data = bytes.fromhex(case["hex"])
    r1, rows1 = run_batch([case])
    check_stream(case, r1, rows1, 0)
    sr, ss, ch, n, it = decoder.decode(io.BytesIO(data))
    got = np.array(list(it), dtype=np.int64).reshape(-1, ch)
    assert hashlib.sha256(got.astype("<i8").tobytes()).hexdigest() == case["samples_sha256"]
    r2, rows2 = run_batch([case])
    check_stream(case, r2, rows2, 0)
    assert np.array_equal(rows1, rows2) and np.array_equal(rows1[0, :, :len(got)].T, got)


def test_stream_that_fails_at_open_takes_no_part():
    bad = next(c for c in ALL if c["name"] == "j_meta_0")
    assert bad["open_exception"] == "ValueError"
    cases = [MONO[0], MONO[20]]
    streams = [bytes.fromhex(cases[0]["hex"]), bytes.fromhex(bad["hex"]), bytes.fromhex(cases[1]["hex"])]
    r = batch.decode_batch(streams)
    assert type(r.errors[1]) is ValueError and r.lengths[1] == 0 and r.sample_rates[1] is None
    assert r.data.shape[0] == 3 and not r.data[1].any().item()
    rows = r.data.cpu().numpy()
    check_stream(cases[0], r, rows, 0)
    check_stream(cases[1], r, rows, 2)


def test_mixed_channels_raise_in_decode_batch_and_group_in_decode_files():
    cases = [MONO[0], GROUPS[(2, 16)][0], GROUPS[(2, 24)][0], MONO[1]]
    streams = [bytes.fromhex(c["hex"]) for c in cases]
    with pytest.raises(ValueError, match="agree"):
        batch.decode_batch(streams)
    res = batch.decode_files(streams, dtype="int32")
    assert len(res) == len(cases)
    for c, r in zip(cases, res):
        assert (r.channels, r.sample_size, r.sample_rate, r.length) == (c["channels"], c["sample_size"],
                                                                        c["sample_rate"], c["n_samples"])
        got = r.data[:, :r.length].cpu().numpy().T
        assert hashlib.sha256(got.astype("<i8").tobytes()).hexdigest() == c["samples_sha256"], c["name"]


def test_a_frame_spelled_across_two_streams_belongs_to_neither(path):
    """[A_j, B_j] adjacent: A_j is a two-frame stream cut at byte j of its second frame and B_j's
    frame region begins with the rest of that frame.  Each must get the reference's verdict on
    it alone: A_j one frame of 192 samples and a silent end (a decoder without per-stream ends
    completes the frame from B_j's bytes and delivers 384)."""
    with open(PAIRS) as f:
        pairs = json.load(f)["pairs"]
    assert len(pairs) >= 11 and len({p["cut"] for p in pairs}) == len(pairs)
    cases = []
    for p in pairs:
        for key in ("a", "b"):
            cases.append(dict(p[key], name=f"{key}_cut_{p['cut']}"))
    r, rows = run_batch(cases)
    bad = []
    for s, c in enumerate(cases):
        try:
            check_stream(c, r, rows, s)
        except AssertionError as e:
            bad.append(f"{c['name']}: {r.lengths[s]} samples, {r.errors[s]!r} ({str(e)[:60]})")
    assert not bad, bad
    # and each pair alone in a call of its own, B first as well (the boundary at another address)
    for p in (pairs[0], pairs[len(pairs) // 2], pairs[-1]):
        for keys in (("a", "b"), ("b", "a")):
            two = [dict(p[k], name=f"{k}_cut_{p['cut']}") for k in keys]
            r, rows = run_batch(two)
            for s, c in enumerate(two):
                check_stream(c, r, rows, s)
