"""Golden fixture for the stereo-decorrelation mode (FLACMI_STEREO_BEST, include/flacmi.h),
written with the reference's own functions and read back by the reference's own decoder.

Run ONLY in the build container, where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_stereo_golden.py

It imports flac.encoder / flac.decoder from the reference checkout (read-only, nothing is copied;
make_fallback_golden.py sets up the path, FLAC_REFERENCE) and put_analysed / dry_run from that script.  The reference's encoder writes
Channels.L_R for every frame; its decoder reads all four assignments (decoder.py:111-122,
:431-451).  For every case of tests/stereo_cases.py and every frame (left, right) this script

  1. dry-runs the four candidate signals left, right, mid = (left + right) >> 1 and
     side = left - right with the reference's own per-channel steps (encoder.py:127-157) at
     widths ss, ss, ss, ss + 1: does the reference raise, and how many bits does it write;
  2. applies the rule of include/flacmi.h: without fallback a candidate the reference raises on
     is not eligible; with fallback a candidate that raises, or is larger than 8 + n w bits,
     counts (and is written) as CONSTANT (8 + w bits) or VERBATIM (8 + n w); the assignments
     L_R, L_S, S_R, M_S are walked in that order and the first with the smallest sum of its two
     sizes among those with both candidates eligible wins; none eligible: the frame fails;
  3. writes the frame with put_frame_header(FrameHeader(channels=Channels.X, ...)) and the
     subframe writers, the side subframe at ss + 1 bits;
  4. reads it back with get_frame + decode_frame, which must return left and right.

tests/golden/stereo_streams.json records per case the parameters (the samples are the recipes of
tests/stereo_cases.py, pinned by a SHA-256), per frame the four candidates' (exception, bits),
and per fallback setting the channel codes, the failing frames' exception and every frame's
bytes as hex (a frame above 4 KB: its length and SHA-256).  The verdicts the cases were designed
for (stereo_cases.EXPECT) are asserted, not merely recorded.  The GPU box never runs this script.
"""
import hashlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_fallback_golden as MF  # noqa: E402  (sets the paths of the reference, tests/ and oracle/)

from flac import decoder as D  # noqa: E402  (the reference, imported read-only)
from flac import encoder as E  # noqa: E402
from flac.binary import Get  # noqa: E402
from flac.common import (BlockingStrategy, Channels, FrameHeader, SubframeHeader,  # noqa: E402
                         SubframeTypeConstant)
from flac.crc import crc16  # noqa: E402

import stereo_cases as SC  # noqa: E402

CHANNELS = {SC.L_R: Channels.L_R, SC.L_S: Channels.L_S, SC.S_R: Channels.S_R, SC.M_S: Channels.M_S}
HEX_LIMIT = 4096


def rule_size(samples, n, w, raised, bits, fallback):
    """A candidate's size under the rule, or None when it is not eligible."""
    if not fallback:
        return None if raised else bits
    if raised is None and bits <= 8 + n * w:
        return bits
    return 8 + w if all(s == samples[0] for s in samples) else 8 + n * w


def put_candidate(put, samples, n, w, raised, bits, fallback, parameters):
    if not fallback or (raised is None and bits <= 8 + n * w):
        MF.put_analysed(put, samples, n, w, parameters)
    elif all(s == samples[0] for s in samples):
        E._put_subframe_header(put, SubframeHeader(type_=SubframeTypeConstant(), wasted_bits=0))
        put.uint(samples[0], w)
    else:
        header, subframe = E.encode_subframe_verbatim(samples)
        E._put_subframe_header(put, header)
        E._put_subframe_verbatim(put, subframe, w)


def frame(index, left, right, ss, parameters, dry, fallback):
    """-> (bytes, code), or (exception name, None) for a frame that fails."""
    n = len(left)
    cands = [[int(v) for v in x] for x in SC.candidates(left, right)]
    widths = (ss, ss, ss, ss + 1)
    sizes = [rule_size(cands[k], n, widths[k], dry[k][0], dry[k][1], fallback) for k in range(4)]
    pick = SC.choose(sizes)
    if pick is None:  # what encode() raises on the L_R frame: the first failing channel's exception
        return next(dry[k][0] for k in (0, 1) if dry[k][0]), None
    code, a, b = pick
    put = E.put_frame_header(FrameHeader(blocking_strategy=BlockingStrategy.Fixed, block_size=n, sample_rate=None,
                                         channels=CHANNELS[code], sample_size=None, coded_number=index))
    for k in (a, b):
        put_candidate(put, cands[k], n, widths[k], dry[k][0], dry[k][1], fallback, parameters)
    put.uint(0b0, put.bits_until_alignment)
    put.uint(crc16(put.buffer, E.CRC16_POLYNOMIAL), 16)
    data = put.buffer
    # the reference decoder returns the input
    get = Get(io.BytesIO(data))
    fr = D.get_frame(get, ss)
    assert fr.header.channels is CHANNELS[code]
    try:
        get.uint(1)
        raise AssertionError("bytes behind the frame")
    except EOFError:
        pass
    assert D.decode_frame(fr) == [cands[0], cands[1]], "the reference decoder returns other samples"
    return data, code


def build():
    out = {}
    for name, c in SC.CASES.items():
        rows, _ = SC.case_rows(name)
        ss = c["ss"]
        parameters = E.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                         lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])
        dry_all = []
        for f in range(c["frames"]):
            n = SC.frame_len(name, f)
            cands = SC.candidates(rows[2 * f, :n], rows[2 * f + 1, :n])
            dry_all.append([MF.dry_run([int(v) for v in x], n, w, parameters)
                            for x, w in zip(cands, (ss, ss, ss, ss + 1))])
        rec = {"params": {k: c[k] for k in ("n", "tail", "frames", "ss", "L", "q", "rmin", "rmax", "first", "seed")},
               "recipes": c["recipes"], "samples_sha256": SC.samples_sha256(name),
               "candidates": [[list(d) for d in dry] for dry in dry_all]}
        for mode in c["modes"]:
            codes, frames = [], []
            for f in range(c["frames"]):
                n = SC.frame_len(name, f)
                data, code = frame(c["first"] + f, rows[2 * f, :n], rows[2 * f + 1, :n], ss, parameters, dry_all[f],
                                   mode == "on")
                codes.append(code)
                if code is None:
                    frames.append({"raises": data})
                else:
                    frames.append(data.hex() if len(data) <= HEX_LIMIT else
                                  {"len": len(data), "sha256": hashlib.sha256(data).hexdigest()})
            assert codes == SC.EXPECT[(name, mode)], f"{name} {mode}: codes {codes}, expected {SC.EXPECT[(name, mode)]}"
            rec[mode] = {"codes": codes, "frames": frames}
            print(f"{name:10s} {mode:3s} codes {codes}", flush=True)
        out[name] = rec
    # the figures the cases were designed around
    st16 = out["st16"]["candidates"]
    bits = [b for _, b in st16[0]]  # the indep frame's four assignment sums
    assert [bits[a] + bits[b] for _, a, b in SC.ASSIGNMENTS] == [2325, 2748, 2609, 2828], st16[0]
    for name in ("st16", "st24"):
        cand = out[name]["candidates"]
        assert cand[4][1][0] == "ZeroDivisionError" and cand[5][3][0] is not None and cand[6][2][0] == "ValueError"
        assert out[name]["off"]["frames"][7] == {"raises": "ZeroDivisionError"}
    assert all(d[0] is not None for dry in out["st_tiny"]["candidates"] for d in dry)
    with open(os.path.join(HERE, "stereo_streams.json"), "w") as fh:
        json.dump({"generator": "tests/golden/make_stereo_golden.py",
                   "reference": "flac.encoder writers (encoder.py:127-157, :194-234, :323-328, :553-578) under "
                                "Channels.L_R / L_S / S_R / M_S, read back by flac.decoder (decoder.py:111-130, "
                                ":431-451)", "cases": out}, fh, separators=(",", ":"))


if __name__ == "__main__":
    build()
