"""Golden fixture for the fallback-subframe mode (FLACMI_FRAME_FALLBACK, include/flacmi.h),
written with the reference's own functions and read back by the reference's own decoder.

Run ONLY in the build container, where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fallback_golden.py

It imports flac.encoder / flac.decoder from /root/reference (read-only, nothing is copied).
For every case of tests/fallback_cases.py it restates the frame loop of encode()
(encoder.py:87-165) with the mode's rule in place of the TODO at :104-125.  Per channel:

  1. a dry run of the reference's own steps (:127-157) into a Put of its own: does the
     reference raise (ZeroDivisionError, AssertionError, ValueError, OverflowError), and how many
     bits does it write;
  2. raising, or more than 8 + n * sample_size bits: the unit is escaped, and written with
     _put_subframe_header(SubframeTypeConstant()) + put.uint(v, sample_size) when its samples are
     all equal, else with encode_subframe_verbatim + _put_subframe_header + _put_subframe_verbatim
     (:323-328, :553-578), the writers the reference never calls;
  3. otherwise the reference's steps again, into the frame.

The frame's bytes are then read by the reference decoder (get_frame_header, get_subframe,
decode_subframe; decoder.py:111-130, :431-498), which must return the input samples.  For
channel counts other than 2 the frame holds `channels` subframes under the L_R header
encode() always writes (the documented choice of include/flacmi.h), so get_frame's loop is
restated over that count.  The GPU box never runs this script.

tests/golden/fallback_streams.json records per case the parameters (the samples are the
recipes of tests/fallback_cases.py, pinned by a SHA-256), the sub-kind of every unit, whether
the reference raised on it, its dry-run bit count, and each frame's bytes as hex (a frame
above 4 KB: its length and SHA-256).
"""
import hashlib
import io
import json
import os
import sys

REF = os.environ.get("FLAC_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"),
          os.path.dirname(os.path.dirname(HERE)), REF):
    sys.path.insert(0, p)

from flac import decoder as D  # noqa: E402  (the reference, imported read-only)
from flac import encoder as E  # noqa: E402
from flac.binary import Get, Put  # noqa: E402
from flac.common import (BlockingStrategy, Channels, FrameHeader, SubframeHeader,  # noqa: E402
                         SubframeTypeConstant)
from flac.crc import crc16  # noqa: E402

import fallback_cases as FC  # noqa: E402

RAISES = (ZeroDivisionError, AssertionError, ValueError, OverflowError)
HEX_LIMIT = 4096


def put_analysed(put, samples, block_size, sample_size, parameters):
    """encode()'s steps 1-2 for one channel (encoder.py:127-157), verbatim."""
    fixed_header, fixed_subframe = E.encode_subframe_fixed(samples)
    lpc_header, lpc_subframe = E.encode_subframe_lpc(samples, parameters.lpc_order, parameters.qlp_precision)
    fixed_size = sum(abs(x) for x in fixed_subframe.residual)
    lpc_size = sum(abs(x) for x in lpc_subframe.residual)
    if fixed_size < lpc_size:
        E._put_subframe_header(put, fixed_header)
        E._put_subframe_fixed(put, fixed_subframe, block_size, sample_size, parameters.rice_partition_order)
    elif lpc_size < fixed_size:
        E._put_subframe_header(put, lpc_header)
        E._put_subframe_lpc(put, lpc_subframe, block_size, sample_size, parameters.rice_partition_order)
    else:
        assert False


def dry_run(samples, block_size, sample_size, parameters):
    """(exception class name or None, bits written or None)"""
    put = Put()
    try:
        put_analysed(put, samples, block_size, sample_size, parameters)
    except RAISES as e:
        return type(e).__name__, None
    pad = put.bits_until_alignment
    put.uint(0, pad)
    return None, 8 * len(put.buffer) - pad


def frame(index, channels, sample_size, parameters):
    """One frame of the mode from per-channel sample lists -> (bytes, per channel (kind, raised, bits))."""
    n = len(channels[0])
    put = E.put_frame_header(FrameHeader(blocking_strategy=BlockingStrategy.Fixed, block_size=n, sample_rate=None,
                                         channels=Channels.L_R, sample_size=None, coded_number=index))
    units = []
    for samples in channels:
        raised, bits = dry_run(samples, n, sample_size, parameters)
        if raised is None and bits <= 8 + n * sample_size:
            put_analysed(put, samples, n, sample_size, parameters)
            kind = 0
        elif all(s == samples[0] for s in samples):
            E._put_subframe_header(put, SubframeHeader(type_=SubframeTypeConstant(), wasted_bits=0))
            put.uint(samples[0], sample_size)
            kind = FC.CONSTANT
        else:
            header, subframe = E.encode_subframe_verbatim(samples)
            E._put_subframe_header(put, header)
            E._put_subframe_verbatim(put, subframe, sample_size)
            kind = FC.VERBATIM
        units.append((kind, raised, bits))
    put.uint(0b0, put.bits_until_alignment)
    put.uint(crc16(put.buffer, E.CRC16_POLYNOMIAL), 16)
    return put.buffer, units


def decode(data, n_channels, sample_size):
    """The reference decoder on one frame holding n_channels subframes (get_frame, decoder.py:111-130,
    over that count) -> per-channel samples."""
    get = Get(io.BytesIO(data))
    header = D.get_frame_header(get)
    assert header.channels is Channels.L_R and header.sample_size is None
    subframes = [D.get_subframe(get, header.block_size, sample_size) for _ in range(n_channels)]
    if get.is_aligned is False:
        assert get.uint(get.bits_until_alignment) == 0
    get.uint(16)
    try:
        get.uint(1)
        raise AssertionError("bytes behind the frame")
    except EOFError:
        pass
    return [D.decode_subframe(s) for s in subframes]


def build():
    out = {}
    for name, c in FC.CASES.items():
        rows, _ = FC.case_rows(name)
        lens = FC.unit_lens(name)
        C, ss = c["C"], c["ss"]
        parameters = E.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                         lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])
        frames, kinds, raised, bits = [], [], [], []
        for f in range(c["frames"]):
            chans = [[int(v) for v in rows[u][: lens[u]]] for u in range(f * C, (f + 1) * C)]
            data, units = frame(c["first"] + f, chans, ss, parameters)
            assert decode(data, C, ss) == chans, f"{name} frame {f}: the reference decoder returns other samples"
            for k, r, b in units:
                kinds.append(k)
                raised.append(r)
                bits.append(b)
            frames.append(data.hex() if len(data) <= HEX_LIMIT else
                          {"len": len(data), "sha256": hashlib.sha256(data).hexdigest()})
        assert kinds == c["expect"], f"{name}: sub-kinds {kinds}, the case expects {c['expect']}"
        for u, k in enumerate(kinds):  # a constant block always fails in the reference
            if k == FC.CONSTANT:
                assert raised[u] is not None, f"{name} unit {u}: constant, and the reference writes it"
        if name == "equal":
            assert bits == [8 + c["n"] * ss], bits
        out[name] = {"params": {k: c[k] for k in ("C", "n", "tail", "frames", "ss", "L", "q", "rmin", "rmax", "first",
                                                  "seed")},
                     "samples_sha256": hashlib.sha256(rows.astype("<i8").tobytes()).hexdigest(),
                     "kinds": kinds, "raised": raised, "bits": bits, "frames": frames}
        print(f"{name:12s} kinds {kinds} raised {sorted({r for r in raised if r})}", flush=True)
    with open(os.path.join(HERE, "fallback_streams.json"), "w") as fh:
        json.dump({"generator": "tests/golden/make_fallback_golden.py",
                   "reference": "flac.encoder writers (encoder.py:127-157, :323-328, :553-578), read back by "
                                "flac.decoder (decoder.py:111-130, :431-498)", "cases": out}, fh, separators=(",", ":"))


if __name__ == "__main__":
    build()
