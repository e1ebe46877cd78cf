"""Golden fixture for wasted-bits subframes (FLACMI_DECODE_WASTED_SPEC and the wasted-bits rule of
flacmi_wasted_rows_device, include/flacmi.h), written with the reference's own writers and read
back by the reference's own decoder.

Run ONLY in the build container, where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_wasted_golden.py

It imports flac.encoder / flac.decoder from /root/reference (read-only, nothing is copied).  The
reference anticipates wasted bits (SubframeHeader.wasted_bits, common.py:309) and has none of it:
every encoder path writes 0 (encoder.py:326, :556), get_wasted_bits (decoder.py:346-355) returns
the zeros before the terminating one, which is k - 1 for k wasted bits, and decode_subframe never
shifts the samples back.

Writing.  For every case of tests/wasted_cases.py the frame loop of encode() (encoder.py:87-165)
is restated as make_fallback_golden.py restates it.  Per channel, with w the unit's wasted bits
(tests/wasted_model.py) and y = x >> w: the reference's own steps (encode_subframe_fixed,
encode_subframe_lpc, the comparison, _put_subframe_fixed / _put_subframe_lpc) on y at sample size
ss - w, with _put_subframe_header replaced for the run by its own three statements (:554-556) of
which only the last, put.uint(0b0, 1), becomes the wasted code: 0 for w == 0, else 1, w - 1 zeros
and a 1.  In a case marked `fallback` a unit the reference raises on, or writes in more than
8 + w + n (ss - w) bits, is written as CONSTANT (y[0] at ss - w bits) when all its samples are
equal, else as VERBATIM at ss - w bits; in every other case the script asserts that the reference
writes every unit without raising.

Reading.  Each frame, alone, is read by make_info_golden.py's read_frame (get_frame's loop
restated over the stream's channel count, noting what get_subframe drops) and decode_subframe,
twice:
  spec     with exactly two corrections applied by monkeypatching: get_wasted_bits returns its
           count + 1, and every sample of the subframe is << wasted.  It must return the input
           samples of every case (asserted), and its account gives each subframe's w and width.
  default  the reference as it is: per frame the samples it returns (a SHA-256 and the first 8 of
           every channel), or the class of the exception it raises, and its account of the frame.

tests/golden/wasted_streams.json records per case the parameters, the samples' SHA-256, per unit
w, the sub-kind (0 analysed, 1 CONSTANT, 2 VERBATIM), the subframe's type, order and bit count,
each frame's bytes as hex (a frame above 4 KB: its length and SHA-256) and the two readings; for a
case marked `twin` also the subframes the reference writes for the unshifted samples x >> w as a
stream of ss - w bits (each must be exactly w bits shorter: the CPU test).
"""
import hashlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_info_golden as MI  # noqa: E402  (puts the reference on sys.path; wraps the decoder's readers with notes)
import make_fallback_golden as MF  # noqa: E402  (put_analysed, dry_run: encode()'s steps for one channel)
from flac import decoder as D  # noqa: E402  (the reference, imported read-only)
from flac import encoder as E  # noqa: E402
from flac.binary import Get  # noqa: E402
from flac.common import (BlockingStrategy, Channels, FrameHeader, SubframeHeader,  # noqa: E402
                         SubframeTypeConstant)
from flac.crc import crc16  # noqa: E402

import wasted_cases as WC  # noqa: E402
import wasted_model as WM  # noqa: E402

HEX_LIMIT = 4096
W = 0  # the wasted bits of the subframe being written


def put_subframe_header(put, header):
    """encoder.py:553-556 with the wasted code in place of its last statement."""
    put.uint(0b0, 1)
    E._put_subframe_type(put, header.type_)
    if W == 0:
        put.uint(0b0, 1)
    else:
        put.uint(0b1, 1)
        if W > 1:
            put.uint(0, W - 1)
        put.uint(0b1, 1)


E._put_subframe_header = put_subframe_header
_wasted_ref = D.get_wasted_bits


def _wasted_spec(get):
    b = get.uint(1)
    if b == 0:
        return 0
    count = 0
    while get.uint(1) == 0:
        count += 1
    return count + 1


def frame(index, channels, sample_size, parameters, fallback):
    """One frame from per-channel sample lists -> (bytes, per channel (w, kind, raised))."""
    global W
    n = len(channels[0])
    put = E.put_frame_header(FrameHeader(blocking_strategy=BlockingStrategy.Fixed, block_size=n, sample_rate=None,
                                         channels=Channels.L_R, sample_size=None, coded_number=index))
    units = []
    for samples in channels:
        W = WM.wasted_of(samples, sample_size)
        y = [s >> W for s in samples]
        b = sample_size - W
        raised, bits = MF.dry_run(y, n, b, parameters)
        if raised is None and (not fallback or bits <= 8 + W + n * b):
            MF.put_analysed(put, y, n, b, parameters)
            kind = 0
        else:
            assert fallback, f"the reference raises {raised} on a unit of a case not marked fallback"
            if all(s == y[0] for s in y):
                E._put_subframe_header(put, SubframeHeader(type_=SubframeTypeConstant(), wasted_bits=W))
                put.uint(y[0], b)
                kind = WC.FC.CONSTANT
            else:
                header, subframe = E.encode_subframe_verbatim(y)
                E._put_subframe_header(put, header)
                E._put_subframe_verbatim(put, subframe, b)
                kind = WC.FC.VERBATIM
        units.append((W, kind, raised))
    W = 0
    put.uint(0b0, put.bits_until_alignment)
    put.uint(crc16(put.buffer, E.CRC16_POLYNOMIAL), 16)
    return put.buffer, units


def read(data, n_channels, sample_size, spec):
    """(account of the frame, per-channel samples or None, exception class or None)"""
    D.get_wasted_bits = _wasted_spec if spec else _wasted_ref
    try:
        bio = io.BytesIO(data)
        get = Get(bio)
        rec, objs = MI.read_frame(get, bio, data, sample_size, n_channels)
        if rec["exception"]:
            return rec, None, rec["exception"]["class"]
        try:
            samples = [[s << (notes.wasted if spec else 0) for s in D.decode_subframe(sub)] for sub, notes in objs["subs"]]
        except Exception as e:  # noqa: BLE001  -- the reference's exception class is the fixture
            return rec, None, type(e).__name__
        return rec, samples, None
    finally:
        D.get_wasted_bits = _wasted_ref


def account(rec):
    return [{k: s[k] for k in ("type", "order", "wasted_bits", "sample_bits", "bit_offset", "bits")}
            for s in rec["subframes"]]


def build():
    out = {}
    types = set()
    for name, c in WC.CASES.items():
        rows, _ = WC.case_rows(name)
        lens = WC.unit_lens(name)
        C, ss = c["C"], c["ss"]
        parameters = E.EncoderParameters(block_size=c["n"], rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                         lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])
        frames, ws, kinds, raised, subs, default = [], [], [], [], [], []
        for f in range(c["frames"]):
            chans = [[int(v) for v in rows[u][: lens[u]]] for u in range(f * C, (f + 1) * C)]
            data, units = frame(c["first"] + f, chans, ss, parameters, c["fallback"])
            rec, samples, exc = read(data, C, ss, True)
            assert exc is None and samples == chans, f"{name} frame {f}: the corrected reference decoder returns other samples"
            assert rec["end"] == len(data)
            acc = account(rec)
            assert [a["wasted_bits"] for a in acc] == [u[0] for u in units]
            assert [a["sample_bits"] for a in acc] == [ss - u[0] for u in units]
            subs += acc
            for w, k, r in units:
                ws.append(w)
                kinds.append(k)
                raised.append(r)
            types |= {a["type"] for a in acc}
            rec0, samples0, exc0 = read(data, C, ss, False)
            d = {"exception": exc0, "parse_exception": rec0["exception"]["class"] if rec0["exception"] else None,
                 "end": rec0["end"], "subframes": account(rec0)}
            if samples0 is not None:
                d["head"] = [ch[:8] for ch in samples0]
                d["sha256"] = hashlib.sha256(b"".join(int(s).to_bytes(8, "little", signed=True)
                                                      for ch in samples0 for s in ch)).hexdigest()
                if all(w == 0 for w in ws[-C:]):
                    assert samples0 == chans
            default.append(d)
            frames.append(data.hex() if len(data) <= HEX_LIMIT else
                          {"len": len(data), "sha256": hashlib.sha256(data).hexdigest()})
        twin = None
        if c["twin"]:  # the same samples unshifted, as a stream of ss - twin bits
            twin = []
            for f in range(c["frames"]):
                chans = [[int(v) >> c["twin"] for v in rows[u][: lens[u]]] for u in range(f * C, (f + 1) * C)]
                data, units = frame(c["first"] + f, chans, ss - c["twin"], parameters, False)
                rec, samples, exc = read(data, C, ss - c["twin"], True)
                assert exc is None and samples == chans and all(u[0] == 0 for u in units)
                twin += account(rec)
        assert ws == WC.wasted(name), f"{name}: wasted bits {ws}, the case says {WC.wasted(name)}"
        if not c["fallback"]:
            assert not any(kinds) and not any(raised)
        out[name] = {"params": {k: c[k] for k in ("C", "n", "tail", "frames", "ss", "L", "q", "rmin", "rmax", "first",
                                                  "seed", "fallback", "twin")},
                     "samples_sha256": WC.samples_sha256(name), "wasted": ws, "kinds": kinds, "raised": raised,
                     "subframes": subs, "frames": frames, "default": default, "twin_subframes": twin}
        print(f"{name:10s} w {ws} kinds {kinds} types {sorted({(s['type'], s['order']) for s in subs})} "
              f"default {[d['exception'] or 'samples' for d in default]} bytes {[len(f) // 2 if isinstance(f, str) else f['len'] for f in frames]}",
              flush=True)
    assert types == {"CONSTANT", "VERBATIM", "FIXED", "LPC"}, types
    fb = out["fb16"]
    assert fb["kinds"][:4] == [1, 1, 2, 2] or fb["kinds"][:3] == [1, 1, 2], fb["kinds"]
    with open(os.path.join(HERE, "wasted_streams.json"), "w") as fh:
        json.dump({"generator": "tests/golden/make_wasted_golden.py",
                   "reference": "flac.encoder writers (encoder.py:127-157, :323-328, :553-578) with the wasted code in "
                                "the subframe header; flac.decoder (decoder.py:111-130, :267-355, :431-498) with and "
                                "without get_wasted_bits + 1 and samples << wasted", "cases": out},
                  fh, separators=(",", ":"))


if __name__ == "__main__":
    build()
