"""Golden fixture for the corrected-LPC-sign mode (FLACMI_FLAG_LPC_SIGN, include/flacmi.h): the
reference's own encode(), with the one change that defines the mode.

Run ONLY in the build container, where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lpc_sign_golden.py

It imports flac.encoder / flac.decoder from the reference checkout (read-only, nothing is copied;
make_fallback_golden.py sets up the paths, FLAC_REFERENCE) and replaces flac.encoder.levinson_durbin
by a wrapper that calls the reference's function and negates its result:

    return [-c for c in levinson_durbin(xs)]

Everything else is the reference as it stands: for every case of tests/lpc_sign_cases.py its
encode() runs on the stream until it ends or raises, and the reference decoder
(make_fallback_golden.decode: get_frame_header, get_subframe, decode_subframe) must return the
input from every frame written.

tests/golden/lpc_sign_streams.json records per case the parameters (the samples are pinned by a
SHA-256), the stream header as hex, each frame's bytes as hex (a frame above 4 KB: its length and
SHA-256), the exception class of the frame encode() raised on (or null), per unit the verdict
["fixed" | "lpc", order] or the exception's name, from the reference's own subframe functions, and
the number of (unit, order) pairs whose quantised negated coefficients differ from the negated
quantised coefficients (the quantiser's clamp is asymmetric).  The conditions that make the fixture
worth having are asserted at the end.  The GPU box never runs this script.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_fallback_golden as MF  # noqa: E402  (sets the paths of the reference, tests/ and oracle/)

from flac import encoder as E  # noqa: E402  (the reference, imported read-only)

import lpc_sign_cases as LC  # noqa: E402

HEX_LIMIT = 4096
_reference_levinson_durbin = E.levinson_durbin


def corrected_levinson_durbin(xs):
    return [-c for c in _reference_levinson_durbin(xs)]


def verdict(samples, parameters):
    """encode()'s steps for one channel (encoder.py:127-157) up to the choice."""
    try:
        fh, fs = E.encode_subframe_fixed(samples)
        lh, ls = E.encode_subframe_lpc(samples, parameters.lpc_order, parameters.qlp_precision)
        fixed_size = sum(abs(x) for x in fs.residual)
        lpc_size = sum(abs(x) for x in ls.residual)
        assert fixed_size != lpc_size
    except MF.RAISES as e:
        return type(e).__name__
    return ["fixed", fh.type_.order] if fixed_size < lpc_size else ["lpc", lh.type_.order]


def asymmetric_orders(samples, parameters):
    """Orders at which quantise(-c) != -quantise(c), c the reference's own Levinson result."""
    try:
        windowed = [x * w for x, w in zip(samples, E.tukey(len(samples), 0.5))]
        ac = [E.autocorrelation(windowed, i) for i in range(parameters.lpc_order.stop)]
        cs = [_reference_levinson_durbin(ac[:i]) for i in range(2, parameters.lpc_order.stop + 1)]
        count = 0
        for c in cs:
            q0, s0 = E.quantize_lpc_coefficients(c, parameters.qlp_precision)
            q1, s1 = E.quantize_lpc_coefficients([-v for v in c], parameters.qlp_precision)
            count += (s0 != s1) or ([-v for v in q0] != q1)
        return count
    except MF.RAISES:
        return 0


def build():
    E.levinson_durbin = corrected_levinson_durbin
    out = {}
    for name, c in LC.CASES.items():
        x = LC.channels(name)
        C, ss, n = c["C"], c["ss"], c["n"]
        parameters = E.EncoderParameters(block_size=n, rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                         lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])
        samples = iter([[int(v) for v in x[:, i]] for i in range(c["frames"])])
        chunks, raised = [], None
        try:
            for chunk in E.encode(c["rate"], ss, C, c["frames"], samples, parameters):
                chunks.append(chunk)
        except MF.RAISES as e:
            raised = type(e).__name__
        header, frames = b"".join(chunks[:3]), chunks[3:]
        assert len(header) == 4 + 4 + 34
        for f, data in enumerate(frames):
            chans = [[int(v) for v in x[k, f * n:(f + 1) * n]] for k in range(C)]
            assert MF.decode(data, C, ss) == chans, f"{name} frame {f}: the reference decoder returns other samples"
        nb = LC.n_blocks(name)
        assert len(frames) == nb if raised is None else len(frames) < nb
        verdicts, asym = [], 0
        for f in range(nb):
            for k in range(C):
                chan = [int(v) for v in x[k, f * n:(f + 1) * n]]
                verdicts.append(verdict(chan, parameters))
                asym += asymmetric_orders(chan, parameters)
        # encode() stops at the first frame with a unit the reference raises on
        first_bad = next((u for u, v in enumerate(verdicts) if isinstance(v, str)), None)
        if first_bad is None:
            assert raised is None
        else:
            assert len(frames) == first_bad // C and verdicts[first_bad] == raised
        out[name] = {"params": dict(c), "samples_sha256": LC.samples_sha256(name), "header": header.hex(),
                     "frames": [d.hex() if len(d) <= HEX_LIMIT else
                                {"len": len(d), "sha256": hashlib.sha256(d).hexdigest()} for d in frames],
                     "raises": raised, "verdicts": verdicts, "asymmetric": asym}
        kinds = [v if isinstance(v, str) else v[0] for v in verdicts]
        print(f"{name:12s} frames {len(frames)}/{nb} raises {raised} fixed {kinds.count('fixed')} "
              f"lpc {kinds.count('lpc')} asymmetric {asym}", flush=True)
    E.levinson_durbin = _reference_levinson_durbin
    # what makes the fixture worth having
    written = [v for g in out.values() for u, v in enumerate(g["verdicts"]) if u // g["params"]["C"] < len(g["frames"])]
    assert any(v[0] == "fixed" for v in written) and any(v[0] == "lpc" for v in written)
    assert sum(g["asymmetric"] for g in out.values()) >= 1
    assert out["silence"]["raises"] == "ZeroDivisionError" and len(out["silence"]["frames"]) == 2
    assert {g["params"]["C"] for g in out.values()} >= {1, 2, 3}
    assert {g["params"]["ss"] for g in out.values()} >= {16, 24}
    assert {g["params"]["q"] for g in out.values()} >= {5, 6, 15}
    assert any(LC.tail_len(name) and len(g["frames"]) == LC.n_blocks(name) for name, g in out.items())
    path = os.path.join(HERE, "lpc_sign_streams.json")
    with open(path, "w") as fh:
        json.dump({"generator": "tests/golden/make_lpc_sign_golden.py",
                   "reference": "flac.encoder.encode (encoder.py:48-165) with levinson_durbin's result negated, "
                                "read back by flac.decoder (decoder.py:111-130, :431-498)", "cases": out}, fh,
                  separators=(",", ":"))
    assert os.path.getsize(path) <= 250_000, os.path.getsize(path)


if __name__ == "__main__":
    build()
