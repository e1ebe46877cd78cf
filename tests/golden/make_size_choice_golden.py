"""Golden fixture for the subframe choice by exact written size (FLACMI_FLAG_SIZE_CHOICE,
include/flacmi.h): the recipe of the TODO in the reference's encode() (encoder.py:104-118), carried
out with the reference's own functions.

Run ONLY in the build container, where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_size_choice_golden.py

It imports flac.encoder / flac.decoder from the reference checkout (read-only, nothing is copied;
make_fallback_golden.py sets up the paths, FLAC_REFERENCE).  Per channel of every case of
tests/size_choice_cases.py, every candidate subframe is built with the reference's functions:
prediction_residual over FIXED_PREDICTOR_COEFFICIENTS (order 0 alone for n <= 4), and tukey,
autocorrelation, levinson_durbin (negated for the cases with the corrected sign, as
make_lpc_sign_golden.py does) and quantize_lpc_coefficients for the LPC orders.  Each candidate is
written by _put_subframe_header + _put_subframe_fixed / _put_subframe_lpc into a Put of its own,
with rice_partitions replaced by make_rice_search_golden.exact_rice_partitions, and its bits are
counted from that Put.  A candidate the writers cannot write (no partition order: the assertion of
exact_rice_partitions; precision 16: encoder.py:619) or write undecodably (the ([], 0) result of the
quantiser) is not eligible.  The first smallest eligible candidate is written into the frame that
make_fallback_golden.frame assembles (its fallback rule applies in the cases marked so; in the
others no unit may be escaped), and the reference decoder must return the input from every frame.

tests/golden/size_choice_streams.json records per case the parameters (the samples are pinned by a
SHA-256), the stream header and each frame's bytes as hex, and per unit every candidate's bits (-1:
not eligible), the choice, what the reference's sum |r| rule chooses (or the exception it raises),
the sub-kind, and the chosen partition order, coding method and parameters.  The conditions that
make the fixture worth having are asserted at the end.  The GPU box never runs this script.
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_fallback_golden as MF  # noqa: E402  (sets the paths of the reference, tests/ and oracle/)
import make_lpc_sign_golden as ML  # noqa: E402  (corrected_levinson_durbin, verdict)
import make_rice_search_golden as MR  # noqa: E402  (exact_rice_partitions)

from flac import encoder as E  # noqa: E402  (the reference, imported read-only)
from flac.binary import Put  # noqa: E402
from flac.common import (FIXED_PREDICTOR_COEFFICIENTS, SubframeFixed, SubframeHeader, SubframeLPC,  # noqa: E402
                         SubframeTypeFixed, SubframeTypeLPC)

import size_choice_cases as SC  # noqa: E402

_reference_rice_partitions = E.rice_partitions
_reference_put_analysed = MF.put_analysed
MODE = {"fixed_only": False}
UNITS = []  # one entry per put_by_size call that reached the choice


def candidates(samples, parameters):
    """[(family, order, header, subframe or None)] in candidate order; None: not eligible before any
    writer runs.  Raises what encode_subframe_lpc raises."""
    n = len(samples)
    out = []
    for k, coefs in enumerate(FIXED_PREDICTOR_COEFFICIENTS):
        if k == 0 or n > 4:
            out.append(("fixed", k, SubframeHeader(SubframeTypeFixed(order=k), 0),
                        SubframeFixed(samples[:k], E.prediction_residual(samples, coefs))))
        else:
            out.append(("fixed", k, None, None))
    if MODE["fixed_only"]:
        return out
    lpc_order, precision = parameters.lpc_order, parameters.qlp_precision
    windowed = [x * w for x, w in zip(samples, E.tukey(n, 0.5))]
    autocorrs = [E.autocorrelation(windowed, i) for i in range(lpc_order.stop)]
    coefficients = [E.levinson_durbin(autocorrs[:i]) for i in range(2, lpc_order.stop + 1)]
    quantized = [E.quantize_lpc_coefficients(c, precision) for c in coefficients]
    if not quantized:
        raise ValueError("min() arg is an empty sequence")  # encoder.py:404
    for order, (coefs, shift) in enumerate(quantized, 1):
        if not coefs:  # the negative-shift branch: ([], 0)
            out.append(("lpc", order, None, None))
            continue
        out.append(("lpc", order, SubframeHeader(SubframeTypeLPC(order=order), 0),
                    SubframeLPC(warmup=samples[:order], precision=precision, shift=shift, coefficients=coefs,
                                residual=E.prediction_residual(samples, coefs, shift))))
    return out


def write(put, family, header, subframe, block_size, sample_size, parameters):
    E._put_subframe_header(put, header)
    if family == "fixed":
        E._put_subframe_fixed(put, subframe, block_size, sample_size, parameters.rice_partition_order)
    else:
        E._put_subframe_lpc(put, subframe, block_size, sample_size, parameters.rice_partition_order)


def put_by_size(put, samples, block_size, sample_size, parameters):
    """make_fallback_golden.put_analysed with the size rule in place of encoder.py:133-157."""
    sized = []
    for family, order, header, subframe in candidates(samples, parameters):
        bits = -1
        if subframe is not None:
            own = Put()
            try:
                write(own, family, header, subframe, block_size, sample_size, parameters)
                pad = own.bits_until_alignment
                own.uint(0, pad)
                bits = 8 * len(own.buffer) - pad
            except AssertionError:  # no partition order; precision 16
                bits = -1
        sized.append((bits, family, order, header, subframe))
    eligible = [c for c in sized if c[0] >= 0]
    assert eligible, "no eligible candidate"
    best = min(eligible, key=lambda c: c[0])  # the first smallest
    del MR.LOG[:]
    write(put, best[1], best[3], best[4], block_size, sample_size, parameters)
    UNITS.append({"fixed": [c[0] for c in sized if c[1] == "fixed"], "lpc": [c[0] for c in sized if c[1] == "lpc"],
                  "choice": [best[1], best[2]], "bits": best[0], "part_order": MR.LOG[-1]["part_order"],
                  "coding_method": MR.LOG[-1]["coding_method"], "rice_params": MR.LOG[-1]["rice_params"]})


def build():
    out = {}
    for name, c in SC.CASES.items():
        x = SC.channels(name)
        C, ss, n = c["C"], c["ss"], c["n"]
        parameters = E.EncoderParameters(block_size=n, rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                         lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])
        total = x.shape[1]
        nb = SC.n_blocks(name)
        header = b"".join(itertools.islice(E.encode(c["rate"], ss, C, total, iter([]), parameters), 3))
        assert len(header) == 4 + 4 + 34
        MODE["fixed_only"] = c["fixed_only"]
        E.levinson_durbin = ML.corrected_levinson_durbin if c["sign"] else ML._reference_levinson_durbin
        E.rice_partitions = MR.exact_rice_partitions
        MF.put_analysed = put_by_size
        frames, units = [], []
        try:
            for f in range(nb):
                chans = [[int(v) for v in x[k, f * n:(f + 1) * n]] for k in range(C)]
                data, verdicts = MF.frame(f, chans, ss, parameters)
                assert MF.decode(data, C, ss) == chans, f"{name} frame {f}: the reference decoder returns other samples"
                frames.append(data.hex())
                for chan, (kind, raised, bits) in zip(chans, verdicts):
                    del UNITS[:]
                    unit = {"kind": kind, "raised": raised}
                    if raised is None:
                        put_by_size(Put(), chan, len(chan), ss, parameters)
                        unit.update(UNITS[-1])
                        assert unit["bits"] == bits
                    if not c["fixed_only"]:
                        E.rice_partitions = _reference_rice_partitions
                        unit["sum_rule"] = ML.verdict(chan, parameters)
                        E.rice_partitions = MR.exact_rice_partitions
                    units.append(unit)
        finally:
            E.rice_partitions = _reference_rice_partitions
            E.levinson_durbin = ML._reference_levinson_durbin
            MF.put_analysed = _reference_put_analysed
        if not c.get("fallback"):
            assert not any(u["kind"] for u in units), f"{name}: a unit is escaped"
        out[name] = {"params": {k: v for k, v in c.items() if k != "plan"}, "plan": [list(p) for p in c["plan"]],
                     "samples_sha256": SC.samples_sha256(name), "header": header.hex(), "frames": frames, "units": units}
        print(f"{name:9s} bytes {[len(d) // 2 for d in frames]} choices {[u.get('choice') for u in units]} "
              f"sum rule {[u.get('sum_rule') for u in units]}", flush=True)
    # what makes the fixture worth having
    mix, nos = out["mix16"]["units"], out["nosign16"]["units"]
    assert any(u["choice"][0] == "fixed" and u["sum_rule"][0] == "lpc" for u in mix)
    assert sum(u["choice"][0] == "lpc" and u["sum_rule"][0] == "lpc" and u["choice"][1] != u["sum_rule"][1] for u in mix) >= 2
    assert any(u["choice"] == u["sum_rule"] for u in mix)
    assert any(u["choice"] != u["sum_rule"] for u in nos)
    for u in out["tie16"]["units"]:
        sizes = [b for b in u["fixed"] + u["lpc"] if b >= 0]
        first = min(range(len(sizes)), key=lambda k: sizes[k])
        assert sizes.count(min(sizes)) >= 2 and u["bits"] == sizes[first]
        assert (u["fixed"] + u["lpc"]).index(u["bits"]) == (u["choice"][1] if u["choice"][0] == "fixed" else 4 + u["choice"][1])
    assert out["st16"]["units"][-1]["part_order"] == 0 and len(out["st16"]["units"][-1]["fixed"]) == 5
    assert {u["kind"] for u in out["fb16"]["units"]} == {0, 1, 2} and out["fb16"]["units"][0]["raised"] == "ZeroDivisionError"
    path = os.path.join(HERE, "size_choice_streams.json")
    with open(path, "w") as fh:
        json.dump({"generator": "tests/golden/make_size_choice_golden.py",
                   "reference": "every candidate subframe of a unit built with flac.encoder's functions and written by "
                                "_put_subframe_fixed / _put_subframe_lpc (encoder.py:581-627) with rice_partitions replaced "
                                "by the exact search; the first smallest is written; read back by flac.decoder "
                                "(decoder.py:111-130, :431-498)", "cases": out}, fh, separators=(",", ":"))
    assert os.path.getsize(path) <= 250_000, os.path.getsize(path)


if __name__ == "__main__":
    build()
