"""Golden fixture for the exact Rice search (FLACMI_FLAG_RICE_SEARCH, include/flacmi.h): the
reference's own encode(), with the one change that defines the mode.

Run ONLY in the build container, where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_rice_search_golden.py

It imports flac.encoder / flac.decoder from the reference checkout (read-only, nothing is copied;
make_fallback_golden.py sets up the paths, FLAC_REFERENCE) and replaces flac.encoder.rice_partitions
by the rule, written with the reference's own split_samples_in_partitions and rice_size: over the
reference's candidate orders in ascending order, with coding method 4 (parameters 0..14) before
method 5 (0..30), every partition takes the smallest parameter of the smallest sum of rice_size,
and the first strictly smallest total of (method + partition size) wins.  Everything else is the
reference as it stands (encode_residual derives the coding method from the parameters, :648-650):
for every case of tests/rice_search_cases.py its encode() runs on the whole stream, must not raise,
and the reference decoder (make_fallback_golden.decode) must return the input from every frame.

tests/golden/rice_search_streams.json records per case the parameters (the samples are pinned by a
SHA-256), the stream header and each frame's bytes as hex, per unit what the unchanged reference
does with it ("ok", or its exception's message: "math domain error" is site 12, "negative shift
count" site 13) and the searched partition order, coding method and parameters.  The conditions
that make the fixture worth having are asserted at the end.  The GPU box never runs this script.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_fallback_golden as MF  # noqa: E402  (sets the paths of the reference, tests/ and oracle/)

from flac import encoder as E  # noqa: E402  (the reference, imported read-only)
from flac.binary import Put  # noqa: E402
from flac.common import RicePartition  # noqa: E402

import rice_search_cases as RC  # noqa: E402

_reference_rice_partitions = E.rice_partitions
LOG = []


def exact_rice_partitions(samples, block_size, predictor_order, partition_order_range):
    candidate_orders = [o for o in partition_order_range
                        if (block_size % (1 << o) == 0 and (block_size >> o) > predictor_order)]
    assert len(candidate_orders) > 0
    best = None
    for o in candidate_orders:
        parts = E.split_samples_in_partitions(samples, o, block_size, predictor_order)
        for method, kmax in ((4, 14), (5, 30)):
            total, ks = 0, []
            for p in parts:
                sizes = [sum(E.rice_size(s, k) for s in p) for k in range(kmax + 1)]
                total += method + min(sizes)
                ks.append(sizes.index(min(sizes)))
            if best is None or total < best[0]:
                best = (total, ks, parts, o, method)
    LOG.append({"part_order": best[3], "coding_method": best[4], "rice_params": best[1], "bits": best[0]})
    return [RicePartition(k, p) for k, p in zip(best[1], best[2])]


def unchanged_reference(samples, n, ss, parameters):
    try:
        MF.put_analysed(Put(), samples, n, ss, parameters)
    except MF.RAISES as e:
        return str(e) or type(e).__name__
    return "ok"


def build():
    out = {}
    for name, c in RC.CASES.items():
        x = RC.channels(name)
        C, ss, n = c["C"], c["ss"], c["n"]
        parameters = E.EncoderParameters(block_size=n, rice_partition_order=range(c["rmin"], c["rmax"] + 1),
                                         lpc_order=range(0, c["L"] + 1), qlp_precision=c["q"])
        nb = RC.n_blocks(name)
        before = []
        for f in range(nb):
            for k in range(C):
                chan = [int(v) for v in x[k, f * n:(f + 1) * n]]
                before.append(unchanged_reference(chan, len(chan), ss, parameters))
        E.rice_partitions = exact_rice_partitions
        del LOG[:]
        try:
            samples = iter([[int(v) for v in x[:, i]] for i in range(c["frames"])])
            chunks = list(E.encode(c["rate"], ss, C, c["frames"], samples, parameters))
        finally:
            E.rice_partitions = _reference_rice_partitions
        header, frames = b"".join(chunks[:3]), chunks[3:]
        assert len(header) == 4 + 4 + 34 and len(frames) == nb and len(LOG) == nb * C
        for f, data in enumerate(frames):
            chans = [[int(v) for v in x[k, f * n:(f + 1) * n]] for k in range(C)]
            assert MF.decode(data, C, ss) == chans, f"{name} frame {f}: the reference decoder returns other samples"
        for u in LOG:
            assert (u["coding_method"] == 5) == any(k > 14 for k in u["rice_params"]) and max(u["rice_params"]) <= 30
        out[name] = {"params": dict(c), "samples_sha256": RC.samples_sha256(name), "header": header.hex(),
                     "frames": [d.hex() for d in frames], "reference": before, "units": list(LOG)}
        print(f"{name:8s} frames {nb} bytes {[len(d) for d in frames]} reference {before} "
              f"orders {[u['part_order'] for u in LOG]} methods {[u['coding_method'] for u in LOG]}", flush=True)
    # what makes the fixture worth having
    seen = {b for g in out.values() for b in g["reference"]}
    assert seen == {"ok", "math domain error", "negative shift count"}, seen
    for name in ("gate16m", "gate16s"):
        assert {"math domain error", "negative shift count"} <= set(out[name]["reference"]), name
    loud = out["loud24"]["units"]
    assert all(u["coding_method"] == 5 and min(u["rice_params"]) <= 14 < max(u["rice_params"]) for u in loud)
    assert RC.tail_len("tail16") == 77 and out["tail16"]["units"][-1]["part_order"] == 0
    assert all(u["part_order"] == 0 for u in out["odd16"]["units"])
    assert any(u["part_order"] > 0 for g in out.values() for u in g["units"])
    path = os.path.join(HERE, "rice_search_streams.json")
    with open(path, "w") as fh:
        json.dump({"generator": "tests/golden/make_rice_search_golden.py",
                   "reference": "flac.encoder.encode (encoder.py:48-165) with rice_partitions (:655-695) replaced by "
                                "the exact search over its own split_samples_in_partitions and rice_size, read back "
                                "by flac.decoder (decoder.py:111-130, :431-498)", "cases": out}, fh,
                  separators=(",", ":"))
    assert os.path.getsize(path) <= 250_000, os.path.getsize(path)


if __name__ == "__main__":
    build()
