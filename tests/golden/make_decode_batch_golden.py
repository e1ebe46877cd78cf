"""Generate tests/golden/decode_batch_streams.json: pairs of streams that, laid back to back,
spell one frame across the boundary between them, each with the reference's verdict on it alone.

Run ONLY where the reference is readable:

    python tests/golden/make_decode_batch_golden.py

A two-frame stream of 192-sample blocks (what e_cut_* of make_stream_decode_golden.py is built
from) is cut at byte j of its second frame: A_j is the stream up to j, B_j is A's metadata
followed by the stream's bytes from j on.  A decoder that reads A_j past its own end into B_j's
frame region completes the cut frame (384 samples instead of 192); the reference, given A_j
alone, ends it silently after the first frame.  The cuts: every byte of the second frame's header
and CRC-8, three positions inside its residual, and its last two bytes (the CRC-16).
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_stream_decode_golden as S  # noqa: E402  (puts the reference on sys.path)

M = S.M


def build():
    rng = random.Random(20261021)
    fr = [S.fixed_frame(rng, 1, 192, k, 16) for k in range(2)]
    whole = S.stream(fr, 1, 16, 192)
    meta = whole[:len(whole) - len(fr[0]) - len(fr[1])]
    p1 = len(meta) + len(fr[0])
    hl = len(M.header(1, 192, fno=1))  # the CRC-8 byte included
    n1 = len(fr[1])
    cuts = list(range(1, hl + 1)) + [hl + 9, n1 // 2, n1 - 11] + [n1 - 2, n1 - 1]
    assert cuts == sorted(set(cuts)) and cuts[-1] < n1
    pairs = []
    for j in cuts:
        pair = {"cut": j}
        for key, data in (("a", whole[:p1 + j]), ("b", meta + whole[p1 + j:])):
            v, _ = S.verdict(data)
            assert v["open_exception"] is None
            pair[key] = {"hex": data.hex(), **v}
        assert pair["a"]["n_samples"] == 192 and pair["a"]["exception"] is None
        pairs.append(pair)
        print(f"cut {j:4d}: A {pair['a']['n_samples']} samples / {pair['a']['exception']}, "
              f"B {pair['b']['n_samples']} samples / {pair['b']['exception']}")
    out = os.path.join(HERE, "decode_batch_streams.json")
    with open(out, "w") as f:
        json.dump({"generator": "tests/golden/make_decode_batch_golden.py",
                   "reference": "flac.decoder.decode (decoder.py:31-63)",
                   "header_bytes": hl, "frame_bytes": [len(fr[0]), n1], "pairs": pairs}, f, separators=(",", ":"))
    print(os.path.getsize(out), "bytes")


if __name__ == "__main__":
    build()
