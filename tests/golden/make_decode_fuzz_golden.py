"""Golden fixture of the decoder fuzz (tests/decode_fuzz_cases.py): the reference decoder's
verdict on every generated frame.

Run ONLY where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_decode_fuzz_golden.py

Every frame of decode_fuzz_cases.frames() is read by the reference's get_frame and decode_frame
(decoder.py:111-130, :431-498, imported read-only).  tests/golden/decode_fuzz.json records per
frame its name, the sha256 of its bytes, the exception class or the sha256 of the decoded samples
(int64 little-endian, channel after channel, as decode.json), the block size and the reader's
position after get_frame, as one row of "cases" in the order of "fields".  Hashes only: the frames themselves are regenerated from the seed.
"""
import hashlib
import io
import json
import os
import sys

REF = os.environ.get("FLAC_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from flac import decoder as D  # noqa: E402  (the reference, imported read-only)
from flac.binary import Get  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import decode_fuzz_cases as G  # noqa: E402
import decode_model as M  # noqa: E402

DROP_CAP = 0.10
FIELDS = ["name", "sha256", "exception", "decoded_sha256", "block_size", "end"]  # one row per frame


def sample_hash(channels):
    """None where a sample does not fit the int64 layout (mutated frames only: far outside the
    kernels' domain, dropped)."""
    if any(not -(1 << 63) <= v < (1 << 63) for ch in channels for v in ch):
        return None
    flat = b"".join(int(v).to_bytes(8, "little", signed=True) for ch in channels for v in ch)
    return hashlib.sha256(flat).hexdigest()


def dropped(case):
    """A mutated frame outside the kernels' documented domain (decode_model.OutOfDomain), as
    the device reads it or as the reference does (an L_R frame: two subframes)."""
    for channels in (case.channels, 2):
        try:
            M.decode(case.data, channels, case.sample_size)
        except M.OutOfDomain:
            return True
    return False


def build():
    out, n_valid, n_mut, n_cut, n_drop = [], 0, 0, 0, 0
    for cs in G.frames(G.SEED):
        res = {"exception": None, "decoded_sha256": None, "block_size": None, "end": None}
        buf = io.BytesIO(cs.data)
        try:
            fr = D.get_frame(Get(buf), cs.sample_size)
            res["block_size"], res["end"] = fr.header.block_size, buf.tell()
            res["decoded_sha256"] = sample_hash(D.decode_frame(fr))
        except Exception as e:  # noqa: BLE001  -- the reference's exception class is the fixture
            res["exception"] = type(e).__name__
        if cs.truth is None:
            n_mut += cs.name[0] == "m"
            n_cut += cs.name[0] == "c"
            n_drop += dropped(cs)
        else:
            n_valid += 1
        out.append([cs.name, hashlib.sha256(cs.data).hexdigest(), res["exception"], res["decoded_sha256"],
                    res["block_size"], res["end"]])
    assert n_drop <= DROP_CAP * n_mut, (n_drop, n_mut)
    for e in out:
        if e[2]:
            print(f"{e[0]:24s} -> {e[2]}")
    print(f"{n_valid} valid, {n_mut} mutated, {n_cut} cut, {n_drop} of the mutated and cut dropped")
    with open(os.path.join(OUT, "decode_fuzz.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_decode_fuzz_golden.py", "reference": "flac.decoder.get_frame + "
                   "decode_frame (decoder.py:111-130, :431-498)", "seed": G.SEED, "valid": n_valid, "mutated": n_mut, "cut": n_cut,
                   "dropped": n_drop, "fields": FIELDS, "cases": out}, f, separators=(",", ":"))


if __name__ == "__main__":
    build()
