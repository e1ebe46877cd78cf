"""Inputs of the corrected-LPC-sign tests (FLACMI_FLAG_LPC_SIGN, include/flacmi.h): small seeded
streams over the oracle's synthetic generator.

Shared by tests/golden/make_lpc_sign_golden.py (the reference's own encode() with its
levinson_durbin's result negated, in tests/golden/lpc_sign_streams.json), the CPU model's test
and the device tests.  Channel c of a stream is one run of oracle.synth_unit(unit0 + c, frames,
ss, seed) over the whole stream, so the fixture holds no samples (they are pinned by a SHA-256);
`silence_from` zeroes every channel from that sample on (digital silence: the reference raises
ZeroDivisionError in levinson_durbin, encoder.py:469, on the first block inside it).
"""
import hashlib
import os

import numpy as np

import oracle
from fallback_cases import same_frame  # noqa: F401  (re-exported for the tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpc_sign_streams.json")


def _case(C, ss, n, frames, L, q, rmax, rate=44100, unit0=0, seed=2024, silence_from=None):
    return dict(C=C, ss=ss, n=n, frames=frames, L=L, q=q, rmin=0, rmax=rmax, rate=rate, unit0=unit0, seed=seed,
                silence_from=silence_from)


CASES = {
    # mono, 16-bit, q 5, a short last block (100 samples)
    "mono16": _case(1, 16, 256, 5 * 256 + 100, 12, 5, 5),
    # the default block size of the command line, and a 1000-sample last block
    "mono4608": _case(1, 16, 4608, 2 * 4608 + 1000, 12, 5, 5, unit0=3),
    # stereo, q 6: quantised coefficients beyond the int8 / f16 ranges of the q 5 kernels
    "stereo16_q6": _case(2, 16, 192, 4 * 192 + 77, 8, 6, 3, unit0=10),
    # three channels, 24-bit, L 32 q 15 (96 kHz: the reference allows L > 12 above 48 kHz)
    "tri24_q15": _case(3, 24, 512, 2 * 512 + 130, 32, 15, 4, rate=96000, unit0=20),
    # 8-sample blocks, L 4: the fixed predictor still wins on some of them
    "tiny8": _case(1, 16, 8, 20 * 8, 4, 5, 1, unit0=30),
    # two blocks of signal, then digital silence: the third frame raises
    "silence": _case(1, 16, 256, 4 * 256, 8, 5, 4, unit0=40, silence_from=2 * 256),
}


def channels(name: str) -> np.ndarray:
    """[C][frames] int64: the stream's channels."""
    c = CASES[name]
    x = np.stack([oracle.synth_unit(c["unit0"] + k, c["frames"], c["ss"], c["seed"]).astype(np.int64)
                  for k in range(c["C"])])
    if c["silence_from"] is not None:
        x[:, c["silence_from"]:] = 0
    return x


def n_blocks(name: str) -> int:
    c = CASES[name]
    return (c["frames"] + c["n"] - 1) // c["n"]


def tail_len(name: str) -> int:
    """The last block's length, 0 when it is a whole block."""
    c = CASES[name]
    return c["frames"] % c["n"]


def block_len(name: str, f: int) -> int:
    t = tail_len(name)
    return t if t and f == n_blocks(name) - 1 else CASES[name]["n"]


def case_rows(name: str) -> np.ndarray:
    """rows [blocks * C][n] int16 or int32 in the flacmi_batch layout: row f * C + k is channel k of
    block f, zero behind a short last block."""
    c = CASES[name]
    x = channels(name)
    nb = n_blocks(name)
    rows = np.zeros((nb * c["C"], c["n"]), dtype=np.int16 if c["ss"] <= 16 else np.int32)
    for f in range(nb):
        seg = x[:, f * c["n"]:(f + 1) * c["n"]]
        rows[f * c["C"]:(f + 1) * c["C"], :seg.shape[1]] = seg
    return rows


def samples_sha256(name: str) -> str:
    return hashlib.sha256(channels(name).astype("<i8").tobytes()).hexdigest()
