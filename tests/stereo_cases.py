"""Inputs of the stereo-decorrelation tests (FLACMI_STEREO_BEST, include/flacmi.h): stereo
frames whose best channel assignment is each of L_R, L_S, S_R and M_S, frames where one of the
four candidate signals (left, right, mid, side) cannot be written by the reference, and silence.

Shared by tests/golden/make_stereo_golden.py (the reference's own verdicts and bytes, in
tests/golden/stereo_streams.json), tests/stereo_model.py's CPU test and the device tests.  Every
frame is a pair recipe over the unit recipes of tests/fallback_cases.py, so the fixture holds no
samples.  For frame f of a case with seed s the four source units are

    W = ("noise", 30)    at u = 4 f        a quiet wide-band signal
    T = ("sine", 3000)   at u = 4 f + 1    a loud tonal signal
    B = ("noise", 1000)  at u = 4 f + 2
    X = ("white",)       at u = 4 f + 3    full scale

and the pair recipes give (left, right):

    indep    (W, T)        nothing in common: L_R
    lside    (W, W - T)    the side is T: L_S
    sright   (W + T, W)    the side is T: S_R
    midside  (W + T, W - T)  mid W, side 2 T: M_S
    rzero    (B, 0)        the right channel is silent (the reference raises on it)
    equal    (B, B)        the side is silent
    anti     (X, -X - 1)   the mid is the constant -1, the side spans all ss + 1 bits
    silence  (0, 0)
    widespike  (hi - 2000 + B, lo + 2000 + W) with one sample of (lo, hi), hi / lo the largest /
               smallest ss-bit value: the side runs near +2^ss and drops to -2^ss + 1, so at
               ss = 31 its order-1 residual needs 33 bits (FLACMI_STATUS_RESIDUAL_WIDE on 32-bit
               residual rows, and the redo of the batch with 64-bit rows)
"""
import hashlib
import os

import numpy as np

from fallback_cases import same_frame, unit  # noqa: F401  (same_frame: re-exported for the tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_streams.json")
L_R, L_S, S_R, M_S = 1, 8, 9, 10  # the frame header's channel-assignment codes
RECIPES = ("indep", "lside", "sright", "midside", "rzero", "equal", "anti", "silence")


def pair(recipe: str, f: int, ln: int, ss: int, seed: int):
    """(left, right) of frame f, int64 [ln] each."""
    w = unit(("noise", 30), ln, ss, seed, 4 * f)
    t = unit(("sine", 3000), ln, ss, seed, 4 * f + 1)
    b = unit(("noise", 1000), ln, ss, seed, 4 * f + 2)
    x = unit(("white",), ln, ss, seed, 4 * f + 3)
    z = np.zeros(ln, dtype=np.int64)
    hi, lo = (1 << (ss - 1)) - 1, -(1 << (ss - 1))
    sl, sr = hi - 2000 + b, lo + 2000 + w
    sl[(100 + f) % ln], sr[(100 + f) % ln] = lo, hi
    return {"widespike": (sl, sr),
            "indep": (w, t), "lside": (w, w - t), "sright": (w + t, w), "midside": (w + t, w - t),
            "rzero": (b, z), "equal": (b, b), "anti": (x, -x - 1), "silence": (z, z)}[recipe]


def _case(n, ss, seed, recipes=RECIPES, tail=0, rmax=3, modes=("off", "on"), L=8, q=12):
    """recipes: one per frame; tail: the last frame's length (0: as long as the others); modes: the
    fallback settings the case runs with."""
    return dict(n=n, ss=ss, seed=seed, recipes=list(recipes), tail=tail, frames=len(recipes), L=L, q=q, rmin=0,
                rmax=rmax, first=0, modes=list(modes))


CASES = {
    "st16": _case(192, 16, 7),
    "st24": _case(192, 24, 8),
    # two tail units become one tail mid unit and one tail side unit
    "st16_tail": _case(192, 16, 7, RECIPES[:4] + ("midside",), tail=77),
    # 7-sample blocks raise in the reference's Tukey window: every candidate is escaped
    "st_tiny": _case(7, 16, 10, rmax=0, modes=("on",)),
    # ss = 31 (the widest the mode takes): a side candidate whose chosen residual needs 64-bit rows,
    # in both two-frame sub-batches of the pipeline test
    "st31_wide": _case(192, 31, 11, ("indep", "widespike", "widespike")),
}

# The reference's verdicts (channel code per frame; None: the frame fails), asserted by
# tests/golden/make_stereo_golden.py from the reference's own run.
EXPECT = {
    ("st16", "off"): [L_R, L_S, S_R, M_S, M_S, L_R, L_R, None],
    ("st16", "on"): [L_R, L_S, S_R, M_S, L_R, L_S, M_S, L_R],
    ("st24", "off"): [L_R, L_S, S_R, M_S, M_S, L_R, L_R, None],
    ("st24", "on"): [L_R, L_S, S_R, M_S, L_R, L_S, M_S, L_R],
    # the 77-sample tail has one Rice partition only (77 is odd); there the reference's sizes put
    # S_R below M_S for the midside pair
    ("st16_tail", "off"): [L_R, L_S, S_R, M_S, S_R],
    ("st16_tail", "on"): [L_R, L_S, S_R, M_S, S_R],
    ("st_tiny", "on"): [L_R, L_R, L_R, L_R, L_R, L_S, M_S, L_R],
    # the side is by far the largest candidate; it is there for its 33-bit residual
    ("st31_wide", "off"): [L_R, L_R, L_R],
    ("st31_wide", "on"): [L_R, L_R, L_R],
}


def frame_len(name: str, f: int) -> int:
    c = CASES[name]
    return c["tail"] if c["tail"] and f == c["frames"] - 1 else c["n"]


def case_rows(name: str):
    """(rows [2 frames][n] int16 or int32 with row 2 f = left and 2 f + 1 = right of frame f,
    n_tail_units) of a case."""
    c = CASES[name]
    rows = np.zeros((2 * c["frames"], c["n"]), dtype=np.int16 if c["ss"] <= 16 else np.int32)
    for f, recipe in enumerate(c["recipes"]):
        ln = frame_len(name, f)
        left, right = pair(recipe, f, ln, c["ss"], c["seed"])
        for ch, x in enumerate((left, right)):
            assert -(1 << (c["ss"] - 1)) <= int(x.min()) and int(x.max()) < 1 << (c["ss"] - 1)
            rows[2 * f + ch, :ln] = x
    return rows, (2 if c["tail"] else 0)


def candidates(left, right):
    """The four candidate signals of a frame, in the rule's order: left, right, mid, side."""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    return left, right, (left + right) >> 1, left - right


# the two candidates (indices into candidates()) of each assignment, in the rule's order
ASSIGNMENTS = ((L_R, 0, 1), (L_S, 0, 3), (S_R, 3, 1), (M_S, 2, 3))


def choose(sizes):
    """The rule: sizes[k] is candidate k's exact subframe bit count, or None when it is not
    eligible -> (code, first candidate, second candidate), or None when no assignment is eligible.
    The first assignment with the smallest sum wins."""
    best = None
    for code, a, b in ASSIGNMENTS:
        if sizes[a] is None or sizes[b] is None:
            continue
        if best is None or sizes[a] + sizes[b] < best[0]:
            best = (sizes[a] + sizes[b], code, a, b)
    return None if best is None else best[1:]


def samples_sha256(name: str) -> str:
    rows, _ = case_rows(name)
    return hashlib.sha256(rows.astype("<i8").tobytes()).hexdigest()
