"""Shapes, inputs and flag sets of the mode-matrix tests: the device encoder's opt-in switches in
combination, at the smallest shape of every production analysis route, against the composed CPU
model of tests/mode_matrix_model.py.  Shared by tests/test_mode_matrix_model.py (no device) and
tests/test_gpu_mode_matrix.py.  Test infrastructure only; importing it needs no GPU.

Every case is a two-channel batch of seeded frames, so no samples are committed.  A frame is
(recipe, left shift, right shift); the recipe gives (left, right) from the unit recipes the suite
already has, made at ss - shift bits and shifted left, so that the unit has that many wasted bits:

    indep lside sright midside   stereo_cases.pair: frames whose best assignment is L_R, L_S, S_R, M_S
    equal    stereo_cases.pair: left == right; with fallback the silent side is CONSTANT and L_S, S_R
             and M_S tie, so the first of them wins
    fb       (silence, full-scale white noise): CONSTANT and VERBATIM with fallback, and a frame the
             reference cannot write without it
    gated    two units of test_gpu_rice_search_paths.gated_units (rice_search_cases.ar2 with a stretch of
             silence or of sparse +-1): the reference's Rice step fails them at sites 12 / 13
    open     two units of the bench's open mix (oracle.synth_batch, as stream_shape_cases.case_units
             takes them): the units k_resid_stream lists
    gopen    the same, gated
    loud     (A, A - B), A and B noise of ss - 1 and ss - 2 bits: about ss - 1 bits a sample in
             either channel, and the side B is the smallest second subframe
    loudq    (quiet noise whose first quarter is +-(7/8 full scale) with random signs, noise): the
             loud partitions take a Rice parameter above 14 (coding method 5) under the search, and
             the subframe stays below its VERBATIM size
    cc cr rc (silence, constant), (constant, ramp), (ramp, constant): blocks whose best fixed residual
             is all zeros (the case const_rescued, which belongs to no route)
"""
import functools
from collections import namedtuple

import numpy as np

import fallback_cases as FC
import mode_matrix_model as MM
import oracle
import stereo_cases as SC
import stream_shape_cases as SSC
import wasted_cases as WC
from test_gpu_rice_search_paths import gated_units

Route = namedtuple("Route", "name n ss L q rmin rmax rate")
_RT = SSC.CASES[0]
ROUTES = {r.name: r for r in (
    Route("general", 192, 16, 8, 5, 0, 4, 44100),
    Route("stream_rt", _RT.n, 16, _RT.L, _RT.q, _RT.rmin, _RT.rmax, 44100),
    Route("stream_const", 4608, 16, 12, 5, 0, 5, 44100),
    Route("sb", 8192, 24, 16, 12, 0, 6, 96000),      # (L > 12: the reference allows it above 48 kHz)
    Route("mfma", 8192, 24, 16, 12, 0, 5, 96000),
)}
LARGE_FRAME = 16384  # k_pack's LDS window, bytes
# The block length of one more runtime-shape stream case: the smallest at which the device rows of the mid
# (the caller's int16) and of the side (int32) have different pitches, and the side's is the larger.
PITCH_N = 1024

# a case: its route's shape (or its own), its frames, the odd length of its last frame (0: a whole block),
# its seed, and whether only the flag sets with lpc_sign run it
Case = namedtuple("Case", "name route n ss L q rmin rmax rate frames tail seed lpc_sign_only")


def _case(name, route, frames, tail=0, seed=1, lpc_sign_only=False, **over):
    r = ROUTES[route]._replace(**over)
    return Case(name, route, r.n, r.ss, r.L, r.q, r.rmin, r.rmax, r.rate, tuple(frames), tail, seed, lpc_sign_only)


def _three(route, hi, tails, seed, seed_c=None):
    """The three 3-frame cases of a route; hi: the large wasted count (8 at 24 bits: 16-bit audio
    in a 24-bit container).  a: the tie and two stereo assignments, w = 0, 2 and hi by frame; b: (0, 2, 0, hi) inside
    one two-frame sub-batch (the method-5 frame and the fallback frame), then the fourth assignment; c: a large
    frame, then units the Rice search rescues, the last frame short and odd."""
    return [
        _case(f"{route}_a", route, [("equal", 0, 0), ("lside", 2, 2), ("sright", hi, hi)], seed=seed),
        _case(f"{route}_b", route, [("loudq", 0, 2), ("fb", 0, hi), ("midside", 0, 0)], seed=seed + 1),
        _case(f"{route}_c", route, [("loud", 0, 0), ("gated", 0, 0), ("gated", 0, 0)], tail=tails, seed=seed_c or seed + 2),
    ]


_BIG = [("indep", 0, 0), ("lside", 2, 2), ("sright", 3, 3), ("midside", 0, 0), ("loudq", 0, 2), ("fb", 0, 3),
        ("loud", 0, 0), ("gated", 0, 0), ("gated", 0, 0)] + [("equal", 0, 0)] + [("open", 0, 0)] * 12 + [("gopen", 0, 0)] * 13
CASES = {c.name: c for c in (
    _three("general", 3, 77, 100)
    # (seed 233, found by search: with lpc_sign an order-12 predictor leaves Rice partitions of 16 samples,
    # and the stretch of silence of these 64-sample units covers one)
    + _three("stream_rt", 3, 33, 200, seed_c=233)
    + [_case("stream_rt_d", "stream_rt", [("open", 0, 0), ("open", 0, 0), ("gopen", 0, 0)], seed=210),
       _case("stream_rt_pitch", "stream_rt", [("indep", 0, 0), ("sright", 0, 0), ("midside", 0, 0)], seed=220, n=PITCH_N)]
    # 35 frames = 70 units: k_lpc_tile's round of 64 and k_lpc behind it
    + [_case("stream_const_big", "stream_const", _BIG, seed=300),
       _case("stream_const_tail", "stream_const", [("lside", 0, 0), ("loud", 0, 0), ("gated", 0, 0)], tail=1001, seed=310)]
    + _three("sb", 8, 3001, 400)
    + _three("mfma", 8, 3001, 500)
    + [_case("mfma_l32", "mfma", [("lside", 8, 8), ("gated", 0, 0), ("fb", 0, 8)], seed=520, lpc_sign_only=True,
             n=1024, L=32, q=15, rmax=4)]
)}
# A constant block the Rice search rescues is CONSTANT under fallback, a ramp stays FIXED (192 samples,
# the general route's parameters; w = 0, 0, 4, 0, 0, 2).
CASES["const_rescued"] = Case("const_rescued", None, 192, 16, 8, 5, 0, 4, 44100,
                              (("cc", 0, 0), ("cr", 4, 0), ("rc", 0, 2)), 0, 600, False)
OPEN_POOL = 26  # units of either open-mix pool of a shape


def cases_of(route: str, flags=None) -> list:
    """The route's cases; with a flag set, those it runs with."""
    return [c for c in CASES.values() if c.route == route and (flags is None or not c.lpc_sign_only or flags["lpc_sign"])]


# ---------------------------------------------------------------------------------------
# flag sets
# ---------------------------------------------------------------------------------------
def _set(*on):
    return {f: f in on for f in MM.FLAGS}


MAXIMAL = [_set("fallback", "stereo", "lpc_sign", "rice_search"), _set("fallback", "wasted", "lpc_sign", "rice_search"),
           _set("fallback", "stereo", "fixed_only", "rice_search"), _set("fallback", "wasted", "fixed_only", "rice_search")]
TEN = [_set()] + [_set(f) for f in ("fallback", "stereo", "lpc_sign", "wasted", "rice_search")] + MAXIMAL
API_SETS = MAXIMAL[:2]


def flag_sets(route: str) -> list:
    return MM.combinations() if route == "general" else TEN


RUNS = [(route, MM.name_of(s)) for route in ROUTES for s in flag_sets(route)]
SETS = {MM.name_of(s): s for s in MM.combinations()}


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def frame_pair(c: Case, f: int, ln: int):
    """(left, right) of frame f of case c, int64 [ln] each, before the shifts."""
    recipe, sl, sr = c.frames[f]
    bl, br = c.ss - sl, c.ss - sr
    if recipe in ("indep", "lside", "sright", "midside", "equal"):
        assert sl == sr
        return SC.pair(recipe, f, ln, bl, c.seed)
    if recipe == "fb":
        return FC.unit(("zero",), ln, bl, c.seed, 2 * f), FC.unit(("white",), ln, br, c.seed, 2 * f + 1)
    if recipe in ("gated", "open", "gopen"):
        assert sl == sr == 0
        if recipe != "gated":
            assert c.ss == 16
            pool = oracle.synth_batch(0, OPEN_POOL, ln, 16, c.seed, dtype=np.int16, open_eighths=5) if recipe == "open" \
                else gated_units(ln, OPEN_POOL, 16, c.seed, open_mix=OPEN_POOL)
            k = 2 * (f - c.frames.index((recipe, 0, 0)))
            return pool[k].astype(np.int64), pool[k + 1].astype(np.int64)
        # units 0, 1, 3, 4 of the pool: a stretch of silence or of sparse +-1 (u % 3 != 2)
        pool = gated_units(ln, 6, c.ss, c.seed + ln)
        k = [0, 1, 3, 4][2 * (f % 2):][:2]
        return pool[k[0]].astype(np.int64), pool[k[1]].astype(np.int64)
    if recipe == "loud":
        assert sl == sr == 0
        a = FC.unit(("noise", 1 << (c.ss - 2)), ln, c.ss, c.seed, 2 * f)
        b = FC.unit(("noise", 1 << (c.ss - 3)), ln, c.ss, c.seed, 2 * f + 1)
        return a, a - b
    if recipe == "loudq":
        x = FC.unit(("noise", 30), ln, bl, c.seed, 2 * f)
        sign = 2 * WC.unit(("bit",), 0, ln, bl, c.seed + 7, 2 * f) + 1
        q = ln // 4
        x[:q] = (sign * (7 << (bl - 4)) + FC.unit(("noise", (1 << (bl - 4)) - 196), ln, bl, c.seed + 8, 2 * f))[:q]
        return x, FC.unit(("noise", 1000 if br > 11 else 100), ln, br, c.seed, 2 * f + 1)
    if recipe in ("cc", "cr", "rc"):
        u = {"c": ("const", 5 if recipe == "cc" else -3 if recipe == "cr" else 77), "r": ("ramp", -1000, 7)}
        first = ("zero",) if recipe == "cc" else u[recipe[0]]
        return FC.unit(first, ln, bl, c.seed, 2 * f), FC.unit(u[recipe[1]], ln, br, c.seed, 2 * f + 1)
    raise ValueError(recipe)


def frame_len(c: Case, f: int) -> int:
    return c.tail if c.tail and f == len(c.frames) - 1 else c.n


@functools.lru_cache(maxsize=None)
def case_rows(name: str) -> np.ndarray:
    """rows [2 frames][n] int16 (ss 16) or int32: row 2 f is the left, 2 f + 1 the right channel of
    frame f, zero behind a short last frame.  Read-only."""
    c = CASES[name]
    rows = np.zeros((2 * len(c.frames), c.n), dtype=np.int16 if c.ss <= 16 else np.int32)
    for f, (_, sl, sr) in enumerate(c.frames):
        ln = frame_len(c, f)
        left, right = frame_pair(c, f, ln)
        for ch, (x, s) in enumerate(((left, sl), (right, sr))):
            lo, hi = -(1 << (c.ss - s - 1)), (1 << (c.ss - s - 1)) - 1
            assert lo <= int(x.min()) and int(x.max()) <= hi, (name, f, ch)
            rows[2 * f + ch, :ln] = x << s
    rows.setflags(write=False)
    return rows


def n_tail_units(c: Case) -> int:
    return 2 if c.tail else 0


def pcm(name: str) -> np.ndarray:
    """planar int64 [2][samples] of a case"""
    c, rows = CASES[name], case_rows(name)
    return np.stack([np.concatenate([rows[2 * f + ch][: frame_len(c, f)] for f in range(len(c.frames))])
                     for ch in range(2)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def model(name: str, flags_name: str) -> MM.Result:
    """The composed model's frames of a case under a flag set, computed once (the analysis behind
    it is shared between the flag sets that differ in the writer only: mode_matrix_model.analysis)."""
    c = CASES[name]
    return MM.frames(case_rows(name), 2, c.n, c.tail, c.ss, c.L, c.q, c.rmin, c.rmax, 0, **SETS[flags_name])


# ---------------------------------------------------------------------------------------
# the routes, from the host dispatch as the suite restates it
# ---------------------------------------------------------------------------------------
def row_pitch(n: int, sample_bytes: int) -> int:
    """flacmi_unit_stride: the pitch, in samples, of the library's device rows (16-byte rows, plus 128
    bytes when the pitch is a multiple of 4 KB)."""
    b = (n * sample_bytes + 15) // 16 * 16
    return (b + 128 if b % 4096 == 0 else b) // sample_bytes


def sb_shape(n, bits, rmin, rmax) -> bool:
    """csrc/k_resid.h sb_shape_ok: k_resid_sb's shapes (a caller that asks for no fixed_sums)."""
    if n < 8192 or n > 16384 or n % 256 != 0 or bits > 24:
        return False
    om = SSC.rmax_eff(n, rmin, rmax)
    if om < 6 or om > 8:
        return False
    ps = n >> om
    cpp = ps >> 3
    return ps % 8 == 0 and cpp <= 64 and cpp & (cpp - 1) == 0


def mf8_shape(n, L, dtype) -> bool:
    """csrc/k_resid.h launch_resid_bucket: the int8-MFMA kernels take 4-byte rows of a multiple of
    256 samples, at least 8192, in the LMAX 16 and 32 buckets."""
    return dtype == np.int32 and L > 12 and n % 256 == 0 and n >= 8192


@functools.lru_cache(maxsize=None)
def _classes(name):
    c, rows = CASES[name], case_rows(name)
    ora = oracle.analyze_batch(rows, oracle.make_params(c.L, c.q, c.rmin, c.rmax), c.n, c.tail, n_tail_units(c),
                               sample_bits=c.ss, threads=8)
    lens = [frame_len(c, u // 2) for u in range(rows.shape[0])]
    return SSC.class_counts(SSC.classify(rows, ora, c.L, lens))


def check_route(route: str) -> dict:
    """Assert that the route's shape takes the analysis path it is named after; returns the facts."""
    r = ROUTES[route]
    dtype = np.int16 if r.ss <= 16 else np.int32
    shape = SSC.stream_shape(r.n, r.L, r.rmin, r.rmax, False)
    facts = {"stream_shape": shape}
    if route == "general":
        assert shape is None and dtype == np.int16
        return facts
    if route in ("stream_rt", "stream_const"):
        assert shape is not None and SSC.narrow_path(r.n, r.L, r.q, False) and dtype == np.int16
        assert shape["NFIX"] == (4608 if route == "stream_const" else 0)
        assert SSC.stream_shape(r.n, 0, r.rmin, r.rmax, True) is not None  # fixed_only: the same kernel, NG 0
        counts = sum((_classes(c.name) for c in cases_of(route) if not c.tail), SSC.Counter())
        facts["classes"] = dict(counts)
        assert counts["batch"] >= 1 and counts["list"] + counts["list2"] >= 1, facts
        if route == "stream_const":
            assert case_rows("stream_const_big").shape[0] >= 64 + 5
        else:
            p = SSC.stream_shape(PITCH_N, r.L, r.rmin, r.rmax, False)
            assert p is not None and p["NFIX"] == 0 and SSC.narrow_path(PITCH_N, r.L, r.q, False)
            assert all(row_pitch(n, 2) == row_pitch(n, 4) for n in (64, 192, 4608)) and row_pitch(8192, 4) == 8192 + 32
            assert row_pitch(PITCH_N, 2) == PITCH_N < row_pitch(PITCH_N, 4)
        return facts
    assert shape is None and mf8_shape(r.n, r.L, dtype)
    assert sb_shape(r.n, r.ss, r.rmin, r.rmax) == (route == "sb")
    assert not sb_shape(r.n, r.ss + 1, r.rmin, r.rmax)  # the 25-bit side batch never takes k_resid_sb
    return facts


# ---------------------------------------------------------------------------------------
# the premises of the inputs, from the model and the oracle alone
# ---------------------------------------------------------------------------------------
def sub_batch_frames(c: Case) -> int:
    """Frames per sub-batch of the pipeline runs: two; four for the 35-frame case, so that k_lpc's
    round of 64 units is split unevenly."""
    return 4 if len(c.frames) > 3 else 2


def wasted_of_units(name: str) -> list:
    import wasted_model as WM
    c, rows = CASES[name], case_rows(name)
    return [WM.wasted_of(rows[u, :frame_len(c, u // 2)], c.ss) for u in range(rows.shape[0])]


@functools.lru_cache(maxsize=None)
def check_premises(route: str) -> dict:
    """Assert, for every flag set of the route, that each mode that is on has something to do in
    the route's cases (the issue's list); returns the facts."""
    r = ROUTES[route]
    facts = {}
    for s in flag_sets(route):
        nm = MM.name_of(s)
        res = {c.name: model(c.name, nm) for c in cases_of(route, s)}
        subs = {k: [x for fr in v.subs for x in fr] for k, v in res.items()}
        every = [x for v in subs.values() for x in v]
        written = [(k, f, fr) for k, v in res.items() for f, fr in enumerate(v.frames) if isinstance(fr, bytes)]
        assert written, (route, nm)
        if s["stereo"]:
            codes = {code for v in res.values() for code in v.codes if code is not None}
            facts[nm, "codes"] = sorted(codes)
            assert codes == {SC.L_R, SC.L_S, SC.S_R, SC.M_S}, (route, nm, codes)
        if s["fallback"]:
            kinds = {k: {x.type for x in v} for k, v in subs.items()}
            assert any({"CONSTANT", "VERBATIM"} <= t and t & {"FIXED", "LPC"} for t in kinds.values()), (route, nm, kinds)
        if s["rice_search"]:
            facts[nm, "rescued"] = sum(x.rescued for x in every)
            assert facts[nm, "rescued"] >= 2, (route, nm)
            facts[nm, "method5"] = sum(x.method == 5 and x.max_param > 14 for x in every)
        if s["lpc_sign"]:
            assert any(x.type == "LPC" for x in every), (route, nm)
        if r.n >= 4608:
            large = [(k, f) for k, f, fr in written if len(fr) > LARGE_FRAME]
            facts[nm, "large"] = len(large)
            assert large, (route, nm)
            if s["stereo"]:
                assert any(x.cand >= 2 for k, f in large for x in res[k].subs[f]), (route, nm)
    # the Rice search alone: the rescued units failed at sites 12 / 13 with the flag clear, and method 5 appears
    for c in cases_of(route):
        for fr, sfr in zip(model(c.name, "none").frames, model(c.name, "rice_search").subs):
            if any(x.rescued for x in sfr):
                assert isinstance(fr, MM.Failed) and fr.status == 3 and fr.site in (12, 13), (c.name, fr)
    assert facts["rice_search", "method5"] >= 1, route
    # wasted bits: three different counts, 0 among them, inside one sub-batch, and a w > 0 unit behind a w = 0 one
    ok = False
    for c in cases_of(route):
        w = wasted_of_units(c.name)
        k = 2 * sub_batch_frames(c)
        for u0 in range(0, len(w), k):
            part = w[u0:u0 + k]
            if len(set(part)) >= 3 and 0 in part and (r.ss != 24 or 8 in part) and \
                    any(a == 0 and b > 0 for a, b in zip(part, part[1:])):
                ok = True
    assert ok, route
    return facts
