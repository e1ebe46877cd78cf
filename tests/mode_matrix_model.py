"""One composed CPU model of the device encoder with any valid set of its six opt-in switches
(fixed_only, fallback, stereo, lpc_sign, wasted, rice_search; encoder.encode's docstring), for the
tests of tests/test_mode_matrix_model.py (no device) and tests/test_gpu_mode_matrix.py.
TEST INFRASTRUCTURE ONLY.

Nothing of any mode is restated here.  The model chains the per-mode models the suite already has,
each tied to the reference's writers by a fixture of its own, in the order the host code applies
them (flacmi_encode_host, include/flacmi.h):

  1. wasted bits    wasted_model.wasted_of per unit; the unit is analysed as x >> w
  2. the analysis   oracle.analyze_batch (FLACMI_MODE_REFERENCE, or FLACMI_MODE_FIXED_ONLY),
                    lpc_sign_model.analyze / stereo_analyse, stereo_model.analyse (the four
                    candidates of every frame)
  3. Rice search    rice_search_model.apply on every analysis dictionary
  4. the writer     fallback_model.frames (with fallback off: the oracle frame writer),
                    stereo_model.frames; a unit with wasted bits is written at ss - w bits behind
                    a header declaring w (include/flacmi.h FLACMI_FRAME_WASTED), the fallback
                    rule applied at that width (wasted_model.constant_bits / verbatim_bits)

frames() returns a Result: per frame its bytes or the Failed(status, site) it fails with, the
channel code per frame in stereo mode, and per written subframe a Sub record (type, wasted count,
coding method, largest Rice parameter, whether the Rice search rescued its unit), from which the
tests check the premises of their inputs.
"""
import hashlib
from collections import namedtuple

import numpy as np

import fallback_model as FM
import frame_writer as FW
import lpc_sign_model as LM
import oracle
import rice_search_model as RM
import stereo_cases as SC
import stereo_model as SM
import wasted_model as WM
from flac_amd import abi

FLAGS = ("fixed_only", "fallback", "stereo", "lpc_sign", "wasted", "rice_search")
STATUS_RESIDUAL_WIDE = 16

# site: the flacmi_site of the failing unit; None where no unit's analysis failed (a frame header
# that cannot be coded, the writer's LPC precision assertion)
Failed = namedtuple("Failed", "status site")
# cand: the channel, or in stereo mode the candidate (0 left, 1 right, 2 mid, 3 side)
Sub = namedtuple("Sub", "type wasted cand method max_param rescued")
# frames: bytes | Failed per frame; codes: the channel code per frame (None for a failed frame; None
# altogether without stereo); subs: per frame the Sub of every written subframe ([] for a failed frame)
Result = namedtuple("Result", "frames codes subs")

_STATUS_OF = {exc: st for st, exc in FW._EXC.items()}


def valid(**flags) -> bool:
    """The combinations encode() takes: all but lpc_sign + fixed_only and wasted + stereo."""
    return not (flags.get("lpc_sign") and flags.get("fixed_only")) and not (flags.get("wasted") and flags.get("stereo"))


def combinations() -> list:
    """Every valid flag set, as dicts of the six switches: 36 of the 64."""
    sets = [dict(zip(FLAGS, ((k >> i) & 1 == 1 for i in range(6)))) for k in range(64)]
    return [s for s in sets if valid(**s)]


def name_of(flags: dict) -> str:
    return "+".join(f for f in FLAGS if flags.get(f)) or "none"


# ---------------------------------------------------------------------------------------
# wasted-bits subframes
# ---------------------------------------------------------------------------------------
def _behind_wasted_header(bits: FW.Bits, t: FW.Bits, w: int):
    """The subframe in t (its 8 header bits first) behind a header that declares w wasted bits:
    0 tttttt 1, w - 1 zeros and a one; unchanged for w == 0."""
    rest = t.n - 8
    bits.put((t.v >> rest) | (1 if w else 0), 8)
    bits.put(1, w)
    bits.put(t.v & ((1 << rest) - 1), rest)


def _wasted_subframe(bits, samples, m, zz, prm, n, width, q, w):
    """frame_writer.subframe at `width` bits behind a header that declares w wasted bits
    (0 tttttt 1, w - 1 zeros and a one)."""
    t = FW.Bits()
    FW.subframe(t, samples, m, zz, prm, n, width, q)
    _behind_wasted_header(bits, t, w)


def _wasted_raw_subframe(bits, samples, n, width, kind, w):
    """fallback_model.raw_subframe (CONSTANT / VERBATIM) at `width` bits behind the same header."""
    t = FW.Bits()
    FM.raw_subframe(t, samples, n, width, kind)
    assert t.n + w == (WM.constant_bits(w, width + w) if kind == FM.CONSTANT else WM.verbatim_bits(n, w, width + w))
    _behind_wasted_header(bits, t, w)


# ---------------------------------------------------------------------------------------
# steps 1 to 3: the analysis, shared between the flag sets that differ in the writer only
# ---------------------------------------------------------------------------------------
_ANALYSES = {}


def _lens(n_units, per_tail, n, tail):
    return [tail if (tail and u >= n_units - per_tail) else n for u in range(n_units)]


def _searched(out, lens, rmin, rmax, done):
    if id(out) not in done:
        done[id(out)] = (out, RM.apply(out, lens, rmin, rmax))  # (keeps `out` alive: ids stay unique)
    return done[id(out)][1]


def analysis(rows, C, n, tail, ss, L, q, rmin, rmax, *, fixed_only=False, stereo=False, lpc_sign=False, wasted=False,
             rice_search=False, threads=8):
    """-> (w per unit, the rows as analysed (x >> w), then without stereo the analysis dictionary
    of the units, with it stereo_model.analyse's candidates per frame).  Cached on the inputs."""
    rows = np.ascontiguousarray(rows)
    key = (hashlib.sha256(rows.tobytes()).hexdigest(), rows.shape, rows.dtype.str, C, n, tail, ss, L, q, rmin, rmax,
           fixed_only, stereo, lpc_sign, wasted, rice_search)
    if key in _ANALYSES:
        return _ANALYSES[key]
    n_units = rows.shape[0]
    lens = _lens(n_units, C, n, tail)
    w = [WM.wasted_of(rows[u, :lens[u]], ss) if wasted else 0 for u in range(n_units)]
    x = rows.copy()
    for u in range(n_units):
        x[u] = WM.shifted(rows[u], w[u])
    params = oracle.make_params(L, q, rmin, rmax, abi.MODE_FIXED_ONLY if fixed_only else abi.MODE_REFERENCE)
    if stereo:
        assert C == 2
        out = (LM.stereo_analyse if lpc_sign else SM.analyse)(x, params, n, tail, ss, threads=threads)
        if rice_search:
            done = {}
            for f in range(len(out)):
                for k, (samples, o, u, width) in enumerate(out[f]):
                    per = _lens(len(o["meta"]), 2 if k < 2 else 1, n, tail)
                    out[f][k] = (samples, _searched(o, per, rmin, rmax, done), u, width)
    else:
        n_tail = C if tail else 0
        if lpc_sign:
            out = LM.analyze(x, params, n, tail, n_tail, sample_bits=ss, threads=threads)
        else:
            out = oracle.analyze_batch(x, params, n, tail, n_tail, sample_bits=ss, threads=threads)
        if rice_search:
            out = RM.apply(out, lens, rmin, rmax)
    _ANALYSES[key] = (w, x, out)
    return _ANALYSES[key]


# ---------------------------------------------------------------------------------------
# step 4: the writers
# ---------------------------------------------------------------------------------------
def _sub(out, u, kind, w, cand):
    m = out["meta"][u]
    if kind != FM.ANALYSED:
        return Sub("CONSTANT" if kind == FM.CONSTANT else "VERBATIM", w, cand, 0, -1, False)
    prm = out["rice_params"][u][: int(m["n_parts"])]
    return Sub("LPC" if int(m["kind"]) == FW.KIND_LPC else "FIXED", w, cand, int(m["coding_method"]),
               max((int(v) for v in prm), default=-1), u in out.get("rescued", ()))


def _failed(exc, units):
    """The status word of a frame the writer gave up on: the first of its units (out, u), in
    subframe order, whose analysis failed; else the exception alone."""
    for out, u in units:
        st = int(out["meta"][u]["status"])
        if st != 0:
            return Failed(st, int(out["meta"][u]["site"]))
    return Failed(_STATUS_OF.get(type(exc), 0), None)


def _plain_frames(x, out, C, n, tail, ss, q, first_frame, fallback):
    got, kinds = FM.frames(x, out, C, n, tail, ss, q, first_frame, fallback=fallback)
    frames, subs = [], []
    for f, fr in enumerate(got):
        us = range(f * C, (f + 1) * C)
        if isinstance(fr, bytes):
            frames.append(fr)
            subs.append([_sub(out, u, kinds[u], 0, u - f * C) for u in us])
        else:
            frames.append(_failed(fr, [(out, u) for u in us if kinds[u] == FM.ANALYSED]))
            subs.append([])
    return Result(frames, None, subs)


def _wasted_frames(x, w, out, C, n, tail, ss, q, first_frame, fallback):
    """fallback_model.frames with every subframe at ss - w bits behind its wasted-bits header."""
    nf = x.shape[0] // C
    frames, subs = [], []
    for f in range(nf):
        ln = tail if (f == nf - 1 and tail) else n
        bits = FW.Bits()
        try:
            for b in FW.frame_header(first_frame + f, ln):
                bits.put(b, 8)
        except ValueError as e:
            frames.append(_failed(e, []))
            subs.append([])
            continue
        recs, err = [], None
        for u in range(f * C, (f + 1) * C):
            width = ss - w[u]
            kind = FM.sub_kind(x[u], out, u, ln, width, q) if fallback else FM.ANALYSED
            recs.append(_sub(out, u, kind, w[u], u - f * C))
            if kind != FM.ANALYSED:
                _wasted_raw_subframe(bits, x[u], ln, width, kind, w[u])
                continue
            m, zz, prm = FM._unit(out, u)
            try:
                if int(m["status"]) != 0:
                    raise FW._EXC.get(int(m["status"]), RuntimeError)()
                _wasted_subframe(bits, x[u], m, zz, prm, ln, width, q, w[u])
            except (ValueError, AssertionError, ZeroDivisionError, OverflowError, RuntimeError) as e:
                err = _failed(e, [(out, u)])
                break
        if err is not None:
            frames.append(err)
            subs.append([])
            continue
        bits.put(0, (8 - bits.n % 8) % 8)
        body = bits.to_bytes()
        frames.append(body + FW.crc16(body).to_bytes(2, "big"))
        subs.append(recs)
    return Result(frames, None, subs)


def _stereo_frames(x, cands, n, tail, q, first_frame, fallback):
    got, codes, sizes = SM.frames(x, cands, n, tail, q, first_frame, fallback)
    frames, subs = [], []
    for f, fr in enumerate(got):
        if isinstance(fr, bytes):
            a, b = next((a, b) for code, a, b in SC.ASSIGNMENTS if code == codes[f])
            frames.append(fr)
            subs.append([_sub(cands[f][k][1], cands[f][k][2], sizes[f][k][0], 0, k) for k in (a, b)])
            continue
        subs.append([])
        wide = [c for c in cands[f] if int(c[1]["meta"][c[2]]["status"]) == STATUS_RESIDUAL_WIDE]
        if wide:
            frames.append(Failed(STATUS_RESIDUAL_WIDE, int(wide[0][1]["meta"][wide[0][2]]["site"])))
        else:  # the status word the L_R frame has without the mode
            frames.append(_failed(fr, [(c[1], c[2]) for c, (kind, _) in zip(cands[f][:2], sizes[f][:2])
                                       if kind == FM.ANALYSED]))
    return Result(frames, codes, subs)


def frames(rows, C, n, tail, ss, L, q, rmin, rmax, first_frame=0, *, fixed_only=False, fallback=False, stereo=False,
           lpc_sign=False, wasted=False, rice_search=False) -> Result:
    """rows [frames * C][>= n] int16 / int32 in the flacmi_batch layout (row f * C + c is channel c of
    frame f, the last frame `tail` samples long when tail != 0) at stream sample size ss, analysed
    with LPC orders up to L, precision q and Rice partition orders rmin..rmax."""
    if not valid(fixed_only=fixed_only, lpc_sign=lpc_sign, wasted=wasted, stereo=stereo):
        raise ValueError("lpc_sign + fixed_only and wasted + stereo are refused")
    w, x, out = analysis(rows, C, n, tail, ss, L, q, rmin, rmax, fixed_only=fixed_only, stereo=stereo,
                         lpc_sign=lpc_sign, wasted=wasted, rice_search=rice_search)
    if stereo:
        return _stereo_frames(x, out, n, tail, q, first_frame, fallback)
    if wasted:
        return _wasted_frames(x, w, out, C, n, tail, ss, q, first_frame, fallback)
    return _plain_frames(x, out, C, n, tail, ss, q, first_frame, fallback)
