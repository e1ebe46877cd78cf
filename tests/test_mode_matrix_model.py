"""The composed CPU model of the encoder's opt-in modes (tests/mode_matrix_model.py), tied down
before any device byte is compared with it (tests/test_gpu_mode_matrix.py).  No GPU.

With exactly one mode on it reproduces every frame of every case of the five single-mode fixtures,
which the reference's own writers produced; every frame it writes for the routes and flag sets of
tests/mode_matrix_cases.py decodes to the input with the plain-integer decoder of
tests/decode_model.py; stereo, rice_search and fallback never make a frame larger and each makes
one smaller; the routes are the ones the host dispatch takes and the inputs give every mode that is
on something to do."""
import numpy as np
import pytest

import decode_model as DM
import fallback_cases as FC
import frame_writer as FW
import golden_util as G
import lpc_sign_cases as LC
import mode_matrix_cases as MC
import mode_matrix_model as MM
import oracle
import rice_search_cases as RC
import stereo_cases as SC
import wasted_cases as WC


def _same(got, want, same_frame, where):
    if isinstance(want, dict) and "raises" in want:
        assert isinstance(got, MM.Failed) and FW._EXC[got.status].__name__ == want["raises"], (where, got)
    else:
        assert isinstance(got, bytes) and same_frame(got, want), where


# ---------------------------------------------------------------------------------------
# single modes against the fixtures
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_fallback_alone_is_the_fallback_fixture(name):
    c, g = FC.CASES[name], G.load("fallback_streams.json")["cases"][name]
    rows, _ = FC.case_rows(name)
    r = MM.frames(rows, c["C"], c["n"], c["tail"], c["ss"], c["L"], c["q"], c["rmin"], c["rmax"], c["first"], fallback=True)
    assert len(r.frames) == len(g["frames"]) == c["frames"]
    for f, (got, want) in enumerate(zip(r.frames, g["frames"])):
        _same(got, want, FC.same_frame, (name, f))
    kinds = {"CONSTANT": FC.CONSTANT, "VERBATIM": FC.VERBATIM}
    assert [kinds.get(s.type, 0) for fr in r.subs for s in fr] == g["kinds"]


@pytest.mark.parametrize("name,mode", [(n, m) for n, c in sorted(SC.CASES.items()) for m in c["modes"]])
def test_stereo_alone_is_the_stereo_fixture(name, mode):
    c, g = SC.CASES[name], G.load("stereo_streams.json")["cases"][name][mode]
    rows, _ = SC.case_rows(name)
    r = MM.frames(rows, 2, c["n"], c["tail"], c["ss"], c["L"], c["q"], c["rmin"], c["rmax"], c["first"], stereo=True,
                  fallback=mode == "on")
    assert r.codes == g["codes"] and len(r.frames) == len(g["frames"])
    for f, (got, want) in enumerate(zip(r.frames, g["frames"])):
        _same(got, want, SC.same_frame, (name, mode, f))


@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_wasted_alone_is_the_wasted_fixture(name):
    """Every case, the fallback=True cases w15, w23 and fb16 among them: the first CPU statement of
    the wasted-bits writer's bytes."""
    c, g = WC.CASES[name], G.load("wasted_streams.json")["cases"][name]
    rows, _ = WC.case_rows(name)
    r = MM.frames(rows, c["C"], c["n"], c["tail"], c["ss"], c["L"], c["q"], c["rmin"], c["rmax"], c["first"], wasted=True,
                  fallback=c["fallback"])
    assert len(r.frames) == len(g["frames"]) == c["frames"]
    for f, (got, want) in enumerate(zip(r.frames, g["frames"])):
        _same(got, want, WC.same_frame, (name, f))
    assert [s.wasted for fr in r.subs for s in fr] == g["wasted"]
    assert [s.type for fr in r.subs for s in fr] == [s["type"] for s in g["subframes"]]


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_rice_search_alone_is_the_rice_search_fixture(name):
    c, g = RC.CASES[name], G.load("rice_search_streams.json")["cases"][name]
    rows, _ = RC.unit_rows(name)
    r = MM.frames(rows, c["C"], c["n"], RC.tail_len(name), c["ss"], c["L"], c["q"], c["rmin"], c["rmax"], rice_search=True)
    assert [f.hex() if isinstance(f, bytes) else repr(f) for f in r.frames] == g["frames"]
    rescued = [u for u, b in enumerate(g["reference"]) if b != "ok"]
    assert [u for u, s in enumerate(s for fr in r.subs for s in fr) if s.rescued] == rescued


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_lpc_sign_alone_is_the_lpc_sign_fixture(name):
    c, g = LC.CASES[name], G.load("lpc_sign_streams.json")["cases"][name]
    r = MM.frames(LC.case_rows(name), c["C"], c["n"], LC.tail_len(name), c["ss"], c["L"], c["q"], c["rmin"], c["rmax"],
                  lpc_sign=True)
    assert len(r.frames) == LC.n_blocks(name)
    for f, want in enumerate(g["frames"]):
        _same(r.frames[f], want, LC.same_frame, (name, f))
    if g["raises"] is not None:
        _same(r.frames[len(g["frames"])], {"raises": g["raises"]}, None, name)


def test_no_mode_is_the_oracle_frame_writer_and_wasted_without_wasted_bits_changes_nothing():
    c = MC.CASES["general_a"]
    rows = MC.case_rows("general_a")[:2]  # the frame whose units have no wasted bits
    out = oracle.analyze_batch(rows, oracle.make_params(c.L, c.q, c.rmin, c.rmax), c.n, sample_bits=c.ss)
    want = FW.frames_from_analysis(rows, out, 2, c.n, 0, c.ss, c.q)
    args = (rows, 2, c.n, 0, c.ss, c.L, c.q, c.rmin, c.rmax)
    assert MM.frames(*args).frames == want == MM.frames(*args, wasted=True).frames


def test_the_valid_combinations():
    sets = MM.combinations()
    assert len(sets) == 36 and len({MM.name_of(s) for s in sets}) == 36
    assert all(not (s["lpc_sign"] and s["fixed_only"]) and not (s["wasted"] and s["stereo"]) for s in sets)
    for bad in (dict(lpc_sign=True, fixed_only=True), dict(wasted=True, stereo=True)):
        with pytest.raises(ValueError):
            MM.frames(MC.case_rows("general_a"), 2, 192, 0, 16, 8, 5, 0, 4, **bad)
    assert len(MC.RUNS) == 36 + 4 * 10 and len(set(MC.RUNS)) == len(MC.RUNS)
    assert [r for r, _ in MC.RUNS].count("general") == 36
    for route in MC.ROUTES:
        if route != "general":
            names = [MM.name_of(s) for s in MC.flag_sets(route)]
            assert names[:6] == ["none", "fallback", "stereo", "lpc_sign", "wasted", "rice_search"]
            assert names[6:] == ["fallback+stereo+lpc_sign+rice_search", "fallback+lpc_sign+wasted+rice_search",
                                 "fixed_only+fallback+stereo+rice_search", "fixed_only+fallback+wasted+rice_search"]


# ---------------------------------------------------------------------------------------
# the routes and the premises of their inputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(MC.ROUTES))
def test_route_and_premises(route):
    MC.check_route(route)
    facts = MC.check_premises(route)
    print(route, facts)
    cases = MC.cases_of(route)
    tails = [c for c in cases if c.tail]
    assert tails and all(c.tail % 2 == 1 and c.tail < c.n for c in tails)
    assert all(len(c.frames) == 3 for c in cases if c.name != "stream_const_big")
    assert len(MC.CASES["stream_const_big"].frames) == 35
    if route == "mfma":
        extra = MC.CASES["mfma_l32"]
        assert (extra.n, extra.ss, extra.L, extra.q, extra.lpc_sign_only) == (1024, 24, 32, 15, True)


# ---------------------------------------------------------------------------------------
# round trip and smallness
# ---------------------------------------------------------------------------------------
_DECODED = {}


def _decodes_to(frame: bytes, ss: int, want: np.ndarray) -> bool:
    """decode_model on the frame (wasted bits as the format codes them), once per distinct frame."""
    key = (frame, ss)
    if key not in _DECODED:
        d = DM.decode(frame, 2, ss, spec_wasted_bits=True)
        _DECODED[key] = np.asarray(d.samples, dtype=np.int64) if isinstance(d, DM.Decoded) and d.end == len(frame) else d
    got = _DECODED[key]
    return isinstance(got, np.ndarray) and np.array_equal(got, want)


@pytest.mark.parametrize("route,flags", MC.RUNS)
def test_every_written_frame_decodes_to_the_input(route, flags):
    seen = 0
    for c in MC.cases_of(route, MC.SETS[flags]):
        rows = MC.case_rows(c.name)
        for f, fr in enumerate(MC.model(c.name, flags).frames):
            if isinstance(fr, bytes):
                ln = MC.frame_len(c, f)
                assert _decodes_to(fr, c.ss, rows[2 * f:2 * f + 2, :ln].astype(np.int64)), (c.name, flags, f)
                seen += 1
    assert seen >= 3


def _without(flags: dict, name: str) -> str:
    return MM.name_of({**flags, name: False})


@pytest.mark.parametrize("route", list(MC.ROUTES))
@pytest.mark.parametrize("mode", ["stereo", "rice_search", "fallback"])
def test_a_size_mode_never_grows_a_frame(route, mode):
    """Frame by frame, on the frames both flag sets can write: the set with the mode is no larger
    than the same set without it, and strictly smaller somewhere."""
    smaller = 0
    for s in MC.flag_sets(route):
        if not s[mode]:
            continue
        for c in MC.cases_of(route, s):
            on, off = MC.model(c.name, MM.name_of(s)).frames, MC.model(c.name, _without(s, mode)).frames
            for f, (a, b) in enumerate(zip(on, off)):
                if isinstance(b, bytes):
                    assert isinstance(a, bytes) and len(a) <= len(b), (c.name, MM.name_of(s), f, len(b))
                    smaller += len(a) < len(b)
    assert smaller >= 1


@pytest.mark.parametrize("flags", ["fixed_only+fallback+rice_search", "fixed_only+fallback+wasted+rice_search",
                                   "fixed_only+fallback+stereo+rice_search", "fallback+rice_search"])
def test_constant_blocks_the_rice_search_rescues_are_constant(flags):
    """const_rescued: a silent or constant block, whose all-zero residual the search rescues at one
    bit a sample, is CONSTANT under fallback (no larger than with rice_search off); a ramp stays
    FIXED.  The device side: tests/test_gpu_mode_matrix.py."""
    c, s = MC.CASES["const_rescued"], MC.SETS[flags]
    rows = MC.case_rows(c.name)
    on, off = MC.model(c.name, flags), MC.model(c.name, _without(s, "rice_search"))
    types = [[x.type for x in fr] for fr in on.subs]
    if s["stereo"]:
        assert on.codes[0] == SC.L_R and types[0] == ["CONSTANT", "CONSTANT"]
    else:
        assert types == [["CONSTANT", "CONSTANT"], ["CONSTANT", "FIXED"], ["FIXED", "CONSTANT"]]
        assert [[x.rescued for x in fr] for fr in on.subs] == [[False, False], [False, True], [True, False]]
    if s["wasted"]:
        assert [[x.wasted for x in fr] for fr in on.subs] == [[0, 0], [4, 0], [0, 2]]
    for f, (a, b) in enumerate(zip(on.frames, off.frames)):
        assert len(a) <= len(b) and _decodes_to(a, c.ss, rows[2 * f:2 * f + 2].astype(np.int64)), f
    assert len(on.frames[0]) == len(off.frames[0]) and len(on.frames[1]) < len(off.frames[1])
