"""The device encoder's opt-in modes in combination, at the smallest shape of every production
analysis route (tests/mode_matrix_cases.py: the general k_resid, k_resid_stream with the runtime and
the constant shape and k_lpc_tile, k_resid_sb, the int8-MFMA kernels), byte for byte against the
composed CPU model (tests/mode_matrix_model.py, tied to the reference's writers by
tests/test_mode_matrix_model.py): all 36 valid flag sets at 192 samples, ten at each of the other
routes; through flacmi_encode_host and flacmi_encode_pipeline with a sub-batch edge inside every
case; with the FLACMI_STREAM_GENERIC and FLACMI_OVERLAP knobs; through encoder.encode_planar and
back through the device decoder; and the two refused combinations at production shapes."""
import ctypes as C

import numpy as np
import pytest

import frame_writer as FW
import mode_matrix_cases as MC
import mode_matrix_model as MM
from flac_amd import abi
from flac_amd import encoder as enc
from flac_amd._lib import FlacmiError
from flac_amd.analysis import Analyzer, device_batch, frame_params, knob, make_params, unit_stride
from flac_amd.decoder import decode

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
MAXIMAL = [MM.name_of(s) for s in MC.MAXIMAL]


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def _params(c, s):
    return make_params(c.L, c.q, c.rmin, c.rmax, abi.MODE_FIXED_ONLY if s["fixed_only"] else abi.MODE_REFERENCE,
                       lpc_sign=s["lpc_sign"], rice_search=s["rice_search"])


def _kw(c, s):
    return dict(sample_bits=c.ss, channels=2, sample_size=c.ss, fallback=s["fallback"], stereo=s["stereo"],
                wasted=s["wasted"])


def _check(c, flags, data, offsets, status, how):
    """Offsets, statuses and every frame's bytes are the model's; a frame the model fails has no
    bytes and the model's status and site."""
    want = MC.model(c.name, flags)
    where = f"{c.name} {flags} {how}"
    assert len(offsets) == len(want.frames) + 1 == len(status) + 1 and offsets[0] == 0, where
    for f, w in enumerate(want.frames):
        got = bytes(data[int(offsets[f]):int(offsets[f + 1])])
        if isinstance(w, MM.Failed):
            word = int(status[f])
            assert got == b"" and word & 0xFFFF == w.status and (w.site is None or word >> 16 == w.site), \
                f"{where}: frame {f} status {word:#x}, the model's {w}"
        else:
            assert int(status[f]) == 0, f"{where}: frame {f} status {int(status[f]):#x}"
            if got != w:
                first = next((i for i, (a, b) in enumerate(zip(got, w)) if a != b), min(len(got), len(w)))
                raise AssertionError(f"{where}: frame {f} has {len(got)} bytes, the model's {len(w)}; first difference at "
                                     f"byte {first}; subframes {want.subs[f]}, code {want.codes[f] if want.codes else None}")
    assert int(offsets[-1]) == len(data) == sum(len(w) for w in want.frames if isinstance(w, bytes)), where


def _host(az, c, flags):
    s = MC.SETS[flags]
    rows = MC.case_rows(c.name)
    data, offsets, status = az.encode_frames(rows, _params(c, s), c.n, c.tail, MC.n_tail_units(c), **_kw(c, s))
    _check(c, flags, data, offsets, status, "encode_host")
    return offsets, status


def _pipeline(az, c, flags):
    s = MC.SETS[flags]
    rows = MC.case_rows(c.name)
    per = MC.sub_batch_frames(c)
    out = np.full(int(rows.shape[0] * (c.n * rows.itemsize * 1.25 + 256)) + (1 << 16), SENTINEL, dtype=np.uint8)
    data, offsets, status, timing = az.encode_pipeline(rows, _params(c, s), c.n, c.tail, MC.n_tail_units(c),
                                                       units_per_batch=2 * per, out=out, **_kw(c, s))
    _check(c, flags, data, offsets, status, "encode_pipeline")
    assert timing["sub_batches"] == (len(c.frames) + per - 1) // per >= 2
    assert (out[int(offsets[-1]):] == SENTINEL).all(), f"{c.name} {flags}: bytes behind the last frame were written"
    return offsets, status


@pytest.mark.parametrize("route,flags", MC.RUNS)
def test_frames_are_the_composed_models(az, route, flags):
    MC.check_route(route)
    MC.check_premises(route)
    if route == "stream_rt":
        assert unit_stride(MC.PITCH_N, 2) == MC.row_pitch(MC.PITCH_N, 2) < unit_stride(MC.PITCH_N, 4) == MC.row_pitch(MC.PITCH_N, 4)
    for c in MC.cases_of(route, MC.SETS[flags]):
        before = MC.case_rows(c.name).copy()
        offsets, status = _host(az, c, flags)
        poff, pst = _pipeline(az, c, flags)
        assert np.array_equal(poff, offsets) and np.array_equal(pst, status)
        assert np.array_equal(MC.case_rows(c.name), before)


@pytest.mark.parametrize("flags", MAXIMAL)
@pytest.mark.parametrize("route", ["stream_rt", "stream_const"])
def test_the_generic_stream_build_writes_the_same_bytes(az, route, flags):
    with knob("FLACMI_STREAM_GENERIC", 1):
        for c in MC.cases_of(route, MC.SETS[flags]):
            _host(az, c, flags)
            _pipeline(az, c, flags)


@pytest.mark.parametrize("flags", MAXIMAL)
@pytest.mark.parametrize("route", list(MC.ROUTES))
def test_the_overlap_split_writes_the_same_bytes(az, route, flags):
    """FLACMI_OVERLAP = -8: chunks of 8-unit rounds; in stereo mode each of the three analyses makes
    its own split."""
    with knob("FLACMI_OVERLAP", -8):
        for c in MC.cases_of(route, MC.SETS[flags]):
            _host(az, c, flags)
            _pipeline(az, c, flags)


def _encoder_parameters(c):
    return enc.EncoderParameters(block_size=c.n, rice_partition_order=range(c.rmin, c.rmax + 1),
                                 lpc_order=range(0, c.L + 1), qlp_precision=c.q)


@pytest.mark.parametrize("flags", [MM.name_of(s) for s in MC.API_SETS])
@pytest.mark.parametrize("route", list(MC.ROUTES))
def test_encode_planar_writes_the_models_stream(route, flags):
    s = MC.SETS[flags]
    for c in MC.cases_of(route, s):
        want = MC.model(c.name, flags).frames
        assert all(isinstance(f, bytes) for f in want), c.name
        pcm = MC.pcm(c.name)
        stream = FW.stream_header(c.rate, c.ss, 2, pcm.shape[1], c.n) + b"".join(want)
        ep = _encoder_parameters(c)
        got = b"".join(enc.encode_planar(c.rate, c.ss, pcm, ep, **s))
        assert got[:42] == stream[:42] and got == stream, c.name
        assert b"".join(enc.encode_planar(c.rate, c.ss, pcm, ep, blocks_per_batch=1, devices=[0, 0], **s)) == stream, c.name
        rate, ss, ch, total, samples = decode(got, check_crc=True, spec_wasted_bits=s["wasted"])
        assert (rate, ss, ch, total) == (c.rate, c.ss, 2, pcm.shape[1])
        assert np.array_equal(np.asarray(list(samples), dtype=np.int64).reshape(-1, 2).T, pcm), c.name


REFUSED = [("lpc_sign", "fixed_only"), ("wasted", "stereo")]


@pytest.mark.parametrize("name", ["stream_const_tail", "sb_a"])
@pytest.mark.parametrize("pair", REFUSED, ids="+".join)
def test_refused_combinations_at_production_shapes(az, name, pair):
    """ValueError from the encoder before any device work (the generator's first step); FLACMI_E_INVALID
    from both C entry points, with nothing written to the frame buffer."""
    c = MC.CASES[name]
    s = {f: f in pair or f == "fallback" for f in MM.FLAGS}
    pcm = MC.pcm(name)
    with pytest.raises(ValueError, match=pair[0]):
        next(enc.encode_planar(c.rate, c.ss, pcm, _encoder_parameters(c), **s))
    with pytest.raises(ValueError, match=pair[0]):
        next(enc.encode(c.rate, c.ss, 2, pcm.shape[1], iter(()), _encoder_parameters(c), **s))
    rows = MC.case_rows(name)
    p = _params(c, s)
    with pytest.raises(FlacmiError) as e:
        az.encode_frames(rows, p, c.n, c.tail, MC.n_tail_units(c), **_kw(c, s))
    assert e.value.code == abi.E_INVALID
    with pytest.raises(FlacmiError) as e:
        az.encode_pipeline(rows, p, c.n, c.tail, MC.n_tail_units(c), units_per_batch=4, **_kw(c, s))
    assert e.value.code == abi.E_INVALID
    # the raw entry points
    hb = device_batch(rows.ctypes.data, rows.itemsize, c.ss, rows.shape[1], rows.shape[0], c.n, c.tail, MC.n_tail_units(c))
    fp = frame_params(2, c.ss, c.q, fallback=True, stereo=s["stereo"], wasted=s["wasted"])
    nf = len(c.frames)
    off, st = np.full(nf + 1, -1, dtype=np.int64), np.full(nf, -1, dtype=np.int32)
    out = np.full(1 << 16, SENTINEL, dtype=np.uint8)
    lib = az.lib
    assert lib.flacmi_encode_host(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), off.ctypes.data, st.ctypes.data) == abi.E_INVALID
    assert lib.flacmi_encode_pipeline(az.ctx, C.byref(hb), C.byref(p), C.byref(fp), 4, out.ctypes.data, out.size,
                                      off.ctypes.data, st.ctypes.data, None) == abi.E_INVALID
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("flags", ["fixed_only+fallback+rice_search", "fixed_only+fallback+wasted+rice_search",
                                   "fixed_only+fallback+stereo+rice_search", "fallback+rice_search"])
def test_constant_blocks_the_rice_search_rescues_are_constant(az, flags):
    """const_rescued (tests/mode_matrix_cases.py): with fixed predictors only, the reference's Rice step
    fails a silent or constant block (its residual is all zeros), the search rescues it at one bit a
    sample, and the fallback rule used to keep that FIXED subframe, 24 bytes where CONSTANT takes 3: the
    stream grew when rice_search was switched on.  Such a unit is CONSTANT; a ramp, whose residual is
    all zeros as well, stays FIXED."""
    c = MC.CASES["const_rescued"]
    want = MC.model(c.name, flags)
    types = [[x.type for x in fr] for fr in want.subs]
    if MC.SETS[flags]["stereo"]:
        assert want.codes[0] == 1 and types[0] == ["CONSTANT", "CONSTANT"]
    else:
        assert types == [["CONSTANT", "CONSTANT"], ["CONSTANT", "FIXED"], ["FIXED", "CONSTANT"]]
    _host(az, c, flags)
    _pipeline(az, c, flags)
