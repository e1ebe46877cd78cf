"""k_planar alone (csrc/k_planar.hip, flacmi_planar_out_device) against a numpy model: the frame
lists of many streams as one padded planar buffer of int16, int32 or float32.

Every case runs between two guard regions, in a buffer whose every byte (the pitch padding
included) is garbage beforehand: the rows must equal the model's element for element up to the
pitch (zeros from each stream's length on), the guards must be untouched, and the status word of
every frame must be the model's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DT = {"int16": np.int16, "int32": np.int32, "float32": np.float32}
BLOCKS = [1, 3, 4, 5, 7, 8, 9, 191, 192, 193]


@pytest.fixture(scope="module")
def az():
    from flac_amd.analysis import Analyzer
    a = Analyzer(0)
    yield a
    a.close()


def model(streams, channels, elem, sample_size, pitch, lengths=None):
    """-> (rows [N * C][pitch], status per frame in list order, mask of the elements that are
    specified: a frame with a range finding leaves its samples unspecified)"""
    n = len(streams)
    ref = np.zeros((n * channels, pitch), dtype=np.int64)
    mask = np.ones((n * channels, pitch), dtype=bool)
    status = []
    for s, frames in enumerate(streams):
        first = 0
        for x, _ in frames:
            x = np.asarray(x, dtype=np.int64).reshape(channels, -1)
            end = min(first + x.shape[1], pitch, x.shape[1] + first if lengths is None else lengths[s])
            k = max(end - first, 0)
            bad = elem == "int16" and k > 0 and bool(((x[:, :k] < -32768) | (x[:, :k] > 32767)).any())
            status.append(4 if bad else 0)  # FLACMI_STATUS_OVERFLOW
            if k > 0:
                ref[s * channels:(s + 1) * channels, first:end] = x[:, :k]
                if bad:
                    mask[s * channels:(s + 1) * channels, first:end] = False
            first += x.shape[1]
    if elem == "float32":
        rows = ref.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -(sample_size - 1))
    else:
        rows = ref.astype(DT[elem])
    return rows, np.array(status, dtype=np.int32), mask


def run(az, streams, channels, elem, sample_size=16, pitch=0, lengths=None, fill=0x5A):
    buf, g, pitch, st = az.planar_out(streams, channels, elem, sample_size, pitch=pitch, lengths=lengths, fill=fill)
    dt = DT[elem]
    assert buf.dtype == dt
    n_rows = len(streams) * channels
    raw = buf.view(np.uint8)
    sb = dt().itemsize
    assert (raw[:g * sb] == fill).all(), "guard before the rows written"
    assert (raw[(g + n_rows * pitch) * sb:] == fill).all(), "guard behind the rows written"
    return buf[g:g + n_rows * pitch].reshape(n_rows, pitch), st, pitch


def same(got, want):
    if got.dtype == np.float32:
        return got.view(np.uint32) == want.view(np.uint32)
    return got == want


def check(az, streams, channels, elem, sample_size=16, pitch=0, lengths=None):
    got, st, pitch = run(az, streams, channels, elem, sample_size, pitch, lengths)
    want, status, mask = model(streams, channels, elem, sample_size, pitch, lengths)
    assert np.array_equal(st, status), (np.nonzero(st)[0], np.nonzero(status)[0])
    bad = np.argwhere(~same(got, want) & mask)
    assert bad.size == 0, f"first differing (row, element): {bad[:5].tolist()}"
    return got, st


def frames_of(rng, sizes, channels, bits, pitches=(0,)):
    """one stream: frames of these sizes, random samples of `bits` bits, source pitches in turn
    (0: the block size rounded up to 4)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    out = []
    for k, bs in enumerate(sizes):
        x = rng.integers(lo, hi, size=(channels, bs), endpoint=True, dtype=np.int64)
        x[:, 0] = (lo, hi)[k & 1]  # the extremes are samples like any other
        fp = pitches[k % len(pitches)] or (bs + 3) // 4 * 4
        out.append((x, max(fp, (bs + 3) // 4 * 4)))
    return out


def library(rng, channels, bits):
    """the shapes of the issue in one list: every block size around a 16-byte group, 300 frames of
    one sample, a frame start at every residue of a group, a row longer than a workgroup's 2048
    elements, rows of two source pitches (pass 1's and pass 2's), a stream with no frame"""
    return [frames_of(rng, BLOCKS, channels, bits),
            frames_of(rng, [1] * 300, channels, bits),
            [],
            frames_of(rng, [9] * 9, channels, bits, pitches=(12, 260)),
            frames_of(rng, [193] * 12, channels, bits, pitches=(196, 4608)),
            frames_of(rng, [192, 192, 50], channels, bits, pitches=(192, 1152)),
            []]


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("elem,bits", [("int16", 16), ("int32", 32), ("float32", 8), ("float32", 16), ("float32", 20),
                                       ("float32", 24), ("float32", 32)])
def test_rows_equal_the_model(az, elem, bits, channels):
    rng = np.random.default_rng(1000 * channels + bits)
    streams = library(rng, channels, bits)
    firsts = np.concatenate([np.cumsum([0] + [f[0].shape[1] for f in s])[:-1] for s in streams if s])
    g = 16 // DT[elem]().itemsize
    assert set(firsts % g) == set(range(g))  # a frame boundary at every residue of a store group
    got, st = check(az, streams, channels, elem, sample_size=bits)
    assert not st.any()
    assert not got[2 * channels:3 * channels].any() and not got[-channels:].any()  # the streams with no frame


@pytest.mark.parametrize("elem", ["int16", "int32", "float32"])
@pytest.mark.parametrize("extra_groups", [0, 1])
def test_pitch_equal_to_the_length_and_one_group_more(az, elem, extra_groups):
    rng = np.random.default_rng(5)
    g = 16 // DT[elem]().itemsize
    streams = [frames_of(rng, [192, 192, 8], 2, 16), frames_of(rng, [192, 7], 2, 16)]
    pitch = 392 + extra_groups * g
    got, _ = check(az, streams, 2, elem, pitch=pitch)
    assert got.shape[1] == pitch and not got[2:, 199:].any() and not got[:2, 392:].any()


@pytest.mark.parametrize("elem", ["int16", "int32", "float32"])
def test_lengths_cut_a_stream_and_the_rest_is_zero(az, elem):
    """lengths[s] inside a frame, at a frame's start, at 0 and past the last frame"""
    rng = np.random.default_rng(6)
    streams = [frames_of(rng, [192, 192, 192], 1, 16) for _ in range(4)]
    lengths = [200, 384, 0, 10 ** 6]
    got, _ = check(az, streams, 1, elem, lengths=lengths)
    for s, n in enumerate(lengths):
        assert not got[s, min(n, 576):].any()
        assert n == 0 or got[s, :min(n, 576)].any()


def test_zero_fill_does_not_depend_on_what_was_there(az):
    rng = np.random.default_rng(7)
    streams = library(rng, 2, 16)
    a, _, _ = run(az, streams, 2, "int16", fill=0x5A)
    b, _, _ = run(az, streams, 2, "int16", fill=0xC3)
    assert np.array_equal(a, b)


def test_int16_finding_marks_its_frame_and_only_that_one(az):
    """32767 and -32768 pass; 32768 and -32769 mark their frame; int32 and float32 check nothing"""
    rng = np.random.default_rng(8)
    streams = [frames_of(rng, [192] * 5, 2, 16), frames_of(rng, [7] * 6, 2, 16), frames_of(rng, [192] * 2, 2, 16)]
    streams[0][0][0][1, 100] = 32767
    streams[0][1][0][0, 5] = -32768
    streams[0][2][0][1, 191] = 32768       # frame 2
    streams[1][4][0][0, 0] = -32769        # frame 5 + 4 = 9
    streams[1][5][0][1, 6] = 32767
    got, st = check(az, streams, 2, "int16")
    assert tuple(np.nonzero(st)[0]) == (2, 9) and set(st[[2, 9]]) == {4}
    for elem in ("int32", "float32"):
        _, st = check(az, streams, 2, elem, sample_size=24)
        assert not st.any()
    # a finding past lengths[s] is not read
    _, st = check(az, streams, 2, "int16", lengths=[384, 28, 384])
    assert not st.any()


def test_status_is_reset_and_arguments_are_checked(az):
    from flac_amd import abi
    from flac_amd._lib import FlacmiError
    rng = np.random.default_rng(9)
    _, st, _ = run(az, [frames_of(rng, [5, 5], 1, 16)], 1, "int16")  # az.planar_out fills the status with -1 first
    assert st.tolist() == [0, 0]
    for kw in ({"pitch": 12}, {"sample_size": 3}, {"sample_size": 33}):
        with pytest.raises(FlacmiError) as e:
            run(az, [frames_of(rng, [5], 1, 16)], 1, "int16", **kw)
        assert e.value.code == abi.E_INVALID
