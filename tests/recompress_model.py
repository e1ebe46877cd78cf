"""numpy restatement of k_units (flacmi_units_out_device, include/flacmi.h) and the cases the
CPU and GPU tests share.

A frame is an int array [channels][block_size]; the frames follow one another, frame f starting
at sample first[f] (the sum of the block sizes before it unless given).  Sample s >= S0 of
channel c goes to unit ((s - S0) // B) * C + c, element (s - S0) % B; n_blocks whole blocks and,
when tail_len > 0, one block of tail_len samples are written, everything from a unit's length
to the pitch as 0, a sample no frame holds as 0.  status[f] = 4 (FLACMI_STATUS_OVERFLOW) where a
sample of frame f that is read does not fit sample_size bits; width = the maximum over the
samples read of x >= 0 ? x : ~x.
"""
import numpy as np

STATUS_OVERFLOW = 4


def firsts_of(frames):
    out, s = [], 0
    for x in frames:
        out.append(s)
        s += np.asarray(x).shape[-1]
    return out


def units_out(frames, channels, s0, block_len, n_blocks, tail_len, sample_size, dtype, stride, firsts=None):
    """-> (units [n_units][stride] of dtype, status [n_frames] int32, width, mask [n_units][stride]
    bool: False where the element comes from a frame with a range finding, which the kernel
    leaves unspecified)."""
    C, B = channels, block_len
    firsts = firsts_of(frames) if firsts is None else list(firsts)
    n_units = (n_blocks + (1 if tail_len else 0)) * C
    need = n_blocks * B + tail_len
    line = np.zeros((C, need), dtype=np.int64)       # the timeline from s0 on
    owner = np.full(need, -1, dtype=np.int64)        # the frame each sample comes from
    for f, x in enumerate(frames):
        x = np.asarray(x, dtype=np.int64).reshape(C, -1)
        lo, hi = firsts[f] - s0, firsts[f] - s0 + x.shape[1]
        a, b = max(lo, 0), min(hi, need)
        if a < b:
            line[:, a:b] = x[:, a - lo:b - lo]
            owner[a:b] = f
    read = owner >= 0
    status = np.zeros(len(frames), dtype=np.int32)
    lo_v, hi_v = -(1 << (sample_size - 1)), (1 << (sample_size - 1)) - 1
    bad = ((line < lo_v) | (line > hi_v)).any(axis=0) & read
    status[np.unique(owner[bad])] = STATUS_OVERFLOW
    mag = np.where(line >= 0, line, ~line)[:, read]
    width = int(mag.max()) if mag.size else 0
    units = np.zeros((n_units, stride), dtype=dtype)
    mask = np.ones((n_units, stride), dtype=bool)
    tainted = read & np.isin(owner, np.nonzero(status)[0])
    for blk in range(n_blocks + (1 if tail_len else 0)):
        n = B if blk < n_blocks else tail_len
        seg = slice(blk * B, blk * B + n)
        units[blk * C:(blk + 1) * C, :n] = line[:, seg].astype(dtype)  # two's complement truncation
        mask[blk * C:(blk + 1) * C, :n] = ~tainted[seg]
    return units, status, width, mask


def units_out_loop(frames, channels, s0, block_len, n_blocks, tail_len, sample_size, dtype, stride, firsts=None):
    """The same, one sample at a time (the definition, word for word)."""
    C, B = channels, block_len
    firsts = firsts_of(frames) if firsts is None else list(firsts)
    n_units = (n_blocks + (1 if tail_len else 0)) * C
    units = np.zeros((n_units, stride), dtype=dtype)
    status = np.zeros(len(frames), dtype=np.int32)
    width = 0
    last = s0 + n_blocks * B + tail_len  # samples at and past it are not read
    lo_v, hi_v = -(1 << (sample_size - 1)), (1 << (sample_size - 1)) - 1
    half = 1 << (8 * np.dtype(dtype).itemsize - 1)
    for f, x in enumerate(frames):
        x = np.asarray(x).reshape(C, -1).tolist()
        for t in range(len(x[0]) if x else 0):
            s = firsts[f] + t
            if s < s0 or s >= last:
                continue
            for c in range(C):
                v = x[c][t]
                if v < lo_v or v > hi_v:
                    status[f] = STATUS_OVERFLOW
                width = max(width, v if v >= 0 else ~v)
                units[((s - s0) // B) * C + c, (s - s0) % B] = ((v + half) & (2 * half - 1)) - half  # truncation
    return units, status, width


def sample_bits(width: int, sample_size: int) -> int:
    """flacmi_batch.sample_bits from the measured width (what encoder._sample_bits measures on the host)."""
    return min(sample_size, max(2, int(width).bit_length() + 1))


def pitch_for(block_len: int, sample_bytes: int, alt: bool) -> int:
    """flacmi_unit_stride's rule (alt False), or another multiple of 16 bytes that holds the block."""
    b = ((block_len * sample_bytes + 15) // 16) * 16
    if alt:
        return (b + 48) // sample_bytes
    if b % 4096 == 0:
        b += 128
    return b // sample_bytes


BLOCKS = (1, 7, 8, 9, 16, 100, 192, 4608)
CHANNELS = (1, 2, 3, 8)
MIXED = (17, 1, 3, 16, 100, 192, 1000, 5000, 17, 1, 192, 3, 1000)


def _frames(rng, C, sizes, bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    out = []
    for n in sizes:
        x = rng.integers(lo, hi + 1, size=(C, n), dtype=np.int64)
        if n:
            x[rng.integers(0, C), rng.integers(0, n)] = (lo, hi)[int(rng.integers(0, 2))]
        out.append(x.astype(np.int32))
    return out


def _pitches(sizes, k):
    """Two different row pitches in one list, as pass-1 rows (one pitch for all) and pass-2 rows
    (another) are."""
    big = ((max(list(sizes) + [1]) + 3) // 4) * 4
    return [big + 8 if (i + k) % 3 == 0 else big for i in range(len(sizes))]


def cases():
    """name -> dict(frames, pitches, channels, s0, block_len, n_blocks, tail_len, sample_size,
    sample_bytes, stride).  Deterministic."""
    out = {}
    i = 0
    for rot in (0, 1):
        for B in BLOCKS:
            for C in CHANNELS:
                k = i + 5 * rot
                i += 1
                rng = np.random.default_rng(1000 + k)
                carry = (0, 1, B - 1)[k % 3]
                sizes = (carry,) + MIXED[: (13 if B >= 100 else 7)]
                sbytes = (2, 4)[(k // 3) % 2]
                ss = 16 if sbytes == 2 else (24, 32, 20)[k % 3]
                frames = _frames(rng, C, sizes, ss)
                total = sum(sizes)
                s0 = (0, 1, B - 1, carry + sizes[1] + 2)[(k // 2) % 4]
                avail = total - s0
                layout = ("whole", "tail", "both")[(k // 4) % 3]
                if layout == "whole":
                    nb, tail = max(avail // B, 1), 0
                elif layout == "tail" and B > 1:
                    nb, tail = 0, min(B - 1, avail)
                    s0 = total - tail if (k % 2) else s0   # the carry extraction: the stream's last samples
                else:
                    nb, tail = avail // B, avail % B
                    if B > 1 and k % 4 == 0:
                        nb, tail = max(nb - 1, 0), B // 2  # frames go on past the last unit: not read
                out[f"b{B}_c{C}_r{rot}_{layout}_s{s0}_k{carry}_{'i16' if sbytes == 2 else 'i32'}"] = dict(
                    frames=frames, pitches=_pitches(sizes, k), channels=C, s0=s0, block_len=B, n_blocks=nb,
                    tail_len=tail, sample_size=ss, sample_bytes=sbytes,
                    stride=pitch_for(B, sbytes, bool((k // 5) % 2)))
    rng = np.random.default_rng(7)
    # 300 one-sample frames inside one unit
    sizes = (5,) + (1,) * 300 + (40,)
    out["one_sample_frames_x300"] = dict(frames=_frames(rng, 2, sizes, 16), pitches=_pitches(sizes, 1), channels=2,
                                         s0=0, block_len=400, n_blocks=0, tail_len=345, sample_size=16,
                                         sample_bytes=2, stride=pitch_for(400, 2, False))
    out["one_sample_frames_x300_whole"] = dict(frames=_frames(rng, 3, sizes, 24), pitches=_pitches(sizes, 2),
                                               channels=3, s0=2, block_len=320, n_blocks=1, tail_len=20,
                                               sample_size=24, sample_bytes=4, stride=pitch_for(320, 4, True))
    # one 5000-sample frame across 27 units of 192
    sizes = (100, 5000, 192)
    out["frame_5000_over_27_units"] = dict(frames=_frames(rng, 2, sizes, 16), pitches=_pitches(sizes, 0), channels=2,
                                           s0=0, block_len=192, n_blocks=27, tail_len=108, sample_size=16,
                                           sample_bytes=2, stride=pitch_for(192, 2, False))
    # a gap in the list and samples no frame holds: zeros
    sizes = (50, 60, 70)
    out["gap_and_short_list"] = dict(frames=_frames(rng, 2, sizes, 16), pitches=_pitches(sizes, 0), channels=2, s0=0,
                                     block_len=64, n_blocks=4, tail_len=10, sample_size=16, sample_bytes=4,
                                     stride=pitch_for(64, 4, False), firsts=(0, 60, 120))
    out["no_frames"] = dict(frames=[], pitches=[], channels=2, s0=0, block_len=16, n_blocks=2, tail_len=3,
                            sample_size=16, sample_bytes=2, stride=pitch_for(16, 2, False))
    # the range check: 16 bits with the two extremes (fit), one past each (status, that frame only)
    for name, ss, sbytes, vals, bad in (
            ("range16_fits", 16, 2, (32767, -32768), False), ("range16_fits_i32", 16, 4, (32767, -32768), False),
            ("range16_over_hi", 16, 4, (32768, 5), True), ("range16_over_lo", 16, 4, (7, -32769), True),
            ("range12_i16_fits", 12, 2, (2047, -2048), False), ("range12_i16_over_hi", 12, 2, (2048, 1), True),
            ("range12_i16_over_lo", 12, 2, (3, -2049), True), ("range24_fits", 24, 4, (8388607, -8388608), False),
            ("range24_over_hi", 24, 4, (8388608, 0), True), ("range24_over_lo", 24, 4, (0, -8388609), True),
            ("range32_extremes", 32, 4, (2147483647, -2147483648), False),
            ("range5_fits", 5, 2, (15, -16), False), ("range5_over", 5, 2, (16, -16), True)):
        sizes = (9, 30, 21, 40)
        quiet = min(ss, 10)
        frames = _frames(np.random.default_rng(ss), 2, sizes, quiet - 1)
        frames[2][0, 20] = vals[0]   # the third frame's last sample
        frames[2][1, 0] = vals[1]    # and its first
        out[name] = dict(frames=frames, pitches=_pitches(sizes, 0), channels=2, s0=0, block_len=32, n_blocks=3,
                         tail_len=4, sample_size=ss, sample_bytes=sbytes, stride=pitch_for(32, sbytes, False),
                         bad_frames=(2,) if bad else ())
    # the finding lies in samples past the last unit: not read, no status
    sizes = (9, 30, 21, 40)
    frames = _frames(np.random.default_rng(3), 1, sizes, 9)
    frames[3][0, 39] = 40000
    out["range16_unread_tail"] = dict(frames=frames, pitches=_pitches(sizes, 0), channels=1, s0=0, block_len=32,
                                      n_blocks=3, tail_len=3, sample_size=16, sample_bytes=4,
                                      stride=pitch_for(32, 4, False), bad_frames=())
    return out


def model_args(case):
    return (case["frames"], case["channels"], case["s0"], case["block_len"], case["n_blocks"], case["tail_len"],
            case["sample_size"], np.int16 if case["sample_bytes"] == 2 else np.int32, case["stride"])
