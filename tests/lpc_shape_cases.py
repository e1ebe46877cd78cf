"""The k_lpc kernels' shape family (flac-py_amd/csrc/k_lpc.hip): the host dispatch and each build's
loop bounds restated in Python, the table of block lengths the suite runs through them, their
inputs and the conditions those inputs must meet on the CPU oracle.  Shared by
tests/test_lpc_shape_cases.py (no device) and tests/test_gpu_lpc_shapes.py.  Test infrastructure
only; importing it needs no GPU.

Three kernel families compute the same f64 chains (Tukey-windowed autocorrelation, Levinson-Durbin,
quantiser), named here
  "tile"  k_lpc_tile<4|8|12>: int16, whole waves of 64 units, 64-sample tiles through LDS;
  "gen16" k_lpc<LMAX,int16_t>: the count % 64 remainder, calls below 64 units, every L > 12;
  "ring"  k_lpc<LMAX,int32_t>: ring cycles of S samples prefetched one cycle ahead."""
import functools
from collections import namedtuple

import numpy as np

import oracle
from flac_amd import abi

WINDOW_PAD = 80   # flacmi_kernels.h kWindowPad: zero weights behind the n of a unit's window
FUSE_MAX_BITS = 26  # flacmi_host.cpp: sample_bits > 26 turns the fused rectangle off
LMAXES = (4, 8, 12, 16, 32)


# ---------------------------------------------------------------------------------------
# the dispatch and the loop bounds, restated line for line
# ---------------------------------------------------------------------------------------
def row_pitch(n, sample_bytes):
    """flacmi_host.cpp row_pitch: the device row pitch in samples."""
    b = ((n * sample_bytes + 15) // 16) * 16
    if b % 4096 == 0:
        b += 128
    return b // sample_bytes


@functools.lru_cache(maxsize=None)
def window_ones(n):
    """get_window: the longest run [lo, hi) of weights exactly 1.0 in the n-sample window (the first
    of equally long runs).  n in 4..7 raises in the reference's tukey(); the kernels return before
    they use the window there (None)."""
    st, w = oracle.tukey(n)
    if st:
        return None
    lo = hi = 0
    i = 0
    while i < n:
        if w[i] != 1.0:
            i += 1
            continue
        j = i
        while j < n and w[j] == 1.0:
            j += 1
        if j - i > hi - lo:
            lo, hi = i, j
        i = j
    return lo, hi


def rectangle(n, sample_bits):
    """LpcArgs.fuse_lo / fuse_hi as analyze_device_impl's lpc_args sets them."""
    r = window_ones(n)
    if r is None:
        return None
    return (0, 0) if sample_bits > FUSE_MAX_BITS else r


def lmax_of(L):
    """launch_lpc: the build's LMAX."""
    return 4 if L <= 4 else 8 if L <= 8 else 12 if L <= 12 else 16 if L <= 16 else 32


def ring_len(lmax):
    """S: ((LMAX + 1 + 7) / 8) * 8."""
    return ((lmax + 1 + 7) // 8) * 8


def load_block(kernel, lmax):
    """Samples per load block: the tile's 64, SB = 2 S (int16) or S (int32) of k_lpc."""
    return 64 if kernel == "tile" else 2 * ring_len(lmax) if kernel == "gen16" else ring_len(lmax)


def launch_split(count, sample_bytes, L, stride):
    """launch_lpc_T: [(kernel, LMAX, first unit, units)] of one chunk (FLACMI_LPC_TILE unset)."""
    lmax = lmax_of(L)
    if count <= 0:
        return []
    if lmax <= 12:
        full = count & ~63
        if sample_bytes == 2 and stride % 8 == 0 and stride >= 8 and full > 0:
            out = [("tile", lmax, 0, full)]
            if full != count:
                out.append(("gen16", lmax, full, count - full))
            return out
    return [("gen16" if sample_bytes == 2 else "ring", lmax, 0, count)]


def tile_split(n, lmax, lo, hi):
    """k_lpc_tile's three loops: (t1, t2 - t1, ntile - t2) tiles."""
    M = n - 1
    ntile = (M + 63) >> 6
    t1 = (lo + lmax + 63) >> 6
    if lo + lmax <= 0:
        t1 = 0
    t2 = min(hi, M) >> 6
    if t2 > ntile:
        t2 = ntile
    if t1 > t2:
        t1 = t2
    return t1, t2 - t1, ntile - t2


def ring_split(n, lmax, lo, hi):
    """k_lpc<LMAX,int32_t>'s four loops: (c1, c2 - c1, cf - c2, ncyc - cf) ring cycles."""
    S = ring_len(lmax)
    M = n - 1
    ncyc = (M + S - 1) // S
    cf = M // S - 1 if M // S - 1 > 0 else 0
    c1 = (lo + lmax + S - 1) // S
    if lo + lmax <= 0:
        c1 = 0
    c2 = hi // S
    if c2 > cf:
        c2 = cf
    if c1 > c2:
        c1 = c2
    return c1, c2 - c1, cf - c2, ncyc - cf


def gen16_subblocks(n, lmax, lo, hi):
    """k_lpc<LMAX,int16_t>: per S-sample sub-block of its nblk load blocks, (m0, fused)."""
    S = ring_len(lmax)
    SB = 2 * S
    M = n - 1
    nblk = (M + SB - 1) // SB
    return [(m0, m0 - lmax >= lo and m0 + S <= hi) for m0 in range(0, nblk * SB, S)]


def gen16_split(n, lmax, lo, hi):
    """(nblk, fused sub-blocks, unfused sub-blocks)."""
    sub = gen16_subblocks(n, lmax, lo, hi)
    fused = sum(1 for _, f in sub if f)
    return len(sub) // 2, fused, len(sub) - fused


def build_split(kernel, n, lmax, sample_bits):
    """The loop split of one build at length n; None at the Tukey site (the kernel returns first)."""
    r = rectangle(n, sample_bits)
    if r is None:
        return None
    return {"tile": tile_split, "ring": ring_split, "gen16": gen16_split}[kernel](n, lmax, *r)


def max_window_index(kernel, n, lmax, sample_bits):
    """The largest index of win[] the build reads at length n (-1: none).  Only the multiply-and-add
    path reads the window, one weight per slot of its tile / cycle / sub-block."""
    r = rectangle(n, sample_bits)
    if r is None:
        return -1
    lo, hi = r
    if kernel == "tile":
        t1, rect, last = tile_split(n, lmax, lo, hi)
        return 64 * (t1 + rect + last) - 1 if last else 64 * t1 - 1
    if kernel == "ring":
        S = ring_len(lmax)
        c1, rect, tap, last = ring_split(n, lmax, lo, hi)
        return S * (c1 + rect + tap + last) - 1 if tap + last else S * c1 - 1
    S = ring_len(lmax)
    return max((m0 + S - 1 for m0, fused in gen16_subblocks(n, lmax, lo, hi) if not fused), default=-1)


BUILDS = [("tile", m) for m in (4, 8, 12)] + [("gen16", m) for m in LMAXES] + [("ring", m) for m in LMAXES]


# ---------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------
# group A: int16, 69 units (64 tile + 5 gen16) and their 40-unit prefix as a call of its own
# group B: int16 at L > 12 (gen16<16>, gen16<32>), 24 units
# group C: int32 container, every ring build, 37 units
Case = namedtuple("Case", "group n L bits units q")
A_LS = (3, 4, 7, 12, 9)            # tile<4>, tile<4>, tile<8>, tile<12>, tile<12> with L < LMAX
A_LENGTHS = (1, 2, 3, 5, 8, 9, 65, 66, 100, 191, 192, 193, 200, 322, 882, 1000, 4410, 2048, 2049)
A_ALL_LS = (1, 192, 322, 4410)     # n = 1: the only length whose last tile loop is empty
A_UNITS, A_PREFIX, A_Q = 69, 40, 6
B_LS = (13, 16, 17, 32)
B_LENGTHS = (8, 49, 82, 97, 322, 576, 882, 4410)
B_UNITS, B_Q = 24, 8
C_LS = (4, 8, 12, 16, 32)
C_LENGTHS = (1, 2, 3, 5, 8, 9, 41, 42, 81, 322, 882, 1000, 2049, 4410)
C_UNITS, C_Q = 37, 12
RMIN, RMAX = 0, 5


def _cases():
    out = []
    for i, n in enumerate(A_LENGTHS):
        for L in (A_LS if n in A_ALL_LS else (A_LS[i % 5],)):
            out.append(Case("A", n, L, 16, A_UNITS, A_Q))
    # 323 = 256 + 64 + 3: the tile kernel's second workgroup has one live wave, the remainder of 3
    # starts at unit 320
    out.append(Case("A", 100, 12, 16, 323, A_Q))
    for n in B_LENGTHS:
        for L in B_LS:
            out.append(Case("B", n, L, 16, B_UNITS, B_Q))
    for n in C_LENGTHS:
        for L in C_LS:
            out.append(Case("C", n, L, 24, C_UNITS, C_Q))
    out.append(Case("C", 81, 32, 24, 293, C_Q))   # 256 + 37: a second workgroup that is not full
    # the widest fused width beside the first unfused one, full scale (28 + 12 <= 44).  Fusing at
    # 27 bits would still be exact (|x| <= 2^26: products up to 2^52 fit a double's 53 bits), so
    # 27 only pins the host's switch; at 28 bits (products up to 2^54) a rectangle left fused
    # changes bits
    for n in (322, 4410):
        out += [Case("C", n, 32, 26, C_UNITS, C_Q), Case("C", n, 12, 26, C_UNITS, C_Q),
                Case("C", n, 32, 27, C_UNITS, C_Q), Case("C", n, 32, 28, C_UNITS, C_Q)]
    return out


CASES = _cases()

# the tile kernel's split at LMAX 12 per length of group A (None: no window, the Tukey site)
TILE12 = {1: (0, 0, 0), 2: (0, 0, 1), 3: (0, 0, 1), 5: None, 8: (0, 0, 1), 9: (0, 0, 1), 65: (0, 0, 1),
          66: (0, 0, 2), 100: (1, 0, 1), 191: (1, 1, 1), 192: (1, 1, 1), 193: (1, 1, 1), 200: (1, 1, 2),
          322: (2, 1, 3), 882: (4, 6, 4), 1000: (5, 6, 5), 4410: (18, 33, 18), 2048: (9, 15, 8),
          2049: (9, 15, 8)}
# the ring's four loops at n = 322, all non-empty (LMAX 8 and 12 share S = 16 and, at this length,
# the same split)
RING322 = {32: (3, 3, 1, 2), 16: (4, 6, 2, 2), 12: (6, 9, 4, 2), 8: (6, 9, 4, 2), 4: (11, 19, 9, 2)}
# group B at LMAX 32: the lengths whose last block read past a 64-entry pad, and the one that
# reads exactly to n + 63
PAST_64 = (8, 82, 322, 882, 4410)
EXACTLY_64 = (576, 4096)

# (block, tail, L, bits, q): 69 body units and 5 tail units; the tail rows keep full-scale noise at
# and past tail_len
TailCall = namedtuple("TailCall", "block tail L bits q")
TAIL_CALLS = [TailCall(4410, 882, 12, 16, A_Q), TailCall(2049, 65, 7, 16, A_Q), TailCall(4410, 322, 32, 24, C_Q)]
TAIL_BODY, TAIL_CUT = 69, 5


def case_id(c):
    return f"{c.group}-n{c.n}-l{c.L}-b{c.bits}-u{c.units}"


def tail_id(t):
    return f"{t.block}-{t.tail}-l{t.L}-b{t.bits}"


def sample_bytes_of(bits):
    return 2 if bits <= 16 else 4


def resolve(n, L, bits, units, block=None):
    """[(kernel, LMAX, first unit, units, split)] of one length class of `units` units (small
    calls: one chunk per class), rows pitched for `block` (a tail class: the call's block length)."""
    sb = sample_bytes_of(bits)
    return [(k, m, u0, cnt, build_split(k, n, m, bits))
            for k, m, u0, cnt in launch_split(units, sb, L, row_pitch(block or n, sb))]


def check_dispatch(c):
    """The case's builds and loop splits against what the table claims -> resolve()'s list."""
    got = resolve(c.n, c.L, c.bits, c.units)
    m = lmax_of(c.L)
    head = [(k, mm, u0, cnt) for k, mm, u0, cnt, _ in got]
    if c.group == "A":
        full = c.units & ~63
        assert head == [("tile", m, 0, full), ("gen16", m, full, c.units - full)], (c, got)
        assert c.units - full in (3, 5) and m <= 12
        assert resolve(c.n, c.L, c.bits, A_PREFIX)[0][:4] == ("gen16", m, 0, A_PREFIX), c
        if m == 12:
            assert got[0][4] == TILE12[c.n], (c, got[0][4], TILE12[c.n])
    elif c.group == "B":
        assert head == [("gen16", m, 0, c.units)] and m in (16, 32), (c, got)
    else:
        assert head == [("ring", m, 0, c.units)], (c, got)
        if c.n == 322 and c.bits <= FUSE_MAX_BITS and m in RING322:
            assert got[0][4] == RING322[m], (c, got)
        if c.bits > FUSE_MAX_BITS:  # fusing off: no rectangle cycle
            assert got[0][4][1] == 0, (c, got)
    return got


def check_tail_dispatch(t):
    body = resolve(t.block, t.L, t.bits, TAIL_BODY)
    cut = resolve(t.tail, t.L, t.bits, TAIL_CUT, block=t.block)
    m = lmax_of(t.L)
    if t.bits <= 16:
        assert [b[:4] for b in body] == [("tile", m, 0, 64), ("gen16", m, 64, 5)], (t, body)
        assert [b[:4] for b in cut] == [("gen16", m, 0, TAIL_CUT)], (t, cut)
    else:
        assert [b[:4] for b in body] == [("ring", m, 0, TAIL_BODY)], (t, body)
        assert [b[:4] for b in cut] == [("ring", m, 0, TAIL_CUT)], (t, cut)
    return body, cut


# ---------------------------------------------------------------------------------------
# inputs and the oracle's results, made once
# ---------------------------------------------------------------------------------------
ZERO_UNIT, IMPULSE_UNIT = 5, 7   # rows of every case (inside group A's 40-unit prefix)


@functools.lru_cache(maxsize=None)
def case_units(n, bits, units):
    """Row i by i % 3: the bench's open mix (oracle.synth_batch, open_eighths = 5), uniform noise
    over the whole declared range, a near-full-scale DC level plus +-50 noise (large accumulators:
    a fused and an unfused taper term then round differently, so a rectangle boundary that is off
    by one cycle changes bits); row 5 all zero (Levinson's ZeroDivisionError), row 7 zero except
    x[n-2] and x[n-1] at full scale."""
    dt = np.int16 if bits <= 16 else np.int32
    hi, lo = (1 << (bits - 1)) - 1, -(1 << (bits - 1))
    rng = np.random.default_rng(100000 * bits + 10 * n + units % 7)
    a = np.zeros((units, n), dtype=np.int64)
    syn = oracle.synth_batch(0, units, n, bits, 9000 + n + bits, dtype=dt, open_eighths=5)
    for i in range(units):
        if i % 3 == 0:
            a[i] = syn[i]
        elif i % 3 == 1:
            a[i] = rng.integers(lo, hi + 1, n)
        else:
            level = hi - 60 - (i * 37) % 200
            a[i] = (level if i % 2 else -level) + rng.integers(-50, 51, n)
    a[ZERO_UNIT] = 0
    a[IMPULSE_UNIT] = 0
    a[IMPULSE_UNIT, max(n - 2, 0):] = hi
    assert a.min() >= lo and a.max() <= hi
    a = np.ascontiguousarray(a.astype(dt))
    a.setflags(write=False)
    return a


def _freeze(ora):
    for v in ora.values():
        v.setflags(write=False)
    return ora


def params_of(L, q):
    return oracle.make_params(L, q, RMIN, RMAX)


@functools.lru_cache(maxsize=None)
def case_reference(c):
    a = case_units(c.n, c.bits, c.units)
    return a, _freeze(oracle.analyze_batch(a, params_of(c.L, c.q), c.n, sample_bits=c.bits, threads=16))


@functools.lru_cache(maxsize=None)
def tail_reference(t):
    n_units = TAIL_BODY + TAIL_CUT
    a = case_units(t.block, t.bits, n_units).copy()
    hi, lo = (1 << (t.bits - 1)) - 1, -(1 << (t.bits - 1))
    rng = np.random.default_rng(77 + t.block + t.tail)
    a[TAIL_BODY:, t.tail:] = rng.integers(lo, hi + 1, (TAIL_CUT, t.block - t.tail))
    a.setflags(write=False)
    return a, _freeze(oracle.analyze_batch(a, params_of(t.L, t.q), t.block, t.tail, TAIL_CUT,
                                           sample_bits=t.bits, threads=16))


def prefix(ora, k):
    return {name: v[:k] for name, v in ora.items()}


# ---------------------------------------------------------------------------------------
# conditions on the oracle alone
# ---------------------------------------------------------------------------------------
LPC_STAGE_SITES = range(1, 10)   # abi.SITE_NAMES 1..9: raised inside encode_subframe_lpc's LPC analysis
SITE_TUKEY, SITE_LEVINSON_DIV = 1, 2


def lpc_stage_failed(om, u):
    """The oracle's unit raised before its LPC record was complete (the record stays zero)."""
    return int(om["status"][u]) != 0 and int(om["site"][u]) in LPC_STAGE_SITES


def check_case_oracle(c):
    """The conditions a case's inputs must meet before any device result counts; returns the facts
    the caller may print."""
    a, ora = case_reference(c)
    om = ora["meta"]
    lpc_ok = np.array([not lpc_stage_failed(om, u) for u in range(len(a))])
    facts = {"units": len(a), "lpc_records_ok": int(lpc_ok.sum()), "status_ok": int((om["status"] == 0).sum())}
    if 4 <= c.n <= 7:
        assert (om["status"] == abi.STATUS_ZERO_DIVISION).all() and (om["site"] == SITE_TUKEY).all(), c
        return facts
    if c.n >= 64:
        assert lpc_ok.sum() >= 0.6 * len(a), (c, facts)
    assert (int(om["status"][ZERO_UNIT]), int(om["site"][ZERO_UNIT])) == \
        (abi.STATUS_ZERO_DIVISION, SITE_LEVINSON_DIV), (c, om["status"][ZERO_UNIT], om["site"][ZERO_UNIT])
    lpc = (om["status"] == 0) & (om["kind"] == abi.KIND_LPC)
    facts["lpc_chosen"] = int(lpc.sum())
    return facts


def check_tail_oracle(t):
    a, ora = tail_reference(t)
    om = ora["meta"]
    # the oracle reads tail_len samples only: the tail rows' results are those of the cut rows alone
    cut = np.ascontiguousarray(a[TAIL_BODY:, :t.tail])
    alone = oracle.analyze_batch(cut, params_of(t.L, t.q), t.tail, sample_bits=t.bits, threads=4)
    assert np.array_equal(alone["acf"].view(np.uint64), ora["acf"][TAIL_BODY:].view(np.uint64)), t
    assert np.array_equal(alone["lpc_records"], ora["lpc_records"][TAIL_BODY:]), t
    assert np.array_equal(alone["meta"]["status"], om["status"][TAIL_BODY:]), t
    ok = np.array([not lpc_stage_failed(om, u) for u in range(len(a))])
    assert ok[:TAIL_BODY].sum() >= 0.6 * TAIL_BODY and ok[TAIL_BODY:].sum() >= 3, (t, ok)
    return {"body_ok": int(ok[:TAIL_BODY].sum()), "tail_ok": int(ok[TAIL_BODY:].sum())}
