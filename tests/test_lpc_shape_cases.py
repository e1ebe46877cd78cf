"""The k_lpc shape table (tests/lpc_shape_cases.py) without a device: the restated dispatch and loop
bounds against the kernel source, the window pad against every build's furthest window read, each
case's expected build and loop split, and every condition the GPU tests place on their inputs, on
the CPU oracle alone."""
import os
import re

import numpy as np
import pytest

import lpc_shape_cases as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flac-py_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_match_the_source():
    """A changed pad, ring length, loop bound or launch condition must change the restatement."""
    h, host, k = _source("flacmi_kernels.h"), _source("flacmi_host.cpp"), _source("k_lpc.hip")
    assert int(re.search(r"constexpr int kWindowPad = (\d+);", h).group(1)) == S.WINDOW_PAD
    assert "tukey_window(n, kWindowPad)" in host
    assert "static_assert(SB <= kWindowPad" in k and "static_assert(64 <= kWindowPad" in k
    assert f"if (b->sample_bits > {S.FUSE_MAX_BITS}) a.fuse_lo = a.fuse_hi = 0;" in host
    assert "int64_t bytes = ((n * sample_bytes + 15) / 16) * 16;" in host and "if (bytes % 4096 == 0) bytes += 128;" in host
    assert k.count("constexpr int S = ((LMAX + 1 + 7) / 8) * 8;") == 2
    assert "constexpr int SB = sizeof(SampleT) == 2 ? 2 * S : S;" in k
    assert "a.sample_bytes == 2 && lpc_tile_enabled() && a.stride % 8 == 0 && a.stride >= 8 && full > 0" in k
    assert "const int64_t full = a.count & ~(int64_t)63;" in k
    for line in ("int t1 = (a.fuse_lo + LMAX + 63) >> 6;", "int t2 = min(a.fuse_hi, M) >> 6;",
                 "const int ntile = (M + 63) >> 6;", "const int cf = M / S - 1 > 0 ? M / S - 1 : 0;",
                 "int c1 = (a.fuse_lo + LMAX + S - 1) / S;", "int c2 = a.fuse_hi / S;",
                 "const int ncyc = (M + S - 1) / S;", "const int nblk = (M + SB - 1) / SB;",
                 "if (m0 - LMAX >= a.fuse_lo && m0 + S <= a.fuse_hi) {",
                 "if (a.L <= 4) return launch_lpc_T<4>(a, s);", "if (a.L <= 8) return launch_lpc_T<8>(a, s);",
                 "if (a.L <= 12) return launch_lpc_T<12>(a, s);", "if (a.L <= 16) return launch_lpc_T<16>(a, s);"):
        assert line in k, line


def test_restated_dispatch():
    assert [S.ring_len(m) for m in S.LMAXES] == [8, 16, 16, 24, 40]
    assert [S.load_block("gen16", m) for m in S.LMAXES] == [16, 32, 32, 48, 80]
    assert max(S.load_block(k, m) for k, m in S.BUILDS) <= S.WINDOW_PAD
    assert [S.lmax_of(L) for L in (0, 4, 5, 8, 9, 12, 13, 16, 17, 32)] == [4, 4, 8, 8, 12, 12, 16, 16, 32, 32]
    assert S.row_pitch(100, 2) == 104 and S.row_pitch(200, 2) == 200 and S.row_pitch(322, 2) == 328
    assert S.row_pitch(2048, 2) == 2048 + 64 and S.row_pitch(2049, 2) == 2056 and S.row_pitch(1, 2) == 8
    assert S.row_pitch(1024, 4) == 1024 + 32 and S.row_pitch(41, 4) == 44
    f = S.launch_split
    assert f(69, 2, 12, 104) == [("tile", 12, 0, 64), ("gen16", 12, 64, 5)]
    assert f(128, 2, 3, 8) == [("tile", 4, 0, 128)]
    assert f(63, 2, 12, 104) == [("gen16", 12, 0, 63)] and f(69, 2, 13, 104) == [("gen16", 16, 0, 69)]
    assert f(69, 2, 12, 100) == [("gen16", 12, 0, 69)]      # rows not made of whole 16-byte segments
    assert f(69, 4, 12, 104) == [("ring", 12, 0, 69)] and f(0, 2, 12, 104) == []
    # the rectangle: the window's run of exact ones, off for samples wider than 26 bits
    for n in (1, 2, 3):
        assert S.window_ones(n) == (0, n)
    for n in (4, 5, 6, 7):
        assert S.window_ones(n) is None
    st, w = S.oracle.tukey(4410)
    lo, hi = S.window_ones(4410)
    assert st == 0 and (w[lo:hi] == 1.0).all() and w[lo - 1] != 1.0 and w[hi] != 1.0 and hi - lo > 4410 // 2
    assert S.rectangle(4410, 26) == (lo, hi) and S.rectangle(4410, 27) == (0, 0)


def test_window_reads_stay_inside_the_pad():
    """Per build and every n in 1..4700 (fusing on, and off as for samples wider than 26 bits): the
    largest window index read lies below n + pad, and comes within one block of it."""
    for kernel, lmax in S.BUILDS:
        blk = S.load_block(kernel, lmax)
        worst = -1
        for n in range(1, 4701):
            for bits in ((16,) if kernel != "ring" else (24, 27)):
                top = S.max_window_index(kernel, n, lmax, bits)
                assert top < n + S.WINDOW_PAD, (kernel, lmax, n, bits, top)
                assert top <= n - 2 + blk - 1, (kernel, lmax, n, bits, top)   # M - 1 + block - 1 at most
                worst = max(worst, top - n)
        assert worst == blk - 3, (kernel, lmax, worst, blk)   # M = 1 mod the block: top = n + block - 3


def test_the_old_64_entry_pad_was_too_short_at_lmax_32():
    """What the pad constant fixes: k_lpc<32,int16_t> (SB 80) read up to n + 77, past a pad of 64,
    at n % 80 in 2..15; no other build read past n + 63."""
    for n in S.PAST_64:
        assert S.max_window_index("gen16", n, 32, 16) >= n + 64, n
    for n in S.EXACTLY_64:
        assert S.max_window_index("gen16", n, 32, 16) == n + 63, n
    past = [n for n in range(1, 4701) if S.max_window_index("gen16", n, 32, 16) >= n + 64]
    # (n in 4..7 is the Tukey site: the kernel returns before it reads the window)
    assert past == [n for n in range(1, 4701) if 2 <= n % 80 <= 15 and not 4 <= n <= 7]
    assert max(S.max_window_index("gen16", n, 32, 16) - n for n in past) == 77
    for kernel, lmax in S.BUILDS:
        if (kernel, lmax) != ("gen16", 32):
            assert all(S.max_window_index(kernel, n, lmax, 24) < n + 64 for n in range(1, 4701)), (kernel, lmax)


def test_table_covers_every_loop_of_every_build():
    """Over the whole table, every loop of every build is empty in one case and non-empty in
    another (k_lpc<LMAX,int16_t>: its fused and its multiply-and-add sub-blocks)."""
    seen = {}
    for c in S.CASES:
        for kernel, lmax, _, _, split in S.check_dispatch(c):
            if split is not None:
                seen.setdefault((kernel, lmax), []).append(split[1:] if kernel == "gen16" else split)
        if c.group == "A":
            kernel, lmax, _, _, split = S.resolve(c.n, c.L, c.bits, S.A_PREFIX)[0]
            if split is not None:
                seen.setdefault((kernel, lmax), []).append(split[1:])
    assert set(seen) == set(S.BUILDS)
    for build, splits in seen.items():
        for loop in range(len(splits[0])):
            counts = {s[loop] > 0 for s in splits}
            if build[0] == "gen16" and build[1] > 12 and loop == 1:
                # groups B's lengths start at 8: every call has a multiply-and-add sub-block (the
                # first sub-block is never fused); the L <= 12 builds see n = 1 (no block at all)
                assert counts == {True}, (build, loop)
                continue
            assert counts == {True, False}, (build, loop, sorted(set(splits)))
    # the conditions the table names, per length
    for n, want in S.TILE12.items():
        assert S.build_split("tile", n, 12, 16) == want, (n, S.build_split("tile", n, 12, 16), want)
    assert S.build_split("tile", 1000, 4, 16)[0] != S.build_split("tile", 1000, 12, 16)[0]
    for m, want in S.RING322.items():
        assert S.build_split("ring", 322, m, 24) == want
    for n in (41, 42):  # M = 40, 41 against S = 40: one whole cycle, and one sample into a second
        assert S.build_split("ring", n, 32, 24) == (0, 0, 0, n - 40)
    assert S.row_pitch(100, 2) - 8 == 96 and S.row_pitch(200, 2) == 200 and S.row_pitch(2048, 2) * 2 == 4096 + 128
    assert {c.L for c in S.CASES if c.group == "A" and c.n in S.A_ALL_LS} == set(S.A_LS)
    assert {(c.n, c.L, c.bits) for c in S.CASES if c.bits > 24} == \
        {(n, L, b) for n in (322, 4410) for L, b in ((32, 26), (12, 26), (32, 27), (32, 28))}


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_case_inputs(case):
    S.check_dispatch(case)
    facts = S.check_case_oracle(case)
    print(S.case_id(case), facts)


def test_lpc_is_chosen_in_every_bucket():
    """Over groups A and C the oracle chooses LPC for at least one unit per LMAX bucket."""
    chosen = {}
    for c in S.CASES:
        if c.group in "AC":
            key = (c.group, S.lmax_of(c.L))
            chosen[key] = chosen.get(key, 0) + S.check_case_oracle(c).get("lpc_chosen", 0)
    print(chosen)
    assert set(chosen) == {("A", m) for m in (4, 8, 12)} | {("C", m) for m in S.LMAXES}
    assert min(chosen.values()) >= 1, chosen


def test_wide_cases_are_full_scale_at_the_fma_edge():
    """26-bit full scale: products up to 2^50 and, at n = 4410, sums past 2^53 -- the widest case
    in which one FMA per term must equal the reference's multiply and add."""
    for n in (322, 4410):
        for bits in (26, 27, 28):
            a = S.case_units(n, bits, S.C_UNITS)
            assert int(np.abs(a.astype(np.int64)).max()) >= (1 << (bits - 1)) - 1, (n, bits)
            assert bits + S.C_Q <= 44
    c = next(c for c in S.CASES if (c.n, c.L, c.bits) == (4410, 32, 26))
    _, ora = S.case_reference(c)
    assert float(ora["acf"][:, 0].max()) > 2.0 ** 53
    assert c.bits + c.q <= 44


@pytest.mark.parametrize("t", S.TAIL_CALLS, ids=S.tail_id)
def test_tail_call_inputs(t):
    S.check_tail_dispatch(t)
    print(S.tail_id(t), S.check_tail_oracle(t))
    a, _ = S.tail_reference(t)
    full = (1 << (t.bits - 1)) * 0.9
    assert (np.abs(a[S.TAIL_BODY:, t.tail:].astype(np.int64)).max(axis=1) > full).all()
