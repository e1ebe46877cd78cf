"""k_resid_stream's Rice data-bits pass sums z >> p once per distinct parameter of a wave's
chunk slot, and its staging sums |x| with packed 16-bit SADs: units built so that every
partition order wins somewhere by a margin of a few bits, every number of distinct sums per
slot occurs, coarse orders win whose parameters differ from the finest order's, flagged (parameter >= 16) rows sit beside uniform rows in one slot, and full-scale
samples fill the order-0 sum.  Everything against the CPU oracle, bit for bit, in production and
debug calls; the conditions on the inputs are asserted on the oracle's own residual, restated in
numpy (encoder.py:655-760), so a change of generator cannot empty a case."""
import functools

import numpy as np
import pytest

import oracle
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params

pytestmark = pytest.mark.gpu

K_SCPT = 5  # k_stream.hip kSCPT: 8-sample chunks per thread


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


# ---------------------------------------------------------------------------------------
# the reference's Rice search and the kernel's chunk layout, restated
# ---------------------------------------------------------------------------------------
def stream_threads(n):
    """k_stream.hip stream_threads: the workgroup of an n-sample unit."""
    nch = n // 8
    return max(64, 64 * ((nch + 64 * K_SCPT - 1) // (64 * K_SCPT)))


def rice_orders(z, n, order, rmin, rmax):
    """{o: (parameters per partition, total bits)} for every candidate partition order of the
    zig-zag residual z (n values, the first `order` are warm-up): rice_partitions,
    find_rice_parameter and rice_size.  floor(log2(sum / len)) as the largest p with
    len * 2^p <= sum (sums here are far below 2^46, where the two agree)."""
    z = z.astype(np.int64).copy()
    z[:order] = 0
    out = {}
    for o in range(rmin, rmax + 1):
        if n % (1 << o) or (n >> o) <= order:
            continue
        parts = z.reshape(1 << o, n >> o)
        lens = np.full(1 << o, n >> o, np.int64)
        lens[0] -= order
        sums = parts.sum(1)
        assert (sums >= lens).all()  # units of status 0 only
        prm = np.array([(int(s) // int(ln)).bit_length() - 1 for s, ln in zip(sums, lens)], np.int64)
        bits = 0
        for k in range(1 << o):
            p = int(prm[k])
            # (the warm-up values are not coded: zeroed above, they add 0 >> p = 0 bits)
            bits += 4 + (5 if p > 14 else 4) + int((parts[k] >> p).sum()) + int(lens[k]) * (1 + p)
        out[o] = (prm, bits)
    return out


def slot_classes(z, n, order, tabs):
    """Per wave slot of the kernel's layout (chunk c = tid + NT j, one 64-lane wave per slot):
    (number of distinct per-order parameter vectors over the voting lanes, number of flagged-row
    lanes).  A lane votes when its chunk is inside the unit, holds no value >= 2^16 and its
    finest partition's row has no parameter >= 16."""
    z = z.astype(np.int64).copy()
    z[:order] = 0
    nt, nch = stream_threads(n), n // 8
    orders = sorted(tabs)
    oo = orders[-1]
    chunk_big = (z.reshape(nch, 8) >> 16).any(1)
    c_all = np.arange(nch)
    vec = np.stack([tabs[o][0][(8 * c_all) // (n >> o)] for o in orders])  # [order][chunk]
    flagged = (vec >= 16).any(0)
    out = []
    for j in range(K_SCPT):
        for w in range(nt // 64):
            c = np.arange(64 * w + nt * j, 64 * w + nt * j + 64)
            c = c[c < nch]
            if len(c) == 0:
                continue
            vote = c[~chunk_big[c] & ~flagged[c]]
            if len(vote) == 0:
                continue
            distinct = len({tuple(vec[i, vote]) for i in range(len(orders))})
            out.append((distinct, int((flagged[c] & ~chunk_big[c]).sum())))
    return out


def unit_facts(a, ora, n, rmin, rmax):
    """Per unit of status 0: (winning order, margin to the runner-up in bits, slot classes,
    whether the winner's parameters differ from the finest order's)."""
    facts = {}
    for u in range(len(a)):
        if int(ora["meta"]["status"][u]) != 0:
            continue
        order = int(ora["meta"]["res_offset"][u])
        z = ora["residual"][u][:n]
        tabs = rice_orders(z, n, order, rmin, rmax)
        tot = sorted((b, o) for o, (_, b) in tabs.items())
        # the restatement itself against the oracle
        assert tot[0][1] == int(ora["meta"]["part_order"][u]) and tot[0][0] == int(ora["meta"]["rice_bits"][u]), u
        margin = tot[1][0] - tot[0][0] if len(tot) > 1 else None
        # the winner's parameters differ from the finest order's on some finest partition
        win, oo = tot[0][1], max(tabs)
        differs = any(int(tabs[win][0][k >> (oo - win)]) != int(tabs[oo][0][k]) for k in range(1 << oo))
        facts[u] = (win, margin, slot_classes(z, n, order, tabs), differs)
    return facts


def compare(out, ora, n):
    gm, om = out["meta"], ora["meta"]
    for u in range(len(om)):
        st = int(om["status"][u])
        assert int(gm["status"][u]) == st, (u, "status", int(gm["status"][u]), st)
        assert int(gm["site"][u]) == int(om["site"][u]), (u, "site")
        if st != 0:
            continue
        bad = oracle.meta_mismatches(gm[u], om[u])
        assert not bad, (u, bad)
        k = int(om["n_parts"][u])
        assert np.array_equal(out["rice_params"][u][:k], ora["rice_params"][u][:k]), (u, "params")
        off, ln = int(om["res_offset"][u]), int(om["res_len"][u])
        assert np.array_equal(out["residual"][u][off:off + ln].astype(np.uint64),
                              ora["residual"][u][off:off + ln]), (u, "residual")
        if "fixed_sums" in out:
            assert np.array_equal(out["fixed_sums"][u], ora["fixed_sums"][u]), (u, "fixed_sums")


def run_both_modes(az, a, ora, n, L, rmin, rmax, mode=abi.MODE_REFERENCE):
    for debug in (False, True):
        out = az.analyze(a, make_params(L, 5, rmin, rmax, mode), n, sample_bits=16, debug=debug)
        compare(out, ora, n)


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def stepped_noise(rng, n, o, scale=1.0):
    """Gaussian noise whose standard deviation scale * 2^k (k in 3..11) steps at the boundaries
    of the 2^o partitions of order o, neighbouring segments different."""
    ks = []
    for _ in range(1 << o):
        k = int(rng.integers(3, 12))
        while ks and k == ks[-1]:
            k = int(rng.integers(3, 12))
        ks.append(k)
    sigma = np.repeat(scale * 2.0 ** np.array(ks), n >> o)
    return np.clip(np.round(rng.normal(0.0, 1.0, n) * sigma), -32768, 32767).astype(np.int16)


# a Gaussian's zig-zag mean is 2 E|x| = 1.596 sigma: at this scale a segment's mean sits on a
# power of two, so the parameters of the partitions inside it fall on either side of it while
# the segment's own order still wins (by the finer orders' headers)
ON_A_POWER_OF_TWO = 1.0 / 1.596


@functools.lru_cache(maxsize=None)
def stepped_units(n, olo, ohi, per_order):
    """per_order units for every target order, then half as many whose segment means sit on
    a power of two."""
    rng = np.random.default_rng(7)
    rows = [stepped_noise(rng, n, o) for o in range(olo, ohi + 1) for _ in range(per_order)]
    rows += [stepped_noise(rng, n, o, ON_A_POWER_OF_TWO) for o in range(olo, ohi + 1) for _ in range(per_order // 2)]
    a = np.stack(rows)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def stepped_reference(n, rmin, rmax, mode, L):
    a = stepped_units(n, rmin, rmax, 8)
    ora = oracle.analyze_batch(a, oracle.make_params(L, 5, rmin, rmax, mode), n, sample_bits=16, threads=16)
    return a, ora, unit_facts(a, ora, n, rmin, rmax)


# ---------------------------------------------------------------------------------------
# 1. every order wins, every dedup class occurs (n = 4608: the constant-shape build)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["constant", "runtime", "fixed-only"])
def test_every_order_wins_and_every_dedup_class(az, build):
    n = 4608
    mode, L = (abi.MODE_FIXED_ONLY, 0) if build == "fixed-only" else (abi.MODE_REFERENCE, 12)
    a, ora, facts = stepped_reference(n, 0, 5, mode, L)
    wins = [sum(1 for w, _, _, _ in facts.values() if w == o) for o in range(6)]
    assert min(wins) >= 4, wins
    assert all(m is not None and m > 0 for _, m, _, _ in facts.values())
    cls = [d for _, _, slots, _ in facts.values() for d, _ in slots]
    count = [sum(1 for d in cls if d == 1), sum(1 for d in cls if d in (2, 3)), sum(1 for d in cls if d >= 4)]
    assert min(count) >= 10, count
    # units a kernel that shifted every order by the finest order's parameter would miscount
    assert sum(1 for _, _, _, d in facts.values() if d) >= 8
    with knob("FLACMI_STREAM_GENERIC", int(build == "runtime")):
        run_both_modes(az, a, ora, n, L, 0, 5, mode)


# ---------------------------------------------------------------------------------------
# 2. runtime order ranges: one- and two-wave units, rmin > 0 (entry 0 holds only the flag)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rmin,rmax", [(4096, 0, 4), (4096, 2, 5), (1024, 3, 5)])
def test_runtime_order_ranges(az, n, rmin, rmax):
    a, ora, facts = stepped_reference(n, rmin, rmax, abi.MODE_REFERENCE, 12)
    assert len({w for w, _, _, _ in facts.values()}) >= 2  # more than one order wins
    cls = {d for _, _, slots, _ in facts.values() for d, _ in slots}
    assert 1 in cls and max(cls) >= 2, cls
    run_both_modes(az, a, ora, n, 12, rmin, rmax)


# ---------------------------------------------------------------------------------------
# 3. a flagged row beside uniform rows in one wave slot
# ---------------------------------------------------------------------------------------
def flagged_units(n=4608, units=8):
    """Loud smooth sines under stationary noise (fixed order 1 wins; its residual is the noise's
    first difference, every partition's zig-zag mean about 1.2 * 2^13) with full-scale
    alternation in the first 9..12 chunks of finest partition 7 (chunks 126..143): that
    partition's mean passes 2^16, so its row is flagged and its quiet chunks take the 32-bit
    path.  The first wave's second slot (chunks 128..191) holds them beside chunks 144..191,
    which share only the order-0 and order-1 ancestors with the loud partition: those means
    rise by less than 2^13 * 0.8, so every order keeps the parameter 13 there."""
    r = np.random.default_rng(11)
    t = np.arange(n)
    a = np.zeros((units, n), np.int16)
    for u in range(units):
        x = (14000 + 100 * u) * np.sin(2 * np.pi * t / (900 + 37 * u) + u) + r.normal(0, 4340, n)
        for c in range(126, 126 + 9 + u % 4):
            x[8 * c: 8 * c + 8] = 32767 * np.array([1, -1] * 4)
        a[u] = np.clip(np.round(x), -32768, 32767)
    return a


def test_flagged_row_beside_uniform_rows(az):
    n = 4608
    a = flagged_units(n)
    ora = oracle.analyze_batch(a, oracle.make_params(12, 5, 0, 5), n, sample_bits=16, threads=16)
    facts = unit_facts(a, ora, n, 0, 5)
    assert len(facts) == len(a)
    # slots whose voting lanes agree on every order while flagged-row lanes sit among them
    mixed = sum(1 for _, _, slots, _ in facts.values() for d, nf in slots if d == 1 and nf > 0)
    assert mixed >= 4, mixed
    for generic in (0, 1):
        with knob("FLACMI_STREAM_GENERIC", generic):
            run_both_modes(az, a, ora, n, 12, 0, 5)


# ---------------------------------------------------------------------------------------
# 4. sum|x| extremes
# ---------------------------------------------------------------------------------------
def full_scale_units(n):
    lo, hi = -32768, 32767
    r = np.random.default_rng(3)
    rows = [np.full(n, lo), np.full(n, hi), np.tile([lo, hi], n // 2), np.tile([hi, lo], n // 2),
            np.tile([lo, lo, hi, hi], n // 4), np.tile([lo, hi, hi, lo, lo, lo, hi, lo], n // 8),
            np.where(r.integers(0, 2, n) == 1, hi, lo), np.where(np.arange(n) % 64 < 32, lo, hi)]
    return np.array(rows).astype(np.int16), [2, 3]  # the alternating ones


@pytest.mark.parametrize("n", [4608, 4096, 1024])
def test_full_scale_sum_abs(az, n):
    a, alternating = full_scale_units(n)
    p = (0, 5, 0, 5, abi.MODE_FIXED_ONLY)
    ora = oracle.analyze_batch(a, oracle.make_params(*p), n, sample_bits=16, threads=8)
    want = np.abs(a.astype(np.int64)).sum(1)
    assert np.array_equal(ora["fixed_sums"][:, 0], want) and int(want[0]) == n * 32768
    for u in alternating:
        assert int(ora["meta"]["status"][u]) == 0 and int(ora["meta"]["fixed_order"][u]) == 0, u
    for generic in (0, 1):
        with knob("FLACMI_STREAM_GENERIC", generic):
            out = az.analyze(a, make_params(*p), n, sample_bits=16, debug=True)
            assert np.array_equal(out["fixed_sums"][:, 0], ora["fixed_sums"][:, 0])
            compare(out, ora, n)
            compare(az.analyze(a, make_params(*p), n, sample_bits=16, debug=False), ora, n)
