"""The order-1 closed form beside the energy bound restated on the CPU oracle's results:
the three words k_lpc adds per unit (flac-py_amd/csrc/k_lpc.hip lpc_finish) and the second test
k_resid_stream runs where the energy bound's pre-test fails (k_stream.hip).  Shared by
tests/test_order1_bound_model.py (no device) and tests/test_gpu_order1_bound.py.  Test
infrastructure only; importing it needs no GPU.

The first test takes the maxima of E_p and U2_p over every order, and on the headline workload it
is order 1 that keeps them up: its properly signed residual is large at q = 5.  Order 1 needs no
energy argument.  With the record's coefficient c and shift s, r_i = x_i - floor(c x_{i-1} / 2^s),
and with d_i = x_i - x_{i-1}
    2^s r_i = (2^s - c) x_i + c d_i + 2^s f,  f in [0, 1),
so over i = 1 .. n - 1
    2^s sum |r_i| >= |2^s - c| sum |x_i| - |c| sum |d_i| - 2^s n
                  >= |2^s - c| max(F0 - 32768, 0) - |c| F1 - 2^s n,
F0 and F1 the exact fixed sums of orders 0 and 1 (F0 counts |x_0| <= 32768, F1 is sum |d_i|).
The second test: orders 2 .. L by the energy bound on maxima over those orders alone, order 1 by
the closed form, both above the best fixed sum by 3 n more than strictly needed: the quarter
tiers' bound after four quarters is at least exact - 2 n - 1024, so a unit this test decides is one
the tiers decide too."""
import math

import numpy as np

import energy_bound_model as M

MARGIN_N = 3  # both inequalities ask for fmin + 3 n
X0_MAX = 32768


def order_terms(acf, s, c):
    """E_p of one order (shift s, coefficients c), as energy_bound_model.words computes it."""
    a = [1 << s] + c
    p = len(c)
    en = 0.0
    for lag in range(p + 1):
        g = sum(a[j] * a[j + lag] for j in range(p + 1 - lag))
        en += float(g if lag == 0 else 2 * g) * float(acf[lag])
    sa = sum(abs(v) for v in a) / float(1 << s)
    return en / float(1 << (2 * s)) + sa * sa * float(acf[0]) * 2.0 ** -39


def words(acf, rec, L, n, kappa, with_order1=False):
    """k_lpc's three new words: the pair (U1, ceil(256 U2)) over orders 2 .. L ((0, 0): there is
    none, the pair that always passes) and (uint16)c_1 | shift_1 << 16; None where the first pair
    is unusable (the new words then mean nothing).  with_order1: the mutation that leaves order 1
    in the maxima."""
    if M.words(acf, rec, L, n, kappa)[0] == M.UNUSABLE:
        return None
    orders = M.record_orders(rec, L)
    s1, c1 = orders[0][0], orders[0][1][0]
    w4 = (c1 & 0xFFFF) | (s1 << 16)
    rest = orders if with_order1 else orders[1:]
    if not rest:
        return 0, 0, w4
    emax = u2max = 0.0
    for s, c in rest:
        emax = max(emax, order_terms(acf, s, c))
        u2max = max(u2max, sum(abs(c[j]) * kappa[j] for j in range(len(c))) / float(1 << s))
    u1 = math.ceil(math.sqrt(n * emax) * (1.0 + 2.0 ** -40)) + 1
    u2 = math.ceil(256.0 * u2max * (1.0 + 2.0 ** -40)) + 1
    return u1, u2, w4


def unpack_order1(w4):
    """(c_1, shift_1) of the order-1 word."""
    c = w4 & 0xFFFF
    return (c - 0x10000 if c & 0x8000 else c), w4 >> 16


def order1_bound(w4, n, f0, f1, drop_n=False, abs_wrong=False, keep_x0=False):
    """(a lower bound of 2^s times order 1's exact sum, s).  The keyword arguments are the
    mutations DESIGN §4 records."""
    c, s = unpack_order1(w4)
    a = ((1 << s) - abs(c)) if abs_wrong else abs((1 << s) - c)
    sx = f0 if keep_x0 else max(f0 - X0_MAX, 0)
    return a * sx - abs(c) * f1 - (0 if drop_n else (n << s)), s


def rest_bound(x, u1, u2, f0):
    """The energy bound of orders 2 .. L times 256 from their own pair (None: no such order)."""
    if u1 == 0 and u2 == 0:
        return None
    n = len(x)
    _, cw = M.tables(n)
    return 16 * M.weighted_eighths(x, cw) - 256 * (u1 + n) - u2 * f0


def bounds(x, acf, rec, L, fixed_sums, with_order1=False, **mut):
    """None where the words are unusable, else (order 1's bound times 2^s, s, the other orders'
    bound times 256 or None)."""
    n = len(x)
    kappa, _ = M.tables(n)
    w = words(acf, rec, L, n, kappa, with_order1)
    if w is None:
        return None
    f0, f1 = int(fixed_sums[0]), int(fixed_sums[1])
    b1, s = order1_bound(w[2], n, f0, f1, **mut)
    return b1, s, rest_bound(x, w[0], w[1], f0)


def margins(x, acf, rec, L, fixed_sums, **mut):
    """None (unusable words), else the two margins of the kernel's second test as fractions of
    their thresholds: (orders 2 .. L or None, order 1); the test passes where both are > 0."""
    b = bounds(x, acf, rec, L, fixed_sums, **mut)
    if b is None:
        return None
    b1, s, br = b
    n = len(x)
    thr = int(min(int(v) for v in fixed_sums)) + MARGIN_N * n
    m1 = (b1 - (thr << s)) / float(max(thr << s, 1))
    mr = None if br is None else (br - 256 * thr) / float(max(256 * thr, 1))
    return mr, m1


def decides(x, acf, rec, L, fixed_sums, **mut):
    """The kernel's second test alone (it runs where the first one failed on usable words)."""
    m = margins(x, acf, rec, L, fixed_sums, **mut)
    return m is not None and (m[0] is None or m[0] > 0) and m[1] > 0
