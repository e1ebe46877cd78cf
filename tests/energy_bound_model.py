"""The energy bound restated on the CPU oracle's results: the two words k_lpc writes
per unit (flac-py_amd/csrc/k_lpc.hip lpc_finish), the host's two window tables
(flacmi_host.cpp bound_tables), the weighted sum k_resid_stream gathers in staging and its
integer pre-test (k_stream.hip).  Shared by tests/test_energy_bound_model.py (no device) and
tests/test_gpu_energy_bound.py.  Test infrastructure only; importing it needs no GPU.

With the record's coefficients c (the reference's Levinson returns the negated predictor) and
shift s, r_i = x_i - floor(P_i), P_i = sum_j c_j x_{i-1-j} / 2^s.  e_i = x_i + P_i is the
residual of the properly signed predictor, so r_i = 2 x_i - e_i + frac and
    sum_i |r_i| >= sum_i w_i |r_i| >= 2 sum_i w_i |x_i| - sum_i |w_i e_i| - n
over i = p .. n - 2, for the window weights 0 <= w <= 1.  w_i e_i = eps_i + delta_i, where
eps = y_i + sum_j gamma_j y_{i-1-j} (y = x w, gamma = c / 2^s) has the energy alpha' R alpha of
the unit's autocorrelation (alpha = (1, gamma)), so sum |eps| <= sqrt(n alpha' R alpha) = U1, and
sum |delta| <= sum_j |gamma_j| kappa_{j+1} F0 = U2 F0 with kappa_k = max_i |w_i - w_{i-k}| and
F0 = sum |x|.  The weighted sum is taken per 8-sample chunk with floor(256 min w) as the chunk's
weight; sample n - 1 (outside the autocorrelation) and the samples below 16 (warm-up samples of
some order: no candidate's sum holds them) count as weight 0.
    sum |r| >= 2 W / 256 - U1 - U2 F0 - n   for every order."""
import math

import numpy as np

import oracle

UNUSABLE = 0xFFFFFFFF
LAGS = 13
K_SCPT = 5  # k_stream.hip kSCPT


def tables(n):
    """(kappa[1..13] as a list indexed k - 1, the chunk weights) of an n-sample unit's window."""
    st, w = oracle.tukey(n)
    assert st == 0, n
    kappa = []
    for k in range(1, LAGS + 1):
        d = np.abs(w[k:n - 1] - w[:n - 1 - k]) if n - 1 > k else np.zeros(1)
        kappa.append(float(d.max()) * (1.0 + 2.0 ** -50) if len(d) else 0.0)
    wz = w.copy()
    wz[n - 1] = 0.0
    cw = np.zeros((n + 7) // 8, dtype=np.int64)
    for c in range(2, n // 8):
        cw[c] = math.floor(256.0 * float(wz[8 * c:8 * c + 8].min()))
    return kappa, cw


def record_orders(rec, L):
    """[(shift, [c_0 .. c_{p-1}])] for p = 1 .. L of an expanded oracle record (stride 32)."""
    out = []
    for p in range(1, L + 1):
        base = 2 + 32 + p * (p - 1) // 2
        out.append((int(rec[2 + p - 1]), [int(v) for v in rec[base:base + p]]))
    return out


def words(acf, rec, L, n, kappa, drop_slack=False, zero_kappa=False):
    """k_lpc's two words (U1, ceil(256 U2)), or (UNUSABLE, UNUSABLE)."""
    if int(rec[0]) != 0 or int(rec[1]) != 0:
        return UNUSABLE, UNUSABLE
    emax = u2max = 0.0
    for s, c in record_orders(rec, L):
        a = [1 << s] + c
        p = len(c)
        en = 0.0
        for lag in range(p + 1):
            g = sum(a[j] * a[j + lag] for j in range(p + 1 - lag))
            en += float(g if lag == 0 else 2 * g) * float(acf[lag])
        sa = sum(abs(v) for v in a) / float(1 << s)
        en = en / float(1 << (2 * s)) + (0.0 if drop_slack else sa * sa * float(acf[0]) * 2.0 ** -39)
        u2 = 0.0 if zero_kappa else sum(abs(c[j]) * kappa[j] for j in range(p)) / float(1 << s)
        if not (0.0 <= en < 2.0 ** 80 and u2 < 2.0 ** 40):
            return UNUSABLE, UNUSABLE
        emax, u2max = max(emax, en), max(u2max, u2)
    u1 = math.ceil(math.sqrt(n * emax) * (1.0 + 2.0 ** -40)) + 1
    u2 = math.ceil(256.0 * u2max * (1.0 + 2.0 ** -40)) + 1
    if u1 >= UNUSABLE or u2 >= UNUSABLE:
        return UNUSABLE, UNUSABLE
    return u1, u2


def stream_threads(n):
    return max(64, 64 * ((n // 8 + 64 * K_SCPT - 1) // (64 * K_SCPT)))


def weighted_eighths(x, cw):
    """The staging sum as the kernel keeps it: thread t holds chunks t, t + NT, ..; each
    thread's weighted sum is cut to whole eighths before the reductions."""
    n = len(x)
    nt = stream_threads(n)
    per_chunk = np.abs(np.asarray(x, dtype=np.int64)).reshape(n // 8, 8).sum(1) * cw[:n // 8]
    lanes = np.zeros(nt, dtype=np.int64)
    np.add.at(lanes, np.arange(n // 8) % nt, per_chunk)
    return int((lanes >> 3).sum())


def lower_bound(x, acf, rec, L, drop_n=False, last_weight=False, **mut):
    """The bound on every LPC order's sum, times 256 (an exact integer), or None where the
    words are unusable.  The keyword arguments are the mutations DESIGN §4 records."""
    n = len(x)
    kappa, cw = tables(n)
    if last_weight:  # mutation: sample n - 1 keeps its window weight
        _, w = oracle.tukey(n)
        cw = cw.copy()
        cw[n // 8 - 1] = math.floor(256.0 * float(w[n - 8:n].min()))
    u1, u2 = words(acf, rec, L, n, kappa, **mut)
    if u1 == UNUSABLE:
        return None
    f0 = int(np.abs(np.asarray(x, dtype=np.int64)).sum())
    return 16 * weighted_eighths(x, cw) - 256 * (u1 + (0 if drop_n else n)) - u2 * f0


def decides(x, acf, rec, L, fixed_sums):
    """The kernel's pre-test: the bound strictly above the best fixed sum."""
    b = lower_bound(x, acf, rec, L)
    return b is not None and b > 256 * int(min(int(v) for v in fixed_sums))
