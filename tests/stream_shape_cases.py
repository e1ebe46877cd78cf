"""k_resid_stream's shape family (flac-py_amd/csrc/k_stream.hip): the host dispatch restated in
Python, the table of shapes the suite runs through the kernel, their inputs and the conditions
those inputs must meet on the CPU oracle.  Shared by tests/test_stream_shape_cases.py (no device)
and tests/test_gpu_stream_shapes.py.  Test infrastructure only; importing it needs no GPU."""
import functools
from collections import Counter, namedtuple

import numpy as np

import oracle
import sign_bound
from flac_amd import abi
from test_gpu_parity import _stream_tap_sums
from test_gpu_rice_dedup import ON_A_POWER_OF_TWO, full_scale_units, stepped_noise

K_SCPT = 5  # k_stream.hip kSCPT (FLACMI_STREAM_CPT): 8-sample chunks per thread
K_CPT = 3   # device_common.h kCPT: k_resid's chunks per thread


# ---------------------------------------------------------------------------------------
# the dispatch, restated line for line
# ---------------------------------------------------------------------------------------
def rmax_eff(n, rmin, rmax):
    """The largest Rice partition order of rmin..rmax that divides n (-1: none)."""
    e = -1
    for o in range(rmin, rmax + 1):
        if n % (1 << o) == 0:
            e = o
    return e


def stream_threads(n):
    """k_stream.hip stream_threads: the workgroup of an n-sample unit."""
    nt = 64 * ((n // 8 + 64 * K_SCPT - 1) // (64 * K_SCPT))
    return max(nt, 64)


def stream_shape(n, L, rmin, rmax, fixed_only):
    """None when stream_shape_ok refuses the shape (16-bit samples, 32-bit residual rows and the
    narrow path taken for granted: narrow_path), else the build launch_stream_G/T/R/K pick:
    nw waves, slots = chunks per thread in use, P finest partitions, the branch-free R05 build
    or the runtime-order one, NG MFMA groups, NFIX (the constant-shape build's block length)."""
    if not fixed_only and not 1 <= L <= 12:           # stream_shape_ok
        return None
    if n % 64 != 0 or n < 64 or n > 8 * K_SCPT * 256:
        return None
    e = rmax_eff(n, rmin, rmax)
    if e < 0 or (1 << e) > 32 or ((n >> e) & 7) != 0:
        return None
    NG = 0 if fixed_only else 1 if L <= 4 else 2 if L <= 8 else 3  # launch_stream_G
    maxord = L if NG > 0 and L > 4 else 4                           # launch_stream_T
    R05 = rmin == 0 and e == 5 and (n >> 5) > maxord
    nfix = 4608 if R05 and n == 4608 and (NG == 0 or L == 4 * NG) else 0  # launch_stream_R
    nt = stream_threads(n)                                          # launch_stream_K
    return {"nw": nt // 64, "slots": (n // 8) / nt, "P": 1 << e, "R05": R05, "NG": NG, "NFIX": nfix}


def narrow_path(n, L, q, fixed_only, bits=16):
    """flacmi_host.cpp: path 0 (the only one stream_shape_ok takes) = not needs_wide, q <= 16."""
    xmax = 2.0 ** (bits - 1)
    rmax = 16.0 * xmax if fixed_only else xmax * (1.0 + L * 2.0 ** (q - 1)) + 16.0 * xmax
    nch = (n + 7) // 8
    nt = max(64, min(64 * ((nch + 64 * K_CPT - 1) // (64 * K_CPT)), 256))  # resid_threads
    per_thread = 8 * ((nch + nt - 1) // nt)                                 # resid_samples_per_thread
    wide = bits > 24 or q > 24 or rmax >= 2.0 ** 26 or rmax * per_thread >= 2.0 ** 32
    return not wide and q <= 16


def list2_lmax(L):
    """The history pad HP = resid_hp(LMAX) of k_resid's list variant behind the stream kernel's
    list kernel (launch_resid_retry_l8 for L <= 8, else _l12): its sign bound runs over [HP, n)."""
    return 8 if L <= 8 else 16


# ---------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------
Case = namedtuple("Case", "n L q rmin rmax nw R05 NG min_list2")
CASES = [
    Case(64, 12, 5, 0, 3, 1, False, 3, 0),     # 1/8 of a slot: 8 chunks on 64 lanes
    Case(128, 4, 5, 0, 4, 1, False, 1, 0),
    Case(256, 12, 5, 0, 5, 1, False, 3, 0),    # n >> 5 = 8 <= L: the runtime-order build
    Case(320, 3, 5, 0, 2, 1, False, 1, 0),
    Case(2560, 12, 5, 0, 5, 1, True, 3, 0),    # one wave, every slot full
    Case(2816, 9, 6, 0, 5, 2, True, 3, 0),     # ragged last slot (2.75)
    Case(4096, 8, 5, 0, 5, 2, True, 2, 0),     # bench.py --config b4096's block and L, orders 0..5
    Case(4096, 8, 5, 0, 4, 2, False, 2, 0),    # b4096's own -r 0,4: the runtime-order build
    Case(5120, 12, 6, 0, 5, 2, True, 3, 4),
    Case(5376, 12, 5, 0, 5, 3, True, 3, 0),    # ragged (3.5)
    Case(6144, 2, 7, 1, 3, 3, False, 1, 0),
    Case(7680, 11, 6, 0, 5, 3, True, 3, 4),
    Case(7936, 6, 5, 0, 5, 4, True, 2, 0),     # ragged (3.875)
    Case(10176, 10, 6, 0, 3, 4, False, 3, 4),  # ragged (4.97), 8 finest partitions
    Case(10240, 12, 5, 0, 5, 4, True, 3, 0),   # the length limit: every slot of four waves
    Case(10240, 12, 6, 2, 5, 4, False, 3, 4),
    Case(10240, 5, 5, 0, 4, 4, False, 2, 0),
]
# MODE_FIXED_ONLY (NG 0) over the same inputs: the largest predictor order is 4 there
FIXED_CASES = [c._replace(L=0, NG=0, min_list2=0) for c in CASES
               if (c.n, c.rmax) in ((64, 3), (320, 2), (2816, 5), (5376, 5), (7936, 5)) or c[:5] == (10240, 12, 5, 0, 5)]
SHORT_FINEST = ((64, 3), (256, 5))  # finest partitions of 8 samples: no longer than orders 8..12

# (block, tail, L): 48 open units at q 6, -r 0,5, the last 6 cut to the tail
TAIL_CALLS = [(5376, 256, 12), (4608, 3328, 8), (10240, 768, 12)]
TAIL_UNITS, TAIL_CUT, TAIL_Q = 48, 6, 6


def case_id(c):
    return f"{c.n}-l{c.L}-q{c.q}-r{c.rmin}{c.rmax}"


def check_dispatch(c, fixed_only=False):
    """The case's expected build through the restated host check."""
    s = stream_shape(c.n, c.L, c.rmin, c.rmax, fixed_only)
    assert s is not None, c
    assert (s["nw"], s["R05"], s["NG"]) == (c.nw, c.R05, c.NG), (c, s)
    assert s["NFIX"] == 0 and narrow_path(c.n, c.L, c.q, fixed_only), (c, s)
    return s


# ---------------------------------------------------------------------------------------
# inputs and the oracle's results, made once
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_units(n, rmin, rmax):
    """32 units of the bench's open mix (5/8 MA(1) noise: LPC wins or nearly ties, and both
    list kernels get units), then per partition order of rmin..rmax_eff four stepped-noise
    units and two whose segment means sit on a power of two (every order wins somewhere)."""
    e = rmax_eff(n, rmin, rmax)
    rng = np.random.default_rng(1000 * n + 10 * rmin + rmax)
    rows = [oracle.synth_batch(0, 32, n, 16, 4000 + n + rmax, dtype=np.int16, open_eighths=5)]
    rows.append(np.stack([stepped_noise(rng, n, o) for o in range(rmin, e + 1) for _ in range(4)]))
    rows.append(np.stack([stepped_noise(rng, n, o, ON_A_POWER_OF_TWO) for o in range(rmin, e + 1) for _ in range(2)]))
    a = np.ascontiguousarray(np.concatenate(rows))
    a.setflags(write=False)
    return a


def _freeze(ora):
    for v in ora.values():
        v.setflags(write=False)
    return ora


@functools.lru_cache(maxsize=None)
def case_reference(c, fixed_only=False):
    a = case_units(c.n, c.rmin, c.rmax)
    mode = abi.MODE_FIXED_ONLY if fixed_only else abi.MODE_REFERENCE
    p = oracle.make_params(0 if fixed_only else c.L, c.q, c.rmin, c.rmax, mode)
    return a, _freeze(oracle.analyze_batch(a, p, c.n, sample_bits=16, threads=16))


@functools.lru_cache(maxsize=None)
def full_scale_reference(fixed_only):
    n = 10240
    a, _ = full_scale_units(n)
    a.setflags(write=False)
    mode = abi.MODE_FIXED_ONLY if fixed_only else abi.MODE_REFERENCE
    p = oracle.make_params(0 if fixed_only else 12, 5, 0, 5, mode)
    return a, _freeze(oracle.analyze_batch(a, p, n, sample_bits=16, threads=8))


@functools.lru_cache(maxsize=None)
def tail_reference(block, tail, L):
    a = oracle.synth_batch(0, TAIL_UNITS, block, 16, 6000 + block + tail, dtype=np.int16, open_eighths=5)
    a[TAIL_UNITS - TAIL_CUT:, tail:] = 0
    a.setflags(write=False)
    p = oracle.make_params(L, TAIL_Q, 0, 5)
    return a, _freeze(oracle.analyze_batch(a, p, block, tail, TAIL_CUT, sample_bits=16, threads=16))


# ---------------------------------------------------------------------------------------
# conditions on the oracle alone
# ---------------------------------------------------------------------------------------
def classify(a, ora, L, lens):
    """Per unit, from the oracle's record: None (an exception other than the choice tie: no
    lpc_tiers), "batch" (inside k_resid_stream's f16 bound (sum|c| + 2^shift) * 33023 < 2^22 for
    every order), "list" (outside it, every sum|c| <= 127: the list kernel's pred-only taps) or
    ("list2", decided): k_resid's list variant, with its sign bound restated on the record."""
    out = []
    for u, n in enumerate(lens):
        if int(ora["meta"]["status"][u]) != 0 and int(ora["meta"]["site"][u]) != abi.SITE_CHOICE_TIE:
            out.append(None)
            continue
        sums = _stream_tap_sums(ora["lpc_records"][u], L)
        if all((c + sh) * 33023 < 2 ** 22 for c, sh in sums):
            out.append("batch")
        elif all(c <= 127 for c, _ in sums):
            out.append("list")
        else:
            out.append(("list2", sign_bound.decides(a[u][:n], ora["lpc_records"][u], L, ora["fixed_sums"][u],
                                                    lmax=list2_lmax(L))))
    return out


def class_counts(classes):
    return Counter("list2" if isinstance(k, tuple) else k for k in classes if k is not None)


def check_case_oracle(c, fixed_only=False):
    """The conditions a case's inputs must meet before any device result counts; returns the
    facts the caller may print."""
    a, ora = case_reference(c, fixed_only)
    om = ora["meta"]
    ok = om["status"] == 0
    e = rmax_eff(c.n, c.rmin, c.rmax)
    facts = {"units": len(a), "ok": int(ok.sum())}
    assert ok.sum() >= 0.8 * len(a), facts
    wins = [int((om["part_order"][ok] == o).sum()) for o in range(c.rmin, e + 1)]
    facts["order_wins"] = wins
    assert min(wins) >= 3, (c, wins)
    if fixed_only:
        assert (om["kind"][ok] == abi.KIND_FIXED).all()
        return facts
    lpc = ok & (om["kind"] == abi.KIND_LPC)
    facts["lpc"] = int(lpc.sum())
    facts["lpc_orders"] = sorted(set(int(v) for v in om["order"][lpc]))
    assert facts["lpc"] >= 8, (c, facts)
    assert len(facts["lpc_orders"]) >= min(c.L, 3), (c, facts)
    if (c.n, c.rmax) in SHORT_FINEST:
        # the reference drops partition orders per unit by (n >> o) > predictor order
        # (encoder.py:664-667): these units cannot take the finest order
        short = ok & (om["order"] >= (c.n >> e))
        facts["short_finest"] = int(short.sum())
        assert (c.n >> e) == 8 and facts["short_finest"] >= 4, (c, facts)
        assert (om["part_order"][short] < e).all()
    cnt = class_counts(classify(a, ora, c.L, [c.n] * len(a)))
    facts["classes"] = dict(cnt)
    assert cnt["batch"] >= 1 and cnt["list"] >= 1 and cnt["list2"] >= c.min_list2, (c, facts)
    return facts


def check_full_scale_oracle(fixed_only):
    a, ora = full_scale_reference(fixed_only)
    n = a.shape[1]
    assert stream_shape(n, 0 if fixed_only else 12, 0, 5, fixed_only) == \
        {"nw": 4, "slots": 5.0, "P": 32, "R05": True, "NG": 0 if fixed_only else 3, "NFIX": 0}
    assert np.array_equal(ora["fixed_sums"][:, 0], np.abs(a.astype(np.int64)).sum(1))
    # full-scale alternation: 524272 per sample at fixed order 4, past 2^32 over 10240 samples
    assert int(ora["fixed_sums"].max()) >= 2 ** 32, int(ora["fixed_sums"].max())
    om = ora["meta"]
    for u in (0, 1):  # constant full scale: log2(0) in the Rice search (ValueError)
        assert (int(om["status"][u]), int(om["site"][u])) == (3, 12), (u, om["status"][u], om["site"][u])
    assert (om["status"][2:4] == 0).all()
    return {"max_fixed_sum": int(ora["fixed_sums"].max()), "status": [int(v) for v in om["status"]]}


def check_tail_oracle(block, tail, L):
    a, ora = tail_reference(block, tail, L)
    body, cut = stream_shape(block, L, 0, 5, False), stream_shape(tail, L, 0, 5, False)
    assert body is not None and cut is not None, (block, tail, body, cut)
    assert narrow_path(block, L, TAIL_Q, False) and narrow_path(tail, L, TAIL_Q, False)
    lens = [block] * (TAIL_UNITS - TAIL_CUT) + [tail] * TAIL_CUT
    cls = classify(a, ora, L, lens)
    nb, nt = class_counts(cls[:-TAIL_CUT]), class_counts(cls[-TAIL_CUT:])
    assert nb["list"] + nb["list2"] >= 1 and nt["list"] + nt["list2"] >= 1, (block, tail, nb, nt)
    return {"body": body, "tail": cut, "body_classes": dict(nb), "tail_classes": dict(nt)}
