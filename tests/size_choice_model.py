"""The subframe choice by exact written size (FLACMI_FLAG_SIZE_CHOICE, include/flacmi.h) in plain
integers over (samples, LPC records, parameters), and its application to analysis results: the CPU
model the device kernel k_size_choice is tested against.  TEST INFRASTRUCTURE ONLY.

For a unit of n samples written at ss bits:
  candidates   fixed orders 0..4 (order 0 alone when n <= 4), then, in the reference mode, the LPC
               orders 1..L with the record's quantised coefficients and shift
  eligible     a partition order exists for predictor order P (rice_search_model.candidate_orders)
               and, if LPC, the order is not in the record's negative-shift mask and q != 16
  size         bits = 8 + P ss + (LPC: 9 + P q) + 6 + W, W = rice_search_model.search_np(...)["W"]
  choice       the first strictly smallest bits in candidate order

Records have the layout of oracle.analyze_batch(...)["lpc_records"] (lpc_sign_model.analyze writes
the same for the corrected sign): word 1 the negative-shift mask, word 2 + (P - 1) the shift of
order P, words 2 + 32 + P (P - 1) / 2 .. its P coefficients.
"""
import numpy as np

import rice_search_model as RM
from flac_amd import abi
from lpc_sign_model import lpc_residual, zigzag

FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))
STATUS_ASSERTION, SITE_RICE_NO_ORDER = 2, 11
STATUS_RESIDUAL_WIDE, SITE_RESIDUAL_WIDTH = 16, 14
LPC_STAGE_SITES = range(1, 10)  # FLACMI_SITE_TUKEY .. FLACMI_SITE_LPC_EMPTY


def record_order(rec, P: int):
    """(coefficients, shift, in the negative-shift branch) of LPC order P."""
    off = 2 + 32 + (P * (P - 1)) // 2
    neg = bool((int(rec[1]) & 0xFFFFFFFF) >> (P - 1) & 1)
    return [int(v) for v in rec[off:off + P]], int(rec[2 + P - 1]), neg


def prefix_bits(lpc: bool, P: int, ss: int, q: int) -> int:
    """Header, warm-up, (precision, shift, coefficients,) coding method and partition order."""
    return 8 + P * ss + (9 + P * q if lpc else 0) + 6


def unit(x, rec, L: int, q: int, rmin: int, rmax: int, ss: int, reference: bool = True) -> dict:
    """Every candidate of one unit and the choice.  x: the n samples; rec: its LPC record (not read
    when reference is False).  -> {"fixed": [5 bits or -1], "lpc": [L bits or -1], "best": None or
    {"lpc", "P", "coefs", "shift", "bits", "z", "search"}, "fixed_best", "lpc_best": (order, bits)}"""
    x = np.asarray(x, dtype=np.int64)
    n = len(x)
    cands = [(False, k, list(FIXED[k]), 0, not (k == 0 or n > 4)) for k in range(5)]
    if reference:
        for P in range(1, L + 1):
            coefs, shift, neg = record_order(rec, P)
            cands.append((True, P, coefs, shift, neg or q == 16))
    out = {"fixed": [], "lpc": [], "best": None, "fixed_best": (-1, -1), "lpc_best": (-1, -1)}
    for lpc, P, coefs, shift, barred in cands:
        bits = -1
        if not barred and RM.candidate_orders(n, P, rmin, rmax):
            z = zigzag(lpc_residual(x, coefs, shift))
            s = RM.search_np(z, n, P, rmin, rmax)
            bits = prefix_bits(lpc, P, ss, q) + s["W"]
            if out["best"] is None or bits < out["best"]["bits"]:
                out["best"] = {"lpc": lpc, "P": P, "coefs": coefs, "shift": shift, "bits": bits, "z": z, "search": s}
            fam = "lpc_best" if lpc else "fixed_best"
            if out[fam][0] < 0 or bits < out[fam][1]:
                out[fam] = (P, bits)
        out["lpc" if lpc else "fixed"].append(bits)
    if not reference:
        out["lpc_best"] = (0, 0)
    return out


def apply(out: dict, rows, lens, L: int, q: int, rmin: int, rmax: int, ss: int, fixed_only: bool = False,
          residual_bytes: int = 8) -> dict:
    """The flag's results from analysis results `out` of the same rows with the flag clear
    (oracle.analyze_batch's, lpc_sign_model.analyze's for the corrected sign): its lpc_records and,
    for the units whose LPC stage fails, its status and site.  rows[u][:lens[u]] are unit u's
    samples.  Returns meta, rice_params, residual (uint64 rows), fixed_sums and lpc_sums as the
    device writes them; a unit whose LPC stage fails has a zero record but for status and site, and
    its other outputs are left as `out` has them."""
    n_units = len(lens)
    meta = np.zeros(n_units, dtype=abi.META_DTYPE)
    rice = out["rice_params"].copy()
    res = out["residual"].copy()
    fs = np.zeros((n_units, 5), dtype=np.int64)
    ls = np.zeros((n_units, 32), dtype=np.int64)
    choices = []
    for u in range(n_units):
        n = int(lens[u])
        m = meta[u]
        st, site = int(out["meta"]["status"][u]), int(out["meta"]["site"][u])
        if not fixed_only and st != 0 and site in LPC_STAGE_SITES:
            m["status"], m["site"] = st, site
            fs[u], ls[u] = out["fixed_sums"][u], out["lpc_sums"][u]
            choices.append(None)
            continue
        r = unit(rows[u][:n], None if fixed_only else out["lpc_records"][u], L, q, rmin, rmax, ss, not fixed_only)
        choices.append(r)
        fs[u] = r["fixed"]
        ls[u, :len(r["lpc"])] = r["lpc"]
        m["fixed_order"], m["fixed_sum"] = r["fixed_best"]
        m["lpc_order"], m["lpc_sum"] = r["lpc_best"]
        b = r["best"]
        if b is None:
            m["status"], m["site"] = STATUS_ASSERTION, SITE_RICE_NO_ORDER
            continue
        P = b["P"]
        m["kind"], m["order"], m["shift"] = (abi.KIND_LPC if b["lpc"] else abi.KIND_FIXED), P, b["shift"]
        if b["lpc"]:
            m["ncoefs"] = P
            m["coefs"][:P] = b["coefs"]
        res[u, :] = 0
        res[u, P:n] = b["z"]
        if residual_bytes == 4 and len(b["z"]) and int(b["z"].max()) >> 32:
            m["status"], m["site"] = STATUS_RESIDUAL_WIDE, SITE_RESIDUAL_WIDTH
            continue
        s = b["search"]
        for f in RM.SEARCHED:
            m[f] = s[f]
        rice[u, :s["n_parts"]] = s["rice_params"]
    return {"meta": meta, "rice_params": rice, "residual": res, "fixed_sums": fs, "lpc_sums": ls, "choices": choices}


COMPARED = tuple(f for f in abi.META_DTYPE.names if f != "coefs")


def mismatches(dev: dict, want: dict, lens, with_sums: bool = True) -> list:
    """(unit, field, device, model) wherever a device run with the flag differs from apply()."""
    bad = []
    for u in range(len(lens)):
        d, w = dev["meta"][u], want["meta"][u]
        bad += [(u, f, int(d[f]), int(w[f])) for f in COMPARED if int(d[f]) != int(w[f])]
        if list(d["coefs"]) != list(w["coefs"]):
            bad.append((u, "coefs", list(d["coefs"]), list(w["coefs"])))
        if want["choices"][u] is None:
            continue
        if with_sums:
            for name in ("fixed_sums", "lpc_sums"):
                if list(dev[name][u]) != list(want[name][u]):
                    bad.append((u, name, list(dev[name][u]), list(want[name][u])))
        if int(w["status"]) == 0:
            n, k = int(lens[u]), int(w["n_parts"])
            if list(dev["rice_params"][u][:k]) != list(want["rice_params"][u][:k]):
                bad.append((u, "rice_params", list(dev["rice_params"][u][:k]), list(want["rice_params"][u][:k])))
            if not np.array_equal(np.asarray(dev["residual"][u][:n], dtype=np.uint64), want["residual"][u][:n]):
                bad.append((u, "residual", None, None))
    return bad
