"""The exact Rice search (FLACMI_FLAG_RICE_SEARCH, include/flacmi.h) in plain Python integers, and
its application to analysis results: the CPU model the device kernel k_rice_search is tested
against.

For a unit of n samples whose zig-zag residual is z = row[P .. n):
  candidate orders  o in [rmin, rmax] with n % 2^o == 0 and (n >> o) > P   (encoder.py:664-667)
  partitions        partition 0 has (n >> o) - P values, the others n >> o  (split_samples_in_partitions)
  partition cost    c_p(k) = sum_i (z_i >> k) + (1 + k) len_p               (sum of rice_size, :756-760)
                    c4_p = min over k in 0..14, c5_p = min over k in 0..30, at the smallest such k
  written bits      W4(o) = sum_p (4 + c4_p), W5(o) = sum_p (5 + c5_p)
  walk              o ascending, method 4 before method 5: the first strictly smallest W wins
"""
import numpy as np

from flac_amd import abi

STATUS_VALUE_ERROR = 3
RICE_SITES = (12, 13)  # FLACMI_SITE_RICE_LOG_DOMAIN, FLACMI_SITE_RICE_NEG_SHIFT
SEARCHED = ("part_order", "n_parts", "coding_method", "rice_bits", "res_offset", "res_len")


def candidate_orders(n: int, P: int, rmin: int, rmax: int) -> list:
    return [o for o in range(rmin, rmax + 1) if n % (1 << o) == 0 and (n >> o) > P]


def partitions(z: list, n: int, P: int, o: int) -> list:
    p0 = (n >> o) - P
    ps = n >> o
    return [z[:p0]] + [z[i:i + ps] for i in range(p0, len(z), ps)]


def partition_cost(part: list, k: int) -> int:
    return sum(v >> k for v in part) + (1 + k) * len(part)


def best_parameter(part: list, kmax: int) -> tuple:
    """(cost, k): the smallest cost over k in 0..kmax and the smallest k that reaches it."""
    costs = [partition_cost(part, k) for k in range(kmax + 1)]
    c = min(costs)
    return c, costs.index(c)


def search(z, n: int, P: int, rmin: int, rmax: int):
    """The rule on the zig-zag values z = row[P .. n) -> dict, or None without a candidate order."""
    z = [int(v) for v in z]
    assert len(z) == n - P
    best = None
    for o in candidate_orders(n, P, rmin, rmax):
        parts = partitions(z, n, P, o)
        assert len(parts) == 1 << o
        for method, kmax in ((4, 14), (5, 30)):
            pk = [best_parameter(p, kmax) for p in parts]
            W = sum(method + c for c, _ in pk)
            if best is None or W < best["W"]:
                best = {"W": W, "part_order": o, "n_parts": 1 << o, "coding_method": method,
                        "rice_params": [k for _, k in pk]}
    if best is None:
        return None
    over = sum(k > 14 for k in best["rice_params"])
    assert (best["coding_method"] == 5) == (over > 0) and max(best["rice_params"]) <= 30
    # meta.rice_bits keeps the reference's estimate convention (encoder.py:714-727)
    best["rice_bits"] = best["W"] + (4 * best["n_parts"] if best["coding_method"] == 4 else 3 * best["n_parts"] + over)
    best["res_offset"], best["res_len"] = P, n - P
    return best


def search_np(z, n: int, P: int, rmin: int, rmax: int):
    """search() with numpy sums (values and partition sums below 2^63): the same dict."""
    row = np.zeros(n, dtype=np.uint64)
    row[P:] = np.asarray(z, dtype=np.uint64)
    best = None
    for o in candidate_orders(n, P, rmin, rmax):
        lens = np.full(1 << o, n >> o, dtype=np.int64)
        lens[0] -= P
        cost = np.stack([(row >> np.uint64(k)).reshape(1 << o, n >> o).sum(axis=1).astype(np.int64) + (1 + k) * lens
                         for k in range(31)])
        for method, kmax in ((4, 14), (5, 30)):
            k = np.argmin(cost[:kmax + 1], axis=0)  # the first, so the smallest, k at the minimum
            W = int(cost[k, np.arange(1 << o)].sum()) + method * (1 << o)
            if best is None or W < best["W"]:
                best = {"W": W, "part_order": o, "n_parts": 1 << o, "coding_method": method,
                        "rice_params": [int(v) for v in k]}
    if best is None:
        return None
    over = sum(k > 14 for k in best["rice_params"])
    best["rice_bits"] = best["W"] + (4 * best["n_parts"] if best["coding_method"] == 4 else 3 * best["n_parts"] + over)
    best["res_offset"], best["res_len"] = P, n - P
    return best


def bit_plane_sum(values, k: int) -> int:
    """sum (z >> k) from the bit-plane counts: sum over b >= k of 2^(b - k) cnt_b."""
    top = max((int(v).bit_length() for v in values), default=0)
    cnt = [sum((int(v) >> b) & 1 for v in values) for b in range(top)]
    return sum(cnt[b] << (b - k) for b in range(k, top))


def searched_unit(status: int, site: int) -> bool:
    return status == 0 or (status == STATUS_VALUE_ERROR and site in RICE_SITES)


def apply(out: dict, lens, rmin: int, rmax: int, rice_only_order=None, fast: bool = True) -> dict:
    """The flag's effect on analysis results `out` (oracle.analyze_batch's, or a device run's with
    the flag clear): meta (abi.META_DTYPE), rice_params and residual rows; lens[u] is unit u's
    length.  Returns copies of meta and rice_params with the searched units rewritten, and the set
    of rescued units.  A rescued unit's residual is row[P .. n) with P = meta.order (RICE_ONLY: the
    call's predictor order)."""
    meta, rice = out["meta"].copy(), out["rice_params"].copy()
    rescued = set()
    for u in range(len(meta)):
        st, site, n = int(meta["status"][u]), int(meta["site"][u]), int(lens[u])
        if not searched_unit(st, site):
            continue
        P = int(meta["res_offset"][u]) if st == 0 else (rice_only_order if rice_only_order is not None else int(meta["order"][u]))
        z = out["residual"][u][P:n]
        r = (search_np if fast else search)(z, n, P, rmin, rmax)
        if r is None:
            continue
        for f in SEARCHED:
            meta[f][u] = r[f]
        rice[u, :r["n_parts"]] = r["rice_params"]
        if st != 0:
            meta["status"][u], meta["site"][u] = 0, 0
            rescued.add(u)
    return {"meta": meta, "rice_params": rice, "residual": out["residual"], "rescued": rescued}


def meta_fields_differ(a, b, fields=None) -> list:
    """Names of the flacmi_unit_meta fields in which rows a and b differ."""
    names = fields or abi.META_DTYPE.names
    return [f for f in names if not np.array_equal(a[f], b[f])]


# what the device and the oracle both fill on a unit the reference's Rice step fails (the device
# zeroes res_offset, res_len and the Rice fields there, the oracle leaves what it had computed)
FAILED_UNIT_FIELDS = ("status", "site", "kind", "order", "shift", "ncoefs", "fixed_order", "fixed_sum")


def baseline_mismatches(dev, ora) -> list:
    """oracle.meta_mismatches for a unit analysed with the flag clear; on a failed unit the fields
    both sides define (and the coefficients)."""
    import oracle
    if int(ora["status"]) == 0:
        return oracle.meta_mismatches(dev, ora)
    if int(ora["site"]) not in RICE_SITES:  # failed before the choice: the exception alone
        return [(f, dev[f], ora[f]) for f in ("status", "site") if dev[f] != ora[f]]
    bad = [(f, dev[f], ora[f]) for f in FAILED_UNIT_FIELDS if dev[f] != ora[f]]
    k = int(ora["ncoefs"])
    if list(dev["coefs"][:k]) != list(ora["coefs"][:k]):
        bad.append(("coefs", list(dev["coefs"][:k]), list(ora["coefs"][:k])))
    return bad
