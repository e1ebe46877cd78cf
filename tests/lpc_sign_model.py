"""CPU model of the corrected-LPC-sign mode (FLACMI_FLAG_LPC_SIGN, include/flacmi.h): the
dictionary oracle.analyze_batch returns (meta, rice_params, residual, lpc_records, fixed_sums,
lpc_sums, acf), as the reference would compute it if its levinson_durbin (encoder.py:453-479)
ended with `return [-c for c in coefs[1:]]`.  TEST INFRASTRUCTURE ONLY.

Built from pieces the oracle exports, so that nothing of the mode is restated in C:

  acf, fixed sums      oracle.analyze_batch in the default mode (sign-independent)
  the fixed subframe   oracle.analyze_batch in FLACMI_MODE_FIXED_ONLY (its meta row, residual and
                       Rice fields are what the reference mode has when the fixed subframe wins)
  Levinson-Durbin      oracle.levinson per order, every order before any quantiser (encoder.py:374)
  the negation         in Python, on the floats (exact)
  the quantiser        oracle.quantize on the negated floats (encoder.py:482-534)
  residuals, sums      numpy int64 (encoder.py:537-548: x[i] - (sum(x[i-1-j] c[j]) >> shift))
  order and choice     the first minimum (encoder.py:404); fixed < LPC, LPC < fixed, else the
                       AssertionError of encoder.py:157
  Rice fields          oracle.analyze_unit in FLACMI_MODE_RICE_ONLY on the chosen LPC residual

Because the result has analyze_batch's shape, oracle/frame_writer.py, fallback_model and
stereo_model's frame functions take it unchanged.
"""
import numpy as np

import oracle
import stereo_model as SM
from flac_amd import abi

SITE_TUKEY, SITE_LPC_EMPTY, SITE_CHOICE_TIE = 1, 9, 10


def zigzag(r: np.ndarray) -> np.ndarray:
    r = r.astype(np.int64)
    return ((r << 1) ^ (r >> 63)).astype(np.uint64)


def lpc_residual(x: np.ndarray, coefs, shift: int) -> np.ndarray:
    """encoder.py:537-548 (sample_bits + q <= 44 keeps every sum inside int64)."""
    k = len(coefs)
    n = len(x)
    if k == 0:
        return x.copy()
    if n <= k:
        return np.zeros(0, dtype=np.int64)
    s = np.zeros(n - k, dtype=np.int64)
    for j, c in enumerate(coefs):
        s += x[k - 1 - j:n - 1 - j] * np.int64(c)
    return x[k:] - (s >> np.int64(shift))


def _rice_python(res, n, order, rmin, rmax):
    """encode_residual (encoder.py:632-760) for the ([], 0) winner, whose residual holds all n
    samples under predictor order `order`: a shape FLACMI_MODE_RICE_ONLY cannot state.
    -> (status, site, part_order, n_parts, coding_method, rice_bits, params)"""
    zz = [int(v) for v in zigzag(np.asarray(res))]
    best = None
    n_parts = 0
    any_order = False
    for o in range(rmin, rmax + 1):
        if not (n % (1 << o) == 0 and (n >> o) > order):
            continue
        any_order = True
        ps, pos, size, params = n >> o, 0, 0, []
        while pos < len(zz):
            ln = min((ps - order) if not params else ps, len(zz) - pos)
            s = sum(zz[pos:pos + ln])
            if s == 0:
                return 3, 12, 0, n_parts, 0, 0, (best[2] if best else [])
            param, _ = oracle.floor_log2(s / ln)
            if param < 0:
                return 3, 13, 0, n_parts, 0, 0, (best[2] if best else [])
            size += 4 + (5 if param > 14 else 4) + sum(v >> param for v in zz[pos:pos + ln]) + ln * (1 + param)
            params.append(param)
            pos += ln
        if best is None or size < best[1]:
            best = (o, size, params)
            n_parts = len(params)
    if not any_order:
        return 2, 11, 0, 0, 0, 0, []
    return 0, 0, best[0], n_parts, 5 if any(p > 14 for p in best[2]) else 4, best[1], best[2]


def analyze(samples2d: np.ndarray, params: abi.Params, block_len: int, tail_len: int = 0, n_tail_units: int = 0,
            sample_bits: int = 16, threads: int = 4) -> dict:
    """oracle.analyze_batch's result for the mode.  params.mode is FLACMI_MODE_REFERENCE or
    FLACMI_MODE_LPC_ONLY; the flag bit of params.reserved[1] is not looked at."""
    assert params.mode in (abi.MODE_REFERENCE, abi.MODE_LPC_ONLY)
    L, q, rmin, rmax = params.max_lpc_order, params.qlp_precision, params.rice_min, params.rice_max
    rows = np.ascontiguousarray(samples2d)
    n_units, stride = rows.shape
    base = oracle.analyze_batch(rows, oracle.make_params(L, q, rmin, rmax), block_len, tail_len, n_tail_units,
                                sample_bits=sample_bits, threads=threads)
    fixed = oracle.analyze_batch(rows, oracle.make_params(0, q, rmin, rmax, abi.MODE_FIXED_ONLY), block_len, tail_len,
                                 n_tail_units, sample_bits=sample_bits, threads=threads)
    pstride = (1 << max(rmax, 0)) + 1
    meta = np.zeros(n_units, dtype=abi.META_DTYPE)
    rice = np.zeros((n_units, pstride), dtype=np.int32)
    res = np.zeros((n_units, stride), dtype=np.uint64)
    ls = np.zeros((n_units, 32), dtype=np.int64)
    rec = np.zeros((n_units, abi.lpc_rec_words(32)), dtype=np.int32)
    rec_ok = np.zeros(n_units, dtype=bool)  # the record of a unit that fails before it is complete is undefined
    asym = 0  # (unit, order) pairs with quantise(-c) != -quantise(c)
    for u in range(n_units):
        n = tail_len if (n_tail_units and u >= n_units - n_tail_units) else block_len
        x = rows[u, :n].astype(np.int64)
        m = meta[u]
        m["fixed_order"], m["fixed_sum"] = fixed["meta"][u]["fixed_order"], fixed["meta"][u]["fixed_sum"]

        def fail(st, site):
            m["status"], m["site"] = st, site

        st, _ = oracle.tukey(n)
        if st:
            fail(abi.STATUS_ZERO_DIVISION, SITE_TUKEY)
            continue
        acf = base["acf"][u]
        cs = []
        for order in range(1, L + 1):
            st, site, c = oracle.levinson(acf[:order + 1], order)
            if st:
                fail(st, site)
                break
            cs.append(c)
        if m["status"]:
            continue
        qs = []
        for c in cs:
            st, site, qc, sh = oracle.quantize(-c, q)
            if st:
                fail(st, site)
                break
            qs.append((qc, sh))
            st0, _, qc0, sh0 = oracle.quantize(c, q)
            asym += st0 == 0 and (sh0 != sh or [-v for v in qc0] != qc)
        if m["status"]:
            continue
        negmask = 0
        for order, (qc, sh) in enumerate(qs, 1):
            if not qc:
                negmask |= 1 << (order - 1)
            rec[u, 2 + order - 1] = sh
            off = 2 + 32 + (order * (order - 1)) // 2
            rec[u, off:off + len(qc)] = qc
        rec[u, 1] = np.array(negmask, dtype=np.uint32).astype(np.int32)
        rec_ok[u] = True
        if L == 0:
            fail(abi.STATUS_VALUE_ERROR, SITE_LPC_EMPTY)
            continue
        rs = [lpc_residual(x, qc, sh) for qc, sh in qs]
        sums = [int(np.abs(r).sum()) for r in rs]
        ls[u, :L] = sums
        best = min(range(L), key=lambda k: sums[k])  # the first minimum
        m["lpc_order"], m["lpc_sum"] = best + 1, sums[best]
        qc, sh = qs[best]

        def take_lpc():
            m["kind"], m["order"], m["shift"], m["ncoefs"] = abi.KIND_LPC, best + 1, sh, len(qc)
            m["coefs"][:len(qc)] = qc
            m["res_offset"], m["res_len"] = len(qc), len(rs[best])
            res[u, len(qc):len(qc) + len(rs[best])] = zigzag(rs[best])

        if params.mode == abi.MODE_LPC_ONLY:
            take_lpc()
            m["part_order"] = -1
            continue
        fsum = int(m["fixed_sum"])
        if fsum < sums[best]:
            meta[u] = fixed["meta"][u]
            meta[u]["lpc_order"], meta[u]["lpc_sum"] = best + 1, sums[best]
            res[u] = fixed["residual"][u]
            rice[u] = fixed["rice_params"][u]
        elif sums[best] < fsum:
            take_lpc()
            if qc:
                p = oracle.make_params(0, q, rmin, rmax, abi.MODE_RICE_ONLY)
                p.reserved[0] = best + 1
                r1 = oracle.analyze_unit(np.concatenate([np.zeros(best + 1, dtype=np.int64), rs[best]]), p)
                fields = [int(r1[f]) for f in ("status", "site", "part_order", "n_parts", "coding_method", "rice_bits")]
                prm = list(r1["rice_params"])
            else:
                *fields, prm = _rice_python(rs[best], n, best + 1, rmin, rmax)
            for f, v in zip(("status", "site", "part_order", "n_parts", "coding_method", "rice_bits"), fields):
                m[f] = v
            rice[u, :len(prm)] = prm
        else:
            fail(abi.STATUS_ASSERTION, SITE_CHOICE_TIE)
    return {"meta": meta, "rice_params": rice, "residual": res, "acf": base["acf"], "fixed_sums": base["fixed_sums"],
            "lpc_sums": ls, "lpc_records": rec, "record_ok": rec_ok, "asymmetric": asym}


def stereo_analyse(rows, params, block_len, tail_len, ss, threads=4):
    """stereo_model.analyse with this model in place of oracle.analyze_batch."""
    nf = rows.shape[0] // 2
    mid, side = SM.candidate_rows(rows, block_len, tail_len)
    tail = 1 if tail_len else 0
    o_lr = analyze(rows, params, block_len, tail_len, 2 * tail, sample_bits=ss, threads=threads)
    o_m = analyze(mid, params, block_len, tail_len, tail, sample_bits=ss, threads=threads)
    o_s = analyze(side, params, block_len, tail_len, tail, sample_bits=ss + 1, threads=threads)
    return [[(rows[2 * f], o_lr, 2 * f, ss), (rows[2 * f + 1], o_lr, 2 * f + 1, ss), (mid[f], o_m, f, ss),
             (side[f], o_s, f, ss + 1)] for f in range(nf)]


# ---------------------------------------------------------------------------------
# a frame reader of its own (decoder.py:111-130, :431-498 of the reference restated over bit
# strings), so that the CPU test can return a frame to its samples without a device
# ---------------------------------------------------------------------------------
_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def decode_frame(data: bytes, C: int, ss: int):
    """One frame under the L_R header encode() writes, holding C subframes of ss-bit samples ->
    (frame number, [C] lists of samples).  Checks CRC-8, CRC-16 and the padding."""
    import frame_writer as FW
    s = bin(int.from_bytes(b"\x01" + data, "big"))[3:]
    pos = 0

    def u(w):
        nonlocal pos
        v = int(s[pos:pos + w], 2) if w else 0
        pos += w
        return v

    def i(w):
        v = u(w)
        return v - (1 << w) if v >> (w - 1) else v

    assert u(16) == 0xFFF8
    code = u(4)
    assert u(12) == 0x010
    first = u(8)
    k = 8 - (first ^ 0xFF).bit_length()  # leading ones
    number = first & (0xFF >> (k + 1)) if k else first
    for _ in range(max(k - 1, 0)):
        b = u(8)
        assert b >> 6 == 2
        number = (number << 6) | (b & 0x3F)
    n = u(8) + 1 if code == 6 else u(16) + 1 if code == 7 else {v: k_ for k_, v in FW.BLOCK_SIZE_CODES.items()}[code]
    assert u(8) == FW.crc8(data[:pos // 8 - 1])
    out = []
    for _ in range(C):
        assert u(1) == 0
        t = u(6)
        assert u(1) == 0
        if t == 0:
            out.append([i(ss)] * n)
            continue
        if t == 1:
            out.append([i(ss) for _ in range(n)])
            continue
        lpc = bool(t & 0b100000)
        assert lpc or t & 0b111000 == 0b001000
        order = (t & 31) + 1 if lpc else t & 7
        x = [i(ss) for _ in range(order)]
        if lpc:
            prec = u(4) + 1
            shift = u(5)
            coefs = [i(prec) for _ in range(order)]
        else:
            coefs, shift = _FIXED[order], 0
        pbits = {0: 4, 1: 5}[u(2)]
        po = u(4)
        for part in range(1 << po):
            prm = u(pbits)
            assert prm != (1 << pbits) - 1
            for _ in range((n >> po) - (order if part == 0 else 0)):
                one = s.index("1", pos)
                zz = ((one - pos) << prm) | (int(s[one + 1:one + 1 + prm], 2) if prm else 0)
                pos = one + 1 + prm
                r = (zz >> 1) ^ -(zz & 1)
                x.append(r + (sum(c * x[-1 - j] for j, c in enumerate(coefs)) >> shift))
        assert len(x) == n
        out.append(x)
    assert u(-pos % 8) == 0
    assert u(16) == FW.crc16(data[:pos // 8 - 2]) and pos == 8 * len(data)
    return number, out
