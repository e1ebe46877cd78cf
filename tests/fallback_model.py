"""CPU model of the fallback-subframe mode (FLACMI_FRAME_FALLBACK, include/flacmi.h) over
oracle.analyze_batch results: the decision rule per unit and the frames it gives, with the
oracle frame writer's pieces (oracle/frame_writer.py) and a CONSTANT / VERBATIM writer of its
own.  TEST INFRASTRUCTURE ONLY.

A unit of n samples at stream sample size ss is escaped when its status is a reference
exception (1..4), when it is an LPC subframe and precision - 1 == 0b1111 (the writer's
assertion), or when its status is 0 and its exact subframe size, counted here by writing it,
is strictly greater than 8 + n * ss.  An escaped unit is CONSTANT when its samples are all
equal, else VERBATIM.  Status 16 (the residual does not fit 32 bits) is not escaped.  A unit of
status 0 whose samples are all equal (the Rice search has rescued its all-zero residual) is
CONSTANT when its size is strictly greater than 8 + ss.
"""
import numpy as np

import frame_writer as FW

ANALYSED, CONSTANT, VERBATIM = 0, 1, 2
REFERENCE_EXCEPTIONS = (1, 2, 3, 4)  # ZeroDivisionError, AssertionError, ValueError, OverflowError


def _unit(out, u):
    m = out["meta"][u]
    off, ln = int(m["res_offset"]), int(m["res_len"])
    return m, out["residual"][u][off:off + ln], out["rice_params"][u][: int(m["n_parts"])]


def subframe_bits(samples, out, u, n, ss, q) -> int:
    """Exact size of unit u's analysed subframe: what frame_writer.subframe writes."""
    m, zz, prm = _unit(out, u)
    b = FW.Bits()
    FW.subframe(b, samples, m, zz, prm, n, ss, q)
    return b.n


def sub_kind(samples, out, u, n, ss, q) -> int:
    m = out["meta"][u]
    st = int(m["status"])
    if st in REFERENCE_EXCEPTIONS:
        escaped = True
    elif st != 0:
        escaped = False
    elif int(m["kind"]) == FW.KIND_LPC and (q - 1) & 15 == 15:
        escaped = True
    else:
        bits = subframe_bits(samples, out, u, n, ss, q)
        escaped = bits > 8 + n * ss
        x = np.asarray(samples[:n])
        if not escaped and bits > 8 + ss and (x == x[0]).all():
            return CONSTANT
    if not escaped:
        return ANALYSED
    x = np.asarray(samples[:n])
    return CONSTANT if (x == x[0]).all() else VERBATIM


def raw_subframe(bits: FW.Bits, samples, n, ss, kind):
    """CONSTANT: 0 000000 0 and the value; VERBATIM: 0 000001 0 and every sample (ss bits each,
    two's complement truncated by Bits.put)."""
    bits.put(0 if kind == CONSTANT else 2, 8)
    for s in samples[: 1 if kind == CONSTANT else n]:
        bits.put(int(s), ss)


def frames(rows, out, C, block_len, tail_len, ss, q, first_frame=0, fallback=True):
    """-> (frames: bytes, or the exception instance of a frame that still fails; sub-kind per unit).
    fallback=False: frame_writer.frames_from_analysis."""
    nf = rows.shape[0] // C
    result, kinds = [], []
    for f in range(nf):
        n = tail_len if (f == nf - 1 and tail_len) else block_len
        bits = FW.Bits()
        try:
            for b in FW.frame_header(first_frame + f, n):
                bits.put(b, 8)
            err = None
        except ValueError as e:
            err = e
        for u in range(f * C, (f + 1) * C):
            kind = sub_kind(rows[u], out, u, n, ss, q) if fallback else ANALYSED
            kinds.append(kind)
            if err is not None:
                continue
            if kind != ANALYSED:
                raw_subframe(bits, rows[u], n, ss, kind)
                continue
            m, zz, prm = _unit(out, u)
            st = int(m["status"])
            try:
                if st != 0:
                    raise FW._EXC.get(st, RuntimeError)()
                FW.subframe(bits, rows[u], m, zz, prm, n, ss, q)
            except (ValueError, AssertionError, ZeroDivisionError, OverflowError, RuntimeError) as e:
                err = e
        if err is not None:
            result.append(err)
            continue
        bits.put(0, (8 - bits.n % 8) % 8)
        body = bits.to_bytes()
        result.append(body + FW.crc16(body).to_bytes(2, "big"))
    return result, kinds
