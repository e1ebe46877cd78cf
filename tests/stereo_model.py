"""CPU model of the stereo-decorrelation mode (FLACMI_STEREO_BEST, include/flacmi.h) over
oracle.analyze_batch results: the four candidate signals of every frame, their sizes, the
choice among L_R, L_S, S_R and M_S, and the frames it gives, built from the fallback model's
pieces (fallback_model.subframe_bits / sub_kind / raw_subframe) and the oracle frame writer's
(oracle/frame_writer.py).  TEST INFRASTRUCTURE ONLY.

Candidate k of frame f (0 left, 1 right, 2 mid, 3 side) is analysed as a unit of its own: the
caller's rows as they are, the mid rows in the caller's element type, the side rows as int32
at sample_bits = ss + 1 (the analysis never looks at the width; it only bounds the arithmetic).
"""
import numpy as np

import fallback_model as FM
import frame_writer as FW
import oracle
import stereo_cases as SC


def candidate_rows(rows, block_len, tail_len):
    """rows [2 F][n] -> (mid rows [F][n] in rows' dtype, side rows [F][n] int32), zero behind a
    short last frame."""
    nf = rows.shape[0] // 2
    mid = np.zeros((nf, rows.shape[1]), dtype=rows.dtype)
    side = np.zeros((nf, rows.shape[1]), dtype=np.int32)
    for f in range(nf):
        n = tail_len if (f == nf - 1 and tail_len) else block_len
        _, _, m, s = SC.candidates(rows[2 * f, :n], rows[2 * f + 1, :n])
        mid[f, :n], side[f, :n] = m, s
    return mid, side


def analyse(rows, params, block_len, tail_len, ss, threads=4):
    """The three analyses -> per frame the four candidates as (samples row, oracle result, unit
    index in it, width)."""
    nf = rows.shape[0] // 2
    mid, side = candidate_rows(rows, block_len, tail_len)
    tail = 1 if tail_len else 0
    o_lr = oracle.analyze_batch(rows, params, block_len, tail_len, 2 * tail, sample_bits=ss, threads=threads)
    o_m = oracle.analyze_batch(mid, params, block_len, tail_len, tail, sample_bits=ss, threads=threads)
    o_s = oracle.analyze_batch(side, params, block_len, tail_len, tail, sample_bits=ss + 1, threads=threads)
    return [[(rows[2 * f], o_lr, 2 * f, ss), (rows[2 * f + 1], o_lr, 2 * f + 1, ss), (mid[f], o_m, f, ss),
             (side[f], o_s, f, ss + 1)] for f in range(nf)]


def candidate(cand, n, q, fallback):
    """-> (sub-kind, size in bits or None when the candidate is not eligible, status)."""
    samples, out, u, w = cand
    m = out["meta"][u]
    st = int(m["status"])
    kind = FM.sub_kind(samples, out, u, n, w, q) if fallback else FM.ANALYSED
    if kind != FM.ANALYSED:
        return kind, 8 + (1 if kind == FM.CONSTANT else n) * w, st
    if st != 0 or (int(m["kind"]) == FW.KIND_LPC and (q - 1) & 15 == 15):
        return kind, None, st
    return kind, FM.subframe_bits(samples, out, u, n, w, q), st


def frame_header(index, n, code):
    """frame_writer.frame_header with the channel assignment code in byte 3."""
    h = bytearray(FW.frame_header(index, n))
    h[3] = code << 4
    h[-1] = FW.crc8(bytes(h[:-1]))
    return bytes(h)


def frames(rows, cands, block_len, tail_len, q, first_frame=0, fallback=False):
    """-> (frames: bytes, or the exception instance of a frame that fails; channel code per frame,
    None for a failing frame; per frame the four candidates' (sub-kind, size))."""
    result, codes, sizes = [], [], []
    for f, cand in enumerate(cands):
        n = tail_len if (f == len(cands) - 1 and tail_len) else block_len
        info = [candidate(c, n, q, fallback) for c in cand]
        sizes.append([(k, b) for k, b, _ in info])
        wide = [st for _, _, st in info if st == 16]  # FLACMI_STATUS_RESIDUAL_WIDE fails the frame
        pick = None if wide else SC.choose([b for _, b, _ in info])
        if pick is None:
            # the status word the L_R frame has without the mode: the first failing channel
            codes.append(None)
            st = next((st for _, b, st in info[:2] if b is None and st), 0)
            result.append(RuntimeError("residual wide") if wide else FW._EXC.get(st, AssertionError)())
            continue
        code, a, b = pick
        codes.append(code)
        bits = FW.Bits()
        for byte in frame_header(first_frame + f, n, code):
            bits.put(byte, 8)
        for k in (a, b):
            samples, out, u, w = cand[k]
            if info[k][0] != FM.ANALYSED:
                FM.raw_subframe(bits, samples, n, w, info[k][0])
            else:
                m, zz, prm = FM._unit(out, u)
                FW.subframe(bits, samples, m, zz, prm, n, w, q)
        bits.put(0, (8 - bits.n % 8) % 8)
        body = bits.to_bytes()
        result.append(body + FW.crc16(body).to_bytes(2, "big"))
    return result, codes, sizes
