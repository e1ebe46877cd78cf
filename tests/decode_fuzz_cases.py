"""Seeded grammar fuzz of FLAC frames for the device frame parsers (k_decode_fx, k_decode,
k_frame_info): frames no encoder of this project writes, with the features combined.

    frames(seed=SEED) -> [Case(name, data, channels, sample_size, truth)]

Valid frames (truth is a dict) are constructive: samples are chosen inside the subframe's width,
the coefficients are integers, the residual is computed with unbounded integers, and a signal
whose residual or prediction leaves int32 is redrawn (the domain the kernels document: an int32
history, values modulo 2^32).  truth records what was written: the header fields, the padding
bits, and per subframe type, order, wasted bits, width read, precision, shift, coefficients,
coding method, partition order, the partitions as ("rice", k) / ("escape", w), the residual's
abs_sum, the constant value, bit offset and bit length.

Mutated frames (truth None, names m###_...) are valid frames with 1 to 3 bits flipped behind the
header's first two bytes, CRC-8 and CRC-16 recomputed so that the parse decides and not the
checksums; cut frames (c###_...) end at a random byte.

All randomness comes from random.Random(seed).getrandbits, and tests/golden/decode_fuzz.json pins
every frame's sha256, so a drift of the generator fails loudly.
"""
import functools
import random
from collections import namedtuple

from frame_assembler import FIXED, Bits, crc8, crc16, header, residual_bits, sub_head

SEED = 20261020
Case = namedtuple("Case", "name data channels sample_size truth")

BLOCK_SIZES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 192, 255, 256, 257, 576, 1000, 1152, 4096)
TABLE_CODE = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
              16384: 14}
LPC_ORDERS = (1, 2, 11, 12, 13, 31, 32)
LPC_PRECISIONS = (1, 2, 5, 12, 15)
LPC_SHIFTS = (0, 1, 14, 15)
ESCAPE_WIDTHS = (1, 2, 16, 31)
TYPES = ("CONSTANT", "VERBATIM", "FIXED0", "FIXED1", "FIXED2", "FIXED3", "FIXED4") + tuple(f"LPC{o}" for o in LPC_ORDERS)
# (sample size, header code): code 0 defers to the sample_size argument
SAMPLE_SIZES = ((8, 1), (12, 2), (16, 4), (20, 5), (24, 6), (32, 7), (8, 0), (12, 0), (16, 0), (20, 0), (24, 0), (32, 0),
                (4, 0), (17, 0), (16, 4), (16, 0))
SAMPLE_RATE = {0: 0, 1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100,
               10: 48000, 11: 96000}
N_VALID_GRID = 384
N_MUTATED = 200
N_CUT = 20
MAX_RUN = 120   # zeros of the longest unary run a valid frame holds (three dwords and a bit)
I32 = (-(1 << 31), (1 << 31) - 1)


class Rng:
    """random.Random(seed).getrandbits and nothing else."""

    def __init__(self, seed):
        self.bits = random.Random(seed).getrandbits

    def below(self, n):
        return self.bits(48) % n

    def span(self, lo, hi):
        return lo + self.below(hi - lo + 1)

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def chance(self, num, den):
        return self.below(den) < num

    def shuffle(self, seq):
        for i in range(len(seq) - 1, 0, -1):
            j = self.below(i + 1)
            seq[i], seq[j] = seq[j], seq[i]


def _zz(v):
    return 2 * v if v >= 0 else -2 * v - 1


def _sbits(v):
    """Width of v as a two's complement number."""
    return (v if v >= 0 else ~v).bit_length() + 1


def _signal(rng, n, order, coefs, shift, width, plan_for, extremes):
    """x[n] inside `width` bits and its residual r[n - order], drawn sample by sample: the target
    residual follows the partition's plan, the sample is the prediction plus it, held inside the
    amplitude at which no prediction can leave int32.  None: the draw left int32 (redraw)."""
    gain = sum(abs(c) for c in coefs)
    amp = width - 1
    while amp > 0 and ((gain << amp) >> shift) + (1 << amp) > (1 << 30):
        amp -= 1
    lo, hi = -(1 << amp), (1 << amp) - 1
    x = [rng.span(lo, hi) if rng.chance(1, 2) else rng.span(-min(4, -lo), min(3, hi)) for _ in range(order)]
    if extremes and order:
        x[rng.below(order)] = rng.pick((lo, hi))
    r = []
    for i in range(order, n):
        pred = sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift
        kind, k = plan_for(i - order)
        if kind == "escape":
            t = rng.span(-(1 << (k - 1)), (1 << (k - 1)) - 1)
            if rng.chance(1, 8):
                t = rng.pick((-(1 << (k - 1)), (1 << (k - 1)) - 1))
        else:
            t = rng.span(-(1 << k), (1 << k)) if k < 31 else 0
            if rng.chance(1, 40):  # a unary run across one, two or three dwords
                t = (rng.pick((33, 40, 64, 70, 97, MAX_RUN - 1)) << k) >> 1
                t = -t if rng.chance(1, 2) else t
        v = pred + t
        if extremes and rng.chance(1, 24):
            v = rng.pick((lo, hi))
        v = max(lo, min(hi, v))
        if not (I32[0] <= pred <= I32[1] and I32[0] <= v - pred <= I32[1]):
            return None
        x.append(v)
        r.append(v - pred)
    return x, r


def _subframe(rng, b, spec, bs, width):
    """Write one subframe; returns (its samples before recombination, truth record)."""
    sub0 = b.n
    kind, wasted, flag = spec["type"], spec["wasted"], spec["flag"]
    w = width - wasted
    rec = {"type": kind.rstrip("0123456789"), "order": 0, "wasted_bits": wasted, "sample_bits": w, "precision": 0, "shift": 0,
           "coefficients": [], "coding_method": 0, "partition_order": 0, "partitions": [], "residual_bits": 0,
           "abs_sum": 0, "constant": 0, "bit_offset": sub0,
           # beyond the device's report, for the coverage assertions: whether the wasted-bits flag
           # is set, and the longest unary run of the subframe's Rice codes
           "wasted_flag": int(bool(wasted or flag)), "max_unary": 0}
    ws = w if w > 0 else 8  # FIXED order 0 reads no sample at the width: any width <= 0 parses
    lo, hi = -(1 << (ws - 1)), (1 << (ws - 1)) - 1
    if kind == "CONSTANT":
        v = rng.pick((lo, hi, rng.span(lo, hi), rng.span(lo, hi)))
        sub_head(b, 0, wasted, flag)
        b.s(v, w)
        rec["constant"] = v
        x = [v] * bs
    elif kind == "VERBATIM":
        x = [rng.pick((lo, hi)) if rng.chance(1, 16) else rng.span(lo, hi) for _ in range(bs)]
        if spec.get("plant") and bs >= 16:  # a false sync: a whole valid header inside the payload
            fake = header(1, 192, sr_code=9, ch_code=0, ss_code=4, fno=5)
            assert w == 16 and len(fake) % 2 == 0
            at = 3
            for k in range(len(fake) // 2):
                v = int.from_bytes(fake[2 * k:2 * k + 2], "big")
                x[at + k] = v - ((v >> 15) << 16)
        if spec.get("ends"):  # both ends of the width, and an odd value
            x[0], x[1], x[2] = lo, hi, x[2] | 1
        sub_head(b, 1, wasted, flag)
        for v in x:
            b.s(v, w)
    else:
        lpc = kind.startswith("LPC")
        order = rec["order"] = int(kind[3:] if lpc else kind[5:])
        assert order < bs or (order == 0 and not lpc)
        if lpc:
            prec, shift = spec["precision"], spec["shift"]
            cl, ch = -(1 << (prec - 1)), (1 << (prec - 1)) - 1
            style = spec["coef_style"]
            coefs = [rng.pick((cl, ch)) if style == 0 or (style == 1 and rng.chance(1, 4)) else rng.span(cl, ch)
                     for _ in range(order)]
            if style == 2:  # a tame predictor: the fixed predictor's taps scaled to the shift
                base = FIXED[min(order, 2)] + (0,) * max(0, order - 2)
                coefs = [max(cl, min(ch, (c << shift) + rng.span(-1, 1))) for c in base]
        else:
            prec, shift, coefs = 0, 0, list(FIXED[order])
        po, method = spec["partition_order"], spec["method"]
        assert bs % (1 << po) == 0 and (bs >> po) > order
        plen, pmax = bs >> po, (30 if method else 14)
        plan = [spec["plan"](p) for p in range(1 << po)]
        plan = [(kd, min(k, pmax) if kd == "rice" else k) for kd, k in plan]

        def plan_for(j):
            return plan[(j + order) // plen]
        for _ in range(64):
            got = _signal(rng, bs, order, coefs, shift, ws, plan_for, spec["extremes"])
            if got is None:
                continue
            x, r = got
            # hold the plan where the residual allows it; otherwise the next parameter that does
            final, i, ok = [], 0, True
            for p, (kd, k) in enumerate(plan):
                n = plen - order if p == 0 else plen
                part = r[i:i + n]
                i += n
                need = max(_sbits(v) for v in part)
                if kd == "escape":
                    ok = ok and max(k, need) <= 31
                    final.append(("escape", max(k, need)))
                else:
                    top = max(_zz(v) for v in part)
                    while (top >> k) > MAX_RUN and k < pmax:
                        k += 1
                    if (top >> k) > MAX_RUN:
                        ok = ok and need <= 31
                        final.append(("escape", need))
                    else:
                        final.append(("rice", k))
            if ok:
                break
        else:
            raise AssertionError(f"no signal for {spec}")
        sub_head(b, (32 | (order - 1)) if lpc else (8 | order), wasted, flag)
        for v in x[:order]:
            b.s(v, w)
        if lpc:
            b.u(prec - 1, 4)
            b.s(shift, 5)
            for c in coefs:
                b.s(c, prec)
            rec.update(precision=prec, shift=shift, coefficients=coefs)
        r0 = b.n
        esc = {p: k for p, (kd, k) in enumerate(final) if kd == "escape"}
        written = residual_bits(b, r, bs, order, po, [k for _, k in final], method, esc, exact=True)
        assert written == final
        rec.update(coding_method=5 if method else 4, partition_order=po, partitions=final, residual_bits=b.n - r0,
                   abs_sum=sum(abs(v) for v in r))
        i = 0
        for p, (kd, k) in enumerate(final):
            n = plen - order if p == 0 else plen
            if kd == "rice":
                rec["max_unary"] = max([rec["max_unary"]] + [_zz(v) >> k for v in r[i:i + n]])
            i += n
    rec["bits"] = b.n - sub0
    return x, rec


def _number(rng, nbytes):
    """A coded number that takes exactly nbytes (1..7)."""
    top = (7, 11, 16, 21, 26, 31, 36)[nbytes - 1]
    low = 0 if nbytes == 1 else (7, 11, 16, 21, 26, 31)[nbytes - 2]
    return rng.pick(((1 << top) - 1, 1 << low if nbytes > 1 else 0, rng.span(1 << low if nbytes > 1 else 0, (1 << top) - 1)))


def build_frame(rng, spec):
    """spec -> (bytes, truth).  spec holds the header choices and one dict per subframe."""
    bs, ss, ss_code, ch_code = spec["block_size"], spec["ss"], spec["ss_code"], spec["ch_code"]
    form = spec["bs_form"]
    bs_code = TABLE_CODE[bs] if form == "table" else 6 if form == "u8" else 7
    sr_code = spec["sr_code"]
    sr_extra = {12: rng.span(1, 255), 13: rng.span(256, 65535), 14: rng.span(1, 65535)}.get(sr_code)
    hdr = header(bs_code, bs, sr_code=sr_code, ch_code=ch_code, ss_code=ss_code, fno=spec["number"], sr_extra=sr_extra,
                 strategy=spec["strategy"])
    b = Bits()
    for byte in hdr:
        b.u(byte, 8)
    subs, recs = [], []
    for c, sub in enumerate(spec["subframes"]):
        side = (ch_code == 8 and c == 1) or (ch_code == 9 and c == 0) or (ch_code == 10 and c == 1)
        x, rec = _subframe(rng, b, sub, bs, ss + int(side))
        subs.append(x)
        recs.append(rec)
    padding = -b.n % 8
    b.pad()
    d = b.data()
    data = d + crc16(d).to_bytes(2, "big")
    if ch_code == 8:
        samples = [subs[0], [p - q for p, q in zip(subs[0], subs[1])]]
    elif ch_code == 9:
        samples = [[p + q for p, q in zip(subs[0], subs[1])], subs[1]]
    elif ch_code == 10:
        right = [m - (s >> 1) for m, s in zip(subs[0], subs[1])]
        samples = [[q + s for q, s in zip(right, subs[1])], right]
    else:
        samples = subs
    truth = {"offset": 0, "end": len(data), "number": spec["number"], "block_size": bs,
             "blocking_strategy": spec["strategy"], "rate_code": sr_code,
             "sample_rate": sr_extra * (10 if sr_code == 14 else 1) if sr_extra else SAMPLE_RATE[sr_code],
             "sample_size": ss if ss_code else 0, "channel_code": ch_code, "n_subframes": len(recs),
             "header_bytes": len(hdr), "crc8": hdr[-1], "crc8_computed": hdr[-1], "crc16": crc16(d),
             "crc16_computed": crc16(d), "padding_bits": padding, "subframes": recs, "bs_form": form,
             "samples": samples, "subframe_samples": subs}
    return data, truth


def _wasted_choice(k, width):
    """(zeros, flag): no flag, or a set flag and 0, 1, 5 or ss - 2 zeros (what get_wasted_bits
    returns), kept below the width."""
    if k < 3:
        return 0, None
    z = (0, 1, 5, width - 2)[k - 3]
    return max(0, min(z, width - 2)), 1


def _plan(rng, i, c, method, po):
    """Partition plan: the Rice parameters walk their whole range over the frames; escapes sit
    first, last, between Rice partitions, or anywhere."""
    nparts, pmax = 1 << po, (31 if method else 15)
    base = (i * 3 + c * 7) % pmax
    where = (i + c) % 6
    esc = set()
    if where == 1:
        esc = {0}
    elif where == 2:
        esc = {nparts - 1}
    elif where == 3 and nparts >= 3:
        esc = {1 + rng.below(nparts - 2)}
    elif where == 4:
        esc = {p for p in range(nparts) if rng.chance(1, 5)}
    widths = {p: ESCAPE_WIDTHS[(i + p) % 4] for p in esc}
    step = rng.below(3)

    def plan(p):
        if p in widths:
            return "escape", widths[p]
        return "rice", (base + p * step) % pmax
    return plan


def _sub_spec(rng, i, c, bs, width, kind=None):
    kind = kind or TYPES[(i * 3 + c * 5 + i // 14) % len(TYPES)]
    if kind.startswith("LPC"):
        order = int(kind[3:])
        if order >= bs:  # the largest order the block allows: bs - 1
            order = bs - 1
        kind = f"LPC{order}" if order else "VERBATIM"
    elif kind.startswith("FIXED"):
        kind = f"FIXED{min(int(kind[5:]), bs - 1)}"
    order = int(kind.lstrip("LPCFIXED")) if kind[0] in "LF" else 0
    zeros, flag = _wasted_choice((i + 2 * c + i // 7) % 7, width)
    spec = {"type": kind, "wasted": zeros, "flag": flag, "extremes": (i + c) % 3 == 0}
    if kind[0] in "LF":
        orders = [po for po in range(16) if bs % (1 << po) == 0 and (bs >> po) > order]
        # the finest split the block allows every other time (partitions of 1, 2, 3 samples)
        spec["partition_order"] = orders[-1] if (i + c) % 2 == 0 else rng.pick(orders)
        spec["method"] = (i + c) % 2 if width - zeros <= 16 else (i + c + 1) % 2
        spec["plan"] = _plan(rng, i, c, spec["method"], spec["partition_order"])
    if kind.startswith("LPC"):
        spec["precision"] = LPC_PRECISIONS[(i + c) % 5] if i % 3 else rng.span(1, 15)
        spec["shift"] = LPC_SHIFTS[(i // 5 + c) % 4] if i % 4 else rng.span(0, 15)
        spec["coef_style"] = (i + c) % 3
    return spec


def _valid(seed):
    rng = Rng(seed)
    out = []

    def add(name, spec, channels, arg):
        data, truth = build_frame(rng, spec)
        out.append(Case(name, data, channels, arg, truth))

    for i in range(N_VALID_GRID):
        bs = BLOCK_SIZES[i % len(BLOCK_SIZES)]
        rnd = i // len(BLOCK_SIZES)
        forms = (["table"] if bs in TABLE_CODE else []) + (["u8"] if bs <= 256 else []) + ["u16"]
        ss, ss_code = SAMPLE_SIZES[(i * 5 + rnd) % len(SAMPLE_SIZES)]
        ch_code = (i * 7 + rnd) % 11
        if bs > 300 and 2 <= ch_code <= 7:
            ch_code %= 2
        if ch_code >= 8 and ss == 32:  # a 33-bit side channel: the pinned frame below only
            ss, ss_code = 24, 6
        channels = ch_code + 1 if ch_code <= 7 else 2
        sr_code = (i * 3 + rnd) % 15
        if sr_code == 11:  # the reference's table has no entry (KeyError): the pinned frame below only
            sr_code = 10
        spec = {"block_size": bs, "bs_form": forms[rnd % len(forms)], "ss": ss, "ss_code": ss_code, "ch_code": ch_code,
                "sr_code": sr_code, "number": _number(rng, 1 + i % 6), "strategy": 0,
                "subframes": [_sub_spec(rng, i, c, bs, ss + int((ch_code in (8, 10) and c == 1) or (ch_code == 9 and c == 0)))
                              for c in range(channels)]}
        add(f"v{i:03d}_bs{bs}_ch{ch_code}_ss{ss}", spec, channels, ss if not ss_code else 16)

    def one(name, bs, form, ss, ss_code, ch_code, subs, sr_code=9, number=0, strategy=0, arg=None):
        channels = len(subs)
        add(name, {"block_size": bs, "bs_form": form, "ss": ss, "ss_code": ss_code, "ch_code": ch_code, "sr_code": sr_code,
                   "number": number, "strategy": strategy, "subframes": subs}, channels, arg or (ss if not ss_code else 16))

    def fixed(order, po, method, plan, wasted=0, flag=None, extremes=True):
        return {"type": f"FIXED{order}", "wasted": wasted, "flag": flag, "extremes": extremes, "partition_order": po,
                "method": method, "plan": plan}

    # every partition order each block size allows, one per channel, the FIXED order as high as
    # the partition length lets it be
    for bs in BLOCK_SIZES:
        orders = [po for po in range(16) if bs % (1 << po) == 0]
        for k in range(0, len(orders), 8):
            subs = [fixed(min((po + bs) % 5, (bs >> po) - 1), po, (po + k) % 2, _plan(rng, bs + po, po, (po + k) % 2, po))
                    for po in orders[k:k + 8]]
            one(f"po_sweep_bs{bs}_{k // 8}", bs, "u16", 16, 4, len(subs) - 1, subs)
    # the largest block, CONSTANT and FIXED (16-bit explicit size), alone at their sample size
    one("big_constant_65535", 65535, "u16", 17, 0, 0, [{"type": "CONSTANT", "wasted": 0, "flag": None}])
    one("big_fixed_65535", 65535, "u16", 17, 0, 0, [fixed(2, 0, 0, lambda p: ("rice", 3))])
    # 256 samples under both of its header forms, 4096 at partition order 12, 16 at order 4
    one("bs256_code8", 256, "table", 16, 4, 0, [fixed(0, 8, 0, lambda p: ("rice", p % 15))])
    one("bs256_u8", 256, "u8", 16, 4, 0, [fixed(1, 7, 1, lambda p: ("rice", p % 31))])
    one("bs4096_po12", 4096, "table", 16, 4, 0, [fixed(0, 12, 0, lambda p: ("escape", 1 + p % 31) if p % 5 == 0 else ("rice", p % 15))])
    one("bs16_po4", 16, "u8", 16, 4, 1, [fixed(0, 4, 1, lambda p: ("rice", 2 * p)), fixed(0, 4, 0, lambda p: ("escape", ESCAPE_WIDTHS[p % 4]))])
    # a 36-bit sample number (7 bytes) under the variable blocking strategy
    one("sample_number_7_bytes", 192, "table", 16, 4, 0, [fixed(2, 2, 0, lambda p: ("rice", 4 + p))], number=(1 << 36) - 192 - 5,
        strategy=1)
    # sample-rate code 11: the device reads 96 kHz, the reference's table lacks the entry
    one("sample_rate_code_11", 64, "u8", 16, 4, 0, [fixed(1, 1, 0, lambda p: ("rice", 2))], sr_code=11)
    # a FIXED order-0 subframe whose zero count reaches the sample size: no sample is read at
    # the (non-positive) width, so the reference decodes the frame
    one("fixed0_wasted_ge_ss", 32, "u8", 4, 0, 0, [fixed(0, 2, 0, lambda p: ("rice", 1), wasted=5, flag=1, extremes=False)])
    # a false sync: a whole header with a good CRC-8 inside a VERBATIM payload
    one("verbatim_false_sync", 64, "u8", 16, 0, 0, [{"type": "VERBATIM", "wasted": 0, "flag": None, "plant": True}])
    # side channels at both ends of ss + 1 bits, M_S with odd sides (VERBATIM: every value reachable)
    for code, nm in ((8, "L_S"), (9, "S_R"), (10, "M_S")):
        one(f"stereo_ends_{nm}", 33, "u8", 16, 4, code, [{"type": "VERBATIM", "wasted": 0, "flag": None, "ends": True} for _ in range(2)])
    return out


def _wide_side_frame():
    """L_S at ss = 32: the side channel is read at 33 bits and its samples leave int32, in an LPC
    subframe with a shift.  Left is a ramp near the top, right near the bottom; the reference
    restores both exactly.  The coefficients sum to 1, so a history kept modulo 2^32 moves every
    prediction by 2^32 >> 1 = 2^31: a decoder with an int32 history that went on would return
    other samples under an intact CRC-16."""
    bs = 16
    left = [(1 << 31) - 1 - 3 * i for i in range(bs)]
    right = [-(1 << 31) + 5 * i for i in range(bs)]
    side = [p - q for p, q in zip(left, right)]
    coefs, shift = [3, -2], 1
    b = Bits()
    hdr = header(6, bs, sr_code=9, ch_code=8, ss_code=7, fno=9)
    for byte in hdr:
        b.u(byte, 8)
    sub_head(b, 1)
    for v in left:
        b.s(v, 32)
    sub_head(b, 32 | 1)
    for v in side[:2]:
        b.s(v, 33)
    b.u(4, 4)
    b.s(shift, 5)
    for c in coefs:
        b.s(c, 5)
    r = [side[i] - ((coefs[0] * side[i - 1] + coefs[1] * side[i - 2]) >> shift) for i in range(2, bs)]
    residual_bits(b, r, bs, 2, 0, [30], 1, exact=True)  # residuals near 2^31: four zeros at parameter 30
    b.pad()
    d = b.data()
    return Case("pinned_L_S_ss32_side33", d + crc16(d).to_bytes(2, "big"), 2, 32, {"samples": [left, right], "wide_side": True})


def _refresh_crcs(data):
    """CRC-8 and CRC-16 recomputed where the frame still has them: the header's length comes
    from the bytes as they now are, the footer is the last two bytes."""
    d = bytearray(data)
    b0 = d[4] if len(d) > 4 else 0
    n = 4 + (6 if b0 >= 0xFE else 5 if b0 >= 0xFC else 4 if b0 >= 0xF8 else 3 if b0 >= 0xF0 else 2 if b0 >= 0xE0
             else 1 if b0 >= 0xC0 else 0)
    if len(d) > 3:
        n += {6: 1, 7: 2}.get(d[2] >> 4, 0) + {12: 1, 13: 2, 14: 2}.get(d[2] & 15, 0)
    if n < len(d) - 2:
        d[n] = crc8(d[:n])
    if len(d) > 2:
        d[-2:] = crc16(d[:-2]).to_bytes(2, "big")
    return bytes(d)


@functools.lru_cache(maxsize=2)
def frames(seed=SEED):
    """Every frame of the fuzz, in a fixed order: valid, pinned, mutated, cut."""
    valid = _valid(seed)
    out = valid + [_wide_side_frame()]
    rng = Rng(seed + 1)
    small = [c for c in valid if len(c.data) <= 600 and c.name[0] == "v"]  # sources: the grid's small frames
    for m in range(N_MUTATED):
        src = small[rng.below(len(small))]
        while True:
            d = bytearray(src.data)
            # every other frame takes its flips in the first bytes, where the structure is
            span = 8 * (min(len(d), 24) if m % 2 else len(d)) - 16
            for _ in range(1 + rng.below(3)):
                bit = 16 + rng.below(span)
                d[bit // 8] ^= 0x80 >> (bit % 8)
            if d[2] & 15 != 11:  # sample-rate code 11: KeyError in the reference, see above
                break
        out.append(Case(f"m{m:03d}_{src.name.split('_')[0]}", _refresh_crcs(bytes(d)), src.channels,
                        src.sample_size, None))
    for m in range(N_CUT):
        src = small[rng.below(len(small))]
        out.append(Case(f"c{m:03d}_{src.name.split('_')[0]}", src.data[:1 + rng.below(len(src.data) - 1)], src.channels, src.sample_size, None))
    return out
