"""A plain-Python model of the device frame parsers (csrc/k_decode.hip, csrc/k_info.hip) with
unbounded integers, written from the statement catalogue of include/flacmi.h
(flacmi_decode_site) and the FLAC frame layout.  It decodes one frame of a byte string the way
the kernels are specified to: the statements in their order, the first failing statement
decides, a read past the last byte is EOFError, a negative LPC shift is raised only after the
whole frame has parsed, get_wasted_bits yields the count of zeros, wasted bits are not shifted
back in, and an L_R frame holds `channels` subframes.  With spec_wasted_bits=True
(FLACMI_DECODE_WASTED_SPEC) the wasted count is the count of zeros plus one, as the format codes
it, and every sample of the subframe is shifted back by it.

    decode(data, channels, sample_size, offset=0) -> Decoded | Failed

tests/test_decode_fuzz_model.py ties this model to the reference decoder's recorded verdicts
(tests/golden/decode_fuzz.json); the GPU tests then take their expectations from it.
"""
from collections import namedtuple

INT32 = (-(1 << 31), (1 << 31) - 1)
MAX_UNARY = 1 << 20
FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))
SAMPLE_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100,
                10: 48000, 11: 96000}
SAMPLE_SIZES = {0: 0, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
TYPE_NAMES = ("CONSTANT", "VERBATIM", "FIXED", "LPC")

# samples: per channel after recombination; subframes: per subframe before it; end: the byte
# offset behind the CRC-16; report: the frame record in the shape of flacmi_frame_info, its
# "subframes" in the shape of flacmi_subframe_info
Decoded = namedtuple("Decoded", "samples subframes end report")
# exception: the class the reference raises; site: the flacmi_decode_site name; end: None, or
# for neg_shift (raised after the parse) the frame's end; report: what was parsed before
Failed = namedtuple("Failed", "exception site end report")


class OutOfDomain(Exception):
    """The frame leaves what the kernels document: it parses to its end with a subframe sample
    outside int32 (their history is int32, values modulo 2^32), or holds a unary run of more
    than 2^20 zeros."""


class _Stop(Exception):
    def __init__(self, exception, site):
        self.exception, self.site = exception, site


class _Reader:
    def __init__(self, data, pos):
        self.d, self.p, self.end = data, pos, 8 * len(data)

    def uint(self, n):
        if n == 0:
            return 0
        if n < 0:  # the reference's reader computes a mask of negative width (after fetching a byte when aligned)
            if self.p % 8 == 0 and self.p + 8 > self.end:
                raise _Stop(EOFError, "eof")
            raise _Stop(ValueError, "escape_zero")
        if self.p + n > self.end:
            raise _Stop(EOFError, "eof")
        lo, hi = self.p // 8, (self.p + n + 7) // 8
        v = int.from_bytes(self.d[lo:hi], "big")
        v = (v >> (8 * hi - self.p - n)) & ((1 << n) - 1)
        self.p += n
        return v

    def sint(self, n):
        x = self.uint(n)
        if n == 0:  # x >> (n - 1): negative shift count
            raise _Stop(ValueError, "escape_zero")
        return x - ((x >> (n - 1)) << n)

    def unary(self):
        """Zeros up to a one."""
        n = 0
        while True:
            if self.p >= self.end:
                raise _Stop(EOFError, "eof")
            # whole zero bytes at a time
            if self.p % 8 == 0 and self.d[self.p // 8] == 0:
                n += 8
                self.p += 8
            else:
                self.p += 1
                if (self.d[(self.p - 1) // 8] >> (7 - (self.p - 1) % 8)) & 1:
                    return n
                n += 1
            if n > MAX_UNARY:
                raise OutOfDomain("unary run")


def _crc8(bs):
    c = 0
    for b in bs:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def _crc16(bs):
    c = 0
    for b in bs:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def _check(x, domain):
    """domain: None, or a list that collects the samples outside int32.  The parse never looks at
    a restored sample, so a frame that fails has its verdict whatever the samples were: only a
    frame that parses to its end is out of the domain (decode raises then)."""
    if domain is not None and not INT32[0] <= x <= INT32[1]:
        domain.append(x)
    return x


def _subframe(g, bs, width, frame_bit0, domain, spec=False):
    """One subframe: (samples, record, negative_shift)."""
    sub0 = g.p
    if g.uint(1) != 0:
        raise _Stop(AssertionError, "subframe_pad")
    t = g.uint(6)
    if not (t <= 1 or 8 <= t <= 12 or t >= 32):
        raise _Stop(AssertionError, "subframe_type")
    wasted = g.unary() + int(spec) if g.uint(1) else 0
    w = width - wasted
    order = (t & 31) + 1 if t >= 32 else (t & 7) if t >= 8 else 0
    rec = {"bit_offset": sub0 - frame_bit0, "type": TYPE_NAMES[0 if t == 0 else 1 if t == 1 else 2 if t < 32 else 3],
           "order": order, "wasted_bits": wasted, "sample_bits": w, "precision": 0, "shift": 0, "coefficients": [],
           "coding_method": 0, "partition_order": 0, "partitions": [], "residual_bits": 0, "abs_sum": 0, "constant": 0}
    neg = False
    if t == 0:
        rec["constant"] = g.sint(w)
        x = [_check(rec["constant"], domain)] * bs
    elif t == 1:
        x = [_check(g.sint(w), domain) for _ in range(bs)]
    else:
        x = [_check(g.sint(w), domain) for _ in range(order)]
        coefs, shift = FIXED[order] if t < 32 else None, 0
        if t >= 32:
            pf = g.uint(4)
            if pf == 15:
                raise _Stop(AssertionError, "lpc_precision")
            rec["precision"] = pf + 1
            shift = rec["shift"] = g.sint(5)
            coefs = rec["coefficients"] = [g.sint(pf + 1) for _ in range(order)]
        r0 = g.p
        cm = g.uint(2)
        if cm > 1:
            raise _Stop(ValueError, "coding_method")
        pbits = rec["coding_method"] = 5 if cm else 4
        po = rec["partition_order"] = g.uint(4)
        if bs % (1 << po) != 0 or (bs >> po) <= order:
            raise _Stop(AssertionError, "partitions")
        if shift < 0:  # `>> shift` raises when the samples are restored, after the frame has parsed
            neg, shift = True, 0
        plen = bs >> po
        for p in range(1 << po):
            n = plen - order if p == 0 else plen
            k = g.uint(pbits)
            if k == (1 << pbits) - 1:
                k = g.uint(5)
                rec["partitions"].append(("escape", k))
                read = lambda: g.sint(k)  # noqa: E731
            else:
                rec["partitions"].append(("rice", k))

                def read():
                    z = (g.unary() << k) | g.uint(k)
                    return (z >> 1) ^ -(z & 1)
            for _ in range(n):
                r = read()
                rec["abs_sum"] += abs(r)
                i = len(x)
                # (a frame that fails with neg_shift has no samples: nothing to hold in int32)
                x.append(_check(r + (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift), None if neg else domain))
        rec["residual_bits"] = g.p - r0
    rec["bits"] = g.p - sub0
    if spec and wasted:
        x = [_check(v << wasted, None if neg else domain) for v in x]
    return x, rec, neg


def decode(data, channels, sample_size, offset=0, domain=True, spec_wasted_bits=False):
    """Frame at data[offset:] of the stream `data` (its end is the stream's end).  domain=False
    keeps going where OutOfDomain would be raised for a sample (unbounded integers throughout)."""
    g = _Reader(data, 8 * offset)
    domain = [] if domain else None
    rep = {"offset": offset, "end": -1, "n_subframes": 0, "subframes": [], "padding_bits": 0, "header_bytes": 0,
           "block_size": 0}
    try:
        if g.uint(15) != 0x7FFC:
            raise _Stop(AssertionError, "sync")
        rep["blocking_strategy"] = g.uint(1)
        bcode = g.uint(4)
        if not 0 < bcode < 15:
            raise _Stop(AssertionError, "block_size_code")
        rcode = g.uint(4)
        if rcode == 15:
            raise _Stop(AssertionError, "sample_rate_code")
        ch_code = rep["channel_code"] = g.uint(4)
        if ch_code > 10:
            raise _Stop(AssertionError, "channels_code")
        scode = g.uint(3)
        if scode == 3:
            raise _Stop(AssertionError, "sample_size_code")
        if g.uint(1) != 0:
            raise _Stop(AssertionError, "reserved")
        b0 = g.uint(8)
        extra = 6 if b0 >= 0xFE else 5 if b0 >= 0xFC else 4 if b0 >= 0xF8 else 3 if b0 >= 0xF0 else 2 if b0 >= 0xE0 \
            else 1 if b0 >= 0xC0 else 0
        if g.p + 8 * extra > g.end:
            raise _Stop(EOFError, "eof")
        num = b0 if extra == 0 else b0 & ((1 << (6 - extra)) - 1)
        for _ in range(extra):
            num = (num << 6) | (g.uint(8) & 0x3F)
        rep["number"] = num
        if bcode == 1:
            bs = 192
        elif bcode <= 5:
            bs = 144 << bcode
        elif bcode == 6:
            bs = g.uint(8) + 1
        elif bcode == 7:
            bs = g.uint(16) + 1
        else:
            bs = 1 << bcode
        rep["block_size"] = bs
        rep["rate_code"] = rcode
        rep["sample_rate"] = g.uint(8) if rcode == 12 else g.uint(16) if rcode == 13 else g.uint(16) * 10 \
            if rcode == 14 else SAMPLE_RATES.get(rcode, 0)
        covered = g.p // 8 - offset
        rep["crc8"] = g.uint(8)
        rep["crc8_computed"] = _crc8(data[offset:offset + covered])
        rep["header_bytes"] = covered + 1
        rep["sample_size"] = SAMPLE_SIZES[scode]
        ss = rep["sample_size"] or sample_size
        nch = channels if ch_code == 1 else ch_code + 1 if ch_code <= 7 else 2
        subs, neg = [], False
        for c in range(nch):
            side = (ch_code == 8 and c == 1) or (ch_code == 9 and c == 0) or (ch_code == 10 and c == 1)
            x, rec, n = _subframe(g, bs, ss + int(side), 8 * offset, domain, spec_wasted_bits)
            subs.append(x)
            rep["subframes"].append(rec)
            rep["n_subframes"] += 1
            neg = neg or n
        if g.p % 8:
            rep["padding_bits"] = 8 - g.p % 8
            if g.uint(rep["padding_bits"]) != 0:
                raise _Stop(AssertionError, "padding")
        rep["crc16_computed"] = _crc16(data[offset:g.p // 8])
        rep["crc16"] = g.uint(16)
        rep["end"] = g.p // 8
        if neg:
            return Failed(ValueError, "neg_shift", rep["end"], rep)
    except _Stop as e:
        return Failed(e.exception, e.site, None, rep)
    if domain:
        raise OutOfDomain("sample outside int32")
    if ch_code == 8:
        out = [subs[0], [a - b for a, b in zip(subs[0], subs[1])]]
    elif ch_code == 9:
        out = [[a + b for a, b in zip(subs[0], subs[1])], subs[1]]
    elif ch_code == 10:
        right = [m - (s >> 1) for m, s in zip(subs[0], subs[1])]
        out = [[r + s for r, s in zip(right, subs[1])], right]
    else:
        out = subs
    return Decoded(out, subs, rep["end"], rep)
