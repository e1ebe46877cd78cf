"""A bit writer and a FLAC frame assembler of the tests' own: frames are put together field by
field, so a test chooses every header form, subframe type, wasted-bits count, Rice parameter and
escape width, including the combinations no encoder of this project writes.  Used by the golden
makers (tests/golden/make_decode_golden.py, make_decode_fuzz_golden.py) and by the fuzz
generator (tests/decode_fuzz_cases.py).  Imports nothing but the standard library.
"""
FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


class Bits:
    """MSB-first bit writer (n: the bits written so far)."""

    def __init__(self):
        self.n = 0
        self._done, self._acc, self._k = bytearray(), 0, 0  # whole bytes; the last _k < 8 bits (after a flush)

    def u(self, x, n):
        assert 0 <= x < (1 << n) or n == 0
        self._acc, self._k, self.n = (self._acc << n) | x, self._k + n, self.n + n
        if self._k >= 64:  # keep the accumulator short: long frames stay linear
            rest = self._k % 8
            self._done += (self._acc >> rest).to_bytes(self._k // 8, "big")
            self._acc, self._k = self._acc & ((1 << rest) - 1), rest

    def s(self, x, n):
        assert -(1 << (n - 1)) <= x < (1 << (n - 1))
        self.u(x & ((1 << n) - 1), n)

    def rice(self, x, p):
        z = (x << 1) ^ (x >> 63) if x >= 0 else ((-x) << 1) - 1
        self.u(0, z >> p)
        self.u(1, 1)
        self.u(z & ((1 << p) - 1), p)

    def pad(self):
        if self.n % 8:
            self.u(0, 8 - self.n % 8)

    def data(self):
        assert self.n % 8 == 0
        return bytes(self._done) + (self._acc.to_bytes(self._k // 8, "big") if self._k else b"")


def crc8(bs):
    c = 0
    for b in bs:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(bs):
    c = 0
    for b in bs:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def coded(x):
    """The UTF-8-like coded number, 1 to 7 bytes (up to 36 bits)."""
    if x < 128:
        return bytes([x])
    n = 2
    while x >= (1 << (5 * n + 1)):
        n += 1
    out = [(0x80 | (x >> (6 * i)) & 0x3F) for i in reversed(range(n - 1))]
    return bytes([((0xFF << (8 - n)) & 0xFF) | (x >> (6 * (n - 1)))] + out)


def header(bs_code, bs, sr_code=0, ch_code=0, ss_code=0, fno=0, sync=0x7FFC, reserved=0, sr_extra=None, strategy=0):
    """Frame header with its CRC-8.  strategy 1: the blocking-strategy bit set (fno is then a
    sample number of up to 36 bits, 7 bytes)."""
    b = Bits()
    b.u(sync, 15)
    b.u(strategy, 1)
    b.u(bs_code, 4)
    b.u(sr_code, 4)
    b.u(ch_code, 4)
    b.u(ss_code, 3)
    b.u(reserved, 1)
    for byte in coded(fno):
        b.u(byte, 8)
    if bs_code == 6:
        b.u(bs - 1, 8)
    elif bs_code == 7:
        b.u(bs - 1, 16)
    if sr_code == 12:
        b.u(sr_extra or 48, 8)
    elif sr_code in (13, 14):
        b.u(sr_extra or 4410, 16)
    h = b.data()
    return h + bytes([crc8(h)])


def predict(x, coefs, shift, order):
    return [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, len(x))]


def residual_bits(b, r, bs, order, po, params, method=0, esc=None, exact=False):
    """Rice partitions of residual r (len bs - order); params per partition; esc: {k: bits}.
    exact: a listed parameter is written as given (else it is a lower bound, below).  Returns
    the partitions as written: ("rice", k) or ("escape", width)."""
    b.u(method, 2)
    b.u(po, 4)
    plen = bs >> po
    i = 0
    pb = 5 if method else 4
    written = []
    for k in range(1 << po):
        n = plen - order if k == 0 else plen
        part = r[i:i + n]
        i += n
        if esc and k in esc:
            b.u((1 << pb) - 1, pb)
            b.u(esc[k], 5)
            for x in part:
                b.s(x, esc[k]) if esc[k] else None
            written.append(("escape", esc[k]))
        else:
            if exact:
                p = params[k]
            else:
                # the listed parameter is a lower bound: raised to the encoder's own choice
                # floor(log2(mean zig-zag)) so no code gets a huge unary part
                zz = [2 * v if v >= 0 else -2 * v - 1 for v in part]
                mean = sum(zz) // max(len(zz), 1)
                p = max(params[k], mean.bit_length() - 1 if mean >= 1 else 0)
            assert p < (1 << pb) - 1
            b.u(p, pb)
            for x in part:
                b.rice(x, p)
            written.append(("rice", p))
    return written


def sub_head(b, type_code, wasted=0, flag=None, pad=0):
    """Subframe header.  wasted: the number of zeros behind a set flag bit, which is what the
    reference's get_wasted_bits returns (wasted 0: flag clear, unless flag=1 asks for a set flag
    followed at once by the one, a count of zero zeros)."""
    b.u(pad, 1)
    b.u(type_code, 6)
    if wasted or flag:
        b.u(1, 1)
        b.u(0, wasted)
        b.u(1, 1)
    else:
        b.u(0, 1)


def sub_constant(b, value, ss, wasted=0, flag=None):
    sub_head(b, 0, wasted, flag)
    b.s(value, ss - wasted)


def sub_verbatim(b, x, ss, wasted=0, flag=None):
    sub_head(b, 1, wasted, flag)
    for v in x:
        b.s(v, ss - wasted)


def sub_fixed(b, x, order, ss, po, params, method=0, esc=None, wasted=0, pad=0, exact=False, flag=None):
    sub_head(b, 8 | order, wasted, flag, pad)
    w = ss - wasted
    for v in x[:order]:
        b.s(v, w)
    return residual_bits(b, predict(x, FIXED[order], 0, order), len(x), order, po, params, method, esc, exact)


def sub_lpc(b, x, coefs, prec, shift, ss, po, params, method=0, esc=None, prec_field=None, raw_resid=None,
            wasted=0, exact=False, flag=None):
    order = len(coefs)
    sub_head(b, 32 | (order - 1), wasted, flag)
    for v in x[:order]:
        b.s(v, ss - wasted)
    b.u(prec - 1 if prec_field is None else prec_field, 4)
    b.s(shift, 5)
    for c in coefs:
        b.s(c, prec)
    r = raw_resid if raw_resid is not None else predict(x, coefs, shift, order)
    return residual_bits(b, r, len(x), order, po, params, method, esc, exact)


def frame(hdr, subs):
    b = Bits()
    for byte in hdr:
        b.u(byte, 8)
    for f in subs:
        f(b)
    b.pad()
    d = b.data()
    return d + crc16(d).to_bytes(2, "big")
