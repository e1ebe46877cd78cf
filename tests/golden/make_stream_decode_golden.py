"""Golden fixtures for the stream decoder (flac_amd.decoder over flacmi_decode_stream_host),
produced by the reference's own `decode` and `cmd_decode`.

Run ONLY where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_stream_decode_golden.py

Whole streams (magic, STREAMINFO, optional metadata, frames) are assembled from the frame
builders of make_decode_golden.py or written by the reference's encoder, then read back by
flac.decoder.decode (decoder.py:31-63) and flac.__main__.cmd_decode (__main__.py:27-55).
Per case the fixture records the stream, the samples the reference yielded (count and
sha-256 of their int64 little-endian bytes), the exception class it raised after them, the
WAV payload cmd_decode wrote (or its exception), the frame-granular PCM this project
delivers for the same stream (whole frames before the first that fails), and the byte
offset of every frame the reference read (the reader's position around get_frame).
"""
import hashlib
import io
import json
import os
import random
import sys
import tempfile
import wave
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_decode_golden as M  # noqa: E402  (puts the reference on sys.path)
from flac import decoder as D  # noqa: E402
from flac import encoder as E  # noqa: E402
from flac.__main__ import cmd_decode  # noqa: E402


def stream(frames, channels, ss, max_bs=0, min_bs=0, samples=0, sr=44100, meta=()):
    """fLaC + STREAMINFO + the extra metadata blocks `meta` [(type, payload)] + frames."""
    b = M.Bits()
    for byte in b"fLaC":
        b.u(byte, 8)
    b.u(0 if meta else 1, 1)
    b.u(0, 7)
    b.u(34, 24)
    b.u(min_bs, 16)
    b.u(max_bs, 16)
    b.u(0, 24)
    b.u(0, 24)
    b.u(sr, 20)
    b.u(channels - 1, 3)
    b.u(ss - 1, 5)
    b.u(samples, 36)
    b.u(0, 128)
    for i, (t, payload) in enumerate(meta):
        b.u(1 if i == len(meta) - 1 else 0, 1)
        b.u(t, 7)
        b.u(len(payload), 24)
        for byte in payload:
            b.u(byte, 8)
    return b.data() + b"".join(frames)


def verdict(data):
    """What the reference makes of the stream."""
    out = {"open_exception": None, "exception": None, "offsets": [], "block_sizes": []}
    bio = io.BytesIO(data)
    real = D.get_frame

    def spy(get, ss):
        at = bio.tell()
        fr = real(get, ss)
        out["offsets"].append(at)
        out["block_sizes"].append(fr.header.block_size)
        return fr

    D.get_frame = spy
    samples = []
    try:
        try:
            (sr, ss, ch, n, it) = D.decode(bio)
        except Exception as e:  # noqa: BLE001
            out["open_exception"] = type(e).__name__
            return out, None
        out.update(sample_rate=sr, sample_size=ss, channels=ch, samples=n)
        try:
            for s in it:
                samples.append(s)
        except Exception as e:  # noqa: BLE001
            out["exception"] = type(e).__name__
    finally:
        D.get_frame = real
    out["n_samples"] = len(samples)
    flat = b"".join(int(v).to_bytes(8, "little", signed=True) for s in samples for v in s)
    out["samples_sha256"] = hashlib.sha256(flat).hexdigest()
    return out, samples


def wav_verdict(data, v, samples, keep_pcm=False):
    """cmd_decode's WAV payload, and the frame-granular PCM of the same stream."""
    res = {"wav_exception": None, "wav_sha256": None, "wav_bytes": None}
    with tempfile.TemporaryDirectory() as d:
        pi, po = Path(d) / "in.flac", Path(d) / "out.wav"
        pi.write_bytes(data)
        stdout = sys.stdout
        sys.stdout = io.StringIO()
        try:
            cmd_decode(pi, po)
        except Exception as e:  # noqa: BLE001
            res["wav_exception"] = type(e).__name__
        finally:
            sys.stdout = stdout
        if res["wav_exception"] is None:
            with wave.open(str(po), "rb") as w:
                payload = w.readframes(w.getnframes())
            res["wav_sha256"], res["wav_bytes"] = hashlib.sha256(payload).hexdigest(), len(payload)
    if samples is not None and v["sample_size"] % 8 == 0:
        B = v["sample_size"] // 8
        pcm, exc, i = b"", v["exception"], 0
        for bs in v["block_sizes"]:
            if i + bs > len(samples):
                break  # read, but decode_frame raised
            try:
                fr = b"".join(int(x).to_bytes(B, "little", signed=True) for s in samples[i:i + bs] for x in s)
            except OverflowError:
                exc = "OverflowError"
                break
            pcm += fr
            i += bs
        res.update(pcm_sha256=hashlib.sha256(pcm).hexdigest(), pcm_bytes=len(pcm), pcm_exception=exc)
        if keep_pcm:
            res["pcm_hex"] = pcm.hex()  # the CLI test builds its WAV from it
        if res["wav_exception"] is None:
            assert res["wav_sha256"] == res["pcm_sha256"]
    return res


def fixed_frame(rng, bs_code, bs, fno, ss, ss_code=0, order=2, ch_code=0, nsub=1, amp_bits=None):
    subs = []
    for _ in range(nsub):
        x = M.signal(rng, bs, amp_bits or ss)
        po = 0
        subs.append(lambda b, x=x: M.sub_fixed(b, x, order, ss, po, [4], method=int(ss > 16)))
    return M.frame(M.header(bs_code, bs, ch_code=ch_code, ss_code=ss_code, fno=fno), subs)


def stereo_frame(rng, code, bs_code, bs, fno):
    L = M.signal(rng, bs, 16)
    R = [max(-32768, min(32767, v + rng.randint(-500, 500))) for v in L]
    if code == 8:
        ch = [L, [a - b for a, b in zip(L, R)]]
    elif code == 9:
        ch = [[a - b for a, b in zip(L, R)], R]
    else:
        ch = [[(a + b) >> 1 for a, b in zip(L, R)], [a - b for a, b in zip(L, R)]]
    ssz = [16 + (code == 9), 16 + (code != 9)]
    return M.frame(M.header(bs_code, bs, ch_code=code, ss_code=4, fno=fno),
                   [lambda b, s=ch[0], w=ssz[0]: M.sub_fixed(b, s, 2, w, 0, [9]),
                    lambda b, s=ch[1], w=ssz[1]: M.sub_fixed(b, s, 1, w, 0, [9])])


def reference_encoded(rng, block, n):
    samples = [[a, b] for a, b in zip(M.signal(rng, n, 16), M.signal(rng, n, 16))]
    p = E.EncoderParameters(block_size=block, rice_partition_order=range(0, 3), lpc_order=range(0, 5), qlp_precision=8)
    return b"".join(E.encode(44100, 16, 2, n, iter(samples), p))


def build():
    rng = random.Random(20261019)
    cases = []

    def add(name, data, **extra):
        v, samples = verdict(data)
        if samples is not None:
            v.update(wav_verdict(data, v, samples, keep_pcm=name == "a_ref_192"))
        cases.append({"name": name, "hex": data.hex(), **v, **extra})
        print(f"{name:28s} {len(data):6d} B  frames {len(v['offsets']):3d}  -> "
              f"{v['open_exception'] or v['exception'] or 'ok'} / wav {v.get('wav_exception')}")
        return v

    # a. the reference encoder's own streams, short last block
    add("a_ref_192", reference_encoded(rng, 192, 192 * 4 + 50))
    add("a_ref_576", reference_encoded(rng, 576, 576 * 3 + 100))

    # b. a false sync: VERBATIM samples that spell a whole valid header (CRC-8 included)
    fake = M.header(2, 576, ch_code=0, ss_code=4, fno=5)
    assert len(fake) == 6
    vb = [rng.randint(-32768, 32767) for _ in range(192)]
    for k in range(3):
        vb[40 + k] = int.from_bytes(fake[2 * k:2 * k + 2], "big", signed=True)
    verb = M.frame(M.header(1, 192, ch_code=0, ss_code=4, fno=1),
                   [lambda b: (b.u(0, 1), b.u(1, 6), b.u(0, 1), [b.s(v, 16) for v in vb])])
    assert fake in verb
    add("b_false_sync", stream([fixed_frame(rng, 1, 192, 0, 16), verb, fixed_frame(rng, 1, 192, 2, 16)], 1, 16, 192),
        false_sync_at_frame=1)

    # c. a true frame whose CRC-8 byte is wrong (the reference reads it unchecked)
    fr = [fixed_frame(rng, 1, 192, k, 16) for k in range(3)]
    hl = len(M.header(1, 192, fno=1))
    bad = bytearray(fr[1])
    bad[hl - 1] ^= 0x55
    add("c_bad_crc8", stream([fr[0], bytes(bad), fr[2]], 1, 16, 192), damaged_frame=1)

    # d. each malformed frame of decode.json after two good frames
    dj = json.load(open(os.path.join(HERE, "decode.json")))["cases"]
    for c in dj:
        if c["site"] is None:
            continue
        good = [fixed_frame(rng, 1, 192, k, 16) for k in range(2)]
        add("d_" + c["name"], stream(good + [bytes.fromhex(c["hex"])], 1, 16, 1000), site=c["site"])

    # e. the last frame cut after its first 1..16 bytes and at half its length
    fr = [fixed_frame(rng, 1, 192, k, 16) for k in range(3)]
    whole = stream(fr, 1, 16, 192)
    for cut in list(range(1, 17)) + [len(fr[2]) // 2]:
        add(f"e_cut_{cut}", whole[:len(whole) - len(fr[2]) + cut])

    # f. mixed block sizes with L_S, S_R and M_S frames
    add("f_mixed", stream([stereo_frame(rng, 8, 1, 192, 0), stereo_frame(rng, 9, 5, 4608, 1),
                           stereo_frame(rng, 10, 6, 200, 2), fixed_frame(rng, 1, 192, 3, 16, ch_code=1, nsub=2)],
                          2, 16, 4608))
    # the same with STREAMINFO's max_block_size 0 (unknown) and one too small (an oversized block)
    fr = [stereo_frame(rng, 8, 1, 192, 0), stereo_frame(rng, 10, 3, 1152, 1), stereo_frame(rng, 9, 1, 192, 2)]
    add("f_maxbs_unknown", stream(fr, 2, 16, 0))
    add("f_maxbs_small", stream(fr, 2, 16, 192))

    # g. 8-, 24- and 32-bit streams; h. a 20-bit stream (cmd_decode asserts)
    for ss in (8, 24, 32, 20):
        fr = [fixed_frame(rng, 1, 192, k, ss, ch_code=1, nsub=2) for k in range(2)]
        fr.append(fixed_frame(rng, 6, 77, 2, ss, ch_code=1, nsub=2))
        add(f"{'h' if ss == 20 else 'g'}_{ss}bit", stream(fr, 2, ss, 192))

    # i. a frame whose header says 24-bit samples in a 16-bit stream, values past 16 bits
    fr = [fixed_frame(rng, 1, 192, 0, 16), fixed_frame(rng, 1, 192, 1, 24, ss_code=6), fixed_frame(rng, 1, 192, 2, 16)]
    add("i_wide_frame", stream(fr, 1, 16, 192), overflow_frame=1)

    # j. extra metadata before the frames: the frame starts take every byte alignment
    fr = [fixed_frame(rng, 1, 192, k, 16) for k in range(2)]
    for n in range(0, 20):
        add(f"j_meta_{n}", stream(fr, 1, 16, 192, meta=[(1, bytes(n)), (4, bytes([rng.randrange(256) for _ in range(7)]))]))

    with open(os.path.join(HERE, "decode_streams.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_stream_decode_golden.py",
                   "reference": "flac.decoder.decode (decoder.py:31-63), flac.__main__.cmd_decode (__main__.py:27-55)",
                   "cases": cases}, f, separators=(",", ":"))
    print(os.path.getsize(os.path.join(HERE, "decode_streams.json")), "bytes")


if __name__ == "__main__":
    build()
