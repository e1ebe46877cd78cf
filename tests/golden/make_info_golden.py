"""Golden fixtures for the stream analysis (flac_amd.info over csrc/k_info.hip), produced by
the reference's own frame reader.

Run ONLY where the reference is readable:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_info_golden.py

The inputs are the ones tests/info_cases.py assembles from the fixtures already committed
(decode.json's frames, streams of decode_streams.json / fallback_streams.json /
stereo_streams.json / lpc_sign_streams.json, and `many_frames`).  Each frame is read by the
reference's functions only: get_frame's loop (decoder.py:111-130) is restated here so that
the reader's bit position (tell() * 8 - bits_until_alignment) can be noted before and after
every get_subframe, with this project's documented choice that an L_R frame holds the
stream's channel count of subframes (include/flacmi.h).  What get_subframe does not return
(wasted bits, the coding method, each partition's parameter or escape width, the residual's
extent) is noted by wrappers around get_subframe_header, get_residual and get_rice_partition
that call the reference's own function and look at its result.  Recorded per frame: the
FrameHeader fields, per subframe its type, order, wasted bits, precision, shift, coefficients,
coding method, partition order, partitions, sum |residual| and constant value, bit offset and
size, the stored CRCs (and, by the reference's crc.py, the computed ones), the frame's end, and
the exception class and statement line where it raised.  No residual or sample lists.

frame_info.json     {"frames": {name: frame record}, "streams": {name: stream record}}
analyze_text.json   for two streams the text `python -m flac_amd analyze` must print, without
                    and with --partitions, formatted by this script's own formatter over the
                    reference's dataclasses (not by flac_amd.info).
"""
import io
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import make_decode_golden as M  # noqa: E402,F401  (puts the reference on sys.path)
import info_cases as IC  # noqa: E402
from flac import decoder as D  # noqa: E402
from flac import common as FC  # noqa: E402
from flac.binary import Get  # noqa: E402
from flac.crc import crc8, crc16  # noqa: E402

TYPES = {FC.SubframeConstant: "CONSTANT", FC.SubframeVerbatim: "VERBATIM", FC.SubframeFixed: "FIXED",
         FC.SubframeLPC: "LPC"}
ASSIGNMENT = {FC.Channels.L_S: "LEFT_SIDE", FC.Channels.S_R: "RIGHT_SIDE", FC.Channels.M_S: "MID_SIDE"}


class Notes:
    """What the wrappers saw during one get_subframe."""
    pos = None

    def __init__(self):
        self.wasted = 0
        self.method = 0
        self.parts = []
        self.r0 = self.r1 = None


NOTES = Notes()
_real = (D.get_subframe_header, D.get_residual, D.get_rice_partition)


def _header(get):
    h = _real[0](get)
    NOTES.wasted = h.wasted_bits
    return h


def _residual(get, block_size, order):
    NOTES.r0 = Notes.pos()
    r = _real[1](get, block_size, order)
    NOTES.r1 = Notes.pos()
    NOTES.method = r.coding_method.value
    return r


def _partition(get, method, count):
    seen = []
    uint = get.uint

    def noting(n):
        v = uint(n)
        if len(seen) < 2:
            seen.append(v)
        return v
    get.uint = noting
    try:
        p = _real[2](get, method, count)
    finally:
        del get.uint
    NOTES.parts.append(["e", seen[1]] if isinstance(p, FC.EscapedPartition) else p.parameter)
    return p


D.get_subframe_header, D.get_residual, D.get_rice_partition = _header, _residual, _partition


def where(e):
    tb = traceback.extract_tb(e.__traceback__)[-1]
    return f"{os.path.basename(tb.filename)}:{tb.lineno}"


def read_frame(get, bio, data, ss_stream, channels):
    """(record, reference objects) of the frame at bio's position; record["exception"] is set
    where the reference raised (the reader is then wherever it stopped)."""
    global NOTES
    Notes.pos = staticmethod(lambda: bio.tell() * 8 - get.bits_until_alignment)
    at = bio.tell()
    rec = {"offset": at, "end": -1, "n_subframes": 0, "subframes": [], "exception": None}
    objs = {"header": None, "subs": []}
    try:
        header = D.get_frame_header(get)
        objs["header"] = header
        hb = bio.tell() - at
        rec.update(number=header.coded_number, block_size=header.block_size,
                   blocking_strategy=header.blocking_strategy.value, sample_rate=header.sample_rate or 0,
                   sample_size=header.sample_size or 0,
                   channel_code=FC.CHANNELS_ENCODING[header.channels], header_bytes=hb, crc8=header.crc,
                   crc8_computed=crc8(data[at:at + hb - 1], FC.CRC8_POLYNOMIAL))
        sample_size = header.sample_size or ss_stream
        l_r = header.channels == FC.Channels.L_R
        count = channels if l_r else header.channels.count
        dbit = [0] * count if l_r else header.channels.decorrelation_bit
        for i in range(count):
            NOTES = Notes()
            p0 = Notes.pos()
            sub = D.get_subframe(get, header.block_size, sample_size + dbit[i])
            p1 = Notes.pos()
            s = {"bit_offset": p0 - 8 * at, "bits": p1 - p0, "type": TYPES[type(sub)],
                 "order": getattr(sub, "order", 0), "wasted_bits": NOTES.wasted,
                 "sample_bits": sample_size + dbit[i] - NOTES.wasted,
                 "precision": getattr(sub, "precision", 0), "shift": getattr(sub, "shift", 0),
                 "coefficients": list(getattr(sub, "coefficients", [])), "coding_method": NOTES.method,
                 "partition_order": len(NOTES.parts).bit_length() - 1 if NOTES.parts else 0,
                 "partitions": NOTES.parts, "residual_bits": (NOTES.r1 - NOTES.r0) if NOTES.r0 is not None else 0,
                 "abs_sum": sum(abs(r) for r in getattr(sub, "residual", [])),
                 "constant": sub.sample if isinstance(sub, FC.SubframeConstant) else 0}
            rec["subframes"].append(s)
            objs["subs"].append((sub, NOTES))
            rec["n_subframes"] += 1
        rec["padding_bits"] = get.bits_until_alignment
        if get.is_aligned is False:
            padding = get.uint(get.bits_until_alignment)
            if padding != 0:  # decoder.py:126 `assert padding == 0`, restated above
                rec["exception"] = {"class": "AssertionError", "line": "decoder.py:126"}
                return rec, objs
        crc = get.uint(16)
        end = bio.tell()
        rec.update(end=end, crc16=crc, crc16_computed=crc16(data[at:end - 2], FC.CRC16_POLYNOMIAL))
    except Exception as e:  # noqa: BLE001  -- the reference's exception class is the fixture
        rec["exception"] = {"class": type(e).__name__, "line": where(e)}
    return rec, objs


def read_stream(data):
    """The reference's decode() up to the frames (decoder.py:34-44, 90-96 restated to list
    the blocks), then get_frames' loop (decoder.py:100-108) over read_frame."""
    bio = io.BytesIO(data)
    get = Get(bio)
    assert get.bytes(4) == FC.MAGIC
    blocks = []
    at = bio.tell()
    h = D.get_metadata_block_header(get)
    assert h.type == FC.MetadataBlockType.Streaminfo
    si = D.get_metadata_block_streaminfo(get)
    blocks.append((h, at))
    while h.last is False:
        at = bio.tell()
        h = D.get_metadata_block_header(get)
        get.bytes(h.length)
        blocks.append((h, at))
    out = {"streaminfo": {k: (v.hex() if isinstance(v, bytes) else v) for k, v in vars(si).items()},
           "metadata": [[b.type.value, b.length, o, int(b.last)] for b, o in blocks],
           "first_frame_offset": bio.tell(), "frames": [], "exception": None}
    objs = []
    good_end = bio.tell()
    while True:
        rec, ob = read_frame(get, bio, data, si.sample_size, si.channels)
        if rec["exception"]:
            if rec["exception"]["class"] != "EOFError":
                out["exception"] = rec["exception"] | {"frame": len(out["frames"]), "n_subframes": rec["n_subframes"]}
            break
        out["frames"].append(rec)
        objs.append(ob)
        good_end = rec["end"]
    out["trailing_bytes"] = len(data) - good_end
    return out, (si, blocks, objs)


# ---- this script's formatter: the text `python -m flac_amd analyze` prints -----------------

def text(out, refs, partitions):
    si, blocks, objs = refs
    lines = []
    for k, (b, off) in enumerate(blocks):
        lines.append(f"metadata={k}\ttype={b.type.name.upper()}\tlength={b.length}\toffset={off}\tlast={int(b.last)}")
    n_sub = {t: 0 for t in TYPES.values()}
    orders, assign, porders = {}, {"INDEPENDENT": 0, "LEFT_SIDE": 0, "RIGHT_SIDE": 0, "MID_SIDE": 0}, {}
    methods = {"RICE": 0, "RICE2": 0}
    escaped = framing = subframe = residual = samples = bad8 = bad16 = 0
    sizes, blocksizes = [], []
    for k, (rec, ob) in enumerate(zip(out["frames"], objs)):
        h = ob["header"]
        name = ASSIGNMENT.get(h.channels, "INDEPENDENT")
        size = rec["end"] - rec["offset"]
        ok8 = rec["crc8"] == rec["crc8_computed"]
        ok16 = rec["crc16"] == rec["crc16_computed"]
        lines.append(f"frame={k}\toffset={rec['offset']}\tbytes={size}\tblocksize={h.block_size}\t"
                     f"sample_rate={h.sample_rate or si.sample_rate}\t"
                     f"sample_size={h.sample_size or si.sample_size}\t"
                     f"channel_assignment={name}\tnumber={h.coded_number}\tcrc8={'ok' if ok8 else 'BAD'}\t"
                     f"crc16={'ok' if ok16 else 'BAD'}")
        assign[name] += 1
        samples += h.block_size
        sizes.append(size)
        blocksizes.append(h.block_size)
        bad8 += not ok8
        bad16 += not ok16
        framing += 8 * rec["header_bytes"] + 16 + rec["padding_bits"]
        for c, ((sub, notes), s) in enumerate(zip(ob["subs"], rec["subframes"])):
            t = TYPES[type(sub)]
            ln = f"\tsubframe={c}\ttype={t}\torder={getattr(sub, 'order', 0)}\twasted_bits={notes.wasted}\tbits={s['bits']}"
            if t == "LPC":
                ln += f"\tprecision={sub.precision}\tshift={sub.shift}\tcoefficients={','.join(map(str, sub.coefficients))}"
            if t in ("FIXED", "LPC"):
                rt = "RICE2" if notes.method == 5 else "RICE"
                ln += (f"\tresidual_type={rt}\tpartition_order={s['partition_order']}"
                       f"\tabs_sum={sum(abs(r) for r in sub.residual)}")
                if partitions:
                    ln += "\tpartitions=" + ",".join(f"e{p[1]}" if isinstance(p, list) else str(p) for p in notes.parts)
                methods[rt] += 1
                porders[s["partition_order"]] = porders.get(s["partition_order"], 0) + 1
                escaped += sum(isinstance(p, list) for p in notes.parts)
                orders[(t, sub.order)] = orders.get((t, sub.order), 0) + 1
            lines.append(ln)
            n_sub[t] += 1
            residual += s["residual_bits"]
            subframe += s["bits"] - s["residual_bits"]
    lines.append(f"summary\tframes={len(objs)}\tsamples={samples}\ttrailing_bytes={out['trailing_bytes']}")
    lines.append("summary\tsubframes\t" + "\t".join(f"{t}={n}" for t, n in n_sub.items()))
    lines.append("summary\torders" + "".join(f"\t{t}:{o}={n}" for (t, o), n in sorted(orders.items())))
    lines.append("summary\tchannel_assignments\t" + "\t".join(f"{t}={n}" for t, n in assign.items()))
    lines.append("summary\tpartition_orders" + "".join(f"\t{o}={n}" for o, n in sorted(porders.items())))
    lines.append("summary\tresidual_types\t" + "\t".join(f"{t}={n}" for t, n in methods.items()))
    lines.append(f"summary\tescaped_partitions={escaped}")
    lines.append(f"summary\tbits\tframing={framing}\tsubframe={subframe}\tresidual={residual}")
    mean = sum(sizes) / len(sizes) if sizes else 0.0
    lines.append(f"summary\tframe_bytes\tmin={min(sizes, default=0)}\tmax={max(sizes, default=0)}\tmean={mean:.2f}")
    raw = si.channels * si.sample_size * samples
    lines.append(f"summary\tcompression_ratio={8 * sum(sizes) / raw if raw else 0.0:.4f}")
    lines.append(f"summary\tcrc_mismatches\tcrc8={bad8}\tcrc16={bad16}")
    if blocksizes and max(blocksizes) > si.max_block_size:
        lines.append(f"summary\tstreaminfo\tmax_block_size {si.max_block_size} < largest block {max(blocksizes)}")
    if blocksizes[:-1] and min(blocksizes[:-1]) < si.min_block_size:
        lines.append(f"summary\tstreaminfo\tmin_block_size {si.min_block_size} > smallest block "
                     f"{min(blocksizes[:-1])} (last frame excluded)")
    if si.max_frame_size and sizes and max(sizes) > si.max_frame_size:
        lines.append(f"summary\tstreaminfo\tmax_frame_size {si.max_frame_size} < largest frame {max(sizes)}")
    if si.min_frame_size and sizes and min(sizes) < si.min_frame_size:
        lines.append(f"summary\tstreaminfo\tmin_frame_size {si.min_frame_size} > smallest frame {min(sizes)}")
    if si.samples and si.samples != samples:
        lines.append(f"summary\tstreaminfo\tsamples {si.samples} != {samples} in the frames")
    return "\n".join(lines) + "\n"


def build():
    frames = {}
    for name, data, channels, ss in IC.single_frames():
        bio = io.BytesIO(data)
        rec, _ = read_frame(Get(bio), bio, data, ss, channels)
        frames[name] = rec
        print(f"{name:28s} {len(data):6d} B -> {rec['exception'] or 'ok'}")
    streams, texts = {}, {}
    for name, data in IC.streams().items():
        try:
            out, refs = read_stream(data)
        except Exception as e:  # noqa: BLE001  -- the metadata the reference cannot read
            streams[name] = {"open_exception": {"class": type(e).__name__, "line": where(e)}}
            print(f"{name:28s} {len(data):6d} B  -> open: {streams[name]['open_exception']}")
            continue
        out["open_exception"] = None
        streams[name] = out
        print(f"{name:28s} {len(data):6d} B  frames {len(out['frames']):3d} trailing {out['trailing_bytes']:4d} "
              f"-> {out['exception'] or 'ok'}")
        if name in IC.TEXT_STREAMS:
            texts[name] = {"plain": text(out, refs, False), "partitions": text(out, refs, True)}
    meta = {"generator": "tests/golden/make_info_golden.py",
            "reference": "flac.decoder get_frame_header / get_subframe / get_residual / get_rice_partition "
                         "(decoder.py:111-421), get_frame's loop restated"}
    for fn, body in (("frame_info.json", {"frames": frames, "streams": streams}), ("analyze_text.json", {"streams": texts})):
        with open(os.path.join(HERE, fn), "w") as f:
            json.dump(meta | body, f, separators=(",", ":"))
        print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    build()
