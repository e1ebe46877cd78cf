"""What a .flac holds, frame by frame and subframe by subframe, read on the device: the tool
flac-py's README lists as its third known issue ("It would be nice to have a tool providing
information about a FLAC file, as `flac -a` does").

The metadata blocks are read on the host the way decoder.read_metadata / skip_metadata read
them, with the same assertions; the frames go through flacmi_info_stream_host chunk by
chunk: the device lists the candidate frame starts, k_frame_info parses every one of them
and reports what it read, the host walks the chain of true frames (include/flacmi.h, "stream
analysis").

    analyze(buffer_or_path)    -> StreamReport (frames is an iterator of FrameReport)
    summarize(report)          -> plain dicts of totals (consumes the iterator)
    format_frame / format_summary / format_metadata: the text `python -m flac_amd analyze` prints

Where the reference raises inside a frame, the reports of the frames before it come first,
then the iterator raises the same exception class (decoder.stop_exception); a frame the
stream's end cuts off ends the iterator silently, as get_frames does, and shows in
`trailing_bytes`.
"""
from dataclasses import asdict, dataclass, field
from typing import Iterator, Optional

import numpy as np

from . import abi
from .binary import Get
from .common import MAGIC, MetadataBlockType, Streaminfo
from .decoder import (DEFAULT_CHUNK_BYTES, _analyzer, _open, get_metadata_block_header, get_metadata_block_streaminfo,
                      stop_exception)

ASSIGNMENTS = {abi.CHANNELS_L_S: "LEFT_SIDE", abi.CHANNELS_S_R: "RIGHT_SIDE", abi.CHANNELS_M_S: "MID_SIDE"}
RESIDUAL_TYPES = {4: "RICE", 5: "RICE2"}
FRAME_CAPACITY = 4096  # frame records per device call


@dataclass
class SubframeReport:
    """flacmi_subframe_info, with the partitions as ("rice", parameter) / ("escape", width)."""
    bit_offset: int
    bits: int
    type: int
    order: int
    wasted_bits: int
    sample_bits: int
    precision: int
    shift: int
    coefficients: list
    coding_method: int
    partition_order: int
    escaped_partitions: int
    residual_bits: int
    abs_sum: int
    constant_value: int
    partitions_stored: int
    partitions: list = field(default_factory=list)
    truncated: bool = False  # the subframe has more partitions than max_partitions

    @property
    def type_name(self) -> str:
        return abi.SUB_TYPE_NAMES[self.type]


@dataclass
class FrameReport:
    """flacmi_frame_info, `offset` / `end` counted from the file's first byte."""
    index: int
    offset: int
    end: int
    coded_number: int
    status: int
    block_size: int
    blocking_strategy: int
    sample_rate: int
    sample_size: int
    channel_code: int
    n_subframes: int
    header_bytes: int
    crc8_stored: int
    crc8_computed: int
    crc16_stored: int
    crc16_computed: int
    padding_bits: int
    subframes: list = field(default_factory=list)

    @property
    def bytes(self) -> int:
        return self.end - self.offset

    @property
    def channel_assignment(self) -> str:
        return ASSIGNMENTS.get(self.channel_code, "INDEPENDENT")

    @property
    def crc8_ok(self) -> bool:
        return self.crc8_stored == self.crc8_computed

    @property
    def crc16_ok(self) -> bool:
        return self.crc16_stored == self.crc16_computed


@dataclass
class StreamReport:
    streaminfo: Streaminfo
    metadata: list            # (type, length, offset, last) per block, STREAMINFO first
    first_frame_offset: int
    frames: Iterator[FrameReport]
    trailing_bytes: Optional[int] = None  # set when `frames` is exhausted (or has raised)
    exception: Optional[Exception] = None  # the stopping exception `frames` raised, if any
    stats: list = field(default_factory=list)  # one dict per device call (flacmi_info_result's fields)


def read_blocks(buffer) -> tuple[Streaminfo, list]:
    """decoder.read_metadata (decoder.py:34-44, 90-96) listing the blocks it passes; leaves
    `buffer` at the first frame."""
    get = Get(buffer)
    assert get.bytes(4) == MAGIC
    at = buffer.tell()
    header = get_metadata_block_header(get)
    assert header.type == MetadataBlockType.Streaminfo
    streaminfo = get_metadata_block_streaminfo(get)
    blocks = [(header.type, header.length, at, header.last)]
    while header.last is False:
        at = buffer.tell()
        header = get_metadata_block_header(get)
        get.bytes(header.length)
        blocks.append((header.type, header.length, at, header.last))
    return streaminfo, blocks


def subframe_report(rec, parts) -> SubframeReport:
    """One flacmi_subframe_info record (a SUBFRAME_INFO_DTYPE scalar) and its part_params row."""
    order = int(rec["order"])
    is_lpc = int(rec["type"]) == abi.SUB_TYPE_LPC
    has_residual = int(rec["coding_method"]) != 0
    stored = int(rec["partitions_stored"])
    plist = [("escape", int(b) & 0x7F) if int(b) & abi.PART_ESCAPE else ("rice", int(b)) for b in parts[:stored]]
    return SubframeReport(
        bit_offset=int(rec["bit_offset"]), bits=int(rec["bits"]), type=int(rec["type"]), order=order,
        wasted_bits=int(rec["wasted_bits"]), sample_bits=int(rec["sample_bits"]), precision=int(rec["precision"]),
        shift=int(rec["shift"]), coefficients=[int(c) for c in rec["coefficients"][:order]] if is_lpc else [],
        coding_method=int(rec["coding_method"]), partition_order=int(rec["partition_order"]),
        escaped_partitions=int(rec["escaped_partitions"]), residual_bits=int(rec["residual_bits"]),
        abs_sum=int(rec["abs_sum"]), constant_value=int(rec["constant_value"]), partitions_stored=stored,
        partitions=plist, truncated=has_residual and (1 << int(rec["partition_order"])) > stored)


def frame_report(index: int, base: int, rec, subs, parts) -> FrameReport:
    fr = FrameReport(index=index, offset=base + int(rec["offset"]), end=base + int(rec["end"]),
                     **{k: int(rec[k]) for k in ("coded_number", "status", "block_size", "blocking_strategy", "sample_rate",
                                                 "sample_size", "channel_code", "n_subframes", "header_bytes",
                                                 "crc8_stored", "crc8_computed", "crc16_stored", "crc16_computed",
                                                 "padding_bits")})
    for c in range(min(fr.n_subframes, len(subs))):
        fr.subframes.append(subframe_report(subs[c], parts[c]))
    return fr


def _frames(report: StreamReport, buffer, owned: bool, chunk_bytes: int, device: int, max_partitions: int,
            frame_capacity: int, spec_wasted_bits: bool = False) -> Iterator[FrameReport]:
    """The FrameReports of the frames at `buffer`'s position, one flacmi_info_stream_host call
    per chunk (decoder._chunks' carry-over of a cut-off frame)."""
    si = report.streaminfo
    try:
        az = _analyzer(device)
        frames = np.zeros(frame_capacity, dtype=abi.FRAME_INFO_DTYPE)
        subs = np.zeros((frame_capacity, si.channels), dtype=abi.SUBFRAME_INFO_DTYPE)
        parts = np.zeros((frame_capacity, si.channels, max_partitions), dtype=np.uint8)
        stage = None
        carry = b""
        base = report.first_frame_offset  # file offset of the chunk's first byte
        final = False
        index = 0
        report.trailing_bytes = 0
        while True:
            want = max(chunk_bytes - len(carry), 0)
            new = buffer.read(want) if want and not final else b""
            if want and not final and len(new) < want:
                final = True
            data = carry + new
            n = len(data)
            report.trailing_bytes = n
            if n == 0:
                break
            if stage is None or n > len(stage):
                stage = az.host_array((n,), np.uint8)
            stage[:n] = np.frombuffer(data, dtype=np.uint8)
            res = az.info_stream(stage.ctypes.data, n, 0, si.channels, si.sample_size, final, frames, subs, parts,
                                 spec_wasted_bits)
            report.stats.append({f: getattr(res, f) for f, _ in abi.InfoResult._fields_} | {"bytes": n, "final": final})
            for k in range(res.frames):
                yield frame_report(index + k, base, frames[k], subs[k], parts[k])
            index += res.frames
            report.trailing_bytes = n - res.consumed
            if res.status:
                report.trailing_bytes += len(buffer.read())  # the failing frame and all behind it
                report.exception = stop_exception(res.status, res.site, index)
                raise report.exception
            carry = data[res.consumed:]
            base += res.consumed
            if res.full:
                continue
            if final:
                break  # the stream's end, or a cut-off last frame (get_frames' EOFError: silent)
            if res.frames == 0:
                chunk_bytes *= 2  # no whole frame in the chunk
    finally:
        if owned:
            buffer.close()


def analyze(buffer_or_path, chunk_bytes: int = DEFAULT_CHUNK_BYTES, device: int = 0, max_partitions: int = 64,
            frame_capacity: int = FRAME_CAPACITY, spec_wasted_bits: bool = False) -> StreamReport:
    """The report of a FLAC stream (a path, bytes or a binary file object).  chunk_bytes: stream
    bytes per device call; max_partitions: Rice parameters kept per subframe (a subframe with
    more is marked `truncated`); frame_capacity: frame records per device call; spec_wasted_bits:
    read wasted bits as the format codes them (FLACMI_DECODE_WASTED_SPEC), so a subframe's
    wasted_bits is the count its encoder declared and sample_bits the width it wrote (off: the
    reference's reading, one less wasted bit and one more sample bit in a flagged subframe)."""
    buffer, owned = _open(buffer_or_path)
    try:
        streaminfo, blocks = read_blocks(buffer)
    except BaseException:
        if owned:
            buffer.close()
        raise
    report = StreamReport(streaminfo=streaminfo, metadata=blocks, first_frame_offset=buffer.tell(), frames=iter(()))
    report.frames = _frames(report, buffer, owned, chunk_bytes, device, max_partitions, max(frame_capacity, 1),
                            spec_wasted_bits)
    return report


def summarize(report: StreamReport, frames=None) -> dict:
    """Totals over the report's frames (consumes report.frames, or takes `frames`, a list of
    FrameReports already read).  A stopping exception is kept in report.exception, not raised."""
    si = report.streaminfo
    if frames is None:
        frames = []
        try:
            for fr in report.frames:
                frames.append(fr)
        except Exception as e:  # noqa: BLE001  -- kept for the caller: the totals are of the frames before it
            report.exception = e
    subframes = {name: 0 for name in abi.SUB_TYPE_NAMES}
    orders, partition_orders = {}, {}
    assignments = {"INDEPENDENT": 0, "LEFT_SIDE": 0, "RIGHT_SIDE": 0, "MID_SIDE": 0}
    methods = {"RICE": 0, "RICE2": 0}
    escaped = framing = subframe_bits = residual = samples = bad8 = bad16 = 0
    for fr in frames:
        assignments[fr.channel_assignment] += 1
        samples += fr.block_size
        bad8 += not fr.crc8_ok
        bad16 += not fr.crc16_ok
        framing += 8 * fr.header_bytes + 16 + fr.padding_bits
        for s in fr.subframes:
            subframes[s.type_name] += 1
            residual += s.residual_bits
            subframe_bits += s.bits - s.residual_bits
            if s.coding_method:
                orders[(s.type_name, s.order)] = orders.get((s.type_name, s.order), 0) + 1
                partition_orders[s.partition_order] = partition_orders.get(s.partition_order, 0) + 1
                methods[RESIDUAL_TYPES[s.coding_method]] += 1
                escaped += s.escaped_partitions
    sizes = [fr.bytes for fr in frames]
    blocks = [fr.block_size for fr in frames]
    raw = si.channels * si.sample_size * samples
    disagree = []
    if blocks and max(blocks) > si.max_block_size:
        disagree.append(f"max_block_size {si.max_block_size} < largest block {max(blocks)}")
    if blocks[:-1] and min(blocks[:-1]) < si.min_block_size:
        disagree.append(f"min_block_size {si.min_block_size} > smallest block {min(blocks[:-1])} (last frame excluded)")
    if si.max_frame_size and sizes and max(sizes) > si.max_frame_size:
        disagree.append(f"max_frame_size {si.max_frame_size} < largest frame {max(sizes)}")
    if si.min_frame_size and sizes and min(sizes) < si.min_frame_size:
        disagree.append(f"min_frame_size {si.min_frame_size} > smallest frame {min(sizes)}")
    if si.samples and si.samples != samples:
        disagree.append(f"samples {si.samples} != {samples} in the frames")
    return {
        "frames": len(frames), "samples": samples, "trailing_bytes": report.trailing_bytes or 0,
        "subframes": subframes, "orders": orders, "channel_assignments": assignments,
        "partition_orders": partition_orders, "residual_types": methods, "escaped_partitions": escaped,
        "bits": {"framing": framing, "subframe": subframe_bits, "residual": residual},
        "frame_bytes": {"min": min(sizes, default=0), "max": max(sizes, default=0),
                        "mean": sum(sizes) / len(sizes) if sizes else 0.0},
        "compression_ratio": 8 * sum(sizes) / raw if raw else 0.0,
        "crc_mismatches": {"crc8": bad8, "crc16": bad16},
        "streaminfo_disagreements": disagree,
    }


# ---- text (python -m flac_amd analyze) -----------------------------------------------------------

def format_metadata(blocks) -> list[str]:
    return [f"metadata={k}\ttype={t.name.upper()}\tlength={length}\toffset={offset}\tlast={int(last)}"
            for k, (t, length, offset, last) in enumerate(blocks)]


def format_frame(fr: FrameReport, streaminfo: Streaminfo, partitions: bool = False) -> list[str]:
    """The frame's line and one indented line per subframe."""
    lines = [f"frame={fr.index}\toffset={fr.offset}\tbytes={fr.bytes}\tblocksize={fr.block_size}\t"
             f"sample_rate={fr.sample_rate or streaminfo.sample_rate}\t"
             f"sample_size={fr.sample_size or streaminfo.sample_size}\tchannel_assignment={fr.channel_assignment}\t"
             f"number={fr.coded_number}\tcrc8={'ok' if fr.crc8_ok else 'BAD'}\tcrc16={'ok' if fr.crc16_ok else 'BAD'}"]
    for c, s in enumerate(fr.subframes):
        ln = f"\tsubframe={c}\ttype={s.type_name}\torder={s.order}\twasted_bits={s.wasted_bits}\tbits={s.bits}"
        if s.type == abi.SUB_TYPE_LPC:
            ln += f"\tprecision={s.precision}\tshift={s.shift}\tcoefficients={','.join(map(str, s.coefficients))}"
        if s.coding_method:
            ln += (f"\tresidual_type={RESIDUAL_TYPES[s.coding_method]}\tpartition_order={s.partition_order}"
                   f"\tabs_sum={s.abs_sum}")
            if partitions:
                ln += "\tpartitions=" + ",".join(f"e{v}" if kind == "escape" else str(v) for kind, v in s.partitions)
                ln += ",..." if s.truncated else ""
        lines.append(ln)
    return lines


def format_summary(summary: dict) -> list[str]:
    def kv(d):
        return "".join(f"\t{k}={v}" for k, v in d.items())
    fb = summary["frame_bytes"]
    lines = [f"summary\tframes={summary['frames']}\tsamples={summary['samples']}\ttrailing_bytes={summary['trailing_bytes']}",
             "summary\tsubframes" + kv(summary["subframes"]),
             "summary\torders" + "".join(f"\t{t}:{o}={n}" for (t, o), n in sorted(summary["orders"].items())),
             "summary\tchannel_assignments" + kv(summary["channel_assignments"]),
             "summary\tpartition_orders" + kv(dict(sorted(summary["partition_orders"].items()))),
             "summary\tresidual_types" + kv(summary["residual_types"]),
             f"summary\tescaped_partitions={summary['escaped_partitions']}",
             "summary\tbits" + kv(summary["bits"]),
             f"summary\tframe_bytes\tmin={fb['min']}\tmax={fb['max']}\tmean={fb['mean']:.2f}",
             f"summary\tcompression_ratio={summary['compression_ratio']:.4f}",
             "summary\tcrc_mismatches" + kv(summary["crc_mismatches"])]
    lines += [f"summary\tstreaminfo\t{d}" for d in summary["streaminfo_disagreements"]]
    return lines


def frame_json(fr: FrameReport) -> dict:
    d = asdict(fr)
    d["bytes"], d["channel_assignment"] = fr.bytes, fr.channel_assignment
    for s, sd in zip(fr.subframes, d["subframes"]):
        sd["type"] = s.type_name
    return d


def summary_json(summary: dict) -> dict:
    return summary | {"orders": {f"{t}:{o}": n for (t, o), n in sorted(summary["orders"].items())},
                      "partition_orders": {str(k): v for k, v in sorted(summary["partition_orders"].items())}}
