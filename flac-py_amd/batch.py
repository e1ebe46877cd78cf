"""Many whole .flac streams decoded in one device call, planar and padded on the device.

    decode_batch(streams, dtype="int32")   streams of one (channels, sample size) -> BatchResult
    decode_files(paths, dtype="auto")      any mix, grouped by (channels, sample size) -> [DecodedStream]

Each stream's metadata is read on the host exactly as flac_amd.decoder reads it (the reference's
assertions, per stream); the frame regions are packed back to back and go through
flacmi_decode_batch_host once: one copy in, one index, one pass 1, the walk per stream, and
k_planar writes `data[s, c, t]` (include/flacmi.h, "batch decoder").  Each stream
decodes exactly as decoder.decode decodes it alone: its own length, and where the reference would
raise inside a frame, `errors[s]` holds the exception decoder.stop_exception builds (class, site,
frame index) and `lengths[s]` counts the samples of the frames before it.  A stream whose
metadata cannot be read takes no part (length 0, its exception in `errors[s]`).
"""
import os
from dataclasses import dataclass, field
from io import BytesIO

import numpy as np

from . import abi
from .common import Streaminfo
from .decoder import _analyzer, read_metadata, stop_exception

DEFAULT_BYTE_BUDGET = 1 << 26  # frame bytes per device call (pass 1's rows must stay under 4 GiB)
DTYPES = ("int16", "int32", "float32")


@dataclass
class BatchResult:
    data: object                 # torch tensor [N, C, T] on the device, T a multiple of 16 bytes of elements
    lengths: list                # samples per channel delivered, per stream
    sample_rates: list           # per stream (None where the metadata could not be read)
    errors: list                 # per stream: None, or the exception that stopped it
    channels: int
    sample_size: int
    stats: list = field(default_factory=list)  # one dict per device call


@dataclass
class DecodedStream:
    data: object                 # [C, T] view of its group's tensor; the first `length` elements of a row count
    length: int
    sample_rate: object
    channels: object
    sample_size: object
    error: object
    streaminfo: object = None    # the stream's STREAMINFO (None where its metadata could not be read)


def read_stream(stream) -> bytes:
    if isinstance(stream, (str, os.PathLike)):
        with open(stream, "rb") as f:
            return f.read()
    return bytes(stream)


def split_stream(data: bytes) -> tuple[Streaminfo, bytes]:
    """(STREAMINFO, the frame region): decoder.read_metadata leaves the buffer at the first frame."""
    buffer = BytesIO(data)
    streaminfo = read_metadata(buffer)
    return streaminfo, data[buffer.tell():]


def open_streams(streams):
    """-> (infos, regions, errors): per stream its STREAMINFO and frame region, or None, b"" and
    the exception reading its metadata raised."""
    infos, regions, errors = [], [], []
    for st in streams:
        try:
            si, region = split_stream(read_stream(st))
            if si.channels < 1 or si.channels > 8 or si.sample_size < 4:
                raise ValueError(f"{si.channels} channels of {si.sample_size} bits")
        except Exception as e:  # noqa: BLE001  -- recorded per stream: the others go on
            si, region = None, b""
            errors.append(e)
        else:
            errors.append(None)
        infos.append(si)
        regions.append(region)
    return infos, regions, errors


def seg_offsets(regions) -> np.ndarray:
    """[len(regions) + 1] int64: region s is bytes [seg[s], seg[s + 1]) of the packed buffer."""
    seg = np.zeros(len(regions) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in regions], out=seg[1:])
    return seg


def split_by_budget(sizes, budget: int):
    """Consecutive index ranges [(lo, hi)] whose sizes sum to at most `budget` each (a single
    stream above the budget gets a range of its own)."""
    out, lo, acc = [], 0, 0
    for i, n in enumerate(sizes):
        if i > lo and acc + n > budget:
            out.append((lo, i))
            lo, acc = i, 0
        acc += n
    if lo < len(sizes):
        out.append((lo, len(sizes)))
    return out


def check_agreement(infos) -> tuple[int, int]:
    """(channels, sample_size) of the streams that opened; ValueError where they disagree."""
    kinds = sorted({(si.channels, si.sample_size) for si in infos if si is not None})
    if len(kinds) > 1:
        raise ValueError(f"streams of one batch must agree on (channels, sample size), got {kinds}: use decode_files")
    return kinds[0] if kinds else (1, 16)


def group_by_kind(infos):
    """{(channels, sample_size) or None: [input indices]} in first-appearance order."""
    groups = {}
    for i, si in enumerate(infos):
        groups.setdefault(None if si is None else (si.channels, si.sample_size), []).append(i)
    return groups


def _torch_dtype(dtype: str):
    import torch
    return {"int16": torch.int16, "int32": torch.int32, "float32": torch.float32}[dtype]


def _device_call(az, regions, lo, hi, channels, sample_size, max_block_size, dtype, check_crc, spec_wasted_bits, out,
                 stats):
    """One flacmi_decode_batch_host + fetch over regions[lo:hi]; splits in two where pass 1's rows
    would exceed the library's bound.  -> [(lo, hi, tensor [hi - lo, C, T], results)]"""
    import torch
    from ._lib import FlacmiError
    seg = seg_offsets(regions[lo:hi])
    packed = np.frombuffer(b"".join(regions[lo:hi]), dtype=np.uint8)
    try:
        res, summary = az.decode_batch(packed.ctypes.data if packed.size else None, seg, channels, sample_size, check_crc,
                                       max_block_size, spec_wasted_bits)
    except FlacmiError as e:
        if e.code != abi.E_UNSUPPORTED or hi - lo < 2 or out is not None:
            raise
        mid = (lo + hi) // 2
        return (_device_call(az, regions, lo, mid, channels, sample_size, max_block_size, dtype, check_crc,
                             spec_wasted_bits, None, stats) +
                _device_call(az, regions, mid, hi, channels, sample_size, max_block_size, dtype, check_crc,
                             spec_wasted_bits, None, stats))
    dev = torch.device("cuda", az.device)
    group = 16 // (2 if dtype == "int16" else 4)
    pitch = (int(summary.max_samples) + group - 1) // group * group
    if out is None:
        out = torch.empty((hi - lo, channels, pitch), dtype=_torch_dtype(dtype), device=dev)
    elif (tuple(out.shape[:2]) != (hi - lo, channels) or out.shape[2] < pitch or out.shape[2] % group or
          out.dtype != _torch_dtype(dtype) or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"out must be a contiguous {dtype} tensor [{hi - lo}, {channels}, T >= {pitch}] on {dev}, "
                         f"T a multiple of {group}")
    if out.shape[2] > 0:
        stream = torch.cuda.current_stream(dev)
        az.batch_fetch(out.data_ptr(), out.shape[2], dtype, res, stream=stream.cuda_stream)
        stream.synchronize()  # the list's rows are the context's: its next decode call reuses them
    stats.append({f: getattr(summary, f) for f, _ in abi.BatchSummary._fields_ if f != "reserved"} |
                 {"streams": hi - lo, "bytes": int(seg[-1]), "pitch": int(out.shape[2])})
    return [(lo, hi, out, res)]


def decode_batch(streams, dtype: str = "int32", device: int = 0, check_crc: bool = False,
                 spec_wasted_bits: bool = False, byte_budget: int = DEFAULT_BYTE_BUDGET, out=None) -> BatchResult:
    """streams: bytes objects or paths of whole .flac streams that agree on channels and sample
    size (ValueError otherwise, before any device work).  dtype "int16" (a sample outside 16 bits
    stops its stream at that frame with OverflowError), "int32" or "float32" (x * 2^-(sample_size
    - 1)).  out: an optional preallocated tensor [N, C, T] (one device call only)."""
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {DTYPES}")
    infos, regions, errors = open_streams(streams)
    channels, sample_size = check_agreement(infos)
    return _decode_opened(infos, regions, errors, channels, sample_size, dtype, device, check_crc, spec_wasted_bits,
                          byte_budget, out)


def _decode_opened(infos, regions, errors, channels, sample_size, dtype, device, check_crc, spec_wasted_bits,
                   byte_budget, out) -> BatchResult:
    import torch
    n = len(infos)
    blocks = [si.max_block_size for si in infos if si is not None]
    max_block_size = 0 if (not blocks or min(blocks) == 0) else max(blocks)
    stats, parts = [], []
    ranges = split_by_budget([len(r) for r in regions], byte_budget)
    if out is not None and len(ranges) > 1:
        raise ValueError("out= needs the whole batch in one device call: raise byte_budget")
    az = _analyzer(device) if n else None
    for lo, hi in ranges:
        parts += _device_call(az, regions, lo, hi, channels, sample_size, max_block_size, dtype, check_crc,
                              spec_wasted_bits, out, stats)
    lengths = [0] * n
    for lo, hi, _, res in parts:
        for k in range(hi - lo):
            r = res[k]
            lengths[lo + k] = int(r.samples)
            if errors[lo + k] is None and r.status:
                errors[lo + k] = stop_exception(r.status, r.site, int(r.frames))
    if len(parts) == 1:
        data = parts[0][2]
    else:
        dev = torch.device("cuda", device)
        pitch = max([p[2].shape[2] for p in parts], default=0)
        data = torch.zeros((n, channels, pitch), dtype=_torch_dtype(dtype), device=dev)
        for lo, hi, t, _ in parts:
            data[lo:hi, :, :t.shape[2]] = t
    return BatchResult(data=data, lengths=lengths, sample_rates=[None if si is None else si.sample_rate for si in infos],
                       errors=errors, channels=channels, sample_size=sample_size, stats=stats)


def auto_dtype(sample_size: int) -> str:
    """What a WAV of this sample size holds: int16 rows for 16-bit streams, else int32."""
    return "int16" if sample_size == 16 else "int32"


def decode_files(paths, dtype: str = "auto", device: int = 0, check_crc: bool = False, spec_wasted_bits: bool = False,
                 byte_budget: int = DEFAULT_BYTE_BUDGET) -> list:
    """Any mix of streams: one decode_batch per (channels, sample size) group, the results in input
    order.  dtype "auto": auto_dtype of each group."""
    if dtype != "auto" and dtype not in DTYPES:
        raise ValueError(f"dtype must be \"auto\" or one of {DTYPES}")
    infos, regions, errors = open_streams(paths)
    results = [None] * len(infos)
    for kind, idx in group_by_kind(infos).items():
        if kind is None:
            for i in idx:
                results[i] = DecodedStream(None, 0, None, None, None, errors[i])
            continue
        r = _decode_opened([infos[i] for i in idx], [regions[i] for i in idx], [None] * len(idx), kind[0], kind[1],
                           auto_dtype(kind[1]) if dtype == "auto" else dtype, device, check_crc, spec_wasted_bits,
                           byte_budget, None)
        for k, i in enumerate(idx):
            results[i] = DecodedStream(r.data[k], r.lengths[k], r.sample_rates[k], kind[0], kind[1], r.errors[k],
                                       infos[i])
    return results
