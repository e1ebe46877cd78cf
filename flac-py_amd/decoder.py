"""flac/decoder.py's `decode` on the device: .flac bytes in, samples or interleaved PCM out.

The stream's metadata is read on the host exactly as the reference reads it
(decoder.py:36-44, 68-96, with the same assertions); the frames go through
flacmi_decode_stream_host chunk by chunk: the device lists the candidate frame starts,
decodes all of them, the host walks the chain of true frames, and the device interleaves
and packs their samples (include/flacmi.h, "stream decoder").

    decode(buffer)                      the reference's signature and return tuple
    decode_pcm(buffer_or_path, ...)     stream parameters + chunks of interleaved PCM bytes
    decode_wav(path_in, path_out, ...)  __main__.py:27-55 cmd_decode

Where the reference raises inside a frame, every sample of the frames before it is
delivered first, then the same exception class is raised; the message names the site and
the frame index.  A verifier finding (check_crc=True) raises VerifyError.
"""
import os
from io import BytesIO
from timeit import default_timer as timer
from typing import Iterator

import numpy as np

from . import abi
from .binary import Get
from .common import MAGIC, MetadataBlockHeader, MetadataBlockType, Streaminfo

DEFAULT_CHUNK_BYTES = 1 << 24


class VerifyError(ValueError):
    """A check the reference does not make failed (CRC-8, CRC-16, channel count): raised only
    with check_crc=True, or for a frame this build cannot decode (see flacmi.h)."""


# ---- metadata (decoder.py:68-96) -----------------------------------------------------------

def get_metadata_block_header(get: Get) -> MetadataBlockHeader:
    return MetadataBlockHeader(last=get.bool(), type=MetadataBlockType(get.uint(7)), length=get.uint(24))


def get_metadata_block_streaminfo(get: Get) -> Streaminfo:
    return Streaminfo(min_block_size=get.uint(16), max_block_size=get.uint(16), min_frame_size=get.uint(24),
                      max_frame_size=get.uint(24), sample_rate=get.uint(20), channels=get.uint(3) + 1,
                      sample_size=get.uint(5) + 1, samples=get.uint(36), md5=get.bytes(16))


def skip_metadata(get: Get) -> None:
    while True:
        header = get_metadata_block_header(get)
        get.bytes(header.length)
        if header.last is True:
            break


def read_metadata(buffer) -> Streaminfo:
    """decoder.py:34-44: leaves `buffer` at the first frame (Get reads no byte ahead)."""
    get = Get(buffer)
    assert get.bytes(4) == MAGIC
    streaminfo_header = get_metadata_block_header(get)
    assert streaminfo_header.type == MetadataBlockType.Streaminfo
    streaminfo = get_metadata_block_streaminfo(get)
    if streaminfo_header.last is False:
        skip_metadata(get)
    return streaminfo


# ---- frames ----------------------------------------------------------------------------------

def stop_exception(status: int, site: int, frame: int) -> Exception:
    """The exception for a stopping (status, site) of flacmi_decode_stream_host."""
    name = abi.DSITE_NAMES.get(site, abi.SITE_NAMES.get(site, str(site)))
    cls = abi.STATUS_EXCEPTION.get(status, VerifyError)
    return cls(f"frame {frame}: {name}")


_ANALYZERS = {}


def _analyzer(device: int):
    """One context per device for the process, as the encoder keeps (its buffers are reused
    call after call; a context is not thread-safe: one decode at a time per device)."""
    from .analysis import Analyzer
    if device not in _ANALYZERS:
        _ANALYZERS[device] = Analyzer(device)
    return _ANALYZERS[device]


def _chunks(buffer, streaminfo: Streaminfo, raw: bool, chunk_bytes: int, device: int, check_crc: bool,
            stats, pcm_buffer_bytes: int = 0, spec_wasted_bits: bool = False) -> Iterator[bytes]:
    """Interleaved PCM of the frames at `buffer`'s position, one bytes object per call of
    flacmi_decode_stream_host; raises the stopping exception after the last good frame."""
    from ._lib import FlacmiError
    az = _analyzer(device)
    channels = streaminfo.channels
    B = 4 if raw else streaminfo.sample_size // 8
    stage = pcm = None  # page-locked, sized by the first chunk, reused chunk after chunk
    carry = b""
    final = False
    frames = 0
    while True:
        want = max(chunk_bytes - len(carry), 0)
        new = buffer.read(want) if want and not final else b""
        if want and not final and len(new) < want:
            final = True
        data = carry + new
        n = len(data)
        if n == 0:
            break
        if stage is None or n > len(stage):
            stage = az.host_array((n,), np.uint8)
        if pcm is None:
            pcm = az.host_array((pcm_buffer_bytes or max(1 << 20, min(8 * n, 1 << 28)),), np.uint8)
        stage[:n] = np.frombuffer(data, dtype=np.uint8)
        while True:
            try:
                res = az.decode_stream(stage.ctypes.data, n, 0, channels, streaminfo.sample_size, check_crc,
                                       streaminfo.max_block_size, final, pcm.ctypes.data, len(pcm), raw, B,
                                       spec_wasted_bits)
                break
            except FlacmiError as e:
                if e.code != abi.E_NOMEM or len(pcm) >= (1 << 33):
                    raise
                pcm = az.host_array((2 * len(pcm),), np.uint8)  # not even one frame fitted
        if stats is not None:
            stats.append({f: getattr(res, f) for f, _ in abi.StreamResult._fields_} | {"bytes": n, "final": final})
        if res.pcm_bytes:
            yield pcm[:res.pcm_bytes].tobytes()
        if res.status:
            raise stop_exception(res.status, res.site, frames + res.frames)
        frames += res.frames
        carry = data[res.consumed:]
        if res.pcm_full:
            continue
        if final:
            break  # the stream's end, or a cut-off last frame (get_frames' EOFError: silent)
        if res.frames == 0:
            chunk_bytes *= 2  # no whole frame in the chunk


def _open(buffer_or_path):
    if isinstance(buffer_or_path, (str, os.PathLike)):
        return open(buffer_or_path, "rb"), True
    if isinstance(buffer_or_path, (bytes, bytearray, memoryview)):
        return BytesIO(bytes(buffer_or_path)), False
    return buffer_or_path, False


def decode(buffer, check_crc: bool = False, chunk_bytes: int = DEFAULT_CHUNK_BYTES, device: int = 0,
           stats=None, pcm_buffer_bytes: int = 0,
           spec_wasted_bits: bool = False) -> tuple[int, int, int, int, Iterator[list[int]]]:
    """flac.decoder.decode (decoder.py:31-63): (sample_rate, sample_size, channels, samples,
    iterator of one list of ints per sample).  chunk_bytes: stream bytes per device call;
    pcm_buffer_bytes: the PCM staging buffer (0: sized by the first chunk; it grows when a frame
    does not fit and is drained in parts when a chunk's frames do not); stats: a list that
    receives one dict per device call (the fields of flacmi_stream_result); spec_wasted_bits:
    read a subframe's wasted bits as the format codes them and shift them back in
    (FLACMI_DECODE_WASTED_SPEC; off: the reference's reading, which does neither)."""
    buffer, _ = _open(buffer)
    streaminfo = read_metadata(buffer)

    def samples() -> Iterator[list[int]]:
        for chunk in _chunks(buffer, streaminfo, True, chunk_bytes, device, check_crc, stats, pcm_buffer_bytes,
                             spec_wasted_bits):
            yield from np.frombuffer(chunk, dtype="<i4").reshape(-1, streaminfo.channels).tolist()

    return (streaminfo.sample_rate, streaminfo.sample_size, streaminfo.channels, streaminfo.samples, samples())


def decode_pcm(buffer_or_path, chunk_bytes: int = DEFAULT_CHUNK_BYTES, device: int = 0, check_crc: bool = False,
               stats=None, pcm_buffer_bytes: int = 0,
               spec_wasted_bits: bool = False) -> tuple[int, int, int, int, Iterator[bytes]]:
    """(sample_rate, sample_size, channels, samples, iterator of interleaved little-endian PCM
    chunks): what cmd_decode writes into the WAV (__main__.py:45-50), packed on the device."""
    buffer, owned = _open(buffer_or_path)
    try:
        streaminfo = read_metadata(buffer)
        # Python's wave module doesn't handle sample sizes that are not multiple of a byte.
        assert streaminfo.sample_size % 8 == 0
    except BaseException:
        if owned:
            buffer.close()
        raise

    def chunks() -> Iterator[bytes]:
        try:
            yield from _chunks(buffer, streaminfo, False, chunk_bytes, device, check_crc, stats, pcm_buffer_bytes,
                               spec_wasted_bits)
        finally:
            if owned:
                buffer.close()

    return (streaminfo.sample_rate, streaminfo.sample_size, streaminfo.channels, streaminfo.samples, chunks())


def decode_wav(path_in, path_out, device: int = 0, check_crc: bool = False,
               chunk_bytes: int = DEFAULT_CHUNK_BYTES, spec_wasted_bits: bool = False) -> float:
    """cmd_decode (__main__.py:27-55): the WAV through the wave module; returns the seconds."""
    from wave import open as wave_open
    with open(path_in, "rb") as f, wave_open(str(path_out), mode="wb") as w:
        (sample_rate, sample_size, channels, frames, chunks) = decode_pcm(f, chunk_bytes, device, check_crc,
                                                                          spec_wasted_bits=spec_wasted_bits)
        w.setframerate(sample_rate)
        w.setsampwidth(sample_size // 8)
        w.setnchannels(channels)
        w.setnframes(frames)
        t0 = timer()
        for bs in chunks:
            w.writeframes(bs)
        return timer() - t0
