"""FLAC in, FLAC out: a stream decoded and encoded again without its samples leaving the device.

    recompress(buffer_or_path, parameters, ...)   the new stream, piece by piece
    recompress_file(path_in, path_out, ...)       the same into a file; returns the seconds

The bytes are those of

    encode(sample_rate, sample_size, channels, STREAMINFO.samples, <samples of decode(x)>,
           parameters, **modes)

whatever chunk_bytes is: the stream header first, then the frames chunk by chunk.  Each chunk
goes through flacmi_recompress_host (include/flacmi.h): the stream decoder's index, two passes
and chain walk, then k_units, which cuts the decoded rows into blocks of parameters.block_size,
then the encoder's analysis and frame writer with every opt-in mode encode() has.  Only
compressed bytes cross PCIe, and the host holds one chunk.

Where the input stops (an exception of the reference decoder, a verifier finding with
check_crc=True, a sample that does not fit the stream's sample size), the whole blocks before
the stopping frame are yielded, then the exception decoder.stop_exception builds is raised;
where a block cannot be written, the frames before it are yielded and encode()'s exception is
raised.
"""
from timeit import default_timer as timer
from typing import Iterator

import numpy as np

from . import abi
from ._lib import FlacmiError
from .analysis import frame_params
from .binary import Get
from .common import MAGIC, MetadataBlockHeader, MetadataBlockType, Streaminfo
from .decoder import (DEFAULT_CHUNK_BYTES, _open, get_metadata_block_header, get_metadata_block_streaminfo,
                      stop_exception)
from .encoder import (EncoderParameters, _check_lpc_sign, _check_rice_search, _check_size_choice, _check_stereo,
                      _check_wasted, _params, _raise_status, _release, _sessions, _stream_header,
                      put_metadata_block_header, put_metadata_block_streaminfo)

__all__ = ["recompress", "recompress_file", "read_metadata_blocks", "stream_header"]

MIN_CHUNK_BYTES = 1 << 16  # a chunk whose pass-1 rows exceed 4 GiB is halved down to this


def read_metadata_blocks(buffer) -> tuple[Streaminfo, list[tuple[int, bytes]]]:
    """decoder.read_metadata (the reference's decoder.py:34-44, same assertions) that keeps what
    it skips: (STREAMINFO, [(block type, body) of every block behind it, in order]).  Leaves
    `buffer` at the first frame."""
    get = Get(buffer)
    assert get.bytes(4) == MAGIC
    header = get_metadata_block_header(get)
    assert header.type == MetadataBlockType.Streaminfo
    streaminfo = get_metadata_block_streaminfo(get)
    blocks = []
    while header.last is False:
        header = get_metadata_block_header(get)
        blocks.append((header.type.value, get.bytes(header.length)))
    return streaminfo, blocks


def stream_header(streaminfo: Streaminfo, parameters: EncoderParameters, blocks=None) -> Iterator[bytes]:
    """The new stream's header.  blocks None: exactly encode()'s (_stream_header: one STREAMINFO,
    md5 zero).  Otherwise (keep_metadata) STREAMINFO carries the input's md5 (the audio is
    unchanged, so the signature stays true) and every given block follows byte for byte, in
    order, except SEEKTABLE (type 3), whose offsets are no longer true; the `last` flags are
    redone."""
    if blocks is None:
        yield from _stream_header(streaminfo.sample_rate, streaminfo.sample_size, streaminfo.channels,
                                  streaminfo.samples, parameters)
        return
    kept = [(t, body) for t, body in blocks if t != MetadataBlockType.Seektable.value]
    yield MAGIC
    yield put_metadata_block_header(
        MetadataBlockHeader(last=not kept, type=MetadataBlockType.Streaminfo, length=34)).buffer
    yield put_metadata_block_streaminfo(Streaminfo(
        min_block_size=parameters.block_size, max_block_size=parameters.block_size, min_frame_size=0,
        max_frame_size=0, sample_rate=streaminfo.sample_rate, channels=streaminfo.channels,
        sample_size=streaminfo.sample_size, samples=streaminfo.samples, md5=streaminfo.md5)).buffer
    for k, (t, body) in enumerate(kept):
        yield put_metadata_block_header(
            MetadataBlockHeader(last=k == len(kept) - 1, type=MetadataBlockType(t), length=len(body))).buffer
        yield body


def _frames(buffer, streaminfo: Streaminfo, parameters: EncoderParameters, params: abi.Params, device: int,
            chunk_bytes: int, check_crc: bool, spec_wasted_bits: bool, fallback: bool, stereo: bool, wasted: bool,
            stats) -> Iterator[bytes]:
    """The new frames of the frames at `buffer`'s position, one flacmi_recompress_host call per
    chunk; the context (its carry and block counter) is held until the generator ends."""
    held = _sessions(device, None)
    try:
        az = held[0].az
        fp = frame_params(streaminfo.channels, streaminfo.sample_size, params.qlp_precision, 0, fallback,
                          stereo=stereo, wasted=wasted)
        stage = None  # page-locked, reused chunk after chunk
        outbuf = [az.host_array((1 << 16,), np.uint8)]  # the same for the frames

        def out_alloc(nbytes: int) -> np.ndarray:
            if nbytes > len(outbuf[0]):
                outbuf[0] = az.host_array((nbytes + nbytes // 4,), np.uint8)
            return outbuf[0]
        pending = b""
        final = False
        restart = True
        frames_in = 0
        while True:
            if not final and len(pending) < chunk_bytes:
                want = chunk_bytes - len(pending)
                new = buffer.read(want)
                final = len(new) < want  # only a short read says the stream has ended
                pending += new
            n = min(len(pending), chunk_bytes)
            last = final and n == len(pending)
            if stage is None or n > len(stage):
                stage = az.host_array((max(n, 1),), np.uint8)
            stage[:n] = np.frombuffer(pending, dtype=np.uint8, count=n)
            try:
                res, out, offsets, status = az.recompress_chunk(
                    stage.ctypes.data, n, 0, streaminfo.channels, streaminfo.sample_size, check_crc,
                    streaminfo.max_block_size, last, restart, parameters.block_size, params, fp, spec_wasted_bits,
                    out_alloc)
            except FlacmiError as e:
                if e.code != abi.E_UNSUPPORTED or chunk_bytes // 2 < MIN_CHUNK_BYTES:
                    raise
                chunk_bytes //= 2  # the candidates' rows exceed 4 GiB: the same bytes in smaller chunks
                continue
            restart = False
            if stats is not None:
                stats.append({f: getattr(res, f) for f, _ in abi.RecompressResult._fields_ if f != "reserved"}
                             | {"bytes": n, "final": last})
            data = out.tobytes()
            for b in range(len(status)):
                st = int(status[b])
                _raise_status(st & 0xFFFF, st >> 16)  # encode()'s exception, after the frames before it
                yield data[int(offsets[b]):int(offsets[b + 1])]
            if res.status:
                raise stop_exception(res.status, res.site, frames_in + res.frames)
            frames_in += res.frames
            pending = pending[res.consumed:]
            if last:
                break  # the stream's end, or a cut-off last frame (get_frames' EOFError: silent)
            if res.frames == 0 and n >= chunk_bytes:
                chunk_bytes *= 2  # no whole frame in the chunk
    finally:
        _release(held)


def recompress(buffer_or_path, parameters: EncoderParameters, *, device: int = 0,
               chunk_bytes: int = DEFAULT_CHUNK_BYTES, check_crc: bool = False, spec_wasted_bits: bool = False,
               keep_metadata: bool = False, fixed_only: bool = False, fallback: bool = False, stereo: bool = False,
               lpc_sign: bool = False, wasted: bool = False, rice_search: bool = False, size_choice: bool = False,
               stats=None) -> Iterator[bytes]:
    """The stream at buffer_or_path (bytes, a binary file object or a path) encoded again with
    `parameters` and encode()'s opt-in modes (fixed_only, fallback, stereo, lpc_sign, wasted,
    rice_search, size_choice: same meaning, same refusals, made before any device work since
    STREAMINFO names the channel count).  check_crc, spec_wasted_bits: how the input is read
    (decoder.decode).  chunk_bytes: input bytes per device call; the output does not depend on
    it.  keep_metadata: copy the input's metadata blocks and md5 (stream_header); off, the
    output equals encode() of the decoded samples.  stats: a list that receives one dict per
    device call (the fields of flacmi_recompress_result, sample_bits among them)."""
    buffer, owned = _open(buffer_or_path)
    try:
        streaminfo, blocks = read_metadata_blocks(buffer)
        _check_lpc_sign(lpc_sign, fixed_only)
        _check_rice_search(rice_search, parameters)
        _check_size_choice(size_choice, rice_search, wasted, parameters)
        _check_stereo(stereo, streaminfo.channels)
        _check_wasted(wasted, stereo)
        if streaminfo.sample_rate <= 48_000:
            assert parameters.lpc_order.stop <= 13
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be positive")
        yield from stream_header(streaminfo, parameters, blocks if keep_metadata else None)
        params = _params(parameters, fixed_only, lpc_sign, rice_search, size_choice)
        yield from _frames(buffer, streaminfo, parameters, params, device, chunk_bytes, check_crc, spec_wasted_bits,
                           fallback, stereo, wasted, stats)
    finally:
        if owned:
            buffer.close()


def recompress_file(path_in, path_out, parameters: EncoderParameters, **kwargs) -> float:
    """recompress(path_in, ...) written to path_out as it is produced (what was written before
    an exception stays); returns the seconds."""
    t0 = timer()
    with open(path_out, "wb") as f:
        for piece in recompress(path_in, parameters, **kwargs):
            f.write(piece)
    return timer() - t0
