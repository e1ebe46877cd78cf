"""Command line with flac/__main__.py's `encode` and `decode` actions (their arguments,
defaults and output bytes), on the device path, and `analyze`, the per-frame report flac-py's
README wishes for ("a tool providing information about a FLAC file, as `flac -a` does").  encode: streamed PCM ingest (ingest.iter_wav_pcm, the
reference reader's byte grouping unless --correct-reader), device analysis and device
frame writer through the streaming pipeline (encoder.encode_wav); --devices spreads the
batches over several GPUs.

    python -m flac_amd encode infile.wav outfile.flac [-b N] [-l N] [-q N] [-r [M,]N]
                                                       [--correct-reader] [--fixed-only] [--fallback] [--stereo]
                                                       [--lpc-sign] [--wasted-bits] [--rice-search] [--size-choice]
                                                       [--device N | --devices N,M,...]

    python -m flac_amd decode infile.flac outfile.wav [--device N] [--check-crc]

decode (__main__.py:27-55 cmd_decode): the stream's frames are found, decoded, interleaved and
packed on the device (decoder.decode_wav over flacmi_decode_stream_host) and written through
the wave module as the reference does; --check-crc also verifies CRC-8 / CRC-16, which the
reference reads unchecked.

    python -m flac_amd decode-many --out-dir DIR in1.flac in2.flac ... [--device N] [--check-crc] [--spec-wasted-bits]

decode-many (flac_amd.batch over flacmi_decode_batch_host): the inputs grouped by (channels, sample
size) and each group decoded in one device call into planar rows; one DIR/<input name>.wav per
input, byte-identical to what decode writes for that file.  Where a stream stops, its WAV holds the
frames before the stop, a `stopped` line on stderr names the file and the exception, the other
streams go on, and the exit status is 1.  16-bit groups come back as range-checked int16 rows; every
other sample size as int32 rows packed on the host, and a file of those that holds a sample outside
its width (to_bytes raises OverflowError) is decoded a second time alone through decode's path, whose
PCM kernel stops it at that frame.

    python -m flac_amd recompress infile.flac outfile.flac [-b N] [-l N] [-q N] [-r [M,]N]
                                                            [--fixed-only] [--fallback] [--stereo] [--lpc-sign]
                                                            [--wasted-bits] [--rice-search] [--size-choice]
                                                            [--check-crc] [--spec-wasted-bits] [--keep-metadata]
                                                            [--device N]

recompress (flac_amd.recompress over flacmi_recompress_host): the stream decoded and encoded again
with encode's parameters and mode switches, its samples never leaving the device; --keep-metadata
copies the input's metadata blocks (but a SEEKTABLE) and its MD5.  Where the input stops or a block
cannot be written, what was produced before is written, the exception is printed and the exit
status is 1.

    python -m flac_amd analyze infile.flac [--partitions] [--json] [--summary-only] [--device N]

analyze (flac_amd.info over flacmi_info_stream_host): tab-separated key=value lines in stream
order, one per metadata block, one per frame (frame=, offset=, bytes=, blocksize=, sample_rate=,
sample_size=, channel_assignment=, number=, crc8=ok|BAD, crc16=ok|BAD) and one indented line per
subframe (subframe=, type=, order=, wasted_bits=, bits=, and where they apply precision=, shift=,
coefficients=, residual_type=, partition_order=, abs_sum=; --partitions adds the Rice parameters,
an escaped partition as e<width>), then the summary block.  --json writes one JSON object per
line instead.  Where the reference would raise inside a frame, a `stopped` line names the frame
and the exception after the summary, and the exit status is 1.
"""
import argparse
import sys
from pathlib import Path
from timeit import default_timer as timer

from .utils import argparse_range

DEFAULT_BLOCK_SIZE = 4608
DEFAULT_MAX_LPC_ORDER = 12
DEFAULT_QLP_COEFF_PRECISION = 5
DEFAULT_RICE_PARTITION_ORDER = "5"


def make_argument_parser():
    parser = argparse.ArgumentParser(prog="flac_amd", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    action = parser.add_subparsers(title="action", dest="action", required=True)
    enc = action.add_parser("encode", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    enc.add_argument("infile", type=Path, metavar="infile.wav")
    enc.add_argument("outfile", type=Path, metavar="outfile.flac")
    enc.add_argument("-b", "--block-size", type=int, default=DEFAULT_BLOCK_SIZE, metavar="N")
    enc.add_argument("-l", "--max-lpc-order", type=int, default=DEFAULT_MAX_LPC_ORDER, metavar="N")
    enc.add_argument("-q", "--qlp-coeff-precision", type=int, default=DEFAULT_QLP_COEFF_PRECISION, metavar="N")
    enc.add_argument("-r", "--rice-partition-order", type=argparse_range, default=DEFAULT_RICE_PARTITION_ORDER,
                     metavar="[M,]N")
    enc.add_argument("--correct-reader", action="store_true",
                     help="read sampwidth-byte samples (the reference groups frame bytes by channel count)")
    enc.add_argument("--fixed-only", action="store_true", help="fixed predictors only (BASELINE config 5)")
    enc.add_argument("--fallback", action="store_true",
                     help="write a subframe the reference cannot write (digital silence, ...) or writes larger "
                          "than raw as CONSTANT / VERBATIM instead of stopping at its frame")
    enc.add_argument("--stereo", action="store_true",
                     help="stereo decorrelation (two-channel input): every frame takes the smallest of the "
                          "left/right, left/side, side/right and mid/side channel assignments")
    enc.add_argument("--lpc-sign", action="store_true",
                     help="corrected LPC predictor sign: the LPC candidates predict x and not -x (the "
                          "reference's levinson_durbin returns the negated predictor)")
    enc.add_argument("--wasted-bits", action="store_true",
                     help="wasted-bits subframes: a block whose samples share w zero low bits (16-bit audio in a "
                          "24-bit file) is written at w bits less a sample; read back with decode --spec-wasted-bits")
    enc.add_argument("--rice-search", action="store_true",
                     help="exact Rice search: every partition takes the parameter that makes it smallest (the "
                          "reference's floor(log2(mean)) has no value for a stretch of digital silence)")
    enc.add_argument("--size-choice", action="store_true",
                     help="choose each subframe's predictor by the exact bits it takes to write and not by the "
                          "magnitude of its residual (needs --rice-search)")
    enc.add_argument("--device", type=int, default=0)
    enc.add_argument("--devices", type=lambda v: [int(x) for x in v.split(",")], default=None, metavar="N,M,...",
                     help="encode on these devices, batches round-robin (frames in block order)")
    dec = action.add_parser("decode", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    dec.add_argument("infile", type=Path, metavar="infile.flac")
    dec.add_argument("outfile", type=Path, metavar="outfile.wav")
    dec.add_argument("--device", type=int, default=0)
    dec.add_argument("--check-crc", action="store_true",
                     help="verify the frames' CRC-8 and CRC-16 (the reference reads them unchecked)")
    dec.add_argument("--spec-wasted-bits", action="store_true",
                     help="read a subframe's wasted bits as the format codes them and shift them back in (the "
                          "reference reads one too few and leaves the samples unshifted)")
    many = action.add_parser("decode-many", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    many.add_argument("infiles", type=Path, nargs="+", metavar="in.flac")
    many.add_argument("--out-dir", type=Path, required=True, metavar="DIR")
    many.add_argument("--device", type=int, default=0)
    many.add_argument("--check-crc", action="store_true", help="verify the frames' CRC-8 and CRC-16")
    many.add_argument("--spec-wasted-bits", action="store_true",
                      help="read wasted bits as the format codes them and shift them back in")
    rec = action.add_parser("recompress", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    rec.add_argument("infile", type=Path, metavar="infile.flac")
    rec.add_argument("outfile", type=Path, metavar="outfile.flac")
    rec.add_argument("-b", "--block-size", type=int, default=DEFAULT_BLOCK_SIZE, metavar="N")
    rec.add_argument("-l", "--max-lpc-order", type=int, default=DEFAULT_MAX_LPC_ORDER, metavar="N")
    rec.add_argument("-q", "--qlp-coeff-precision", type=int, default=DEFAULT_QLP_COEFF_PRECISION, metavar="N")
    rec.add_argument("-r", "--rice-partition-order", type=argparse_range, default=DEFAULT_RICE_PARTITION_ORDER,
                     metavar="[M,]N")
    for flag, text in (("--fixed-only", "fixed predictors only"),
                       ("--fallback", "CONSTANT / VERBATIM subframes where the reference cannot write one"),
                       ("--stereo", "stereo decorrelation (two-channel input)"),
                       ("--lpc-sign", "corrected LPC predictor sign"),
                       ("--wasted-bits", "wasted-bits subframes"),
                       ("--rice-search", "exact Rice search"),
                       ("--size-choice", "subframe choice by exact written size (needs --rice-search)")):
        rec.add_argument(flag, action="store_true", help=text + " (as encode's switch)")
    rec.add_argument("--check-crc", action="store_true", help="verify the input frames' CRC-8 and CRC-16")
    rec.add_argument("--spec-wasted-bits", action="store_true",
                     help="read the input's wasted bits as the format codes them and shift them back in")
    rec.add_argument("--keep-metadata", action="store_true",
                     help="copy the input's metadata blocks (all but a SEEKTABLE) and its MD5 signature")
    rec.add_argument("--device", type=int, default=0)
    ana = action.add_parser("analyze", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ana.add_argument("infile", type=Path, metavar="infile.flac")
    ana.add_argument("--partitions", action="store_true", help="list every subframe's Rice parameters")
    ana.add_argument("--json", action="store_true", help="one JSON object per line instead of key=value text")
    ana.add_argument("--summary-only", action="store_true", help="no metadata, frame and subframe lines")
    ana.add_argument("--device", type=int, default=0)
    ana.add_argument("--spec-wasted-bits", action="store_true",
                     help="report wasted bits and subframe sample widths as the format codes them")
    return parser


def cmd_analyze(args) -> int:
    import json
    from . import info
    report = info.analyze(args.infile, device=args.device, spec_wasted_bits=args.spec_wasted_bits)
    out = sys.stdout
    if not args.summary_only:
        if args.json:
            si = report.streaminfo
            out.write(json.dumps({"streaminfo": {k: (v.hex() if isinstance(v, bytes) else v) for k, v in vars(si).items()},
                                  "first_frame_offset": report.first_frame_offset}) + "\n")
            for k, (t, length, offset, last) in enumerate(report.metadata):
                out.write(json.dumps({"metadata": k, "type": t.name.upper(), "length": length, "offset": offset,
                                      "last": int(last)}) + "\n")
        else:
            out.write("".join(ln + "\n" for ln in info.format_metadata(report.metadata)))
    frames = []
    try:
        for fr in report.frames:
            frames.append(fr)
            if args.summary_only:
                continue
            if args.json:
                out.write(json.dumps({"frame": info.frame_json(fr)}) + "\n")
            else:
                out.write("".join(ln + "\n" for ln in info.format_frame(fr, report.streaminfo, args.partitions)))
    except Exception as e:  # noqa: BLE001  -- reported after the summary of the frames before it
        report.exception = e
    summary = info.summarize(report, frames)
    if args.json:
        out.write(json.dumps({"summary": info.summary_json(summary)}) + "\n")
    else:
        out.write("".join(ln + "\n" for ln in info.format_summary(summary)))
    if report.exception is not None:
        e = report.exception
        if args.json:
            out.write(json.dumps({"stopped": {"frame": len(frames), "exception": type(e).__name__, "message": str(e)}}) + "\n")
        else:
            out.write(f"stopped\tframe={len(frames)}\texception={type(e).__name__}\tmessage={e}\n")
        return 1
    return 0


def cmd_decode(args) -> None:
    from .decoder import decode_wav
    seconds = decode_wav(args.infile, args.outfile, device=args.device, check_crc=args.check_crc,
                         spec_wasted_bits=args.spec_wasted_bits)
    print(f"Decoding completed in {seconds:.6g} seconds")


def cmd_decode_many(args) -> int:
    from wave import open as wave_open

    import numpy as np

    from . import batch
    from .decoder import decode_pcm
    names = [p.with_suffix(".wav").name for p in args.infiles]
    if len(set(names)) != len(names):
        raise SystemExit("decode-many: two inputs would write the same file in --out-dir")
    args.out_dir.mkdir(parents=True, exist_ok=True)
    t0 = timer()
    results = batch.decode_files(args.infiles, dtype="auto", device=args.device, check_crc=args.check_crc,
                                 spec_wasted_bits=args.spec_wasted_bits)
    failed = 0
    for path, name, r in zip(args.infiles, names, results):
        error = r.error
        if r.data is None or r.sample_size % 8:
            # Python's wave module doesn't handle sample sizes that are not multiple of a byte.
            error = error or AssertionError(f"sample size {r.sample_size}")
            pcm = None
        else:
            B = r.sample_size // 8
            x = r.data[:, :r.length].cpu().numpy().T  # [length][channels]: decoder.py:52 zip(*samples)
            if B == 2:
                pcm = np.ascontiguousarray(x, dtype="<i2").tobytes()
            else:
                if B < 4 and x.size and (x.min() < -(1 << (8 * B - 1)) or x.max() >= 1 << (8 * B - 1)):
                    # to_bytes raises OverflowError: the stream alone, whose PCM kernel stops at that frame
                    pcm, error = b"", None
                    try:
                        for bs in decode_pcm(path, device=args.device, check_crc=args.check_crc,
                                             spec_wasted_bits=args.spec_wasted_bits)[4]:
                            pcm += bs
                    except Exception as e:  # noqa: BLE001
                        error = e
                else:
                    pcm = np.ascontiguousarray(x, dtype="<i4").view(np.uint8).reshape(-1, 4)[:, :B].tobytes()
        if pcm is not None:
            info = r.streaminfo
            with wave_open(str(args.out_dir / name), mode="wb") as w:
                w.setframerate(info.sample_rate)
                w.setsampwidth(info.sample_size // 8)
                w.setnchannels(info.channels)
                w.setnframes(info.samples)
                w.writeframes(pcm)
        if error is not None:
            failed += 1
            print(f"stopped\tfile={path}\texception={type(error).__name__}\tmessage={error}", file=sys.stderr)
    print(f"Decoding of {len(results)} streams completed in {timer() - t0:.6g} seconds, {failed} stopped")
    return 1 if failed else 0


def cmd_recompress(args) -> int:
    from .encoder import EncoderParameters
    from .recompress import recompress
    parameters = EncoderParameters(block_size=args.block_size, lpc_order=range(args.max_lpc_order + 1),
                                   qlp_precision=args.qlp_coeff_precision,
                                   rice_partition_order=args.rice_partition_order)
    t0 = timer()
    with args.outfile.open("wb") as f:
        try:
            for bs in recompress(args.infile, parameters, device=args.device, check_crc=args.check_crc,
                                 spec_wasted_bits=args.spec_wasted_bits, keep_metadata=args.keep_metadata,
                                 fixed_only=args.fixed_only, fallback=args.fallback, stereo=args.stereo,
                                 lpc_sign=args.lpc_sign, wasted=args.wasted_bits, rice_search=args.rice_search,
                                 size_choice=args.size_choice):
                f.write(bs)
        except Exception as e:  # noqa: BLE001  -- what was produced before it is written, as analyze reports
            print(f"stopped\texception={type(e).__name__}\tmessage={e}")
            return 1
    print(f"Recompression completed in {timer() - t0:.6g} seconds")
    return 0


def cmd_encode(args) -> None:
    from .encoder import EncoderParameters, encode_wav
    parameters = EncoderParameters(block_size=args.block_size, lpc_order=range(args.max_lpc_order + 1),
                                   qlp_precision=args.qlp_coeff_precision,
                                   rice_partition_order=args.rice_partition_order)
    t0 = timer()
    with args.outfile.open("wb") as f:
        for bs in encode_wav(args.infile, parameters, quirk=not args.correct_reader, device=args.device,
                             devices=args.devices, fixed_only=args.fixed_only, fallback=args.fallback,
                             stereo=args.stereo, lpc_sign=args.lpc_sign, wasted=args.wasted_bits,
                             rice_search=args.rice_search, size_choice=args.size_choice):
            f.write(bs)
    print(f"Encoding completed in {timer() - t0:.6g} seconds")


def main(argv=None) -> int:
    args = make_argument_parser().parse_args(argv)
    if args.action == "encode":
        cmd_encode(args)
    if args.action == "decode":
        cmd_decode(args)
    if args.action == "decode-many":
        return cmd_decode_many(args)
    if args.action == "recompress":
        return cmd_recompress(args)
    if args.action == "analyze":
        return cmd_analyze(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
