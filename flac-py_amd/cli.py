"""Command line with flac/__main__.py's `encode` and `decode` actions (their arguments,
defaults and output bytes), on the device path.  encode: streamed PCM ingest (ingest.iter_wav_pcm, the
reference reader's byte grouping unless --correct-reader), device analysis and device
frame writer through the streaming pipeline (encoder.encode_wav); --devices spreads the
batches over several GPUs.

    python -m flac_amd encode infile.wav outfile.flac [-b N] [-l N] [-q N] [-r [M,]N]
                                                       [--correct-reader] [--fixed-only] [--fallback] [--stereo]
                                                       [--lpc-sign]
                                                       [--device N | --devices N,M,...]

    python -m flac_amd decode infile.flac outfile.wav [--device N] [--check-crc]

decode (__main__.py:27-55 cmd_decode): the stream's frames are found, decoded, interleaved and
packed on the device (decoder.decode_wav over flacmi_decode_stream_host) and written through
the wave module as the reference does; --check-crc also verifies CRC-8 / CRC-16, which the
reference reads unchecked.
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
    enc.add_argument("--device", type=int, default=0)
    enc.add_argument("--devices", type=lambda v: [int(x) for x in v.split(",")], default=None, metavar="N,M,...",
                     help="encode on these devices, batches round-robin (frames in block order)")
    dec = action.add_parser("decode", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    dec.add_argument("infile", type=Path, metavar="infile.flac")
    dec.add_argument("outfile", type=Path, metavar="outfile.wav")
    dec.add_argument("--device", type=int, default=0)
    dec.add_argument("--check-crc", action="store_true",
                     help="verify the frames' CRC-8 and CRC-16 (the reference reads them unchecked)")
    return parser


def cmd_decode(args) -> None:
    from .decoder import decode_wav
    seconds = decode_wav(args.infile, args.outfile, device=args.device, check_crc=args.check_crc)
    print(f"Decoding completed in {seconds:.6g} seconds")


def cmd_encode(args) -> None:
    from .encoder import EncoderParameters, encode_wav
    parameters = EncoderParameters(block_size=args.block_size, lpc_order=range(args.max_lpc_order + 1),
                                   qlp_precision=args.qlp_coeff_precision,
                                   rice_partition_order=args.rice_partition_order)
    t0 = timer()
    with args.outfile.open("wb") as f:
        for bs in encode_wav(args.infile, parameters, quirk=not args.correct_reader, device=args.device,
                             devices=args.devices, fixed_only=args.fixed_only, fallback=args.fallback,
                             stereo=args.stereo, lpc_sign=args.lpc_sign):
            f.write(bs)
    print(f"Encoding completed in {timer() - t0:.6g} seconds")


def main(argv=None) -> int:
    args = make_argument_parser().parse_args(argv)
    if args.action == "encode":
        cmd_encode(args)
    if args.action == "decode":
        cmd_decode(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
