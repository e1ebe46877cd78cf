"""Price and gain of the stereo-decorrelation mode (FLACMI_STEREO_BEST, include/flacmi.h) on a
config-2-shaped stereo input (4608-sample int16 blocks, two channels, -l 12 -q 5 -r 0,5):

    python tools/bench_stereo.py [--frames 100000] [--reps 5] [--out FILE.json]

The input is made on the device from flacmi_synth_device units A (unit 2f) and B (unit 2f + 1):
left = A >> 1, right = left + (B >> 4), so the channels correlate and the side signal is the
quieter independent unit.  flacmi_encode_pipeline runs over page-locked host rows, the same call
with the mode off and on, alternated --reps times after a warm-up of each.  Prints one JSON
line: per setting the wall time of the call and the pipeline's own HIP-event times of its steps
(analysis, which in the mode holds k_stereo_rows and the three analyses; choice + sizes + scan;
frame writing) as the sorted list over the reps with median and min-max, the frames written,
the output bytes and the channel codes chosen; and k_stereo_rows alone (flacmi_stereo_rows_device
over the device rows, HIP events around each launch): ms and TB/s over its algorithmic bytes
(two rows read, the mid row and the int32 side row written), to set beside the 5.4-5.6 TB/s copy
rate of tools/experiments/stream_floor.hip.  Kernel times by name come from a
separate run under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_stereo.py --reps 2
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def summary(values):
    v = sorted(round(x, 4) for x in values)
    return {"all": v, "median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from flac_amd.analysis import Analyzer, device_batch, make_params, unit_stride

    n, bits, nf = 4608, 16, args.frames
    az = Analyzer(0)
    dev = torch.device("cuda", 0)
    stride = unit_stride(n, 2)
    g = torch.empty((2 * nf, stride), dtype=torch.int16, device=dev)
    az.synth_device(g.data_ptr(), 2, bits, stride, 0, 2 * nf, n, args.seed)
    torch.cuda.synchronize(dev)
    g[0::2] >>= 1                       # left = A >> 1
    g[1::2] >>= 4                       # B >> 4, the quieter independent unit
    g[1::2] += g[0::2]                  # right = left + (B >> 4): |right| < 2^14 + 2^11
    g[:, n:] = 0

    # k_stereo_rows alone
    side_stride = unit_stride(n, 4)
    mid = torch.empty((nf, stride), dtype=torch.int16, device=dev)
    side = torch.empty((nf, side_stride), dtype=torch.int32, device=dev)
    lr = device_batch(g.data_ptr(), 2, bits, stride, 2 * nf, n)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows_ms = []
    for i in range(3 + 20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        az.stereo_rows_device(lr, mid.data_ptr(), stride, side.data_ptr(), side_stride, stream)
        e1.record()
        torch.cuda.synchronize(dev)
        if i >= 3:
            rows_ms.append(e0.elapsed_time(e1))
    left, right = g[0::2, :n].to(torch.int32), g[1::2, :n].to(torch.int32)
    assert torch.equal(mid[:, :n].to(torch.int32), (left + right) >> 1) and torch.equal(side[:, :n], left - right)
    del left, right, mid, side
    algorithmic = nf * n * (2 + 2 + 2 + 4)  # two int16 rows in, the int16 mid and the int32 side out
    rows = summary(rows_ms)
    rows["algorithmic_bytes"] = algorithmic
    rows["tb_per_s_at_median"] = round(algorithmic / (rows["median"] * 1e-3) / 1e12, 3)
    rows["tb_per_s_at_min"] = round(algorithmic / (rows["min"] * 1e-3) / 1e12, 3)

    host = az.host_array((2 * nf, stride), np.int16)
    host[:] = g.cpu().numpy()
    del g
    out = az.host_array((nf * (2 * n * 2 + 128),), np.uint8)
    params = make_params(12, 5, 0, 5)
    kw = dict(sample_bits=bits, channels=2, sample_size=bits, out=out)

    def run(stereo):
        data, offsets, status, t = az.encode_pipeline(host, params, n, stereo=stereo, **kw)
        codes = np.bincount(data[offsets[:-1][status == 0] + 3] >> 4, minlength=11)
        return t, int((status == 0).sum()), int(offsets[-1]), {str(c): int(codes[c]) for c in (1, 8, 9, 10)}

    per = {False: [], True: []}
    written = {}
    for st in (False, True):
        run(st)  # warm-up
    for _ in range(args.reps):
        for st in (False, True):
            t, ok, nbytes, codes = run(st)
            per[st].append(t)
            written[st] = (ok, nbytes, codes)
    result = {"frames": nf, "reps": args.reps, "block": n, "k_stereo_rows_ms": rows}
    for st, key in ((False, "stereo_off"), (True, "stereo_on")):
        result[key] = {k: summary(t[k] for t in per[st]) for k in ("wall_ms", "analyze_ms", "sizes_ms", "pack_ms")}
        result[key]["frames_written"], result[key]["bytes"], result[key]["channel_codes"] = written[st]
    w0, w1 = result["stereo_off"]["wall_ms"], result["stereo_on"]["wall_ms"]
    result["wall_ratio_of_medians"] = round(w1["median"] / w0["median"], 4)
    result["stereo_off_wall_spread"] = round((w0["max"] - w0["min"]) / w0["median"], 4)
    result["bytes_ratio"] = round(result["stereo_on"]["bytes"] / result["stereo_off"]["bytes"], 5)
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    az.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
