"""Price of the fallback-subframe mode (FLACMI_FRAME_FALLBACK, include/flacmi.h) on the
config-2 shape (mono 4608-sample int16 blocks, -l 12 -q 5 -r 0,5):

    python tools/bench_fallback.py [--frames 100000] [--reps 5] [--out FILE.json]

flacmi_encode_pipeline over page-locked host rows, the same call with the flag clear and set,
alternated --reps times after a warm-up of each, for the synthetic signal as it is (0% silent
units: the flagged call pays k_sub_kinds' read of every unit's meta and nothing else) and with
5% of the units replaced by digital silence (unflagged those frames fail and are not written;
flagged they are CONSTANT subframes through the general writer's hand-off list).  Prints one
JSON line: per mix and per flag the wall time of the call and the pipeline's own HIP-event
times of its steps (analysis, k_sub_kinds + sizes + scan, frame writing), each as the sorted
list over the reps, and the frames written.  Kernel times by name come from a separate run
under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_fallback.py --reps 2
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from flac_amd.analysis import Analyzer, make_params, unit_stride

    n, bits, nf = 4608, 16, args.frames
    az = Analyzer(0)
    dev = torch.device("cuda", 0)
    stride = unit_stride(n, 2)
    g = torch.empty((nf, stride), dtype=torch.int16, device=dev)
    az.synth_device(g.data_ptr(), 2, bits, stride, 0, nf, n, args.seed)
    torch.cuda.synchronize(dev)
    rows = az.host_array((nf, stride), np.int16)
    rows[:] = g.cpu().numpy()
    del g
    out = az.host_array((nf * (n * 2 + 64),), np.uint8)
    params = make_params(12, 5, 0, 5)
    kw = dict(sample_bits=bits, channels=1, sample_size=bits, out=out)
    silent = np.flatnonzero((np.arange(nf) * 2654435761 % (1 << 32)) < 0.05 * (1 << 32))  # 5% of the units

    def run(fallback):
        data, offsets, status, t = az.encode_pipeline(rows, params, n, fallback=fallback, **kw)
        return t, int((status == 0).sum()), int(offsets[-1])

    result = {"frames": nf, "reps": args.reps}
    for mix in ("silent_0pct", "silent_5pct"):
        if mix == "silent_5pct":
            rows[silent, :] = 0
        per = {False: [], True: []}
        written = {}
        for fb in (False, True):
            run(fb)  # warm-up
        for _ in range(args.reps):
            for fb in (False, True):
                t, ok, nbytes = run(fb)
                per[fb].append(t)
                written[fb] = (ok, nbytes)
        entry = {"silent_units": int(len(silent)) if mix == "silent_5pct" else 0}
        for fb, key in ((False, "flag_clear"), (True, "flag_set")):
            entry[key] = {k: sorted(round(t[k], 4) for t in per[fb])
                          for k in ("wall_ms", "analyze_ms", "sizes_ms", "pack_ms")}
            entry[key]["frames_written"], entry[key]["bytes"] = written[fb]
        w0, w1 = entry["flag_clear"]["wall_ms"], entry["flag_set"]["wall_ms"]
        entry["wall_overhead_of_median"] = w1[len(w1) // 2] / w0[len(w0) // 2] - 1.0
        entry["flag_clear_wall_spread"] = (w0[-1] - w0[0]) / w0[len(w0) // 2]
        result[mix] = entry
    if result["silent_0pct"]["flag_set"]["bytes"] > result["silent_0pct"]["flag_clear"]["bytes"]:
        raise SystemExit("bench_fallback: the flag made a stream without failing units larger")
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
