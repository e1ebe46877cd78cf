"""Price and gain of the subframe choice by exact written size (FLACMI_FLAG_SIZE_CHOICE,
include/flacmi.h):

    python tools/bench_size_choice.py [--units 50000] [--reps 10] [--q 5] [--out FILE.json]

At config 2's shape (synthetic mono 4608-sample int16 units, -l 12 -q 5 -r 0,5), with the corrected
LPC sign and the exact Rice search in both runs:

  time   the same flacmi_analyze_device call on device rows with the flag clear and set, alternated
         --reps times after a warm-up of each, HIP events around the call: sorted times, median and
         extremes, and the ratio of the medians (the flag evaluates 5 + L candidates a unit where
         the other run evaluates one; there is no bar)
  size   the same units through flacmi_encode_host as mono frames with the flag clear and set: the
         frames both runs write, their bytes, the ratio, and how the chosen kinds and orders differ
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def spread(values):
    v = sorted(round(x, 4) for x in values)
    return {"all": v, "median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=50000)
    ap.add_argument("--size-units", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--q", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from flac_amd import abi
    from flac_amd.analysis import Analyzer, make_params, params_stride_for, unit_stride

    az = Analyzer(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    nu, n, L, q, rmax = args.units, 4608, 12, args.q, 5
    result = {"reps": args.reps, "block": n, "L": L, "q": q, "rice": [0, rmax], "device": torch.cuda.get_device_name(0)}

    def params(flag):
        return make_params(L, q, 0, rmax, lpc_sign=True, rice_search=True, size_choice=flag, sample_size=16 if flag else 0)

    # ---- the analysis step, flag clear against flag set ----
    stride = unit_stride(n, 2)
    rows = torch.empty((nu, stride), dtype=torch.int16, device=dev)
    az.synth_device(rows.data_ptr(), 2, 16, stride, 0, nu, n, args.seed)
    pstride = params_stride_for(rmax)
    rstride = ((n * 4 + 15) // 16) * 4
    meta = torch.zeros((nu, abi.META_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    rice = torch.zeros((nu, pstride), dtype=torch.int32, device=dev)
    res = torch.zeros((nu, rstride), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    per, choice = {False: [], True: []}, {}
    for i in range(2 + args.reps):
        for flag in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            az.analyze_device(rows.data_ptr(), 2, 16, stride, nu, n, params(flag), meta.data_ptr(), rice.data_ptr(),
                              pstride, res.data_ptr(), rstride, 4, stream)
            e1.record()
            torch.cuda.synchronize(dev)
            if i >= 2:
                per[flag].append(e0.elapsed_time(e1))
            if i == 0:
                m = meta.cpu().numpy().view(abi.META_DTYPE).reshape(-1)
                ok = m["status"] == 0
                choice[flag] = {"units_written": int(ok.sum()),
                                "fixed_by_order": [int((ok & (m["kind"] == 0) & (m["order"] == k)).sum()) for k in range(5)],
                                "lpc_by_order": [int((ok & (m["kind"] == 1) & (m["order"] == k)).sum()) for k in range(1, L + 1)]}
    result["time"] = {"units": nu, "flag_clear_ms": spread(per[False]), "flag_set_ms": spread(per[True]),
                      "ratio_of_medians": round(spread(per[True])["median"] / spread(per[False])["median"], 3),
                      "choice": {"flag_clear": choice[False], "flag_set": choice[True]}}

    # ---- the frame bytes of the same two runs ----
    ns = min(nu, args.size_units)
    host = np.ascontiguousarray(rows[:ns].cpu().numpy())
    sizes = {}
    for flag in (False, True):
        data, offsets, status = az.encode_frames(host, params(flag), n, sample_bits=16, channels=1, sample_size=16)
        sizes[flag] = (np.diff(offsets), status == 0)
    both = sizes[False][1] & sizes[True][1]
    a, b = int(sizes[False][0][both].sum()), int(sizes[True][0][both].sum())
    result["size"] = {"units": ns, "frames_both_write": int(both.sum()), "bytes_flag_clear": a, "bytes_flag_set": b,
                      "bytes_ratio": round(b / a, 5) if a else None, "raw_bytes": int(both.sum()) * n * 2}

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
