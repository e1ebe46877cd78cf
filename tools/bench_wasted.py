"""Price and gain of the wasted-bits mode (FLACMI_FRAME_WASTED, include/flacmi.h), and k_wasted_rows
beside k_stereo_rows, this repository's other memory-bound row kernel, on the same device rows:

    python tools/bench_wasted.py [--frames 100000] [--reps 20] [--pipe-reps 5] [--out FILE.json]

The rows are 2 x frames config-2 units (4608-sample int16 blocks of flacmi_synth_device), which
have no wasted bits, and the same samples << 8 in int32 rows at sample size 24 (the common
"24-bit" file).

Pipeline: the same flacmi_encode_pipeline call (-l 12 -q 5 -r 0,5, one channel, `frames` units from
page-locked host rows) with the mode off and on, alternated --pipe-reps times after a warm-up of
each, on (i) the int16 rows, where the mode buys nothing and costs the scan plus the general
writer in place of the fast writers, and (ii) the int32 rows << 8.  Per input and setting: the
wall time of the call and the pipeline's own HIP-event times of its steps as sorted lists with
median and extremes, the frames written and the total frame bytes.

Kernels: each launch is timed by HIP events; per kernel and input the sorted times, their median
and extremes, the algorithmic bytes (k_wasted_rows in place reads every sample once and, where a
unit has wasted bits, stores it once; its second read of such a unit is not counted) and the TB/s
they give:

    int16_in_place      no unit has wasted bits: one read, no store
    int16_out_of_place  one read, one store
    int24_in_place      every unit has w = 8: one read, one store (the rows are shifted back
                        between the launches, outside the events)
    int24_out_of_place  one read, one store
    stereo_int16/int24  k_stereo_rows: two rows read, the mid row and the int32 side row stored

Kernel times by name come from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_wasted.py --reps 3 --pipe-reps 1
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def summary(values, algorithmic):
    v = sorted(round(x, 4) for x in values)
    return {"all": v, "median": v[len(v) // 2], "min": v[0], "max": v[-1], "algorithmic_bytes": algorithmic,
            "tb_per_s_at_median": round(algorithmic / (v[len(v) // 2] * 1e-3) / 1e12, 3),
            "tb_per_s_at_min": round(algorithmic / (v[0] * 1e-3) / 1e12, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipe-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from flac_amd.analysis import Analyzer, device_batch, make_params, unit_stride

    n, nf = 4608, args.frames
    nu = 2 * nf
    az = Analyzer(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    s16, s32 = unit_stride(n, 2), unit_stride(n, 4)
    g16 = torch.empty((nu, s16), dtype=torch.int16, device=dev)
    az.synth_device(g16.data_ptr(), 2, 16, s16, 0, nu, n, args.seed)
    torch.cuda.synchronize(dev)
    g16[:, 0] |= 1                      # no unit without an odd sample: w = 0 everywhere
    g24 = torch.zeros((nu, s32), dtype=torch.int32, device=dev)
    g24[:, :n] = g16[:, :n].to(torch.int32) << 8
    want16 = g16.clone()
    wasted = torch.empty(nu, dtype=torch.int32, device=dev)

    def timed(launch, before=None):
        ms = []
        for i in range(3 + args.reps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            torch.cuda.synchronize(dev)
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return ms

    result = {"frames": nf, "units": nu, "block": n, "reps": args.reps}
    b16 = device_batch(g16.data_ptr(), 2, 16, s16, nu, n)
    b24 = device_batch(g24.data_ptr(), 4, 24, s32, nu, n)

    ms = timed(lambda: az.wasted_rows_device(b16, g16.data_ptr(), s16, wasted.data_ptr(), stream))
    assert not wasted.any() and torch.equal(g16, want16)
    result["int16_in_place"] = summary(ms, nu * n * 2)

    o16 = torch.empty_like(g16)
    ms = timed(lambda: az.wasted_rows_device(b16, o16.data_ptr(), s16, wasted.data_ptr(), stream))
    assert torch.equal(o16[:, :n], g16[:, :n])
    result["int16_out_of_place"] = summary(ms, nu * n * 4)
    del o16

    def restore():
        g24[:, :n] = g16[:, :n].to(torch.int32) << 8

    ms = timed(lambda: az.wasted_rows_device(b24, g24.data_ptr(), s32, wasted.data_ptr(), stream), before=restore)
    assert (wasted == 8).all() and torch.equal(g24[:, :n], g16[:, :n].to(torch.int32))
    result["int24_in_place"] = summary(ms, nu * n * 8)

    restore()
    o24 = torch.empty_like(g24)
    ms = timed(lambda: az.wasted_rows_device(b24, o24.data_ptr(), s32, wasted.data_ptr(), stream))
    assert (wasted == 8).all() and torch.equal(o24[:, :n], g16[:, :n].to(torch.int32))
    result["int24_out_of_place"] = summary(ms, nu * n * 8)
    del o24

    # the yardstick on the same rows
    side = torch.empty((nf, s32), dtype=torch.int32, device=dev)
    mid = torch.empty((nf, s16), dtype=torch.int16, device=dev)
    ms = timed(lambda: az.stereo_rows_device(b16, mid.data_ptr(), s16, side.data_ptr(), s32, stream))
    result["stereo_int16"] = summary(ms, nf * n * (2 + 2 + 2 + 4))
    del mid
    mid = torch.empty((nf, s32), dtype=torch.int32, device=dev)
    ms = timed(lambda: az.stereo_rows_device(b24, mid.data_ptr(), s32, side.data_ptr(), s32, stream))
    result["stereo_int24"] = summary(ms, nf * n * (4 + 4 + 4 + 4))

    del mid, side, wasted, want16

    # the pipeline with the mode off and on
    def spread(values):
        v = sorted(round(x, 4) for x in values)
        return {"all": v, "median": v[len(v) // 2], "min": v[0], "max": v[-1]}

    params = make_params(12, 5, 0, 5)
    for key, g, dt, bits in (("pipeline_int16", g16, np.int16, 16), ("pipeline_int24", g24, np.int32, 24)):
        host = az.host_array((nf, g.shape[1]), dt)
        host[:] = g[:nf].cpu().numpy()
        out = az.host_array((nf * (n * np.dtype(dt).itemsize + 128),), np.uint8)
        kw = dict(sample_bits=bits, channels=1, sample_size=bits, out=out)
        per, written = {False: [], True: []}, {}
        for on in (False, True):
            az.encode_pipeline(host, params, n, wasted=on, **kw)  # warm-up
        for _ in range(args.pipe_reps):
            for on in (False, True):
                data, offsets, status, t = az.encode_pipeline(host, params, n, wasted=on, **kw)
                per[on].append(t)
                written[on] = (int((status == 0).sum()), int(offsets[-1]))
        r = {}
        for on, name in ((False, "wasted_off"), (True, "wasted_on")):
            r[name] = {k: spread(t[k] for t in per[on]) for k in ("wall_ms", "analyze_ms", "sizes_ms", "pack_ms")}
            r[name]["frames_written"], r[name]["bytes"] = written[on]
        r["wall_ratio_of_medians"] = round(r["wasted_on"]["wall_ms"]["median"] / r["wasted_off"]["wall_ms"]["median"], 4)
        r["bytes_saved_per_subframe"] = round((r["wasted_off"]["bytes"] - r["wasted_on"]["bytes"]) / nf, 2)
        result[key] = r
        del host, out

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
