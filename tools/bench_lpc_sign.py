"""Price and gain of the corrected-LPC-sign mode (FLACMI_FLAG_LPC_SIGN, include/flacmi.h):

    python tools/bench_lpc_sign.py [--c2-units 1000000] [--c3-units 200000] [--frames 100000]
                                   [--reps 5] [--legs analysis,pipeline,stereo] [--out FILE.json]

analysis  The analysis step (flacmi_analyze_device over device rows made by flacmi_synth_device,
          HIP events around each call) of config 2 (4608 x int16, -l 12 -q 5 -r 0,5) and config 3
          (16384 x 24-bit, -l 32 -q 15 -r 0,8): the same call with the flag clear and set,
          alternated --reps times after a warm-up of each, with the kinds chosen.
pipeline  flacmi_encode_pipeline over --frames mono config-2 frames in page-locked host rows:
          fixed_only, the default mode and the mode, alternated: wall time, the pipeline's own
          HIP-event times of its steps (analysis; sizes + scan; frame writing) and the bytes
          written; then the wall time of decoding the default and the mode's stream
          (decoder.decode_pcm, all chunks drained).
stereo    The correlated stereo signal of tools/bench_stereo.py (left = A >> 1,
          right = left + (B >> 4)) with stereo=True, flag clear and set: bytes and wall time.

Every timing is the sorted list over the reps with median and min-max.  The signals are the
synthetic generator's (three sines plus noise per unit); no recorded audio is measured.  Prints
one JSON line.  Kernel times by name come from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_lpc_sign.py --legs analysis --reps 2
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = {"c2": dict(n=4608, bits=16, L=12, q=5, rmax=5), "c3": dict(n=16384, bits=24, L=32, q=15, rmax=8)}


def summary(values):
    v = sorted(round(x, 4) for x in values)
    return {"all": v, "median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def analysis_leg(az, name, units, reps, seed):
    import numpy as np
    import torch

    from flac_amd import abi
    from flac_amd.analysis import make_params, params_stride_for, unit_stride

    cfg = CONFIGS[name]
    dev = torch.device("cuda", 0)
    n, bits = cfg["n"], cfg["bits"]
    sbytes = 2 if bits <= 16 else 4
    sstride = unit_stride(n, sbytes)
    rstride = ((n * 4 + 15) // 16) * 16 // 4
    pstride = params_stride_for(cfg["rmax"])
    samples = torch.empty((units, sstride), dtype=torch.int16 if sbytes == 2 else torch.int32, device=dev)
    meta = torch.empty((units, abi.META_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    rparams = torch.empty((units, pstride), dtype=torch.int32, device=dev)
    residual = torch.empty((units, rstride), dtype=torch.int32, device=dev)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    az.synth_device(samples.data_ptr(), sbytes, bits, sstride, 0, units, n, seed, sptr)

    def step(flag):
        p = make_params(cfg["L"], cfg["q"], 0, cfg["rmax"], lpc_sign=flag)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        az.analyze_device(samples.data_ptr(), sbytes, bits, sstride, units, n, p, meta.data_ptr(), rparams.data_ptr(),
                          pstride, residual.data_ptr(), rstride, 4, sptr)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def verdicts():
        m = np.frombuffer(meta.cpu().numpy().tobytes(), dtype=abi.META_DTYPE)
        ok = m["status"] == 0
        lpc = ok & (m["kind"] == abi.KIND_LPC)
        return {"ok": int(ok.sum()), "lpc": int(lpc.sum()), "fixed": int((ok & ~lpc).sum()),
                "pruned": int((m["lpc_order"] == abi.LPC_PRUNED).sum()),
                "residual_wide": int((m["status"] == abi.STATUS_RESIDUAL_WIDE).sum()),
                "rice_bits": int(m["rice_bits"][ok].sum())}

    per, seen = {False: [], True: []}, {}
    for flag in (False, True):
        step(flag)  # warm-up
        seen[flag] = verdicts()
    for _ in range(reps):
        for flag in (False, True):
            per[flag].append(step(flag))
    out = {"units": units, **cfg, "flag_clear_ms": summary(per[False]), "flag_set_ms": summary(per[True]),
           "flag_clear": seen[False], "flag_set": seen[True]}
    out["ratio_of_medians"] = round(out["flag_set_ms"]["median"] / out["flag_clear_ms"]["median"], 4)
    out["flag_clear_spread"] = round((out["flag_clear_ms"]["max"] - out["flag_clear_ms"]["min"]) /
                                     out["flag_clear_ms"]["median"], 4)
    return out


def pipeline_leg(az, frames, reps, seed, stereo):
    import numpy as np
    import torch

    from flac_amd import abi
    from flac_amd.analysis import make_params, unit_stride
    from flac_amd.decoder import decode_pcm

    n, bits, C = 4608, 16, 2 if stereo else 1
    dev = torch.device("cuda", 0)
    stride = unit_stride(n, 2)
    g = torch.empty((C * frames, stride), dtype=torch.int16, device=dev)
    az.synth_device(g.data_ptr(), 2, bits, stride, 0, C * frames, n, seed)
    torch.cuda.synchronize(dev)
    if stereo:
        g[0::2] >>= 1
        g[1::2] >>= 4
        g[1::2] += g[0::2]
    g[:, n:] = 0
    host = az.host_array((C * frames, stride), np.int16)
    host[:] = g.cpu().numpy()
    del g
    out = az.host_array((frames * C * (n * 2 + 128),), np.uint8)
    kw = dict(sample_bits=bits, channels=C, sample_size=bits, out=out, stereo=stereo)
    modes = {"default": make_params(12, 5, 0, 5), "lpc_sign": make_params(12, 5, 0, 5, lpc_sign=True)}
    if not stereo:
        modes["fixed_only"] = make_params(0, 5, 0, 5, abi.MODE_FIXED_ONLY)

    def run(p, keep=False):
        t0 = time.perf_counter()
        data, offsets, status, t = az.encode_pipeline(host, p, n, **kw)
        t["call_ms"] = (time.perf_counter() - t0) * 1e3
        return t, int((status == 0).sum()), int(offsets[-1]), (bytes(data) if keep else None)

    per = {k: [] for k in modes}
    written, streams = {}, {}
    for k, p in modes.items():
        run(p)  # warm-up
    for r in range(reps):
        for k, p in modes.items():
            t, ok, nbytes, data = run(p, keep=r == 0 and not stereo and k != "fixed_only")
            per[k].append(t)
            written[k] = (ok, nbytes)
            if data is not None:
                streams[k] = data
    result = {"frames": frames, "channels": C, "reps": reps}
    for k in modes:
        result[k] = {f: summary(t[f] for t in per[k]) for f in ("wall_ms", "analyze_ms", "sizes_ms", "pack_ms")}
        result[k]["frames_written"], result[k]["bytes"] = written[k]
    result["bytes_vs_default"] = round(result["lpc_sign"]["bytes"] / result["default"]["bytes"], 5)
    if not stereo:
        result["bytes_vs_fixed_only"] = round(result["lpc_sign"]["bytes"] / result["fixed_only"]["bytes"], 5)
        result["default_bytes_vs_fixed_only"] = round(result["default"]["bytes"] / result["fixed_only"]["bytes"], 5)
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        import frame_writer as FW
        dec = {k: [] for k in streams}
        for r in range(reps + 1):
            for k, data in streams.items():
                buf = FW.stream_header(44100, 16, 1, written[k][0] * n, n) + data
                t0 = time.perf_counter()
                total = sum(len(chunk) for chunk in decode_pcm(buf)[4])
                ms = (time.perf_counter() - t0) * 1e3
                assert total == written[k][0] * n * 2, (k, total)
                if r:
                    dec[k].append(ms)
        result["decode_pcm_wall_ms"] = {k: summary(v) for k, v in dec.items()}
    return result


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2-units", type=int, default=1_000_000)
    ap.add_argument("--c3-units", type=int, default=200_000)
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--legs", default="analysis,pipeline,stereo")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from flac_amd._lib import LIB_PATH
    from flac_amd.analysis import Analyzer

    legs = args.legs.split(",")
    az = Analyzer(0)
    result = {"library": os.path.relpath(LIB_PATH, REPO), "prune_env": os.environ.get("FLACMI_NO_PRUNE", "")}
    if "analysis" in legs:
        for name, units in (("c2", args.c2_units), ("c3", args.c3_units)):
            if units > 0:
                result[name] = analysis_leg(az, name, units, args.reps, args.seed)
                torch.cuda.empty_cache()
    if "pipeline" in legs:
        result["pipeline"] = pipeline_leg(az, args.frames, args.reps, args.seed, stereo=False)
    if "stereo" in legs:
        result["stereo"] = pipeline_leg(az, args.frames // 2, args.reps, args.seed, stereo=True)
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
