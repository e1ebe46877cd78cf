"""Price and gain of the exact Rice search (FLACMI_FLAG_RICE_SEARCH, include/flacmi.h):

    python tools/bench_rice_search.py [--units2 200000] [--units3 20000] [--reps 10]
                                      [--frames 100000] [--pipe-reps 3] [--out FILE.json]

Analysis step: the same flacmi_analyze_device call on device rows with the flag clear and set,
alternated --reps times after a warm-up of each, HIP events around the call, at config 2 (--units2
synthetic mono 4608-sample int16 units, -l 12 -q 5 -r 0,5) and config 3 (--units3 24-bit
16384-sample units, -l 32 -q 15 -r 0,8): sorted times, median and extremes, and for the flag the
difference of the medians against k_rice_search's algorithmic bytes (the residual rows once, the
meta record read and written, the parameters written), which is what the kernel alone may cost.
The kernel's own time by name comes from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_rice_search.py --reps 3 --frames 0

Gated signal: --frames mono frames of 4608 int16 samples of AR(2) noise x[i] = 1.6 x[i-1] -
0.8 x[i-2] + N(0, 400), gated over the whole stream with on-bursts of 2000..20000 samples and
gaps of 200..6000 samples of digital silence, through flacmi_encode_pipeline (-l 12 -q 5 -r 0,5)
four times: with the fallback mode alone and with the search, each without and with the
corrected LPC sign.  Per run: frames written, stream bytes, wall time.
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
    ap.add_argument("--units2", type=int, default=200000)
    ap.add_argument("--units3", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--pipe-reps", type=int, default=3)
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
    result = {"reps": args.reps}

    # ---- the analysis step, flag clear against flag set ----
    for key, nu, n, sb, bits, L, q, rmax in (("config2", args.units2, 4608, 2, 16, 12, 5, 5),
                                             ("config3", args.units3, 16384, 4, 24, 32, 15, 8)):
        if nu <= 0:
            continue
        stride = unit_stride(n, sb)
        rows = torch.empty((nu, stride), dtype=torch.int16 if sb == 2 else torch.int32, device=dev)
        az.synth_device(rows.data_ptr(), sb, bits, stride, 0, nu, n, args.seed)
        pstride = params_stride_for(rmax)
        rstride = ((n * 4 + 15) // 16) * 4
        meta = torch.zeros((nu, abi.META_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        rice = torch.zeros((nu, pstride), dtype=torch.int32, device=dev)
        res = torch.zeros((nu, rstride), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def call(flag):
            az.analyze_device(rows.data_ptr(), sb, bits, stride, nu, n, make_params(L, q, 0, rmax, rice_search=flag),
                              meta.data_ptr(), rice.data_ptr(), pstride, res.data_ptr(), rstride, 4, stream)

        per, bits_written, ok = {False: [], True: []}, {}, {}
        for i in range(2 + args.reps):
            for flag in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(flag)
                e1.record()
                torch.cuda.synchronize(dev)
                if i >= 2:
                    per[flag].append(e0.elapsed_time(e1))
                if i == 0:
                    m = meta.cpu().numpy().view(abi.META_DTYPE).reshape(-1)
                    good = m["status"] == 0
                    ok[flag] = int(good.sum())
                    # written residual bits of the units both runs write are compared below
                    over = np.zeros(nu, dtype=np.int64)
                    r = rice.cpu().numpy()
                    for u in np.flatnonzero(good & (m["coding_method"] == 5)):
                        over[u] = int((r[u, : m["n_parts"][u]] > 14).sum())
                    bits_written[flag] = (np.where(m["coding_method"] == 5, m["rice_bits"] - 3 * m["n_parts"] - over,
                                                   m["rice_bits"] - 4 * m["n_parts"]), good)
        both = bits_written[False][1] & bits_written[True][1]
        n_parts = int(meta.cpu().numpy().view(abi.META_DTYPE).reshape(-1)["n_parts"].astype(np.int64).sum())
        alg = nu * (n * 4 + 2 * abi.META_DTYPE.itemsize) + 4 * n_parts
        r = {"units": nu, "block": n, "flag_clear_ms": spread(per[False]), "flag_set_ms": spread(per[True]),
             "units_written": {"flag_clear": ok[False], "flag_set": ok[True]},
             "residual_bits_of_units_both_write": {"flag_clear": int(bits_written[False][0][both].sum()),
                                                   "flag_set": int(bits_written[True][0][both].sum())},
             "k_rice_search_algorithmic_bytes": alg}
        d = r["flag_set_ms"]["median"] - r["flag_clear_ms"]["median"]
        r["difference_of_medians_ms"] = round(d, 4)
        r["ratio_of_medians"] = round(r["flag_set_ms"]["median"] / r["flag_clear_ms"]["median"], 4)
        r["tb_per_s_if_the_difference_is_the_kernel"] = round(alg / (d * 1e-3) / 1e12, 3) if d > 0 else None
        result[key] = r
        del rows, meta, rice, res

    # ---- the gated signal through the pipeline ----
    if args.frames > 0:
        n, nf = 4608, args.frames
        total = n * nf
        rng = np.random.default_rng(7)
        k = total // 2200 + 1  # a cycle is at least 2200 samples
        lens_arr = np.stack([rng.integers(2000, 20001, k), rng.integers(200, 6001, k)], axis=1).reshape(-1)
        gate_vals = torch.tensor([1, 0], dtype=torch.int16, device=dev).repeat(len(lens_arr) // 2)
        gate = torch.repeat_interleave(gate_vals, torch.from_numpy(lens_arr).to(dev))[:total].reshape(nf, n)
        g = torch.Generator(device=dev)
        g.manual_seed(args.seed)
        # the recursion runs along time, all frames side by side (each frame its own noise, zero history)
        e = torch.randn((n, nf), generator=g, device=dev, dtype=torch.float32) * 400.0
        x = torch.zeros((n, nf), dtype=torch.float32, device=dev)
        for i in range(n):
            x[i] = e[i] + (1.6 * x[i - 1] if i >= 1 else 0) - (0.8 * x[i - 2] if i >= 2 else 0)
        pcm = (x.round().clamp(-32768, 32767).to(torch.int16).t().contiguous() * gate)
        del e, x, gate, gate_vals
        stride = unit_stride(n, 2)
        host = az.host_array((nf, stride), np.int16)
        host[:] = 0
        host[:, :n] = pcm.cpu().numpy()
        silent = int((pcm == 0).all(dim=1).sum())
        del pcm
        out = az.host_array((nf * (n * 2 + 128),), np.uint8)
        runs = {}
        for sign in (False, True):
            for search in (False, True):
                p = make_params(12, 5, 0, 5, lpc_sign=sign, rice_search=search)
                kw = dict(sample_bits=16, channels=1, sample_size=16, out=out, fallback=True)
                az.encode_pipeline(host, p, n, **kw)  # warm-up
                walls = []
                for _ in range(args.pipe_reps):
                    data, offsets, status, t = az.encode_pipeline(host, p, n, **kw)
                    walls.append(t["wall_ms"])
                name = ("fallback" + ("+rice_search" if search else "")) + ("+lpc_sign" if sign else "")
                runs[name] = {"frames_written": int((status == 0).sum()), "bytes": int(offsets[-1]),
                              "wall_ms": spread(walls)}
        for sign in ("", "+lpc_sign"):
            a, b = runs["fallback" + sign], runs["fallback+rice_search" + sign]
            b["bytes_ratio_to_fallback_alone"] = round(b["bytes"] / a["bytes"], 4)
        result["gated"] = {"frames": nf, "block": n, "raw_bytes": nf * n * 2, "silent_frames": silent, "runs": runs}

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
