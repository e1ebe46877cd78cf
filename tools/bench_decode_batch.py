"""Measure the batch decoder against a loop of stream-decoder calls, on the config-2 stream of
tools/bench_decode.py (mono 4608-sample int16 blocks, -l 12 -q 5 -r 0,5) cut into many short
streams:

    python tools/bench_decode_batch.py [--frames 100000] [--per-stream 50 5] [--reps 5] [--out FILE.json]

Per shape (frames / K streams of K frames each):
  route A  one flacmi_decode_stream_host call per stream, host bytes to host int16 PCM (the only
           route before the batch decoder);
  route B  one flacmi_decode_batch_host and one fetch of int16 rows [N][1][T] that stay on the device.
The two alternate --reps times after a warm-up of each; wall clock, median and range.  Beside them
the kernels alone (HIP events, averaged over --reps launches after a warm-up): k_index over the
packed buffer, pass 1 over every candidate, k_planar and k_pcm<2> on the same frame list, and the
rate of a pinned host-to-device copy of the stream bytes.  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--per-stream", type=int, nargs="+", default=[50, 5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from flac_amd import abi
    from flac_amd._lib import check
    from flac_amd.analysis import Analyzer, make_params, unit_stride

    n, bits, nf = 4608, 16, args.frames
    az = Analyzer(0)
    dev = torch.device("cuda", 0)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    stride = unit_stride(n, 2)
    g = torch.empty((nf, stride), dtype=torch.int16, device=dev)
    az.synth_device(g.data_ptr(), 2, bits, stride, 0, nf, n, args.seed)
    torch.cuda.synchronize(dev)
    rows = g.cpu().numpy()
    del g
    data, offsets, status, _ = az.encode_pipeline(rows, make_params(12, 5, 0, 5), n, sample_bits=bits, channels=1,
                                                  sample_size=bits)
    assert not status.any()
    nb = int(offsets[-1])
    h_in = az.host_array((nb,), np.uint8)
    h_in[:] = data[:nb]
    h_out = az.host_array((nf * n * 2,), np.uint8)

    def timed(call):
        call()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / args.reps

    def spread(ms):
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}

    # ---- the copy, k_index and pass 1 over the whole buffer (the same for every shape but the
    # stream starts pass 1 adds, which the index lists anyway on this stream) ----
    d_stream = torch.zeros(((nb + 3) // 4) * 4 + 16, dtype=torch.uint8, device=dev)
    copy_ms = timed(lambda: check(az.lib.flacmi_memcpy_h2d(az.ctx, d_stream.data_ptr(), h_in.ctypes.data, nb)))
    cap = 2 * nf + 1024
    d_table = torch.zeros((cap, abi.CANDIDATE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    index_ms = timed(lambda: check(az.lib.flacmi_index_frames_device(az.ctx, d_stream.data_ptr(), nb, 0,
                                                                    d_table.data_ptr(), cap, d_count.data_ptr(), sptr)))
    nc = int(d_count.item())
    table = d_table.cpu().numpy().view(abi.CANDIDATE_DTYPE).reshape(-1)[:nc]
    off = torch.from_numpy(np.append(table["offset"], nb).astype(np.int64)).to(dev)
    ostride = (n + 3) // 4 * 4
    out = torch.empty((nc, ostride), dtype=torch.int32, device=dev)
    st = torch.empty(nc, dtype=torch.int32, device=dev)
    mm = torch.empty(nc, dtype=torch.int64, device=dev)
    fe = torch.empty(nc, dtype=torch.int64, device=dev)
    dp = abi.DecodeParams()
    dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = 1, bits, -1, 0
    pass1_ms = timed(lambda: check(az.lib.flacmi_decode_frames_end_device(
        az.ctx, d_stream.data_ptr(), nb, off.data_ptr(), nc, C.byref(dp), None, out.data_ptr(), ostride,
        st.data_ptr(), mm.data_ptr(), fe.data_ptr(), sptr)))
    idx = {int(o): k for k, o in enumerate(table["offset"])}

    shapes = []
    for K in args.per_stream:
        ns = nf // K
        used = ns * K
        seg = np.asarray(offsets[0:used + 1:K], dtype=np.int64)
        assert len(seg) == ns + 1 and seg[0] == 0

        # ---- the kernels on the same list: k_planar (int16 rows) beside k_pcm<2> (one timeline) ----
        t = np.zeros(used, dtype=abi.PCM_FRAME_DTYPE)
        for f in range(used):
            t[f] = (out.data_ptr() + 4 * idx[int(offsets[f])] * ostride, ostride, (f % K) * n, n, f // K)
        d_t = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
        fst = torch.empty(used, dtype=torch.int32, device=dev)
        planar = torch.empty((ns, 1, K * n), dtype=torch.int16, device=dev)
        planar_ms = timed(lambda: check(az.lib.flacmi_planar_out_device(az.ctx, d_t.data_ptr(), used, ns, 1, None, bits,
                                                                       abi.PLANAR_INT16, planar.data_ptr(), K * n,
                                                                       fst.data_ptr(), sptr)))
        planar_same = bool(np.array_equal(planar.cpu().numpy().reshape(used, n), rows[:used, :n]))
        t["first_sample"] = np.arange(used, dtype=np.int64) * n
        d_t2 = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
        pcm = torch.empty(used * n * 2 + 16, dtype=torch.uint8, device=dev)
        pcm_ms = timed(lambda: check(az.lib.flacmi_pcm_out_device(az.ctx, d_t2.data_ptr(), used, 1, 2, abi.PCM_PACKED,
                                                                 pcm.data_ptr(), used * n * 2, fst.data_ptr(), sptr)))
        del planar, pcm

        # ---- the two routes, alternating ----
        def route_a():
            frames = 0
            for s in range(ns):
                r = az.decode_stream(h_in.ctypes.data + int(seg[s]), int(seg[s + 1] - seg[s]), 0, 1, bits, False, n, True,
                                     h_out.ctypes.data + s * K * n * 2, K * n * 2, False, 2)
                frames += r.frames
            return frames

        def route_b():
            res, summary = az.decode_batch(h_in.ctypes.data, seg, 1, bits, False, n)
            pitch = (int(summary.max_samples) + 7) // 8 * 8
            rows_b = torch.empty((ns, 1, pitch), dtype=torch.int16, device=dev)
            az.batch_fetch(rows_b.data_ptr(), pitch, "int16", res, stream=sptr)
            torch.cuda.synchronize(dev)
            return rows_b, summary

        assert route_a() == used
        rows_b, summary = route_b()
        a_same = bool(np.array_equal(h_out[:used * n * 2].view("<i2").reshape(used, n), rows[:used, :n]))
        b_same = bool(int(summary.frames) == used and
                      np.array_equal(rows_b.cpu().numpy().reshape(used, n), rows[:used, :n]))
        del rows_b
        wa, wb = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            route_a()
            wa.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            route_b()
            wb.append((time.perf_counter() - t0) * 1e3)
        shapes.append({"streams": ns, "frames_per_stream": K, "frames": used, "bytes": int(seg[-1]),
                       "route_a_stream_calls": spread(wa) | {"equals_source": a_same},
                       "route_b_batch": spread(wb) | {"equals_source": b_same, "probes": int(summary.probes),
                                                      "pass2_frames": int(summary.pass2_frames)},
                       "b_over_a_median": statistics.median(wb) / statistics.median(wa),
                       "b_beats_a_by_more_than_a_range": statistics.median(wa) - statistics.median(wb) > max(wa) - min(wa),
                       "k_planar_int16": {"ms": planar_ms, "GBs": used * n * 6 / (planar_ms * 1e-3) / 1e9,
                                          "equals_source": planar_same},
                       "k_pcm_2": {"ms": pcm_ms, "GBs": used * n * 6 / (pcm_ms * 1e-3) / 1e9}})

    line = {"frames": nf, "stream_bytes": nb, "candidates": nc,
            "h2d_copy": {"ms": copy_ms, "GBs": nb / (copy_ms * 1e-3) / 1e9},
            "k_index": {"ms": index_ms}, "pass1_decode": {"ms": pass1_ms}, "shapes": shapes}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    az.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
