"""Measure recompress against the two-step route, and k_units alone, on a stream this project
encodes from the config-2 synthetic signal (mono 4608-sample int16 blocks, -l 12 -q 5 -r 0,5):

    python tools/bench_recompress.py [--frames 100000] [--reps 5] [--block 4608] [--out FILE.json]

Prints one JSON line.

a. Two routes from host .flac bytes to host .flac bytes, in one process, alternated --reps times
   after a warm-up of each, wall clock:
     two_step    flacmi_decode_stream_host to page-locked host PCM, then flacmi_encode_pipeline
                 from that PCM (its own per-step times are reported beside the walls);
     recompress  flacmi_recompress_host + flacmi_recompress_fetch, the stream in one call, and
                 again in chunks of --chunk bytes (what flac_amd.recompress does by default);
   with the bytes each route moves over PCIe each way.  Both write the same frames.
b. k_units alone (HIP events, --launches launches) beside k_pcm<2> on the same frame list and
   k_stereo_rows on int16 rows of the same size, as TB/s over algorithmic bytes (int32 rows read,
   rows written).  The copy-rate yardstick is tools/experiments/stream_floor.hip, run apart.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--block", type=int, default=4608, help="output block size")
    ap.add_argument("--chunk", type=int, default=1 << 24)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from flac_amd import abi
    from flac_amd._lib import check
    from flac_amd.analysis import Analyzer, device_batch, frame_params, make_params, unit_stride

    n, bits, nf, B = 4608, 16, args.frames, args.block
    az = Analyzer(0)
    dev = torch.device("cuda", 0)
    sptr = torch.cuda.current_stream(dev).cuda_stream
    stride = unit_stride(n, 2)
    g = torch.empty((nf, stride), dtype=torch.int16, device=dev)
    az.synth_device(g.data_ptr(), 2, bits, stride, 0, nf, n, args.seed)
    torch.cuda.synchronize(dev)
    rows = g.cpu().numpy()
    params = make_params(12, 5, 0, 5)
    data, offsets, status, _ = az.encode_pipeline(rows, params, n, sample_bits=bits, channels=1, sample_size=bits)
    assert not status.any()
    nb = int(offsets[-1])
    h_in = az.host_array((nb,), np.uint8)
    h_in[:] = data[:nb]
    del data

    # ---- a. the two routes ----
    total = nf * n
    nblk, tail = total // B, total % B
    h_pcm = az.host_array((total * 2,), np.uint8)
    h_out = az.host_array((int(nb * 1.3) + (1 << 20),), np.uint8)
    fp = frame_params(1, bits, params.qlp_precision, 0)

    def two_step():
        t0 = time.perf_counter()
        r = az.decode_stream(h_in.ctypes.data, nb, 0, 1, bits, False, n, True, h_pcm.ctypes.data, len(h_pcm), False, 2)
        t1 = time.perf_counter()
        assert r.frames == nf and r.status == 0
        pcm = h_pcm.view(np.int16)
        units = pcm[:nblk * B].reshape(nblk, B)
        if tail:  # the short last block goes through a second, tiny call
            raise SystemExit("--block must divide frames * 4608 for the two-step route")
        out, off, st, tm = az.encode_pipeline(units, params, B, sample_bits=bits, channels=1, sample_size=bits, out=h_out)
        t2 = time.perf_counter()
        return out, {"decode_ms": (t1 - t0) * 1e3, "encode_ms": (t2 - t1) * 1e3, "wall_ms": (t2 - t0) * 1e3,
                     "pipeline": {k: tm[k] for k in ("h2d_ms", "analyze_ms", "sizes_ms", "pack_ms", "d2h_ms")}}

    h_rc = az.host_array((len(h_out),), np.uint8)

    def recompress(chunk, keep=False):
        t0 = time.perf_counter()
        pieces, pos, restart, calls = [], 0, True, 0
        while True:
            m = min(chunk, nb - pos)
            last = pos + m == nb
            res, out, off, st = az.recompress_chunk(h_in.ctypes.data + pos, m, 0, 1, bits, False, n, last, restart, B,
                                                    params, fp, out_alloc=lambda k: h_rc)
            assert res.status == 0 and not st.any()
            pieces.append(out.copy() if keep else None)
            restart = False
            calls += 1
            pos += int(res.consumed)
            if last:
                break
            assert res.frames > 0
        return pieces, {"wall_ms": (time.perf_counter() - t0) * 1e3, "calls": calls}

    ref, _ = two_step()
    ref = ref.tobytes()
    one, _ = recompress(nb, True)
    same = b"".join(p.tobytes() for p in one) == ref
    chunked, _ = recompress(args.chunk, True)
    same_chunked = b"".join(p.tobytes() for p in chunked) == ref
    runs = {"two_step": [], "recompress_one_call": [], "recompress_chunked": []}
    for _ in range(args.reps):
        runs["two_step"].append(two_step()[1])
        runs["recompress_one_call"].append(recompress(nb)[1])
        runs["recompress_chunked"].append(recompress(args.chunk)[1])

    def summary(rs):
        w = sorted(r["wall_ms"] for r in rs)
        return {"wall_ms_median": w[len(w) // 2], "wall_ms_min": w[0], "wall_ms_max": w[-1], "runs": rs}

    # ---- b. k_units beside k_pcm<2> and k_stereo_rows ----
    def timed(call):
        call()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / args.launches

    ostride = (n + 3) // 4 * 4
    rows32 = g[:, :n].to(torch.int32).contiguous()
    assert rows32.shape == (nf, ostride)
    t = np.zeros(nf, dtype=abi.PCM_FRAME_DTYPE)
    base = rows32.data_ptr()
    t["rows"] = base + 4 * ostride * np.arange(nf, dtype=np.uint64)
    t["stride"], t["first_sample"], t["block_size"] = ostride, n * np.arange(nf, dtype=np.int64), n
    d_t = torch.from_numpy(t.view(np.uint8)).to(dev)
    st = torch.empty(nf, dtype=torch.int32, device=dev)
    w = torch.empty(1, dtype=torch.int32, device=dev)
    kernels = {}
    for ub in sorted({B, 4608, 4096, 1152}):
        us = unit_stride(ub, 2)
        k_blocks, k_tail = total // ub, total % ub
        units = torch.empty(((k_blocks + (1 if k_tail else 0)) * us,), dtype=torch.int16, device=dev)
        ms = timed(lambda: check(az.lib.flacmi_units_out_device(az.ctx, d_t.data_ptr(), nf, 1, 0, ub, k_blocks, k_tail, bits,
                                                                units.data_ptr(), 2, us, st.data_ptr(), w.data_ptr(), sptr)))
        nbytes = total * 4 + (units.numel()) * 2
        got = units.view(-1, us)[:k_blocks, :ub].reshape(-1)
        kernels[f"k_units_block_{ub}"] = {"ms": ms, "TBs": nbytes / (ms * 1e-3) / 1e12, "bytes": nbytes,
                                          "equals_source": bool(torch.equal(got, g[:, :n].reshape(-1)[:k_blocks * ub])),
                                          "width": int(w.item())}
        del units
    pcm = torch.empty(total * 2 + 16, dtype=torch.uint8, device=dev)
    ms = timed(lambda: check(az.lib.flacmi_pcm_out_device(az.ctx, d_t.data_ptr(), nf, 1, 2, abi.PCM_PACKED, pcm.data_ptr(),
                                                          total * 2, st.data_ptr(), sptr)))
    kernels["k_pcm_2"] = {"ms": ms, "TBs": total * 6 / (ms * 1e-3) / 1e12, "bytes": total * 6}
    F = nf // 2
    mid = torch.empty((F, stride), dtype=torch.int16, device=dev)
    sstride = unit_stride(n, 4)
    side = torch.empty((F, sstride), dtype=torch.int32, device=dev)
    lr = device_batch(g.data_ptr(), 2, bits, stride, 2 * F, n)
    ms = timed(lambda: az.stereo_rows_device(lr, mid.data_ptr(), stride, side.data_ptr(), sstride, sptr))
    sbytes = 2 * F * n * 2 + F * n * 2 + F * n * 4
    kernels["k_stereo_rows"] = {"ms": ms, "TBs": sbytes / (ms * 1e-3) / 1e12, "bytes": sbytes}

    out_bytes = len(ref)
    line = {
        "frames": nf, "block": B, "stream_bytes": nb, "out_bytes": out_bytes, "pcm_bytes": total * 2,
        "same_frames": bool(same), "same_frames_chunked": bool(same_chunked),
        "pcie_bytes": {"two_step": {"h2d": nb + total * 2, "d2h": total * 2 + out_bytes},
                       "recompress": {"h2d": nb, "d2h": out_bytes}},
        "two_step": summary(runs["two_step"]), "recompress_one_call": summary(runs["recompress_one_call"]),
        "recompress_chunked": summary(runs["recompress_chunked"]) | {"chunk_bytes": args.chunk},
        "kernels": kernels,
    }
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
