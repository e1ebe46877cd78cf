"""Measure the stream decoder on a stream this project encodes from the config-2 synthetic
signal (mono 4608-sample int16 blocks, -l 12 -q 5 -r 0,5):

    python tools/bench_decode.py [--frames 100000] [--reps 5] [--out FILE.json]

Prints one JSON line: k_index (ms, GB/s of stream read), the pass-1 decode of every
candidate (ms), candidates against frames, k_pcm (ms, GB/s of rows read + PCM written) and
the end-to-end host-bytes-to-host-PCM rate of flacmi_decode_stream_host.  Times are HIP
events on the launch stream after a warm-up call, averaged over --reps calls; the shares
of peak are against the 8.0 TB/s HBM3E spec figure (and the 6.3 TB/s a copy achieves).
Kernel times by name come from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_decode.py --frames 100000
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100000)
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
    stream = np.ascontiguousarray(data[:nb])

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

    # ---- k_index ----
    d_stream = torch.zeros(((nb + 3) // 4) * 4 + 16, dtype=torch.uint8, device=dev)
    d_stream[:nb] = torch.from_numpy(stream).to(dev)
    cap = 2 * nf + 1024
    d_table = torch.zeros((cap, abi.CANDIDATE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    index_ms = timed(lambda: check(az.lib.flacmi_index_frames_device(az.ctx, d_stream.data_ptr(), nb, 0,
                                                                    d_table.data_ptr(), cap, d_count.data_ptr(), sptr)))
    nc = int(d_count.item())
    table = d_table.cpu().numpy().view(abi.CANDIDATE_DTYPE).reshape(-1)[:nc]
    true_starts = set(int(o) for o in offsets[:-1])
    assert true_starts <= set(int(o) for o in table["offset"]), "a frame start is missing from the index"

    # ---- pass 1: every candidate, proposed to end at the next ----
    off = torch.from_numpy(np.append(table["offset"], nb).astype(np.int64)).to(dev)
    ostride = (n + 3) // 4 * 4
    out = torch.empty((nc, ostride), dtype=torch.int32, device=dev)
    st = torch.empty(nc, dtype=torch.int32, device=dev)
    mm = torch.empty(nc, dtype=torch.int64, device=dev)
    fe = torch.empty(nc, dtype=torch.int64, device=dev)
    dp = abi.DecodeParams()
    dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = 1, bits, -1, 0
    import ctypes as C
    pass1_ms = timed(lambda: check(az.lib.flacmi_decode_frames_end_device(
        az.ctx, d_stream.data_ptr(), nb, off.data_ptr(), nc, C.byref(dp), None, out.data_ptr(), ostride,
        st.data_ptr(), mm.data_ptr(), fe.data_ptr(), sptr)))
    st_np = st.cpu().numpy()

    # ---- k_pcm over the true frames ----
    idx = {int(o): k for k, o in enumerate(table["offset"])}
    t = np.zeros(nf, dtype=abi.PCM_FRAME_DTYPE)
    for f in range(nf):
        t[f] = (out.data_ptr() + 4 * idx[int(offsets[f])] * ostride, ostride, f * n, n, 0)
    d_t = torch.from_numpy(t.view(np.uint8)).to(dev)
    pcm = torch.empty(nf * n * 2 + 16, dtype=torch.uint8, device=dev)
    pst = torch.empty(nf, dtype=torch.int32, device=dev)
    pcm_ms = timed(lambda: check(az.lib.flacmi_pcm_out_device(az.ctx, d_t.data_ptr(), nf, 1, 2, abi.PCM_PACKED,
                                                             pcm.data_ptr(), nf * n * 2, pst.data_ptr(), sptr)))
    same = bool(np.array_equal(pcm[:nf * n * 2].cpu().numpy().view("<i2").reshape(nf, n), rows[:, :n]))

    # ---- end to end: host bytes -> host PCM ----
    h_in = az.host_array((nb,), np.uint8)
    h_in[:] = stream
    h_out = az.host_array((nf * n * 2,), np.uint8)

    def e2e():
        return az.decode_stream(h_in.ctypes.data, nb, 0, 1, bits, False, n, True, h_out.ctypes.data, len(h_out), False, 2)

    res = e2e()
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = e2e()
        walls.append((time.perf_counter() - t0) * 1e3)
    e2e_same = bool(res.frames == nf and np.array_equal(h_out.view("<i2").reshape(nf, n), rows[:, :n]))

    pcm_bytes = nf * n * (4 + 2)
    line = {
        "frames": nf, "stream_bytes": nb, "candidates": nc, "false_candidates": nc - nf,
        "k_index": {"ms": index_ms, "GBs": nb / (index_ms * 1e-3) / 1e9,
                    "share_of_hbm_spec": nb / (index_ms * 1e-3) / HBM_SPEC,
                    "share_of_hbm_copy": nb / (index_ms * 1e-3) / HBM_COPY},
        "pass1_decode": {"ms": pass1_ms, "frames_status_0": int((st_np == 0).sum()),
                         "samples_per_s": nf * n / (pass1_ms * 1e-3)},
        "k_pcm": {"ms": pcm_ms, "GBs": pcm_bytes / (pcm_ms * 1e-3) / 1e9,
                  "share_of_hbm_spec": pcm_bytes / (pcm_ms * 1e-3) / HBM_SPEC,
                  "share_of_hbm_copy": pcm_bytes / (pcm_ms * 1e-3) / HBM_COPY, "equals_source": same},
        "end_to_end": {"wall_ms": sorted(walls), "samples_per_s": nf * n / (min(walls) * 1e-3),
                       "probes": int(res.probes), "pass2_frames": int(res.pass2_frames), "equals_source": e2e_same},
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
