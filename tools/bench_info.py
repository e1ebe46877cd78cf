"""Measure the stream analysis (k_frame_info, flacmi_info_stream_host) on the stream
tools/bench_decode.py uses: this project's encoding of the config-2 synthetic signal (mono
4608-sample int16 blocks, -l 12 -q 5 -r 0,5):

    python tools/bench_info.py [--frames 100000] [--reps 5] [--partitions 64] [--out FILE.json]

Prints one JSON line: k_index (ms), k_frame_info over every candidate (ms), the records'
copy-out plus flacmi_host_chain_walk plus the gather of the chain frames' records (ms, wall),
the end-to-end host-bytes-to-host-records wall time of flacmi_info_stream_host, and beside
them, from the same process and stream, the stream decoder's pass 1 over the same candidates
(k_decode_fx + k_decode through flacmi_decode_frames_end_device, as bench_decode.py times it):
the yardstick, since k_frame_info does strictly less per frame.  Kernel times are HIP events on
the launch stream after a warm-up call, averaged over --reps calls.  Kernel times by name come
from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_info.py --frames 100000
"""
import argparse
import ctypes as C
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
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--partitions", type=int, default=64, help="part_stride")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from flac_amd import abi
    from flac_amd._lib import check
    from flac_amd.analysis import Analyzer, make_params, unit_stride

    n, bits, nf, ps = 4608, 16, args.frames, args.partitions
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
    table = d_table.cpu().numpy().view(abi.CANDIDATE_DTYPE).reshape(-1)[:nc].copy()

    # ---- k_frame_info over every candidate ----
    off = torch.from_numpy(np.append(table["offset"], nb).astype(np.int64)).to(dev)
    dp = abi.DecodeParams()
    dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = 1, bits, -1, 0
    d_fi = torch.zeros(nc * abi.FRAME_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_si = torch.zeros(nc * abi.SUBFRAME_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_pp = torch.zeros(max(nc * ps, 8), dtype=torch.uint8, device=dev)
    info_ms = timed(lambda: check(az.lib.flacmi_frame_info_device(
        az.ctx, d_stream.data_ptr(), nb, off.data_ptr(), nc, C.byref(dp), d_fi.data_ptr(), d_si.data_ptr(),
        d_pp.data_ptr() if ps else None, ps, sptr)))

    # ---- the decoder's pass 1 over the same candidates (bench_decode.py's pass1_decode) ----
    ostride = (n + 3) // 4 * 4
    out = torch.empty((nc, ostride), dtype=torch.int32, device=dev)
    st = torch.empty(nc, dtype=torch.int32, device=dev)
    mm = torch.empty(nc, dtype=torch.int64, device=dev)
    fe = torch.empty(nc, dtype=torch.int64, device=dev)
    pass1_ms = timed(lambda: check(az.lib.flacmi_decode_frames_end_device(
        az.ctx, d_stream.data_ptr(), nb, off.data_ptr(), nc, C.byref(dp), None, out.data_ptr(), ostride,
        st.data_ptr(), mm.data_ptr(), fe.data_ptr(), sptr)))
    del out

    # ---- copy-out + walk + gather (what flacmi_info_stream_host does after the kernels) ----
    def host_side():
        fi = d_fi.cpu().numpy().view(abi.FRAME_INFO_DTYPE)
        si = d_si.cpu().numpy().view(abi.SUBFRAME_INFO_DTYPE)
        pp = d_pp.cpu().numpy()[:nc * ps].reshape(nc, ps)
        parsed = (abi.DSITE["frame_end"] << 16) | abi.STATUS_VERIFY
        st1 = np.where(fi["status"] == 0, parsed, fi["status"]).astype(np.int32)
        end1 = np.ascontiguousarray(fi["end"])
        chain = np.zeros(nc + 16, dtype=np.dtype([("offset", "<i8"), ("end", "<i8"), ("candidate", "<i8"),
                                                  ("status", "<i4"), ("reserved0", "<i4")]))
        w = abi.Walk()
        check(az.lib.flacmi_host_chain_walk(table.ctypes.data, nc, st1.ctypes.data, end1.ctypes.data, nb, 1, C.byref(w),
                                            chain.ctypes.data, len(chain)))
        k = chain["candidate"][:w.n_chain]
        return w, fi[k], si[k], pp[k]

    host_side()
    hosts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        w, fi, si, pp = host_side()
        hosts.append((time.perf_counter() - t0) * 1e3)
    walk_ok = bool(w.state == abi.WALK_DONE and w.n_chain == nf and np.array_equal(fi["offset"], offsets[:-1])
                   and np.array_equal(fi["end"], offsets[1:]))
    crc_ok = bool((fi["crc16_stored"] == fi["crc16_computed"]).all() and (fi["crc8_stored"] == fi["crc8_computed"]).all())

    # ---- end to end: host bytes -> host records ----
    h_in = az.host_array((nb,), np.uint8)
    h_in[:] = stream
    frames = np.zeros(nf + 1, dtype=abi.FRAME_INFO_DTYPE)
    subs = np.zeros((nf + 1, 1), dtype=abi.SUBFRAME_INFO_DTYPE)
    parts = np.zeros((nf + 1, 1, ps), dtype=np.uint8)

    def e2e():
        return az.info_stream(h_in.ctypes.data, nb, 0, 1, bits, True, frames, subs, parts)

    res = e2e()
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = e2e()
        walls.append((time.perf_counter() - t0) * 1e3)
    e2e_ok = bool(res.frames == nf and res.status == 0 and np.array_equal(frames["end"][:nf], offsets[1:])
                  and np.array_equal(subs["abs_sum"][:nf, 0], si["abs_sum"]))

    line = {
        "frames": nf, "stream_bytes": nb, "candidates": nc, "false_candidates": nc - nf, "part_stride": ps,
        "k_index": {"ms": index_ms, "GBs": nb / (index_ms * 1e-3) / 1e9},
        "k_frame_info": {"ms": info_ms, "samples_per_s": nf * n / (info_ms * 1e-3), "GBs": nb / (info_ms * 1e-3) / 1e9,
                         "vs_pass1": info_ms / pass1_ms},
        "pass1_decode": {"ms": pass1_ms, "samples_per_s": nf * n / (pass1_ms * 1e-3)},
        "copy_walk_gather": {"wall_ms": sorted(hosts), "chain_equals_frames": walk_ok, "crcs_hold": crc_ok},
        "end_to_end": {"wall_ms": sorted(walls), "samples_per_s": nf * n / (min(walls) * 1e-3),
                       "probes": int(res.probes), "records_equal": e2e_ok},
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
