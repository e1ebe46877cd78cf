"""Batched encode-analysis on the GPU through libflacmi.so.

`Analyzer` owns one flacmi context (one HIP device).  `analyze()` takes a 2-D array of
planar units (one row per (block, channel)), runs fixed + LPC + choice + Rice search
on the device and returns numpy views of the per-unit results (the fields of
flac/common.py's SubframeHeader / SubframeFixed / SubframeLPC / Residual, see
include/flacmi.h).  `analyze_device()` is the zero-copy form on device pointers used by
bench.py.
"""
import ctypes as C
import weakref

import numpy as np

from . import abi
from ._lib import FlacmiError, check, load


def make_params(max_lpc_order: int, qlp_precision: int, rice_min: int, rice_max: int,
                mode: int = abi.MODE_REFERENCE, all_candidates: bool = False,
                tiers_only: bool = False, lpc_sign: bool = False, rice_search: bool = False,
                size_choice: bool = False, sample_size: int = 0) -> abi.Params:
    """all_candidates: exact sum(|r|) for every LPC candidate (meta.lpc_order / lpc_sum always
    exact); by default a unit whose LPC candidates provably lose reports abi.LPC_PRUNED there.
    tiers_only (diagnostic): the int8-MFMA path prunes with its partial-sum tiers alone.
    lpc_sign: FLACMI_FLAG_LPC_SIGN, the corrected LPC predictor sign (MODE_REFERENCE and
    MODE_LPC_ONLY; never prunes).  rice_search: FLACMI_FLAG_RICE_SEARCH, the exact Rice search (every
    mode but MODE_LPC_ONLY, rice_max <= 8): each partition's smallest parameter, the smallest order and
    coding method; units the reference's Rice step fails on (sites 12, 13) get status 0.
    size_choice: FLACMI_FLAG_SIZE_CHOICE, the fixed order, the LPC order and the subframe type by exact
    written size (MODE_REFERENCE and MODE_FIXED_ONLY, with rice_search); sample_size: the bits a
    warm-up sample is written at (0: the batch's sample_bits)."""
    p = abi.Params()
    p.max_lpc_order = max_lpc_order
    p.qlp_precision = qlp_precision
    p.rice_min = rice_min
    p.rice_max = rice_max
    p.mode = mode
    p.reserved[1] = (abi.FLAG_ALL_CANDIDATES if all_candidates else 0) | (abi.FLAG_TIERS_ONLY if tiers_only else 0) | \
                    (abi.FLAG_LPC_SIGN if lpc_sign else 0) | (abi.FLAG_RICE_SEARCH if rice_search else 0) | \
                    (abi.FLAG_SIZE_CHOICE if size_choice else 0)
    p.reserved[2] = sample_size
    return p


def frame_params(channels: int, sample_size: int, qlp_precision: int, first_frame: int = 0,
                 fallback: bool = False, sub_kind_ptr: int = 0, stereo: bool = False,
                 wasted: bool = False) -> abi.FrameParams:
    """fallback: FLACMI_FRAME_FALLBACK (a unit the reference cannot write, or writes larger than
    raw, becomes a CONSTANT / VERBATIM subframe); sub_kind_ptr: the device int32 [n_units] array
    the *_device entry points then need (the host entry points keep their own).  stereo:
    FLACMI_STEREO_BEST (each two-channel frame takes the smallest of L_R, L_S, S_R, M_S; the host
    entry points only).  wasted: FLACMI_FRAME_WASTED (a unit whose samples share w zero low bits is
    written as x >> w at sample_size - w bits behind a header that declares w; the host entry points
    only, not together with stereo)."""
    fp = abi.FrameParams()
    fp.reserved0 = (abi.FRAME_FALLBACK if fallback else 0) | (abi.FRAME_WASTED if wasted else 0)
    fp.reserved[0] = sub_kind_ptr
    fp.reserved[1] = abi.STEREO_BEST if stereo else abi.STEREO_OFF
    fp.channels = channels
    fp.sample_size = sample_size
    fp.qlp_precision = qlp_precision
    fp.first_frame = first_frame
    return fp


def device_batch(samples_ptr: int, sample_bytes: int, sample_bits: int, unit_stride: int, n_units: int,
                 block_len: int, tail_len: int = 0, n_tail_units: int = 0) -> abi.Batch:
    b = abi.Batch()
    b.samples = samples_ptr
    b.sample_bytes = sample_bytes
    b.sample_bits = sample_bits
    b.unit_stride = unit_stride
    b.n_units = n_units
    b.block_len = block_len
    b.tail_len = tail_len
    b.n_tail_units = n_tail_units
    return b


def unit_stride(block_len: int, sample_bytes: int) -> int:
    """The row pitch (samples) the library lays device rows out at (flacmi_unit_stride): 16-byte
    rows, plus 128 bytes when the pitch is a multiple of 4 KB."""
    v = load().flacmi_unit_stride(block_len, sample_bytes)
    check(v if v < 0 else 0, "flacmi_unit_stride")
    return v


def get_knob(name: str) -> int:
    """A test/diagnostic knob of the library (flacmi_get_knob)."""
    v = C.c_int32(0)
    check(load().flacmi_get_knob(name.encode(), C.byref(v)), "flacmi_get_knob")
    return v.value


def set_knob(name: str, value: int) -> None:
    """Set a test/diagnostic knob (flacmi_set_knob): FLACMI_OVERLAP, FLACMI_MF8_GRID,
    FLACMI_STREAM_GENERIC, FLACMI_DECODE_GENERIC, FLACMI_ENERGY_BOUND, FLACMI_RICE_GRID.  The library reads their environment variables once; this is the
    thread-safe way to change them afterwards.  FLACMI_ENERGY_BOUND (the stream kernel's pruning
    calls): 0 the tiers alone; 1 (default) both pre-tests (the energy bound over every order, then
    orders 2 .. L by it and order 1 by the closed form), then the tiers; 2 the first pre-test,
    then the exact pass; 3 both, then the exact pass; 4 the first, then the tiers."""
    check(load().flacmi_set_knob(name.encode(), int(value)), "flacmi_set_knob")


class knob:
    """`with knob("FLACMI_OVERLAP", 0): ...` sets a knob and restores its previous value."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = get_knob(self.name)
        set_knob(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_knob(self.name, self.prev)
        return False


def params_stride_for(rice_max: int) -> int:
    return (1 << max(rice_max, 0)) + 1


class Analyzer:
    def __init__(self, device: int = 0):
        self.lib = load()
        self.device = device
        self.ctx = self.lib.flacmi_create(device)
        if not self.ctx:
            raise FlacmiError(f"flacmi_create({device}) failed: "
                              f"{self.lib.flacmi_last_error().decode(errors='replace')}")

    def close(self):
        if self.ctx:
            self.lib.flacmi_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------
    def analyze(self, samples: np.ndarray, params: abi.Params, block_len: int, tail_len: int = 0,
                n_tail_units: int = 0, sample_bits: int = 16, residual_bytes: int = 4,
                debug: bool = False, extras=()) -> dict:
        """Host arrays in, host arrays out (synchronous).  debug: every optional output (acf,
        fixed_sums, lpc_sums, lpc_records); extras: a subset of those names instead (lpc_sums
        turns LPC pruning off, the others do not)."""
        s = np.ascontiguousarray(samples)
        if s.dtype not in (np.int16, np.int32) or s.ndim != 2:
            raise ValueError("samples must be a 2-D int16 or int32 array")
        n_units, stride = s.shape
        b = abi.Batch()
        b.samples = s.ctypes.data
        b.sample_bytes = s.dtype.itemsize
        b.sample_bits = sample_bits
        b.unit_stride = stride
        b.n_units = n_units
        b.block_len = block_len
        b.tail_len = tail_len
        b.n_tail_units = n_tail_units
        pstride = params_stride_for(params.rice_max)
        rdt = np.uint32 if residual_bytes == 4 else np.uint64
        rstride = ((block_len * residual_bytes + 15) // 16) * 16 // residual_bytes
        out = {
            "meta": np.zeros(n_units, dtype=abi.META_DTYPE),
            "rice_params": np.zeros((n_units, pstride), dtype=np.int32),
            "residual": np.zeros((n_units, rstride), dtype=rdt),
        }
        o = abi.Outputs()
        o.meta = out["meta"].ctypes.data
        o.rice_params = out["rice_params"].ctypes.data
        o.params_stride = pstride
        o.residual = out["residual"].ctypes.data
        o.residual_bytes = residual_bytes
        o.residual_stride = rstride
        want = ("acf", "fixed_sums", "lpc_sums", "lpc_records") if debug else tuple(extras)
        shapes = {"acf": (33, np.float64), "fixed_sums": (5, np.int64), "lpc_sums": (32, np.int64),
                  "lpc_records": (abi.lpc_rec_words(32), np.int32)}
        for k in want:
            w, dt = shapes[k]
            out[k] = np.zeros((n_units, w), dtype=dt)
            setattr(o, k, out[k].ctypes.data)
        check(self.lib.flacmi_analyze_host(self.ctx, C.byref(b), C.byref(params), C.byref(o)),
              "flacmi_analyze_host")
        wide = np.flatnonzero(out["meta"]["status"] == abi.STATUS_RESIDUAL_WIDE) if residual_bytes == 4 else []
        if len(wide):
            # a chosen residual needs more than 32 bits: redo only those units with 64-bit
            # rows and widen the batch's rows (the other units' results stand)
            first_tail = n_units - n_tail_units
            sub = self.analyze(np.ascontiguousarray(s[wide]), params, block_len, tail_len,
                               int(np.count_nonzero(wide >= first_tail)), sample_bits, 8, debug, extras)
            w = max(out["residual"].shape[1], sub["residual"].shape[1])
            res = np.zeros((n_units, w), dtype=np.uint64)
            res[:, :out["residual"].shape[1]] = out["residual"]
            res[wide] = 0
            res[wide, :sub["residual"].shape[1]] = sub["residual"]
            out["residual"] = res
            for k, v in sub.items():
                if k != "residual":
                    out[k][wide] = v
        return out

    def analyze_device(self, samples_ptr: int, sample_bytes: int, sample_bits: int, unit_stride: int,
                       n_units: int, block_len: int, params: abi.Params, meta_ptr: int,
                       params_ptr: int, params_stride: int, residual_ptr: int, residual_stride: int,
                       residual_bytes: int = 4, stream: int = 0, tail_len: int = 0,
                       n_tail_units: int = 0) -> None:
        """Device pointers in/out; enqueued on `stream`, returns without synchronising."""
        b = abi.Batch()
        b.samples = samples_ptr
        b.sample_bytes = sample_bytes
        b.sample_bits = sample_bits
        b.unit_stride = unit_stride
        b.n_units = n_units
        b.block_len = block_len
        b.tail_len = tail_len
        b.n_tail_units = n_tail_units
        o = abi.Outputs()
        o.meta = meta_ptr
        o.rice_params = params_ptr
        o.params_stride = params_stride
        o.residual = residual_ptr
        o.residual_bytes = residual_bytes
        o.residual_stride = residual_stride
        check(self.lib.flacmi_analyze_device(self.ctx, C.byref(b), C.byref(params), C.byref(o), stream),
              "flacmi_analyze_device")

    # ------------------------------------------------------------------------------
    # frame writer (include/flacmi.h flacmi_frame_sizes_device / flacmi_pack_frames_device)
    # ------------------------------------------------------------------------------
    def encode_frames(self, samples: np.ndarray, params: abi.Params, block_len: int, tail_len: int = 0,
                      n_tail_units: int = 0, sample_bits: int = 16, channels: int = 1,
                      sample_size: int = 16, first_frame: int = 0, fallback: bool = False,
                      stereo: bool = False, wasted: bool = False):
        """Host rows in -> (frame bytes, frame offsets [n_frames + 1], frame status [n_frames]).
        fallback, stereo, wasted: see frame_params.

        Row f*channels + c is channel c of frame f.  A frame whose status is non-zero
        (the reference's exception, (site << 16) | status) has no bytes."""
        s = np.ascontiguousarray(samples)
        if s.dtype not in (np.int16, np.int32) or s.ndim != 2:
            raise ValueError("samples must be a 2-D int16 or int32 array")
        n_units, stride = s.shape
        b = abi.Batch()
        b.samples = s.ctypes.data
        b.sample_bytes = s.dtype.itemsize
        b.sample_bits = sample_bits
        b.unit_stride = stride
        b.n_units = n_units
        b.block_len = block_len
        b.tail_len = tail_len
        b.n_tail_units = n_tail_units
        fp = frame_params(channels, sample_size, params.qlp_precision, first_frame, fallback, stereo=stereo, wasted=wasted)
        n_frames = n_units // channels if channels else 0
        offsets = np.zeros(n_frames + 1, dtype=np.int64)
        status = np.zeros(max(n_frames, 1), dtype=np.int32)
        check(self.lib.flacmi_encode_host(self.ctx, C.byref(b), C.byref(params), C.byref(fp),
                                          offsets.ctypes.data, status.ctypes.data), "flacmi_encode_host")
        total = int(offsets[-1])
        out = np.empty(total, dtype=np.uint8)
        check(self.lib.flacmi_encode_fetch(self.ctx, out.ctypes.data, total), "flacmi_encode_fetch")
        return out, offsets, status[:n_frames]

    def encode_pipeline(self, samples: np.ndarray, params: abi.Params, block_len: int, tail_len: int = 0,
                        n_tail_units: int = 0, sample_bits: int = 16, channels: int = 1, sample_size: int = 16,
                        first_frame: int = 0, units_per_batch: int = 8192, capacity: int = 0,
                        out: np.ndarray = None, fallback: bool = False, stereo: bool = False,
                        wasted: bool = False):
        """encode_frames through flacmi_encode_pipeline: host rows in (any row stride), the
        batch streamed through the device in sub-batches of units_per_batch units with the
        PCIe copies overlapping the kernels.  `out` (optional, uint8): the caller's frame
        buffer, reused across calls (with host_register it stays page-locked).  Returns
        (frame bytes, frame offsets [n_frames + 1], frame status [n_frames], timing dict)."""
        s = samples
        if s.dtype not in (np.int16, np.int32) or s.ndim != 2 or s.strides[1] != s.itemsize:
            raise ValueError("samples must be a 2-D int16 or int32 array with contiguous rows")
        if s.strides[0] % s.itemsize:
            raise ValueError("the row stride must be a whole number of samples")
        if s.shape[1] < max(block_len, tail_len if n_tail_units else 0):
            raise ValueError(f"rows hold {s.shape[1]} samples, fewer than the block length")
        n_units = s.shape[0]
        b = abi.Batch()
        b.samples = s.ctypes.data
        b.sample_bytes = s.itemsize
        b.sample_bits = sample_bits
        b.unit_stride = s.strides[0] // s.itemsize
        b.n_units = n_units
        b.block_len = block_len
        b.tail_len = tail_len
        b.n_tail_units = n_tail_units
        fp = frame_params(channels, sample_size, params.qlp_precision, first_frame, fallback, stereo=stereo, wasted=wasted)
        n_frames = n_units // channels if channels else 0
        offsets = np.zeros(n_frames + 1, dtype=np.int64)
        status = np.zeros(max(n_frames, 1), dtype=np.int32)
        upb = max(channels, (units_per_batch // channels) * channels)
        if out is not None:
            if out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
                raise ValueError("out must be a contiguous 1-D uint8 array")
            capacity = out.size
        cap = capacity or int(n_units * (block_len * s.itemsize * 1.25 + 256)) + (1 << 20)
        given = out
        while True:
            out = given if given is not None else np.empty(cap, dtype=np.uint8)
            t = abi.EncodeTiming()
            rc = self.lib.flacmi_encode_pipeline(self.ctx, C.byref(b), C.byref(params), C.byref(fp), upb,
                                                 out.ctypes.data, cap, offsets.ctypes.data, status.ctypes.data,
                                                 C.byref(t))
            if rc == abi.E_NOMEM and not capacity:
                cap *= 2
                continue
            check(rc, "flacmi_encode_pipeline")
            break
        timing = {f: getattr(t, f) for f, _ in abi.EncodeTiming._fields_}
        return out[:int(offsets[-1])], offsets, status[:n_frames], timing

    def host_register(self, a: np.ndarray) -> None:
        """Page-lock a host array until host_unregister (flacmi_host_register)."""
        check(self.lib.flacmi_host_register(self.ctx, a.ctypes.data, a.nbytes), "flacmi_host_register")

    def host_unregister(self, a: np.ndarray) -> None:
        check(self.lib.flacmi_host_unregister(self.ctx, a.ctypes.data), "flacmi_host_unregister")

    def host_array(self, shape, dtype) -> np.ndarray:
        """A numpy array over page-locked host memory (flacmi_host_alloc), freed with the
        array: staging rows and frame buffers reused call after call without page-locking."""
        dt = np.dtype(dtype)
        count = int(np.prod(shape)) if len(shape) else 1
        nbytes = max(count * dt.itemsize, 1)
        p = self.lib.flacmi_host_alloc(self.ctx, nbytes)
        if not p:
            raise FlacmiError(f"flacmi_host_alloc({nbytes}): {self.lib.flacmi_last_error().decode(errors='replace')}")
        raw = (C.c_uint8 * nbytes).from_address(p)
        # every numpy view of the memory keeps `raw` alive: free with the last view (valid
        # after close() too)
        weakref.finalize(raw, self.lib.flacmi_host_free, None, p)
        return np.frombuffer(raw, dtype=dt, count=count).reshape(shape)

    def frame_sizes_device(self, batch: abi.Batch, fp: abi.FrameParams, meta_ptr: int, params_ptr: int,
                           params_stride: int, offsets_ptr: int, status_ptr: int, stream: int = 0) -> None:
        check(self.lib.flacmi_frame_sizes_device(self.ctx, C.byref(batch), C.byref(fp), meta_ptr, params_ptr,
                                                 params_stride, offsets_ptr, status_ptr, stream),
              "flacmi_frame_sizes_device")

    def pack_frames_device(self, batch: abi.Batch, fp: abi.FrameParams, meta_ptr: int, params_ptr: int,
                           params_stride: int, residual_ptr: int, residual_bytes: int, residual_stride: int,
                           offsets_ptr: int, status_ptr: int, out_ptr: int, capacity: int,
                           stream: int = 0) -> None:
        check(self.lib.flacmi_pack_frames_device(self.ctx, C.byref(batch), C.byref(fp), meta_ptr, params_ptr,
                                                 params_stride, residual_ptr, residual_bytes, residual_stride,
                                                 offsets_ptr, status_ptr, out_ptr, capacity, stream),
              "flacmi_pack_frames_device")

    def stereo_rows_device(self, lr: abi.Batch, mid_ptr: int, mid_stride: int, side_ptr: int, side_stride: int,
                           stream: int = 0) -> None:
        """flacmi_stereo_rows_device: mid = (L + R) >> 1 rows (lr's element type) and side = L - R
        rows (int32) of a two-channel device batch (rows 2f, 2f + 1 = left, right of frame f)."""
        check(self.lib.flacmi_stereo_rows_device(self.ctx, C.byref(lr), mid_ptr, mid_stride, side_ptr, side_stride,
                                                 stream),
              "flacmi_stereo_rows_device")

    def wasted_rows_device(self, rows: abi.Batch, out_ptr: int, out_stride: int, wasted_ptr: int,
                           stream: int = 0) -> None:
        """flacmi_wasted_rows_device: wasted[u] (int32; 0 for an all-zero unit, else the count of
        trailing zero bits of the OR of the unit's samples, at most sample_bits - 1) and the rows
        shifted right by it, of a device batch.  out_ptr may be the batch's own rows."""
        check(self.lib.flacmi_wasted_rows_device(self.ctx, C.byref(rows), out_ptr, out_stride, wasted_ptr, stream),
              "flacmi_wasted_rows_device")

    # ------------------------------------------------------------------------------
    # decoder verifier (include/flacmi.h flacmi_decode_frames_device)
    # ------------------------------------------------------------------------------
    def decode_frames_device(self, data_ptr: int, data_bytes: int, offsets_ptr: int, n_frames: int,
                             dp: abi.DecodeParams, expect: abi.Batch = None, out_ptr: int = 0,
                             out_stride: int = 0, status_ptr: int = 0, mismatch_ptr: int = 0,
                             stream: int = 0) -> None:
        check(self.lib.flacmi_decode_frames_device(self.ctx, data_ptr, data_bytes, offsets_ptr, n_frames,
                                                   C.byref(dp), C.byref(expect) if expect is not None else None,
                                                   out_ptr or None, out_stride, status_ptr, mismatch_ptr, stream),
              "flacmi_decode_frames_device")

    def decode_frames(self, data: np.ndarray, offsets: np.ndarray, channels: int, sample_size: int,
                      first_frame: int = -1, expect: np.ndarray = None, block_len: int = 0, tail_len: int = 0,
                      n_tail_units: int = 0, out_stride: int = 0, check_crc: bool = True,
                      spec_wasted_bits: bool = False, samples_out: bool = True, frame_end: bool = False):
        """Host bytes in -> (decoded int32 rows [n_frames*channels][out_stride], frame status,
        mismatches per frame), decoded on the device.  `expect` (int16/int32 rows of the
        source units) turns on the in-kernel comparison.  spec_wasted_bits:
        FLACMI_DECODE_WASTED_SPEC.  samples_out=False passes no rows to the device (the builds
        that only compare; the rows returned stay zero).  frame_end=True goes through
        flacmi_decode_frames_end_device and returns the frame ends as a fourth array."""
        import torch
        dev = torch.device("cuda", self.device)
        n_frames = len(offsets) - 1
        nb = int(len(data))
        buf = torch.zeros(((nb + 3) // 4) * 4 + 16, dtype=torch.uint8, device=dev)
        if nb:
            buf[:nb] = torch.from_numpy(np.array(data, dtype=np.uint8, copy=True)).to(dev)
        off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(dev)
        if out_stride <= 0:
            out_stride = ((max(block_len, 1) + 3) // 4) * 4
        out = torch.zeros((max(n_frames * channels, 1), out_stride), dtype=torch.int32, device=dev)
        st = torch.zeros(max(n_frames, 1), dtype=torch.int32, device=dev)
        mm = torch.zeros(max(n_frames, 1), dtype=torch.int64, device=dev)
        dp = abi.DecodeParams()
        dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = channels, sample_size, first_frame, int(check_crc)
        dp.reserved0 = abi.DECODE_WASTED_SPEC if spec_wasted_bits else 0
        eb = None
        if expect is not None:
            e = torch.from_numpy(np.ascontiguousarray(expect)).to(dev)
            eb = device_batch(e.data_ptr(), e.element_size(), 16 if e.element_size() == 2 else 32, e.shape[1],
                              e.shape[0], block_len, tail_len, n_tail_units)
        stream = torch.cuda.current_stream(dev).cuda_stream
        out_ptr = out.data_ptr() if samples_out else 0
        if frame_end:
            fe = torch.full((max(n_frames, 1),), -2, dtype=torch.int64, device=dev)
            check(self.lib.flacmi_decode_frames_end_device(self.ctx, buf.data_ptr(), nb, off.data_ptr(), n_frames,
                                                           C.byref(dp), C.byref(eb) if eb is not None else None,
                                                           out_ptr or None, out_stride, st.data_ptr(), mm.data_ptr(),
                                                           fe.data_ptr(), stream), "flacmi_decode_frames_end_device")
        else:
            self.decode_frames_device(buf.data_ptr(), nb, off.data_ptr(), n_frames, dp, eb, out_ptr, out_stride,
                                      st.data_ptr(), mm.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        res = out.cpu().numpy(), st.cpu().numpy()[:n_frames], mm.cpu().numpy()[:n_frames]
        return res + (fe.cpu().numpy()[:n_frames],) if frame_end else res

    def index_frames(self, data, first_byte: int = 0, capacity: int = 0, base_offset: int = 0):
        """Host bytes in -> (candidate table as a CANDIDATE_DTYPE array, the true count), from
        the device frame index.  capacity 0: retried until the table holds every candidate.
        base_offset (a multiple of 4): the stream starts that many bytes into its device
        buffer, so its base is not 16-byte aligned."""
        import torch
        dev = torch.device("cuda", self.device)
        nb = int(len(data))
        assert base_offset % 4 == 0
        buf = torch.full((base_offset + ((nb + 3) // 4) * 4 + 16,), 0xFF, dtype=torch.uint8, device=dev)
        if nb:
            buf[base_offset:base_offset + nb] = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        cap = capacity if capacity > 0 else max(64, nb // 512)
        while True:
            table = torch.zeros((max(cap, 1), abi.CANDIDATE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            check(self.lib.flacmi_index_frames_device(self.ctx, buf.data_ptr() + base_offset, nb, first_byte, table.data_ptr(), cap,
                                                      count.data_ptr(), stream), "flacmi_index_frames_device")
            torch.cuda.synchronize(dev)
            n = int(count.item())
            if n <= cap or capacity > 0:
                break
            cap = n
        return table.cpu().numpy().view(abi.CANDIDATE_DTYPE).reshape(-1)[:min(n, cap)].copy(), n

    def pcm_out(self, rows: np.ndarray, block_sizes, channels: int, bytes_per_sample: int, raw: bool = False,
                lead_bytes: int = 0):
        """int32 rows [n_frames*channels][stride] and the frames' block sizes -> (interleaved PCM
        bytes, status per frame, total bytes) from the device PCM writer.  The frames follow each
        other; the first starts at byte lead_bytes (a multiple of channels * B), so a test
        chooses the alignment of every frame's first byte."""
        import torch
        dev = torch.device("cuda", self.device)
        B = 4 if raw else bytes_per_sample
        assert lead_bytes % (channels * B) == 0
        r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
        stride = r.shape[1]
        t = np.zeros(len(block_sizes), dtype=abi.PCM_FRAME_DTYPE)
        first = lead_bytes // (channels * B)
        for f, bs in enumerate(block_sizes):
            t[f] = (r.data_ptr() + 4 * f * channels * stride, stride, first, bs, 0)
            first += bs
        total = first * channels * B
        tab = torch.from_numpy(t.view(np.uint8)).to(dev)
        out = torch.full((((total + 3) // 4) * 4 + 16,), 0xA5, dtype=torch.uint8, device=dev)
        st = torch.zeros(max(len(block_sizes), 1), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(self.lib.flacmi_pcm_out_device(self.ctx, tab.data_ptr(), len(block_sizes), channels, bytes_per_sample,
                                             abi.PCM_RAW32 if raw else abi.PCM_PACKED, out.data_ptr(), total,
                                             st.data_ptr(), stream), "flacmi_pcm_out_device")
        torch.cuda.synchronize(dev)
        return out.cpu().numpy(), st.cpu().numpy()[:len(block_sizes)], total

    def units_out(self, frames, channels: int, first_sample: int, block_len: int, n_blocks: int, tail_len: int,
                  sample_size: int, sample_bytes: int, stride: int = 0, guard: int = 64, fill: int = 0x5A, firsts=None):
        """flacmi_units_out_device alone.  frames: a list of (int32 array [channels][block_size], row
        pitch) in stream order, each placed on the device at its own pitch (firsts: their first samples
        when they do not simply follow one another); the unit rows lie
        between two guard regions of `guard` elements and every byte of the buffer is `fill`
        beforehand.  -> (the whole buffer as a 1-D array of the unit type, the index of unit 0's
        first element in it, the pitch, status per frame, the width word)."""
        import torch
        dev = torch.device("cuda", self.device)
        dt = np.int16 if sample_bytes == 2 else np.int32
        stride = stride or unit_stride(block_len, sample_bytes)
        n_units = (n_blocks + (1 if tail_len else 0)) * channels
        keep = []
        t = np.zeros(len(frames), dtype=abi.PCM_FRAME_DTYPE)
        first = 0
        for f, (x, pitch) in enumerate(frames):
            x = np.asarray(x, dtype=np.int32).reshape(channels, -1)
            bs = x.shape[1]
            rows = np.full((channels, pitch), 0x7BADBAD, dtype=np.int32)  # what lies past a frame's length
            rows[:, :bs] = x
            r = torch.from_numpy(rows).to(dev)
            keep.append(r)
            if firsts is not None:
                first = firsts[f]
            t[f] = (r.data_ptr(), pitch, first, bs, 0)
            first += bs
        tab = torch.from_numpy(t.view(np.uint8).copy()).to(dev) if len(frames) else torch.zeros(8, dtype=torch.uint8, device=dev)
        guard = ((guard * sample_bytes + 15) // 16) * 16 // sample_bytes
        buf = torch.from_numpy(np.full((2 * guard + max(n_units, 1) * stride) * sample_bytes, fill, dtype=np.uint8)).to(dev)
        st = torch.full((max(len(frames), 1),), -1, dtype=torch.int32, device=dev)
        w = torch.full((1,), -1, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(self.lib.flacmi_units_out_device(self.ctx, tab.data_ptr() if len(frames) else None, len(frames), channels,
                                               first_sample, block_len, n_blocks, tail_len, sample_size,
                                               buf.data_ptr() + guard * sample_bytes, sample_bytes, stride,
                                               st.data_ptr(), w.data_ptr(), stream), "flacmi_units_out_device")
        torch.cuda.synchronize(dev)
        return (buf.cpu().numpy().view(dt), guard, stride, st.cpu().numpy()[:len(frames)],
                int(w.cpu().numpy().view(np.uint32)[0]))

    def planar_out(self, streams, channels: int, elem: str, sample_size: int = 16, pitch: int = 0, lengths=None,
                   guard: int = 64, fill: int = 0x5A):
        """flacmi_planar_out_device alone.  streams: per stream a list of (int32 array [channels][block_size],
        row pitch) in stream order, each frame placed on the device at its own pitch; elem "int16" | "int32" |
        "float32"; pitch in elements (0: the longest stream, rounded up to 16 bytes); lengths: optional cut per
        stream.  The rows lie between two guard regions of `guard` elements and every byte of the buffer is
        `fill` beforehand.  -> (the whole buffer as a 1-D array of the element type, the index of row 0's first
        element in it, the pitch, status per frame in list order)."""
        import torch
        dev = torch.device("cuda", self.device)
        dt = {"int16": np.int16, "int32": np.int32, "float32": np.float32}[elem]
        sb = np.dtype(dt).itemsize
        g = 16 // sb
        keep, recs = [], []
        longest = 0
        for si, frames in enumerate(streams):
            first = 0
            for x, fp in frames:
                x = np.asarray(x, dtype=np.int32).reshape(channels, -1)
                bs = x.shape[1]
                rows = np.full((channels, fp), 0x7BADBAD, dtype=np.int32)  # what lies past a frame's length
                rows[:, :bs] = x
                r = torch.from_numpy(rows).to(dev)
                keep.append(r)
                recs.append((r.data_ptr(), fp, first, bs, si))
                first += bs
            longest = max(longest, first)
        pitch = pitch or max(g, (longest + g - 1) // g * g)
        t = np.array(recs, dtype=abi.PCM_FRAME_DTYPE) if recs else np.zeros(0, dtype=abi.PCM_FRAME_DTYPE)
        tab = torch.from_numpy(t.view(np.uint8).copy()).to(dev) if recs else None
        guard = (guard + g - 1) // g * g
        n_rows = len(streams) * channels
        buf = torch.from_numpy(np.full((2 * guard + max(n_rows, 1) * pitch) * sb, fill, dtype=np.uint8)).to(dev)
        st = torch.full((max(len(recs), 1),), -1, dtype=torch.int32, device=dev)
        ln = torch.from_numpy(np.asarray(lengths, dtype=np.int64)).to(dev) if lengths is not None else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(self.lib.flacmi_planar_out_device(self.ctx, tab.data_ptr() if recs else None, len(recs), len(streams), channels,
                                                ln.data_ptr() if ln is not None else None, sample_size,
                                                abi.PLANAR_ELEM[elem], buf.data_ptr() + guard * sb, pitch, st.data_ptr(),
                                                stream), "flacmi_planar_out_device")
        torch.cuda.synchronize(dev)
        return buf.cpu().numpy().view(dt), guard, pitch, st.cpu().numpy()[:len(recs)]

    def decode_batch(self, data_ptr: int, seg_offsets: np.ndarray, channels: int, sample_size: int, check_crc: bool,
                     max_block_size: int, spec_wasted_bits: bool = False):
        """flacmi_decode_batch_host: the frame regions of len(seg_offsets) - 1 whole streams, packed back to
        back in host memory at data_ptr -> (BatchStreamResult array, BatchSummary).  The frame list stays in the
        context for batch_fetch."""
        seg = np.ascontiguousarray(seg_offsets, dtype=np.int64)
        n = len(seg) - 1
        dp = abi.DecodeParams()
        dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = channels, sample_size, -1, int(check_crc)
        dp.reserved0 = abi.DECODE_WASTED_SPEC if spec_wasted_bits else 0
        res = (abi.BatchStreamResult * max(n, 1))()
        summary = abi.BatchSummary()
        check(self.lib.flacmi_decode_batch_host(self.ctx, data_ptr, seg.ctypes.data, n, C.byref(dp), max_block_size,
                                                C.cast(res, C.c_void_p), C.byref(summary)), "flacmi_decode_batch_host")
        return res, summary

    def batch_fetch(self, out_ptr: int, pitch: int, elem: str, res, host: bool = False, stream: int = 0):
        """flacmi_decode_batch_fetch: the kept frame list as [streams][channels][pitch] rows of `elem` at
        out_ptr (device memory, written on `stream`; host memory with host=True); `res` receives the final
        per-stream results (int16: a range finding stops its stream)."""
        check(self.lib.flacmi_decode_batch_fetch(self.ctx, out_ptr, pitch, abi.PLANAR_ELEM[elem], int(host),
                                                 C.cast(res, C.c_void_p), stream), "flacmi_decode_batch_fetch")

    def recompress_chunk(self, data_ptr: int, nbytes: int, first_byte: int, channels: int, sample_size: int,
                         check_crc: bool, max_block_size: int, final_chunk: bool, restart: bool, block_len: int,
                         params: abi.Params, fp: abi.FrameParams, spec_wasted_bits: bool = False, out_alloc=None):
        """flacmi_recompress_host + flacmi_recompress_fetch: one chunk of host stream bytes ->
        (result, frame bytes, frame offsets [blocks_out + 1], frame status [blocks_out]).  out_alloc(nbytes)
        -> a uint8 array of at least nbytes for the frame bytes (page-locked memory copies at PCIe rate)."""
        dp = abi.DecodeParams()
        dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = channels, sample_size, -1, int(check_crc)
        dp.reserved0 = abi.DECODE_WASTED_SPEC if spec_wasted_bits else 0
        res = abi.RecompressResult()
        check(self.lib.flacmi_recompress_host(self.ctx, data_ptr, nbytes, first_byte, C.byref(dp), max_block_size,
                                              int(final_chunk), int(restart), block_len, C.byref(params), C.byref(fp),
                                              C.byref(res)), "flacmi_recompress_host")
        nb = int(res.blocks_out)
        offsets = np.zeros(nb + 1, dtype=np.int64)
        status = np.zeros(max(nb, 1), dtype=np.int32)
        out = (out_alloc(int(res.frame_bytes))[:int(res.frame_bytes)] if out_alloc is not None
               else np.empty(int(res.frame_bytes), dtype=np.uint8))
        check(self.lib.flacmi_recompress_fetch(self.ctx, offsets.ctypes.data, status.ctypes.data, nb,
                                               out.ctypes.data if out.size else None, out.size),
              "flacmi_recompress_fetch")
        return res, out, offsets, status[:nb]

    def decode_stream(self, data_ptr: int, nbytes: int, first_byte: int, channels: int, sample_size: int,
                      check_crc: bool, max_block_size: int, final_chunk: bool, pcm_ptr: int, pcm_capacity: int,
                      raw: bool, bytes_per_sample: int, spec_wasted_bits: bool = False) -> abi.StreamResult:
        """flacmi_decode_stream_host: one chunk of host stream bytes -> host PCM."""
        dp = abi.DecodeParams()
        dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = channels, sample_size, -1, int(check_crc)
        dp.reserved0 = abi.DECODE_WASTED_SPEC if spec_wasted_bits else 0
        res = abi.StreamResult()
        check(self.lib.flacmi_decode_stream_host(self.ctx, data_ptr, nbytes, first_byte, C.byref(dp), max_block_size,
                                                 int(final_chunk), pcm_ptr, pcm_capacity,
                                                 abi.PCM_RAW32 if raw else abi.PCM_PACKED, bytes_per_sample,
                                                 C.byref(res)), "flacmi_decode_stream_host")
        return res

    # ------------------------------------------------------------------------------
    # stream analysis (include/flacmi.h flacmi_frame_info_device / flacmi_info_stream_host)
    # ------------------------------------------------------------------------------
    def frame_info(self, data, offsets, channels: int, sample_size: int, part_stride: int = 64,
                   sentinel: int = 0xEE, spec_wasted_bits: bool = False):
        """Host bytes and frame starts in -> (FRAME_INFO_DTYPE [n], SUBFRAME_INFO_DTYPE [n][channels],
        part_params uint8 [n][channels][part_stride]) from k_frame_info.  The three arrays are
        filled with `sentinel` bytes first, so what the kernel did not write shows."""
        import torch
        dev = torch.device("cuda", self.device)
        nb, n = int(len(data)), len(offsets)
        buf = torch.zeros(((nb + 3) // 4) * 4 + 16, dtype=torch.uint8, device=dev)
        if nb:
            buf[:nb] = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(dev)
        off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(dev)

        def filled(nbytes):
            return torch.full((max(nbytes, 8),), sentinel, dtype=torch.uint8, device=dev)
        fi = filled(n * abi.FRAME_INFO_DTYPE.itemsize)
        si = filled(n * channels * abi.SUBFRAME_INFO_DTYPE.itemsize)
        pp = filled(n * channels * part_stride)
        dp = abi.DecodeParams()
        dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = channels, sample_size, -1, 0
        dp.reserved0 = abi.DECODE_WASTED_SPEC if spec_wasted_bits else 0
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(self.lib.flacmi_frame_info_device(self.ctx, buf.data_ptr(), nb, off.data_ptr(), n, C.byref(dp),
                                                fi.data_ptr(), si.data_ptr(), pp.data_ptr() if part_stride else None,
                                                part_stride, stream), "flacmi_frame_info_device")
        torch.cuda.synchronize(dev)
        return (fi.cpu().numpy()[:n * abi.FRAME_INFO_DTYPE.itemsize].view(abi.FRAME_INFO_DTYPE),
                si.cpu().numpy()[:n * channels * abi.SUBFRAME_INFO_DTYPE.itemsize].view(abi.SUBFRAME_INFO_DTYPE)
                .reshape(n, channels),
                pp.cpu().numpy()[:n * channels * part_stride].reshape(n, channels, part_stride))

    def info_stream(self, data_ptr: int, nbytes: int, first_byte: int, channels: int, sample_size: int,
                    final_chunk: bool, frames: np.ndarray, subframes: np.ndarray, parts: np.ndarray,
                    spec_wasted_bits: bool = False) -> abi.InfoResult:
        """flacmi_info_stream_host: one chunk of host stream bytes -> the records of its frames
        in frames [capacity] (FRAME_INFO_DTYPE), subframes [capacity][channels]
        (SUBFRAME_INFO_DTYPE) and parts [capacity][channels][part_stride] (uint8)."""
        dp = abi.DecodeParams()
        dp.channels, dp.sample_size, dp.first_frame, dp.check_crc = channels, sample_size, -1, 0
        dp.reserved0 = abi.DECODE_WASTED_SPEC if spec_wasted_bits else 0
        res = abi.InfoResult()
        part_stride = parts.shape[2]
        assert subframes.shape == (len(frames), channels) and parts.shape[:2] == (len(frames), channels)
        check(self.lib.flacmi_info_stream_host(self.ctx, data_ptr, nbytes, first_byte, C.byref(dp), int(final_chunk),
                                               frames.ctypes.data, subframes.ctypes.data,
                                               parts.ctypes.data if part_stride else None, part_stride, len(frames),
                                               C.byref(res)), "flacmi_info_stream_host")
        return res

    def timing(self) -> dict:
        """Average k_lpc / k_resid / whole-call milliseconds over the analyze calls since
        the last timing_reset() (HIP events recorded on each call's stream)."""
        ms = (C.c_float * 4)()
        k = self.lib.flacmi_last_timing(self.ctx, ms, 4)
        if k < 0:
            check(k, "flacmi_last_timing")
        return {"lpc_ms": ms[0], "resid_ms": ms[1], "call_ms": ms[2], "calls": int(ms[3])}

    def timing_reset(self) -> None:
        check(self.lib.flacmi_timing_reset(self.ctx), "flacmi_timing_reset")

    def synth_device(self, dst_ptr: int, sample_bytes: int, sample_bits: int, unit_stride: int,
                     first_unit: int, n_units: int, length: int, seed: int, stream: int = 0,
                     open_eighths: int = 0) -> None:
        """Synthetic units on the device (flacmi_synth_mix_device; open_eighths / 8 of them the
        "open" mix's near-white noise)."""
        done = 0
        while done < n_units:
            k = min(1 << 30, n_units - done)
            check(self.lib.flacmi_synth_mix_device(self.ctx, dst_ptr + done * unit_stride * sample_bytes,
                                                   sample_bytes, sample_bits, unit_stride, first_unit + done,
                                                   k, length, seed, open_eighths, stream), "flacmi_synth_mix_device")
            done += k

    def stream_stats(self, meta_ptr: int, n_units: int, block_len: int, stats_ptr: int,
                     stream: int = 0, tail_len: int = 0, n_tail_units: int = 0) -> None:
        check(self.lib.flacmi_stream_stats(self.ctx, meta_ptr, n_units, block_len, tail_len,
                                           n_tail_units, stats_ptr, stream), "flacmi_stream_stats")


class StatsComm:
    """The cross-GPU stream-statistics reduce of the C-ABI (flacmi_comm_* /
    flacmi_allreduce_stats: RCCL over xGMI), for callers without torch.distributed.  Rank 0
    calls comm_id() and hands the bytes to every rank; every rank builds StatsComm(az,
    nranks, rank, id) (a collective call)."""

    def __init__(self, az: "Analyzer", nranks: int, rank: int, comm_id: bytes):
        if len(comm_id) != abi.COMM_ID_BYTES:
            raise ValueError(f"comm id must be {abi.COMM_ID_BYTES} bytes")
        self.lib = az.lib
        buf = C.create_string_buffer(bytes(comm_id), abi.COMM_ID_BYTES)
        h = C.c_void_p()
        check(self.lib.flacmi_comm_init(az.ctx, nranks, rank, buf, C.byref(h)), "flacmi_comm_init")
        self.comm = h.value

    @staticmethod
    def available(lib) -> None:
        """Raises FlacmiError unless RCCL loads here (no id made: the check every rank runs
        before rank 0's comm_id and the collective init)."""
        check(lib.flacmi_comm_available(), "flacmi_comm_available")

    @staticmethod
    def comm_id(lib) -> bytes:
        buf = C.create_string_buffer(abi.COMM_ID_BYTES)
        check(lib.flacmi_comm_id(buf), "flacmi_comm_id")
        return buf.raw

    def allreduce_stats(self, stats_ptr: int, stream: int = 0) -> None:
        check(self.lib.flacmi_allreduce_stats(self.comm, stats_ptr, stream), "flacmi_allreduce_stats")

    def close(self) -> None:
        if self.comm:
            check(self.lib.flacmi_comm_destroy(self.comm), "flacmi_comm_destroy")
            self.comm = None


def unit_result(out: dict, i: int) -> dict:
    """Per-unit dict view of analyze() results (the keys tests/golden_util.check reads)."""
    m = out["meta"][i]
    r = {name: int(m[name]) for name in abi.META_DTYPE.names if name != "coefs"}
    r["coefs"] = [int(c) for c in m["coefs"][: int(m["ncoefs"])]]
    r["rice_params"] = out["rice_params"][i][: int(m["n_parts"])]
    off, ln = int(m["res_offset"]), int(m["res_len"])
    r["residual"] = out["residual"][i][off: off + ln].astype(np.uint64)
    for k in ("acf", "fixed_sums", "lpc_sums"):
        r[k] = out[k][i] if k in out else None
    r["lpc_record"] = out["lpc_records"][i] if "lpc_records" in out else None
    return r
