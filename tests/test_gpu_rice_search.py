"""k_rice_search alone (FLACMI_FLAG_RICE_SEARCH, csrc/k_rice.hip): FLACMI_MODE_RICE_ONLY calls on
device buffers, with and without the flag, against tests/rice_search_model.py.

Every call runs twice on identically pre-filled device buffers.  The run with the flag clear is
what the analysis leaves; the run with it set must differ from that only in the searched fields of
the units the rule covers: part_order, n_parts, coding_method, rice_bits, res_offset, res_len, the
first n_parts rice_params words and, on a rescued unit, status and site.  The searched values are
the model's on the zig-zag of the input rows, computed here, not read from the device.  Residual
rows, rice_params words at and past n_parts (guard words included) and every other meta field are
compared byte for byte between the two runs."""
import numpy as np
import pytest

import oracle
import rice_search_model as RM
from flac_amd import abi
from flac_amd.analysis import Analyzer, knob, make_params, unit_stride

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def az():
    a = Analyzer(0)
    yield a
    a.close()


def zigzag(x):
    x = np.asarray(x, dtype=np.int64)
    return ((x << 1) ^ (x >> 63)).astype(np.uint64)


def device_call(az, rows, n, P, rmin, rmax, flag, tail=0, n_tail=0, residual_bytes=4, bits=32):
    """One RICE_ONLY flacmi_analyze_device call on pre-filled buffers -> numpy copies."""
    import torch
    dev = torch.device("cuda", 0)
    nu = rows.shape[0]
    stride = unit_stride(n, rows.dtype.itemsize)
    s = np.zeros((nu, stride), dtype=rows.dtype)
    s[:, :rows.shape[1]] = rows
    d_s = torch.from_numpy(s).to(dev)
    pstride = (1 << rmax) + 1 + 3  # three guard words more than the interface asks for
    rstride = ((n * residual_bytes + 15) // 16) * 16 // residual_bytes
    d_meta = torch.full((nu, abi.META_DTYPE.itemsize), 0xEE, dtype=torch.uint8, device=dev)
    d_rice = torch.full((nu, pstride), GUARD, dtype=torch.int32, device=dev)
    d_res = torch.full((nu, rstride * residual_bytes), 0xEE, dtype=torch.uint8, device=dev)
    p = make_params(0, 5, rmin, rmax, abi.MODE_RICE_ONLY, rice_search=flag)
    p.reserved[0] = P
    az.analyze_device(d_s.data_ptr(), rows.dtype.itemsize, bits, stride, nu, n, p, d_meta.data_ptr(),
                      d_rice.data_ptr(), pstride, d_res.data_ptr(), rstride, residual_bytes,
                      torch.cuda.current_stream(dev).cuda_stream, tail, n_tail)
    torch.cuda.synchronize(dev)
    return {"meta": d_meta.cpu().numpy().view(abi.META_DTYPE).reshape(-1), "rice_params": d_rice.cpu().numpy(),
            "residual": d_res.cpu().numpy()}


def check_call(az, rows, n, P, rmin, rmax, tail=0, n_tail=0, residual_bytes=4, bits=32, expect_rescued=None):
    nu = rows.shape[0]
    lens = [tail if u >= nu - n_tail else n for u in range(nu)]
    base = device_call(az, rows, n, P, rmin, rmax, False, tail, n_tail, residual_bytes, bits)
    got = device_call(az, rows, n, P, rmin, rmax, True, tail, n_tail, residual_bytes, bits)
    assert np.array_equal(got["residual"], base["residual"]), "a residual row changed"
    rescued = 0
    for u in range(nu):
        b, g, ln = base["meta"][u], got["meta"][u], lens[u]
        st, site = int(b["status"]), int(b["site"])
        want = RM.search_np(zigzag(rows[u, P:ln]), ln, P, rmin, rmax) if ln > P else None
        if want is None:  # no candidate order: the unit keeps the reference's AssertionError
            assert (st, site) == (abi.STATUS_ASSERTION, 11), (u, st, site)
        if want is None or not RM.searched_unit(st, site):
            assert g.tobytes() == b.tobytes() and np.array_equal(got["rice_params"][u], base["rice_params"][u]), u
            continue
        assert (int(g["status"]), int(g["site"])) == (0, 0), u
        rescued += st != 0
        for f in RM.SEARCHED:
            assert int(g[f]) == want[f], (u, f, int(g[f]), want[f])
        k = want["n_parts"]
        assert [int(v) for v in got["rice_params"][u][:k]] == want["rice_params"], u
        assert np.array_equal(got["rice_params"][u][k:], base["rice_params"][u][k:]), f"unit {u}: a word past n_parts changed"
        assert (got["rice_params"][u][-3:] == GUARD).all()
        same = [f for f in abi.META_DTYPE.names if f not in RM.SEARCHED + ("status", "site")]
        assert not RM.meta_fields_differ(g, b, same), (u, RM.meta_fields_differ(g, b, same))
        if st == 0:  # where the reference succeeds (parameters <= 30) the search writes no more bits
            ref = [int(v) for v in base["rice_params"][u][: int(b["n_parts"])]]
            if max(ref) <= 30:
                np_ = int(b["n_parts"])
                written = int(b["rice_bits"]) - (4 * np_ if int(b["coding_method"]) == 4 else 3 * np_ + sum(v > 14 for v in ref))
                assert want["W"] <= written, u
    if expect_rescued is not None:
        assert rescued >= expect_rescued, rescued
    return base, got


def value_rows(n, P, omax, seed):
    """The value patterns of the issue, one unit each, as int32 residual rows of n samples (the
    first P are warm-up and never read).  omax: the finest order the call can reach."""
    rng = np.random.default_rng(seed)
    plen = max(n >> max(omax, 0), 1)
    rows = []
    rows.append(np.zeros(n, np.int64))                                   # all zero
    loud = rng.integers(-3000, 3000, n)
    a = loud.copy()
    a[plen:2 * plen] = 0                                                 # one silent partition among loud ones
    rows.append(a)
    b = np.zeros(n, np.int64)
    b[rng.choice(n, max(1, (n * 2) // 5), replace=False)] = -1            # zig-zag mean just below 1
    rows.append(b)
    rows.append(np.ones(n, np.int64) * -1)                               # every value zig-zag 1: the k = 0 / 1 tie
    rows.append(np.full(n, 3 << 12, np.int64))                           # zig-zag 3 << 13: best parameter 14
    rows.append(np.full(n, 3 << 13, np.int64))                           # zig-zag 3 << 14: best parameter 15
    c = np.full(n, 3 << 12, np.int64)
    c[n // 2:] = 3 << 13                                                 # both in one unit
    rows.append(c)
    rows.append(rng.integers(-(1 << 30), 1 << 30, n))                    # near +-2^30
    rows.append(np.where(rng.integers(0, 2, n) == 1, (1 << 30) - 1, -(1 << 30)))
    d = np.zeros(n, np.int64)
    d[min(n - 1, P + (n - P) // 2)] = 1 << 15                            # a spike of 2^15 in silence
    rows.append(d)
    rows.append(loud)
    rows.append(rng.integers(-3, 4, n))
    e = rng.integers(-2, 3, n)
    e[rng.choice(n, max(1, n // 32), replace=False)] = 5000              # outliers carry the mean
    rows.append(e)
    return np.stack(rows).astype(np.int32)


SHAPES = [  # n, predictor order, rice range: what it reaches
    (16, 0, 0, 4),      # partitions of 1
    (16, 3, 0, 4),      # orders cut by (n >> o) > P
    (24, 0, 0, 5),      # orders cut by divisibility
    (23, 0, 0, 5),      # order 0 only
    (23, 0, 1, 5),      # FLACMI_SITE_RICE_NO_ORDER kept
    (192, 2, 2, 2),     # a single-order range
    (4096, 0, 0, 8),    # 256 partitions of 16
    (4608, 12, 0, 5),   # the config-2 shape
    (16384, 32, 0, 8),  # the config-3 shape
]


@pytest.mark.parametrize("n,P,rmin,rmax", SHAPES, ids=lambda v: str(v))
def test_shapes_and_values(az, n, P, rmin, rmax):
    orders = RM.candidate_orders(n, P, rmin, rmax)
    rows = value_rows(n, P, orders[-1] if orders else 0, 100 * n + P)
    base, got = check_call(az, rows, n, P, rmin, rmax, expect_rescued=2 if orders else 0)
    if orders:
        # all zero: k = 0 everywhere and the tie between the orders goes to rice_min
        m = got["meta"][0]
        assert int(m["part_order"]) == rmin and not got["rice_params"][0][: int(m["n_parts"])].any()
        assert int(base["meta"]["status"][0]) == abi.STATUS_VALUE_ERROR and int(base["meta"]["site"][0]) == 12
        assert {int(v) for v in got["meta"]["coding_method"]} == {4, 5}
        assert {int(v) for v in base["meta"]["site"]} >= {0, 12, 13}


def test_partitions_of_one_value_take_the_smaller_parameter_of_a_tie(az):
    rows = value_rows(16, 0, 4, 1)[3:4]
    _, got = check_call(az, rows, 16, 0, 4, 4)
    assert int(got["meta"]["n_parts"][0]) == 16 and not got["rice_params"][0][:16].any()


def test_tail_units_in_a_batch(az):
    """192-sample units, the last two cut to 77 samples (order 0 only there); int16 rows."""
    rng = np.random.default_rng(7)
    rows = rng.integers(-900, 900, (10, 192)).astype(np.int16)
    rows[2, 48:96] = 0
    rows[3] = 0
    rows[8, 20:60] = 0
    rows[8:, 77:] = 0
    _, got = check_call(az, rows, 192, 1, 0, 4, tail=77, n_tail=2, bits=16, expect_rescued=2)
    assert [int(v) for v in got["meta"]["part_order"][8:]] == [0, 0]
    assert [int(v) for v in got["meta"]["res_len"][8:]] == [76, 76]


@pytest.mark.parametrize("grid", [0, 7])
def test_grid_loop(az, grid):
    """300 units: more than the grid holds once FLACMI_RICE_GRID caps it (and the default grid)."""
    rng = np.random.default_rng(300)
    rows = rng.integers(-200, 200, (300, 192)).astype(np.int32)
    amp = rng.integers(0, 12, 300)
    rows = (rows.astype(np.int64) << amp[:, None]).astype(np.int32)
    for u in range(0, 300, 3):
        rows[u, 24 * (u % 8): 24 * (u % 8) + 24] = 0
    with knob("FLACMI_RICE_GRID", grid):
        check_call(az, rows, 192, 0, 0, 3, expect_rescued=50)


def test_uint64_rows(az):
    """The same search on 8-byte residual rows, as the FLACMI_STATUS_RESIDUAL_WIDE redo runs it."""
    for n, P, rmin, rmax in [(16, 3, 0, 4), (23, 0, 0, 5), (192, 2, 0, 4), (4096, 0, 0, 8), (4608, 12, 0, 5)]:
        rows = value_rows(n, P, RM.candidate_orders(n, P, rmin, rmax)[-1], 64 * n)
        check_call(az, rows, n, P, rmin, rmax, residual_bytes=8, expect_rescued=2)


def test_residual_wide_then_the_uint64_redo(az):
    """32-bit samples whose chosen fixed residual needs 33 bits and more: the 4-byte call reports
    FLACMI_STATUS_RESIDUAL_WIDE and the search leaves the unit alone; the redo on 8-byte rows
    carries the flag and takes parameter 30 in the partition (two values, order 3 of 16) where
    floor(log2(mean)) is 31, the 5-bit escape code."""
    n = 16
    x = np.zeros((3, n), dtype=np.int64)
    x[0] = np.arange(n) * 3 - (1 << 31) + 5
    x[0, 10:] += (1 << 32) - 64                   # one step of almost 2^32: order 1 wins, its residual needs 33 bits
    x[1] = np.random.default_rng(2).integers(-5000, 5000, n)
    x[2] = x[0][::-1]
    rows = x.astype(np.int32)
    assert np.array_equal(rows.astype(np.int64), x)
    ora = oracle.analyze_batch(rows, oracle.make_params(0, 5, 3, 3, abi.MODE_FIXED_ONLY), n, sample_bits=32)
    assert int(ora["meta"]["status"][0]) == 0 and 31 in [int(v) for v in ora["rice_params"][0][: int(ora["meta"]["n_parts"][0])]]
    assert int(ora["residual"][0].max()) >= 1 << 32
    want = RM.apply(ora, [n] * 3, 3, 3, fast=False)
    out = az.analyze(rows, make_params(0, 5, 3, 3, abi.MODE_FIXED_ONLY, rice_search=True), n, sample_bits=32)
    assert out["residual"].dtype == np.uint64
    for u in range(3):
        assert not oracle.meta_mismatches(out["meta"][u], want["meta"][u]), (u, oracle.meta_mismatches(out["meta"][u], want["meta"][u]))
        k = int(want["meta"]["n_parts"][u])
        assert np.array_equal(out["rice_params"][u][:k], want["rice_params"][u][:k])
        off, ln = int(want["meta"]["res_offset"][u]), int(want["meta"]["res_len"][u])
        assert np.array_equal(out["residual"][u][off:off + ln], ora["residual"][u][off:off + ln])
    prm = [int(v) for v in out["rice_params"][0][: int(out["meta"]["n_parts"][0])]]
    assert max(prm) == 30 and int(out["meta"]["coding_method"][0]) == 5
    # the 4-byte pass alone: the wide unit is left as the analysis reported it
    p4 = make_params(0, 5, 3, 3, abi.MODE_FIXED_ONLY, rice_search=True)
    import ctypes as C
    stride = unit_stride(n, 4)
    s = np.zeros((3, stride), dtype=np.int32)
    s[:, :n] = rows
    b = abi.Batch()
    b.samples, b.sample_bytes, b.sample_bits, b.unit_stride, b.n_units, b.block_len = s.ctypes.data, 4, 32, stride, 3, n
    meta = np.zeros(3, dtype=abi.META_DTYPE)
    rice = np.zeros((3, 9), dtype=np.int32)
    res = np.zeros((3, 16), dtype=np.uint32)
    o = abi.Outputs()
    o.meta, o.rice_params, o.params_stride = meta.ctypes.data, rice.ctypes.data, 9
    o.residual, o.residual_bytes, o.residual_stride = res.ctypes.data, 4, 16
    assert az.lib.flacmi_analyze_host(az.ctx, C.byref(b), C.byref(p4), C.byref(o)) == 0
    assert [int(v) for v in meta["status"]] == [abi.STATUS_RESIDUAL_WIDE, 0, abi.STATUS_RESIDUAL_WIDE]
    assert int(meta["n_parts"][0]) == 0 and int(meta["n_parts"][1]) >= 1


def test_refused_combinations(az):
    from flac_amd._lib import FlacmiError
    a = np.zeros((1, 64), dtype=np.int16)
    a[0, ::3] = 100
    with pytest.raises(FlacmiError):
        az.analyze(a, make_params(8, 5, 0, 3, abi.MODE_LPC_ONLY, rice_search=True), 64)
    with pytest.raises(FlacmiError):
        az.analyze(np.zeros((1, 1024), dtype=np.int16), make_params(8, 5, 0, 9, rice_search=True), 1024)
    az.analyze(np.zeros((1, 1024), dtype=np.int16), make_params(8, 5, 0, 9), 1024)  # without the flag: as before
