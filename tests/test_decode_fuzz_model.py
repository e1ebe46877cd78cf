"""The decoder fuzz without a device: the generator (decode_fuzz_cases.py), the plain model
(decode_model.py) and the reference's recorded verdicts (golden/decode_fuzz.json, made by
golden/make_decode_fuzz_golden.py) agree on every frame, the generator's axes are all present, and
few mutated frames leave the kernels' documented domain.  tests/test_gpu_decode_fuzz.py then
takes its expectations from the model.

The reference reads an L_R frame as two subframes; the model's `channels` matters for L_R
frames only, so the model is held to the fixture with channels = 2.
"""
import hashlib
import json
import os

import pytest

import decode_fuzz_cases as G
import decode_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_fuzz.json")
DROP_CAP = 0.10
# the reference's sample-rate table has no entry for code 11 (KeyError); the device reads 96 kHz
# (flacmi.h, the stream analysis), so this one frame has no reference verdict
NO_REFERENCE = {"sample_rate_code_11": "KeyError"}
PINNED_WIDE = "pinned_L_S_ss32_side33"


def load_fixture():
    with open(GOLDEN) as f:
        fx = json.load(f)
    fx["by_name"] = {row[0]: dict(zip(fx["fields"], row)) for row in fx["cases"]}
    return fx


def sample_hash(channels):
    if any(not -(1 << 63) <= v < (1 << 63) for ch in channels for v in ch):
        return None  # no int64 layout (mutated frames far outside the domain): the fixture holds None too
    return hashlib.sha256(b"".join(int(v).to_bytes(8, "little", signed=True) for ch in channels for v in ch)).hexdigest()


def is_dropped(case):
    """Outside the kernels' documented domain, as the device reads the frame or as the reference does."""
    for channels in (case.channels, 2):
        try:
            M.decode(case.data, channels, case.sample_size)
        except M.OutOfDomain:
            return True
    return False


@pytest.fixture(scope="module")
def cases():
    return G.frames(G.SEED)


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_generated_bytes_are_the_fixtures(cases, fixture):
    assert fixture["seed"] == G.SEED
    assert [c.name for c in cases] == [row[0] for row in fixture["cases"]]
    for c in cases:
        assert hashlib.sha256(c.data).hexdigest() == fixture["by_name"][c.name]["sha256"], c.name
    assert (fixture["valid"], fixture["mutated"], fixture["cut"]) == \
        (sum(c.truth is not None for c in cases), sum(c.name[0] == "m" and c.truth is None for c in cases),
         sum(c.name[0] == "c" and c.truth is None for c in cases))
    assert fixture["valid"] >= 390 and fixture["mutated"] == 200 and fixture["cut"] == 20


def test_model_gives_the_references_verdict(cases, fixture):
    """Exception class, or sample hash, block size and the reader's end, for every frame (the
    unbounded model: the reference has no int32 domain)."""
    for c in cases:
        want = fixture["by_name"][c.name]
        if c.name in NO_REFERENCE:
            assert want["exception"] == NO_REFERENCE[c.name]
            continue
        try:
            got = M.decode(c.data, 2, c.sample_size, domain=False)
        except M.OutOfDomain:  # a unary run of more than 2^20 zeros: dropped (counted below)
            assert c.truth is None, c.name
            continue
        if isinstance(got, M.Failed):
            assert want["exception"] == got.exception.__name__, (c.name, got.site)
            if got.site == "neg_shift":  # raised by decode_frame: get_frame had read the frame
                assert (want["block_size"], want["end"]) == (got.report["block_size"], got.end), c.name
            else:
                assert want["end"] is None, c.name
        else:
            assert want["exception"] is None, (c.name, want["exception"])
            assert want["decoded_sha256"] == sample_hash(got.samples), c.name
            assert (want["block_size"], want["end"]) == (got.report["block_size"], got.end), c.name


def test_model_report_equals_the_generators_truth(cases):
    """Every field of the frame and subframe records, the samples before and after recombination."""
    for c in cases:
        if c.truth is None or "subframes" not in c.truth:
            continue
        got = M.decode(c.data, c.channels, c.sample_size)
        assert isinstance(got, M.Decoded), (c.name, got)
        assert got.samples == c.truth["samples"] and got.subframes == c.truth["subframe_samples"], c.name
        assert got.end == c.truth["end"] == len(c.data), c.name
        for k, v in got.report.items():
            if k != "subframes":
                assert v == c.truth[k], (c.name, k, v, c.truth[k])
        assert len(got.report["subframes"]) == len(c.truth["subframes"]), c.name
        for n, (s, t) in enumerate(zip(got.report["subframes"], c.truth["subframes"])):
            for k, v in s.items():
                assert v == t[k], (c.name, n, k, v, t[k])


def test_pinned_wide_side_frame(cases, fixture):
    """L_S at 32 bits: the side channel is read at 33 bits and leaves int32.  The reference (and
    the unbounded model) restore left and right exactly; inside the kernels' domain the frame
    does not lie."""
    c = next(c for c in cases if c.name == PINNED_WIDE)
    got = M.decode(c.data, 2, 32, domain=False)
    assert got.samples == c.truth["samples"]
    assert max(got.subframes[1]) > M.INT32[1] and got.report["subframes"][1]["sample_bits"] == 33
    assert got.report["subframes"][1]["type"] == "LPC" and got.report["subframes"][1]["shift"] > 0
    assert fixture["by_name"][c.name]["decoded_sha256"] == sample_hash(c.truth["samples"])
    with pytest.raises(M.OutOfDomain):
        M.decode(c.data, 2, 32)
    # the frame tells the two apart: the same residual over a history kept modulo 2^32 restores
    # another right channel, so going on with int32 would be status 0 with wrong samples
    def wrap(v):
        return (v + (1 << 31)) % (1 << 32) - (1 << 31)
    sub = got.report["subframes"][1]
    side, (c0, c1), sh = got.subframes[1], sub["coefficients"], sub["shift"]
    resid = [side[i] - ((c0 * side[i - 1] + c1 * side[i - 2]) >> sh) for i in range(2, len(side))]
    x = [wrap(side[0]), wrap(side[1])]
    for r in resid:
        x.append(wrap(r + ((c0 * x[-1] + c1 * x[-2]) >> sh)))
    assert [wrap(p - q) for p, q in zip(got.subframes[0], x)] != c.truth["samples"][1]


def test_drop_cap(cases, fixture):
    mutated = [c for c in cases if c.truth is None]
    n = sum(is_dropped(c) for c in mutated)
    assert n == fixture["dropped"]
    assert n <= DROP_CAP * fixture["mutated"]
    assert not any(is_dropped(c) for c in cases if c.truth is not None and c.name != PINNED_WIDE)


def test_mutations_reach_many_statements(cases):
    """Not all EOFError: the mutated frames stop at a spread of the catalogue's statements, and
    some still decode."""
    sites = set()
    for c in cases:
        if c.truth is None and not is_dropped(c):
            got = M.decode(c.data, c.channels, c.sample_size)
            sites.add(got.site if isinstance(got, M.Failed) else "ok")
    assert {"ok", "eof", "partitions", "subframe_pad", "subframe_type", "coding_method"} <= sites


# ---- coverage: every axis value of the issue occurs among the valid frames, read from truth ----

def _subs(cases):
    for c in cases:
        if c.truth and "subframes" in c.truth:
            for n, s in enumerate(c.truth["subframes"]):
                code = c.truth["channel_code"]
                side = (code == 8 and n == 1) or (code == 9 and n == 0) or (code == 10 and n == 1)
                yield c, n, s, side


def _ss(c):
    return c.truth["sample_size"] or c.sample_size


def test_coverage_block_sizes_and_header_forms(cases):
    v = [c for c in cases if c.truth and "subframes" in c.truth]
    sizes = {c.truth["block_size"] for c in v}
    assert set(G.BLOCK_SIZES) | {65535} <= sizes
    big = {s["type"] for c, n, s, _ in _subs(cases) if c.truth["block_size"] == 65535}
    assert big == {"CONSTANT", "FIXED"}
    forms = {(c.truth["block_size"], c.truth["bs_form"]) for c in v}
    assert {f for _, f in forms} == {"table", "u8", "u16"}
    assert {(256, "table"), (256, "u8")} <= forms


def test_coverage_partitions(cases):
    seen_len, seen = set(), set()
    for c, n, s, _ in _subs(cases):
        if not s["coding_method"]:
            continue
        bs, po, order = c.truth["block_size"], s["partition_order"], s["order"]
        plen = bs >> po
        seen_len.add(plen)
        seen.add((bs, po))
        if plen - order == 1:
            seen.add("first_partition_of_one")
        kinds = [k for k, _ in s["partitions"]]
        if plen % 4 and len(kinds) > 1:
            seen.add("block_of_4_spans_header")
            if "rice" in kinds and "escape" in kinds:
                seen.add("block_of_4_spans_escape_switch")
        if "escape" in kinds and "rice" in kinds:
            seen |= {"escape_first"} if kinds[0] == "escape" else set()
            seen |= {"escape_last"} if kinds[-1] == "escape" else set()
            if any(kinds[k] == "escape" and "rice" in kinds[:k] and "rice" in kinds[k + 1:] for k in range(len(kinds))):
                seen.add("escape_between")
    assert {1, 2, 3} <= seen_len
    assert {(16, 4), (4096, 12), "first_partition_of_one", "block_of_4_spans_header", "block_of_4_spans_escape_switch",
            "escape_first", "escape_last", "escape_between"} <= seen
    # every partition order a listed block size allows
    for bs in G.BLOCK_SIZES:
        for po in range(13):
            if bs % (1 << po) == 0:
                assert (bs, po) in seen, (bs, po)


def test_coverage_subframe_types_and_lpc(cases):
    types, orders, precs, shifts, ext = set(), set(), set(), set(), set()
    full = False
    for c, n, s, _ in _subs(cases):
        types.add((s["type"], s["order"]) if s["type"] == "FIXED" else s["type"])
        if s["type"] == "LPC":
            orders.add(s["order"])
            precs.add(s["precision"])
            shifts.add(s["shift"])
            p = s["precision"]
            ext |= {"lo"} if -(1 << (p - 1)) in s["coefficients"] else set()
            ext |= {"hi"} if (1 << (p - 1)) - 1 in s["coefficients"] else set()
            full = full or s["order"] == c.truth["block_size"] - 1
    assert {"CONSTANT", "VERBATIM", "LPC"} | {("FIXED", o) for o in range(5)} <= types
    assert set(G.LPC_ORDERS) <= orders and set(G.LPC_PRECISIONS) <= precs and set(G.LPC_SHIFTS) <= shifts
    assert ext == {"lo", "hi"} and full


def test_coverage_residual_coding(cases):
    rice4, rice5, esc, runs = set(), set(), set(), set()
    for c, n, s, _ in _subs(cases):
        for kind, k in s["partitions"]:
            if kind == "escape":
                esc.add(k)
            else:
                (rice4 if s["coding_method"] == 4 else rice5).add(k)
        runs.add(min(s["max_unary"] // 32, 3))
    assert rice4 == set(range(15)) and rice5 == set(range(31))
    assert set(G.ESCAPE_WIDTHS) <= esc
    assert {1, 2, 3} <= runs  # unary runs across one, two and three dwords


def test_coverage_wasted_bits(cases):
    by_type, side = {}, set()
    for c, n, s, is_side in _subs(cases):
        if s["wasted_flag"]:
            z = s["wasted_bits"]
            tag = "ss-2" if s["sample_bits"] == 2 else z
            by_type.setdefault(s["type"], set()).add(tag)
            by_type[s["type"]].add(z)
            if is_side:
                side.add(z)
    for t in ("CONSTANT", "VERBATIM", "FIXED", "LPC"):
        assert {0, 1, 5, "ss-2"} <= by_type[t], (t, by_type[t])
    assert side


def test_coverage_channels_and_stereo(cases):
    codes, mixed = set(), False
    ends = {}
    for c in cases:
        if c.truth and "subframes" in c.truth:
            codes.add(c.truth["channel_code"])
            mixed = mixed or len({(s["type"], s["order"]) for s in c.truth["subframes"]}) == len(c.truth["subframes"]) >= 3
    for c, n, s, is_side in _subs(cases):
        if is_side:
            ss, x = _ss(c), c.truth["subframe_samples"][n]
            if s["wasted_bits"] == 0 and -(1 << ss) in x and (1 << ss) - 1 in x:
                ends[c.truth["channel_code"]] = True
            if c.truth["channel_code"] == 10 and any(v & 1 for v in x):
                ends["odd"] = True
    assert codes == set(range(11)) and mixed
    assert ends == {8: True, 9: True, 10: True, "odd": True}


def test_coverage_sample_sizes_rates_and_numbers(cases):
    v = [c for c in cases if c.truth and "subframes" in c.truth]
    assert {c.truth["sample_size"] for c in v} == {0, 8, 12, 16, 20, 24, 32}
    assert {c.sample_size for c in v if c.truth["sample_size"] == 0} == {4, 8, 12, 16, 17, 20, 24, 32}
    assert {c.truth["rate_code"] for c in v} == set(range(15))
    sizes = {c.truth["header_bytes"] - 5 - {"table": 0, "u8": 1, "u16": 2}[c.truth["bs_form"]]
             - {12: 1, 13: 2, 14: 2}.get(c.truth["rate_code"], 0) for c in v}
    assert sizes == {1, 2, 3, 4, 5, 6, 7}  # coded numbers of 1 to 7 bytes
    seven = [c for c in v if c.truth["number"] >= 1 << 31]
    assert len(seven) == 1 and seven[0].truth["blocking_strategy"] == 1
