"""libflacmi.so loads, reports its ABI version and exports every symbol include/flacmi.h
declares (CPU-only: no compute call needs a GPU here)."""
import ctypes
import os
import re

from flac_amd import abi
from flac_amd._lib import LIB_PATH, load

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flacmi.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"\b(flacmi_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_abi_version():
    lib = load()
    assert lib.flacmi_abi_version() == abi.ABI_VERSION


def test_every_declared_symbol_is_exported_and_typed():
    lib = ctypes.CDLL(LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 15
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/flacmi.h but not exported"
        assert name in abi.SIGNATURES, f"{name} missing from flac_amd.abi.SIGNATURES"


def test_struct_layouts_match_header(tmp_path):
    """Every field offset of the ctypes mirror equals the C compiler's offsetof()."""
    import subprocess
    structs = {"flacmi_params": abi.Params, "flacmi_batch": abi.Batch,
               "flacmi_unit_meta": abi.UnitMeta, "flacmi_outputs": abi.Outputs,
               "flacmi_frame_params": abi.FrameParams, "flacmi_decode_params": abi.DecodeParams,
               "flacmi_encode_timing": abi.EncodeTiming}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                  check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, f"{cname}.{f}"
    assert abi.META_DTYPE.itemsize == ctypes.sizeof(abi.UnitMeta)


def test_unit_stride_pads_4k_multiple_rows():
    """flacmi_unit_stride: 16-byte rows, plus 128 bytes when the pitch is a multiple of 4 KB
    (config 3's 16384 x int32 rows: k_lpc FETCH 1.72x -> 1.03x of the sample bytes)."""
    from flac_amd.analysis import unit_stride
    lib = load()
    assert unit_stride(4608, 2) == 4608          # config 2: 9216-byte rows, unpadded
    assert unit_stride(1152, 2) == 1152
    assert unit_stride(4097, 2) == 4104          # rounded up to 16 bytes
    assert unit_stride(16384, 4) == 16384 + 32   # config 3
    assert unit_stride(4096, 2) == 4096 + 64
    assert unit_stride(2048, 4) == 2048 + 32
    for n in range(1, 5000, 7):
        for b in (2, 4):
            v = unit_stride(n, b)
            assert v >= n and (v * b) % 16 == 0 and (v * b) % 4096 != 0
    assert lib.flacmi_unit_stride(0, 2) < 0 and lib.flacmi_unit_stride(16, 3) < 0


def test_knobs_set_get_and_reject_unknown_names():
    """flacmi_set_knob / flacmi_get_knob: the test knobs live in atomics, read from the
    environment once; launches never call getenv."""
    from flac_amd.analysis import get_knob, knob
    lib = load()
    for name in ("FLACMI_OVERLAP", "FLACMI_MF8_GRID", "FLACMI_STREAM_GENERIC", "FLACMI_DECODE_GENERIC",
                 "FLACMI_PACK_GENERIC", "FLACMI_DECODE_LPC"):
        before = get_knob(name)
        with knob(name, 7):
            assert get_knob(name) == 7
        assert get_knob(name) == before
    if "FLACMI_DECODE_LPC" not in os.environ:
        assert get_knob("FLACMI_DECODE_LPC") == 1  # the fast decoder's LPC pass is on by default
    assert lib.flacmi_set_knob(b"FLACMI_NOPE", 1) == abi.E_INVALID
    assert b"unknown knob" in lib.flacmi_last_error()
    v = ctypes.c_int32(0)
    assert lib.flacmi_get_knob(None, ctypes.byref(v)) == abi.E_INVALID


def test_create_without_device_fails_loudly():
    lib = load()
    if lib.flacmi_device_count() > 0:
        return
    assert not lib.flacmi_create(0)
    assert b"device" in lib.flacmi_last_error()


def test_decode_site_and_status_codes_match_header():
    """abi.DSITE / STATUS_* mirror enum flacmi_decode_site and the decoder status codes."""
    text = open(HEADER).read()
    body = text[text.index("enum flacmi_decode_site {"):]
    body = body[:body.index("};")]
    names = re.findall(r"FLACMI_DSITE_([A-Z0-9_]+)", body)
    assert [n.lower() for n in names] == list(abi.DSITE)
    assert re.search(r"FLACMI_DSITE_SYNC = 32\b", body)
    assert int(re.search(r"#define FLACMI_STATUS_EOF (\d+)", text).group(1)) == abi.STATUS_EOF
    assert int(re.search(r"#define FLACMI_STATUS_VERIFY (\d+)", text).group(1)) == abi.STATUS_VERIFY


def test_decode_golden_covers_every_reference_exception_site():
    """tests/golden/decode.json (the reference decoder's own verdicts) holds one malformed
    frame per decoder assertion / exception and valid frames of every subframe type."""
    import json
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "decode.json")))["cases"]
    sites = {c["site"] for c in g if c["site"]}
    ref_sites = [n for n in abi.DSITE if abi.DSITE[n] < abi.DSITE["crc8"]]
    assert sorted(sites) == sorted(ref_sites)
    for c in g:
        assert (c["exception"] is None) == (c["site"] is None), c["name"]
        if c["exception"]:
            assert c["exception"] in {e.__name__ for e in abi.STATUS_EXCEPTION.values()}
    names = {c["name"] for c in g if c["exception"] is None}
    for must in ("constant_192", "verbatim_256", "fixed2_wasted2", "lpc32_p15", "stereo_M_S",
                 "lpc6_rice5_escape_bs16", "fixed3_32bit"):
        assert must in names


# The one kernel allowed to spill: k_resid's 64-bit list variant at L <= 32 (kVarList1, the
# units k_resid_sb / kVarMf8 hand over: int64 chains, planes and tiers at 256 VGPRs).  It loops
# over the list with one workgroup per CU (round 5: a workgroup per unit of the batch cost
# 0.09 ms of dispatch per 2e5 units even for an empty list), and the loop costs 52 bytes of
# scratch per lane (212 before its thread id was re-read per unit).  It runs only for listed
# units (none on config 3's data).
ALLOWED_SPILLS = {"_ZN6flacmi7k_residILi32ELi2EjLi4EEEvNS_9ResidArgsE": 64}


def _scratch_instructions(obj):
    """{kernel symbol: number of scratch / buffer memory instructions} in the gfx950 code object
    embedded in a build object (objcopy + clang-offload-bundler + llvm-objdump), or None when
    the tools are missing."""
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb.bin"), os.path.join(d, "k.co")
        try:
            subprocess.run(["objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(d, "x.o")],
                           check=True, capture_output=True)
            subprocess.run([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}"],
                           check=True, capture_output=True)
            dis = subprocess.run([f"{llvm}/llvm-objdump", "-d", co], check=True, capture_output=True,
                                 text=True).stdout
        except (OSError, subprocess.CalledProcessError):
            return None
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif cur and re.search(r"\s(scratch_|buffer_)(load|store)", line):
            out[cur] += 1
    return out


def test_no_kernel_spills_to_scratch():
    """Every kernel in libflacmi.so fits its registers: the Makefile keeps the compiler's
    per-kernel resource report next to each object, and a scratch (spill) size other than 0
    is a several-fold slowdown that no parity test notices (round-2 regression: the generic
    k_resid grew from 75 VGPRs to 256 + 692 B/lane of scratch when its body moved into an
    inlined helper).  A kernel that reports a scratch size but whose machine code holds no
    scratch or buffer memory instruction passes: that is the register scavenger's emergency
    slot, reserved when SGPRs spill to VGPR lanes and never touched (k_pack32 at 106 SGPRs)."""
    import glob
    import pytest
    build = os.path.join(os.path.dirname(LIB_PATH), "csrc", "build")
    reports = sorted(glob.glob(os.path.join(build, "*.res")))
    if not reports:
        pytest.skip("no resource reports (library built elsewhere)")
    spills, kernels = [], 0
    for rep in reports:
        name = None
        isa = None
        for line in open(rep):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name, kernels = m.group(1), kernels + 1
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and int(m.group(1)):
                if name in ALLOWED_SPILLS and int(m.group(1)) <= ALLOWED_SPILLS[name]:
                    continue
                if isa is None:
                    isa = _scratch_instructions(rep[:-4] + ".o") or {}
                if isa.get(name) == 0:
                    continue  # reserved, never used
                spills.append((os.path.basename(rep), name, int(m.group(1))))
    assert kernels >= 40, f"only {kernels} kernels reported"
    assert not spills, f"kernels spilling to scratch: {spills}"
