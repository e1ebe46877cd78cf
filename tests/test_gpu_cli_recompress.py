"""`python -m flac_amd recompress` in a fresh process (flac-py_amd/cli.py) on cases of
tests/golden/recompress_streams.json (the reference's decode feeding the reference's encode): the
file written equals the fixture's bytes; --keep-metadata; and a stream that stops: what was
produced before the stop is written, the exception is printed and the exit status is 1, as the
analyze action does."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "recompress_streams.json")))["cases"]}
SOURCES = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "decode_streams.json")))["cases"]}


def run(tmp_path, name, *extra):
    case = GOLD[name]
    src, out = tmp_path / "in.flac", tmp_path / "out.flac"
    src.write_bytes(bytes.fromhex(SOURCES[case["source"]]["hex"] if "source" in case else case["hex"]))
    p = case["parameters"]
    assert p["rice"][0] == 0
    r = subprocess.run([sys.executable, "-m", "flac_amd", "recompress", str(src), str(out), "-b", str(p["block_size"]),
                        "-l", str(p["lpc_stop"] - 1), "-q", str(p["qlp"]), "-r", str(p["rice"][1] - 1), *extra],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    return case, r, out.read_bytes()


@pytest.mark.parametrize("name", ["a_ref_192_to_100", "g_24bit_to_192", "l_3ch_to_100"])
def test_cli_recompress_writes_the_reference_bytes(tmp_path, name):
    case, r, got = run(tmp_path, name, "--check-crc")
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("Recompression completed in ") and r.stdout.rstrip().endswith(" seconds")
    assert got.hex() == case["out_hex"]


def test_cli_keep_metadata(tmp_path):
    case, r, got = run(tmp_path, "k_seektable_keep", "--keep-metadata")
    assert r.returncode == 0, r.stderr
    assert got.hex() == case["out_hex"]
    case, r, got = run(tmp_path, "k_seektable_drop")
    assert r.returncode == 0 and got.hex() == case["out_hex"]


@pytest.mark.parametrize("name", ["d_err_sync_to_100", "m_silent_block_to_64"])
def test_cli_stopping_stream(tmp_path, name):
    case, r, got = run(tmp_path, name)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert got.hex() == case["out_hex"] and case["frames"] > 0      # what it had is written
    assert f"exception={case['exception']}" in r.stdout and r.stdout.startswith("stopped\t")
