"""The command line's wasted-bits flags on a stream of tests/golden/wasted_streams.json (16-bit
samples << 8 in a 24-bit stream, blocks of 4608): `decode --spec-wasted-bits` writes the WAV of the
input samples and `analyze --spec-wasted-bits` prints wasted_bits=8 for every subframe; and
`encode --wasted-bits` on a WAV file."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import golden_util as G
import wasted_cases as WC

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "big24"


def run(*args):
    return subprocess.run([sys.executable, "-m", "flac_amd", *args], cwd=REPO, capture_output=True, text=True,
                          timeout=300)


@pytest.fixture(scope="module")
def flac(tmp_path_factory):
    p = tmp_path_factory.mktemp("wasted") / f"{NAME}.flac"
    p.write_bytes(WC.stream(NAME, G.load("wasted_streams.json")["cases"][NAME]))
    return p


def test_decode_spec_wasted_bits(flac, tmp_path):
    c = WC.CASES[NAME]
    out = tmp_path / "out.wav"
    r = run("decode", str(flac), str(out), "--spec-wasted-bits", "--check-crc")
    assert r.returncode == 0, r.stderr
    rows, _ = WC.case_rows(NAME)
    want = np.concatenate([rows[u, :ln] for u, ln in enumerate(WC.unit_lens(NAME))])
    with wave.open(str(out), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getnframes()) == (c["C"], 3, len(want))
        raw = np.frombuffer(w.readframes(len(want)), dtype=np.uint8).reshape(-1, 3).astype(np.int32)
    got = (raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)) << 8 >> 8  # 24-bit little-endian, sign-extended
    assert np.array_equal(got, want)


def test_analyze_spec_wasted_bits(flac):
    c = WC.CASES[NAME]
    r = run("analyze", str(flac), "--spec-wasted-bits")
    assert r.returncode == 0, r.stderr
    subs = [ln for ln in r.stdout.splitlines() if ln.startswith("\tsubframe=")]
    assert len(subs) == c["frames"] * c["C"] and all("\twasted_bits=8\t" in ln for ln in subs)


def test_encode_wasted_bits(tmp_path):
    """A 24-bit WAV of 16-bit samples << 8: `encode --wasted-bits` writes a smaller file than without
    the flag, whose subframes declare 8 wasted bits and which `decode --spec-wasted-bits` turns back
    into the same PCM."""
    n = 576
    t = np.arange(4 * n + 100)
    x = (np.stack([np.round(9000 * np.sin(t / 7.0)) + t % 5, np.round(4000 * np.sin(t / 3.0)) - t % 3]).astype(np.int32) | 1) << 8
    wav, plain, small, back = (tmp_path / k for k in ("in.wav", "plain.flac", "small.flac", "back.wav"))
    raw = np.ascontiguousarray(x.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(3)
        w.setframerate(44100)
        w.writeframes(raw)
    args = ["encode", str(wav), "-b", str(n), "-l", "8", "-q", "12", "-r", "3", "--correct-reader"]
    for out, flags in ((plain, []), (small, ["--wasted-bits"])):
        r = run(args[0], args[1], str(out), *args[2:], *flags)
        assert r.returncode == 0, r.stderr
    assert small.stat().st_size < plain.stat().st_size - x.size * 7 // 8  # about 8 bits a sample less
    r = run("analyze", str(small), "--spec-wasted-bits")
    subs = [ln for ln in r.stdout.splitlines() if ln.startswith("\tsubframe=")]
    assert r.returncode == 0 and len(subs) == 10 and all("\twasted_bits=8\t" in ln for ln in subs)
    r = run("decode", str(small), str(back), "--spec-wasted-bits", "--check-crc")
    assert r.returncode == 0, r.stderr
    with wave.open(str(back), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getnframes()) == (2, 3, x.shape[1])
        assert w.readframes(x.shape[1]) == raw
