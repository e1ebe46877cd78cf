"""`python -m flac_amd decode-many` in a fresh process over six fixture streams of three
(channels, sample size) groups (tests/golden/decode_streams.json): one WAV per input whose payload
is the reference cmd_decode's, a failing stream's WAV holds the frames before its stop, the exit
status and stderr name the failing streams, and each file equals what `decode` writes."""
import hashlib
import os
import subprocess
import sys
import wave

import pytest

import frame_index_cases as FI

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["a_ref_192", "j_meta_5", "d_err_sync", "g_24bit", "i_wide_frame", "e_cut_3"]


def payload(path):
    with wave.open(str(path), "rb") as w:
        return (w.getframerate(), w.getsampwidth(), w.getnchannels()), w.readframes(w.getnframes())


def test_cli_decode_many_writes_one_reference_wav_per_input(tmp_path):
    cases = {c["name"]: c for c in FI.load_cases()}
    out = tmp_path / "wav"
    srcs = []
    for n in NAMES:
        p = tmp_path / f"{n}.flac"
        p.write_bytes(bytes.fromhex(cases[n]["hex"]))
        srcs.append(p)
    r = subprocess.run([sys.executable, "-m", "flac_amd", "decode-many", "--out-dir", str(out)] + [str(p) for p in srcs],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    failing = [n for n in NAMES if cases[n]["wav_exception"]]
    assert failing == ["d_err_sync", "i_wide_frame"]
    assert r.returncode == 1, r.stderr
    assert f"Decoding of {len(NAMES)} streams completed in " in r.stdout and "2 stopped" in r.stdout
    stopped = [ln for ln in r.stderr.splitlines() if ln.startswith("stopped\t")]
    assert len(stopped) == 2, r.stderr
    for ln, n in zip(stopped, failing):
        assert f"file={tmp_path / (n + '.flac')}" in ln and f"exception={cases[n]['wav_exception']}" in ln
    assert "frame 2: sync" in stopped[0] and "frame 1: pcm_range" in stopped[1]
    from flac_amd import decoder
    for n, src in zip(NAMES, srcs):
        c = cases[n]
        params, data = payload(out / f"{n}.wav")
        assert params == (c["sample_rate"], c["sample_size"] // 8, c["channels"]), n
        if c["wav_exception"] is None:
            assert hashlib.sha256(data).hexdigest() == c["wav_sha256"] and len(data) == c["wav_bytes"], n
        else:  # the frames before the stop
            assert hashlib.sha256(data).hexdigest() == c["pcm_sha256"] and len(data) == c["pcm_bytes"] > 0, n
        one = tmp_path / f"one_{n}.wav"
        try:
            decoder.decode_wav(src, one)
        except Exception as e:  # noqa: BLE001  -- the file is written up to the stop, as by the CLI
            assert type(e).__name__ == c["wav_exception"], n
        assert (out / f"{n}.wav").read_bytes() == one.read_bytes(), n


def test_cli_decode_many_stops_a_24_bit_stream_at_a_sample_outside_its_width(tmp_path):
    """g_24bit with one more frame whose header declares 32-bit samples and holds 2^23: the int32 rows
    carry it, to_bytes(3) cannot, so the WAV ends before that frame, as `decode` writes it."""
    import frame_assembler as FA
    cases = {c["name"]: c for c in FI.load_cases()}
    c = cases["g_24bit"]
    wide = FA.frame(FA.header(6, 16, ch_code=1, ss_code=7, fno=len(c["block_sizes"])),
                    [lambda b: FA.sub_verbatim(b, [1 << 23] * 16, 32), lambda b: FA.sub_verbatim(b, [-5] * 16, 32)])
    src, good, out = tmp_path / "wide24.flac", tmp_path / "j_meta_7.flac", tmp_path / "wav"
    src.write_bytes(bytes.fromhex(c["hex"]) + wide)
    good.write_bytes(bytes.fromhex(cases["j_meta_7"]["hex"]))
    r = subprocess.run([sys.executable, "-m", "flac_amd", "decode-many", "--out-dir", str(out), str(src), str(good)],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stderr
    stopped = [ln for ln in r.stderr.splitlines() if ln.startswith("stopped\t")]
    assert len(stopped) == 1 and f"file={src}" in stopped[0] and "exception=OverflowError" in stopped[0], r.stderr
    assert f"frame {len(c['block_sizes'])}: pcm_range" in stopped[0]
    _, data = payload(out / "wide24.wav")
    assert hashlib.sha256(data).hexdigest() == c["wav_sha256"] and len(data) == c["wav_bytes"]
    _, data = payload(out / "j_meta_7.wav")
    assert hashlib.sha256(data).hexdigest() == cases["j_meta_7"]["wav_sha256"]
    from flac_amd import decoder
    one = tmp_path / "one.wav"
    with pytest.raises(OverflowError):
        decoder.decode_wav(src, one)
    assert (out / "wide24.wav").read_bytes() == one.read_bytes()
