"""Sanitizer build of the library's host-side parser ("compile host C++ with -fsanitize=address,undefined in
tests"; VERDICT r2 hygiene item).  csrc/flac.hip - host code only, the one place where the library walks untrusted
bytes - is compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer together with tests/sanitize/
flac_driver.cpp, and run over well-formed streams of every coding variant plus ~600 truncated and bit-flipped versions
of each: the good ones must decode (exit code 0), the damaged ones must be refused with an error code, and the
sanitizers must stay silent throughout (an out-of-bounds read on a truncated residual, a shift by a corrupted Rice
parameter, a signed overflow in the LPC sum would all abort the run)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_writer as FW
from test_flac_cpu import _lpc, _speechlike

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_flac_decoder_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "flac_driver")
    # host code only: -fno-gpu-sanitize keeps the sanitizers off any device code the driver might still form
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-g", "-O1", "-std=c++17", "-w", os.path.join(ROOT, "nspeech_amd", "csrc", "flac.hip"),
           os.path.join(ROOT, "tests", "sanitize", "flac_driver.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    files = []
    # mono LPC (LibriSpeech-like), 16 bit
    pcm = _speechlike(4096 + 700, 1)
    frames = [dict(size=4096, subframes=[dict(_lpc(pcm[:4096, 0], 8), porder=3)]),
              dict(size=700, subframes=[dict(_lpc(pcm[4096:, 0], 6), porder=0)])]
    files.append(("lpc.flac", FW.encode(pcm, 16, 16000, frames)))
    # stereo: every subframe type / decorrelation / Rice method / escape partitions / wasted bits
    n = 576 + 256 * 3 + 100
    st = _speechlike(n, 2, channels=2)
    st[:576] = (st[:576] >> 2) << 2
    frames = [
        dict(size=576, assignment="left_side", subframes=[dict(type="fixed", order=2, wasted=2, method=1, porder=1), dict(type="verbatim", wasted=2)]),
        dict(size=256, assignment="side_right", subframes=[dict(type="fixed", order=4, method=1, params=[17]),
                                                          dict(type="fixed", order=2, porder=1, params=[("esc", 17), 9])]),
        dict(size=256, assignment="mid_side", subframes=[_lpc(((st[832:1088, 0] + st[832:1088, 1]) >> 1), 12, prec=15), dict(type="fixed", order=1, porder=3)]),
        dict(size=256, assignment="independent", subframes=[dict(type="fixed", order=3, porder=4), dict(type="fixed", order=0)]),
        dict(size=100, assignment="independent", subframes=[dict(type="fixed", order=4), dict(type="verbatim")]),
    ]
    files.append(("stereo.flac", FW.encode(st, 16, 22050, frames, variable=True, padding_block=40)))
    # 24-bit, no total / no MD5 in STREAMINFO
    p24 = _speechlike(1152, 3, bps=24)
    files.append(("b24.flac", FW.encode(p24, 24, 48000, [dict(size=1152, subframes=[dict(type="fixed", order=2, porder=2)])],
                                        total_in_header=False, md5=False)))
    paths = []
    for name, blob in files:
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(blob)
        paths.append(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    good = [l for l in lines if not l.startswith("  ")]
    assert len(good) == 3 and all(" rc 0 " in l for l in good), good
    # decoded sample counts of the intact files
    for l, want in zip(good, (len(pcm), n, 1152)):
        assert (" decoded %d " % want) in l, l
    damaged = [l for l in lines if l.startswith("  ")]
    assert len(damaged) > 300
    # a truncated stream is never accepted as complete when STREAMINFO carries the total
    cuts = [l for l in damaged if l.startswith("  cut@")]
    assert sum(" rc 0 " in l for l in cuts) <= len(cuts) // 10, [l for l in cuts if " rc 0 " in l][:5]
