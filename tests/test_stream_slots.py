"""rc_stream_slot (raycore.jl_amd/csrc/rc_stream_slots.h): the rule behind the scene's per-stream stack spill regions (8) and totals scratch
areas (16) -- one entry per stream; one stream too many takes over the first idle entry, else waits for the oldest; a taken entry moves to
the back, is re-keyed and keeps its buffer.  The header includes no HIP header, so this CPU test compiles tests/host/stream_slots_main.cpp --
a fake entry type with a scripted `last`, N = 3 -- with the host compiler under AddressSanitizer / UBSan and runs it as a child process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_stream_slot_pool_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_slots")
    base = ["g++", "-std=c++17", "-g", "-I", os.path.join(ROOT, "raycore.jl_amd", "csrc"), os.path.join(HERE, "host", "stream_slots_main.cpp"), "-o", exe]
    # (the sanitizer runtimes linked statically: the program then runs the same whatever libraries its environment preloads)
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if p.returncode != 0 and "san" in p.stderr and "stream_slots_main.cpp:" not in p.stderr:  # no sanitizer runtime on this machine: the plain build still checks the rule
        p = subprocess.run(base, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "stream slots ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
