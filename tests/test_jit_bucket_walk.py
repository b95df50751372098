"""The generated bucketed matcher (shb_match) for C2, checked on the CPU: the phase
clocks are generated only under SH_BK_PROFILE (read once per process, so both
forms are generated and compiled in child processes), and the per-lane count
walk raises its premise flags once per wave, after its loop."""
import ctypes as C
import os
import subprocess
import sys

from siddhi_amd import abi, build, compiler, synth

HERE = os.path.dirname(os.path.abspath(__file__))

CHILD = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
from siddhi_amd import abi, build, compiler, synth
lib = abi.bind_product(C.CDLL(build.build()))
d = compiler.compile_app(synth.C2_QUERY).descriptor()
h = C.c_void_p()
assert lib.sh_compile(C.byref(d), C.byref(h)) == abi.SH_OK
buf = C.create_string_buffer(1 << 20)
rc = lib.shx_bucket_compile(h, buf, 1 << 20)
src = buf.value.decode()
assert rc == abi.SH_OK, lib.sh_last_error(h)
body = src[src.index("shb_match(shb_plan P)"):]
if {clocks}:
    assert body.count("SHB_PROF(") == 7 and "wall_clock64()" in body and "t_prev" in body
else:
    assert "SHB_PROF" not in body and "wall_clock64" not in body and "t_prev" not in body
print("source ok")
"""


def _bucket_source():
    lib = abi.bind_product(C.CDLL(build.build()))
    d = compiler.compile_app(synth.C2_QUERY).descriptor()
    h = C.c_void_p()
    assert lib.sh_compile(C.byref(d), C.byref(h)) == abi.SH_OK
    buf = C.create_string_buffer(1 << 20)
    rc = lib.shx_bucket_compile(h, buf, 1 << 20)
    src = buf.value.decode()
    assert rc == abi.SH_OK, lib.sh_last_error(h)
    lib.sh_destroy(h)
    return src[src.index("shb_match(shb_plan P)"):]


def _child(clocks):
    env = {k: v for k, v in os.environ.items() if k != "SH_BK_PROFILE"}
    if clocks:
        env["SH_BK_PROFILE"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=os.path.dirname(HERE), clocks=clocks)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "source ok" in r.stdout, r.stderr[-2000:]


def test_no_phase_clocks_unless_asked_for():
    _child(False)


def test_phase_clocks_under_sh_bk_profile():
    _child(True)


def test_count_walk_raises_flags_after_its_loop():
    body = _bucket_source()
    walk = body[body.index("const int dl_ ="):]
    loop = walk[:walk.index("if (__ballot(flg_ != 0u) != 0ull)")]
    assert "atomicOr" not in loop and loop.count("s_cons[") == 1
    tail = walk[len(loop):walk.index("__syncthreads();", len(loop))]
    assert tail.count("atomicOr(P.flag") == 1
