"""glibc_sincosf_both (liorf_amd/csrc/s2m_glibc_trig.hpp, the twin of s2m_device.hpp's) against the build host's sinf / cosf,
bit for bit, on the CPU: tools/micro/trig_host_check.hip is compiled for the host and run.  Its arguments: 2e6 random values
in [-4, 4], the neighbours (three ulps each side, both signs) of the branch boundaries 2^-12, 0x1.921FB6p-1 and 120, and
k*pi/2 with its neighbours (two ulps each side) for k = -76..76.

glibc's reduction for pi/4 <= |x| < 120 is reduce_fast, ours is the same statement; DESIGN.md records seven mismatches in 1e7
random arguments beyond |x| = 4, all next to a multiple of pi/2.  The set below is what the code gave on these arguments
before its table became literals (the polynomial's sign or quadrant is decided one ulp differently from glibc at 37, 41 and
74 times pi/2): exactly this set is admitted, nothing else and nothing less."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ADMITTED = {("c2e87a55", "s"), ("c280ce28", "c"), ("c2687a55", "c"), ("42687a55", "c"), ("4280ce28", "c"), ("42e87a55", "s")}
N_ARGS = 2000000 + 3 * 7 * 2 + 153 * 5


def test_host_twin_is_the_hosts_libm(tmp_path):
    exe = str(tmp_path / "trig_host_check")
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.check_call([cc, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "trig_host_check.hip"), "-lm"])
    out = subprocess.check_output([exe], text=True).split("\n")
    lines = [l.split() for l in out if l.strip()]
    assert lines[-1][0] == "checked" and int(lines[-1][1]) == N_ARGS, lines[-1]
    got = {(a, w) for a, w in lines[:-1]}
    print("mismatches:", sorted(got))
    assert got == ADMITTED
