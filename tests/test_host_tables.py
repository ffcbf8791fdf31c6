"""Host-only check of avec_amd/csrc/host_tables.h, the HIP-free bookkeeping behind api.hip: the reduction-workspace registry (a stream-bound entry wins, one that is too
small gives none, replace in place, (NULL, 0) unregisters, the fifth stream-bound entry is refused) and the dynamic-LDS opt-in table (at most 48 KB makes no call, growth
makes one more, the same or a smaller size none, a refusal is remembered, devices are independent), then both classes from two threads at once.

tests/host_tables_main.cpp is a stand-alone program with its own main; it is built with -fsanitize=thread and run directly (nothing is loaded into Python), so a data race
in either class is a failure of this test and not a rare wrong workspace on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_tables_main.cpp")
INC = os.path.join(ROOT, "avec_amd", "csrc")
PROBE = "#include <thread>\nint main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }\n"


def _compilers():
    c = [shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
    return [x for x in c if x and os.path.exists(x)]


def _tsan_compiler(tmp):
    """the first compiler that builds AND runs a threaded program under the thread sanitizer (the runtime library may be missing, or the kernel's address-space
    layout unsupported by it)"""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write(PROBE)
    why = []
    for cxx in _compilers():
        exe = os.path.join(tmp, "probe")
        r = subprocess.run([cxx, "-std=c++17", "-fsanitize=thread", "-pthread", probe, "-o", exe], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        if r.returncode == 0:
            return cxx, why
        why.append("%s: %s" % (cxx, (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200]))
    return None, why


def test_registry_and_lds_optin_rules_under_thread_sanitizer(tmp_path):
    cxx, why = _tsan_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with a working thread sanitizer: " + ("; ".join(why) or "no compiler found"))
    exe = str(tmp_path / "host_tables")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I" + INC, SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66"))
    assert r.returncode == 0 and "host_tables OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
