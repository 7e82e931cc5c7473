"""rt_handle, the base of every host object but the context, with rt_retain / rt_release / rt_make and the context's own count, under
AddressSanitizer + UndefinedBehaviorSanitizer on the host.

tests/cpp/handle_semantics.cpp includes the product's csrc/rt_internal.h, restates the few HIP calls behind the base so that each writes
a line to an event log, and stands in for ~rt_context with one that logs.  With a toy type that owns two DevBufs: the last release
selects the device, joins the stream for a type that says so and for no other, frees the buffers and only then lets the context go; an
object retained twice dies at the third release and a null release does nothing; a creation that fails after the object exists leaves
the context's count, the live blocks and *out as they were; of two objects whose context handle went first, the second to go takes the
context with it, whichever that is.  No device, no library: g++ only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build_san")
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]


def test_handle_semantics_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "handle_semantics")
    src = os.path.join(ROOT, "tests", "cpp", "handle_semantics.cpp")
    r = subprocess.run(["g++"] + FLAGS + [src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "0 failures, 0 live allocations" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
