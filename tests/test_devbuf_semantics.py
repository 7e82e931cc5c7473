"""DevBuf, the owning device allocation every object of the library is made of, Carver, which slices the build arena, and
PinnedReadback, the page-locked block + event a scalar comes back from the device through, under AddressSanitizer +
UndefinedBehaviorSanitizer on the host.

tests/cpp/devbuf_semantics.cpp includes the product's csrc/rt_internal.h and puts a malloc-backed allocator with a live-block count and
an injectable refusal behind it: scope exit frees, a move leaves its source empty and frees once, move-assignment frees the old block,
an adopted slice is never freed, a failed growth keeps the buffer, out-of-memory-then-retry ends with the new block or an empty buffer,
the allocation limit holds, and a sizing run of the carver ends at the offset of the real one.  The read-back (page-locked memory, events
and the asynchronous copy restated the same way): creation is all or nothing and tried again, a failed send leaves nothing in flight,
landed() is true once per flight, a move empties its source, destruction frees once and never touches the block.  No device, no
library: g++ only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build_san")
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]


def test_devbuf_and_carver_semantics_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "devbuf_semantics")
    src = os.path.join(ROOT, "tests", "cpp", "devbuf_semantics.cpp")
    r = subprocess.run(["g++"] + FLAGS + [src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "0 failures, 0 live allocations" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
