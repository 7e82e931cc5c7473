"""rt_fbx.cpp's hierarchy flattening under AddressSanitizer + UndefinedBehaviorSanitizer: the fuzz driver of
tests/test_sanitized_parsers.py (tests/cpp/fuzz_parsers.cpp, unchanged, built the same way by that module's fixture) run over seeds
that reach the new code -- a three-level chain with a pre-rotation, pivots and offsets, geometric transforms with a child mesh, an
instanced geometry.  Mutations of those files bend parent connections into cycles, long chains and dangling ids, and property values
into NaN, infinities and enum values no enum holds.  Zero sanitizer reports, and every unmutated seed accepted."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from test_sanitized_parsers import fuzzer  # noqa: F401  (the module-scoped fixture that builds the sanitized driver)

import fbx_hierarchy_tools as H

SEEDS = ("a_three_levels", "b_pivots_and_offsets", "e_geometric_not_inherited", "g_instanced_geometry")
CASES_PER_SEED = 60000


def test_mutation_fuzz_of_the_fbx_hierarchy_code_under_asan_ubsan(fuzzer, tmp_path):  # noqa: F811
    cases = H.cases()
    jobs = []
    for k, name in enumerate(SEEDS):
        geoms, models = cases[name]
        path = str(tmp_path / (name + ".fbx"))
        H.write(path, geoms, models, version=7500 if k % 2 else 7400, compress=False)      # raw arrays: mutations reach the values, not a zlib checksum
        jobs.append((k, path))
    scratch = "/dev/shm" if os.access("/dev/shm", os.W_OK) else str(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:allocator_may_return_null=1:max_allocation_size_mb=2048", UBSAN_OPTIONS="print_stacktrace=1")

    def run(job):
        k, path = job
        tmpf = os.path.join(scratch, "dxr_fuzz_hier_%d_%d" % (os.getpid(), k))
        try:
            return path, subprocess.run([fuzzer, "fbx", path, str(CASES_PER_SEED), str(7000 + k), tmpf], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                        text=True, timeout=600)
        finally:
            if os.path.exists(tmpf):
                os.remove(tmpf)

    with ThreadPoolExecutor(len(jobs)) as ex:
        results = list(ex.map(run, jobs))
    for path, r in results:
        # (exit 1 with "the unmutated seed ... was refused" is the driver's word for a seed the reader does not accept)
        assert r.returncode == 0, "fbx fuzz of %s: exit %d\n%s\n%s" % (path, r.returncode, r.stdout[-500:], r.stderr[-4000:])
        assert "%d cases" % CASES_PER_SEED in r.stdout and "0 sanitizer reports" in r.stdout, r.stdout[-500:]
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        read = int(r.stdout.split(" read,")[0].split()[-1])
        assert read >= 1, r.stdout
