"""The registry of rt_debug_set_option's options (csrc/rt_api.hip) as plain data: for every option the values the suite runs it
with, or the reason why it is exempt.  tests/test_option_registry.py (CPU) fails when the library has an option this table does
not name, or the other way round; tests/test_gpu_option_matrix.py, tests/test_gpu_update_options.py (scenes that are updated:
rt_scene_update) and tests/fuzz_parity.py take their option lists from here, so that an option entered here is run against the
oracle and an option not entered here fails the CPU suite.

kind "build": read when a model / scene is built (another traversal tree, same hits); "launch": read when a pipeline or a batch
of rays is launched (another shape of launch, same image).  DESIGN.md section 2.1 S2.7: neither may change a bit."""

OPTIONS = {
    # ---- builders
    "leaf_max": dict(kind="build", values=[1, 2, 3, 4, 8]),
    "fast_bvh": dict(kind="build", values=["ploc", "lbvh"]),
    "wide_sah": dict(kind="build", values=[0, 1]),
    "split_refs": dict(kind="build", values=[0, 1]),
    "build_batch": dict(kind="build", values=[0, 1]),
    "sah_node": dict(kind="build", values=[2.5], needs={"wide_sah": 1}),       # (the costs are read by the surface-area collapse only)
    "sah_prim": dict(kind="build", values=[0.25], needs={"wide_sah": 1}),
    "fail_ploc_rounds": dict(kind="build", values=[1]),
    # ---- launches
    "lds_top": dict(kind="launch", values=[0]),
    "lds_stack_rows": dict(kind="launch", values=[6]),
    "persistent_blocks_per_cu": dict(kind="launch", values=[1, 3]),           # (above what is resident is legal but another matter)
    "shadow_cache_res": dict(kind="launch", values=[0, 16, 1024]),
    "shadow_cache_pixels": dict(kind="launch", values=[0, 1]),
    "seven_waves_always": dict(kind="launch", values=[1]),
    "primary_persistent": dict(kind="launch", values=[0, 1]),
    "free_radius": dict(kind="launch", values=[0]),
    "batch_max": dict(kind="launch", values=[1, 2], frames=5),                # (a set of 5 frames: sets of 1 / of 2, 2 and 1)
    "queue_budget_mb": dict(kind="launch", values=[1]),
    "primary_retry_cap": dict(kind="launch", values=[7], needs={"lds_stack_rows": 6}),      # (as test_gpu_deferred_and_queues.py: the list overflows)
    # ---- exempt
    "verbose": dict(kind="exempt", reason="prints build timings to stderr; selects no code path that computes anything"),
    "dist_check_seconds": dict(kind="exempt", reason="a time-out of the multi-process rendezvous (rt_dist.hip); needs several ranks, covered by test_gpu_scale.py"),
}


def exercised(kind=None):
    """[(name, value)] of every option value the registry says is run, in the table's order"""
    return [(n, v) for n, o in OPTIONS.items() if o["kind"] != "exempt" and kind in (None, o["kind"]) for v in o["values"]]


def with_needs(opts):
    """the option set plus what its members need to have an effect (sah_node without wide_sah=1 would test nothing)"""
    out = dict(opts)
    for n in opts:
        for k, v in OPTIONS[n].get("needs", {}).items():
            out.setdefault(k, v)
    return out


def draw(r):
    """1 - 4 options with values from the registry, drawn from the numpy Generator r (tests/fuzz_parity.py)"""
    names = [n for n, o in OPTIONS.items() if o["kind"] != "exempt"]
    picked = r.choice(len(names), size=int(r.integers(1, 5)), replace=False)
    opts = {}
    for k in sorted(int(x) for x in picked):
        vals = OPTIONS[names[k]]["values"]
        opts[names[k]] = vals[int(r.integers(len(vals)))]
    return with_needs(opts)


def apply(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)


def library_options(source):
    """every option name rt_debug_set_option compares against: the `n == "<name>"` inside the function's body in csrc/rt_api.hip"""
    import re
    at = source.index('int rt_debug_set_option(')
    body = source[at:source.index("\n}\n", at)]
    return sorted(set(re.findall(r'\bn == "(\w+)"', body)))
