#!/usr/bin/env python3
"""What posing a crowd costs (rt_crowd_set_times = one upload + one k_crowd_pose) beside the loop it replaces: one rt_skeleton_set_time
(k_skeleton_sample + k_skeleton_pose) per actor on separate skeletons, the code as it was before crowds.

  python3 tools/crowd_update.py [--actors N ...] [--joints J] [--boxes B] [--steps S] [--warmup W] [--repeats R] [--layers L ...] [--no-loop]

A rig of J joints (default 64: the random tree of tools/skeleton_timing.py, about six levels) with a three-key clip; per actor count
(default 16, 256 and 1000), every actor at its own time:
  stream time: R frames of posing back to back between two events on the context's stream, per frame (the gaps between launches included);
  host time:   the host clock around the posing calls of one frame, enqueue only, per frame -- through ctypes, whose own cost per call
               (about a microsecond) is part of the loop's figure as it is of any caller's through this binding;
for the crowd with the block width the rig gives (64 lanes up to 64 joints, 128 up to 128, else 256; a library built with
-DRT_CROWD_BLOCK=64, 128 or 256 -- `make clean; make EXTRA=-DRT_CROWD_BLOCK=128`, or that library named by DXR_AMD_LIB -- forces one width,
for the three side by side); and for B boxes attached per actor (default 6), the device time of the rt_scene_update behind the pose (rt_scene_update_ms) under both.  Medians and interquartile
ranges over S >= 20 samples after W warm-up samples.  For the kernels alone, run ONE actor count under
`rocprofv3 --kernel-trace --stats -- python3 tools/crowd_update.py --actors N`: the trace names k_crowd_pose, k_skeleton_sample and
k_skeleton_pose.
With --layers L ... the crowd is also posed with L layers per actor (layer 0 the clip at the actor's time, every later layer the same clip at
another time with weight 0.25, replacing and additive in turn), both ways: rt_crowd_set_blend (rt_crowd_set_times for L = 1) with the layers
packed on the host and uploaded every frame, and rt_crowd_set_blend_device over a layout set once, its times read from a table of 64 frames
that was uploaded once -- one launch, and nothing crosses.  --no-loop leaves out the loop of skeletons and the scene (10,000 skeletons are
not what is being measured).  With DXR_AMD_LIB naming a library from before rt_crowd_set_blend_device, the host rows alone are taken.
Nothing here gates: the figures are recorded."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from skeleton_timing import Events, character  # noqa: E402
from dxrexperiments_amd import capi, rtypes as T  # noqa: E402


def cube():
    v = np.zeros(24, T.VERTEX)
    idx = []
    k = 0
    for axis in range(3):
        for side in (-1, 1):
            for corner in range(4):
                p = np.zeros(3, np.float32)
                p[axis] = 0.5 * side
                p[(axis + 1) % 3] = 0.5 if corner & 1 else -0.5
                p[(axis + 2) % 3] = 0.5 if corner & 2 else -0.5
                v["position"][k + corner] = p
                v["normal"][k + corner][axis] = side
            idx += [k, k + 1, k + 3, k, k + 3, k + 2] if side > 0 else [k, k + 3, k + 1, k, k + 2, k + 3]
            k += 4
    return v, np.array(idx, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", type=int, nargs="+", default=[16, 256, 1000])
    ap.add_argument("--joints", type=int, default=64)
    ap.add_argument("--boxes", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--layers", type=int, nargs="*", default=[])
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed samples"
    if os.environ.get("DXR_AMD_LIB"):                    # an older build of the library: what it lacks is not bound, and not measured
        import ctypes
        older = ctypes.CDLL(capi.LIB_PATH)
        for name in [name for name in capi.SIGNATURES if not hasattr(older, name)]:
            del capi.SIGNATURES[name]
    has_device = "rt_crowd_set_blend_device" in capi.SIGNATURES
    ctx = capi.Context(0)
    ev = Events(ctx)
    lib = capi.lib()
    n = args.joints
    parents, ib, times, keys = character(n, n)
    times, keys = times[:3], keys[:3]

    def timed(frame):
        stream, host = [], []
        for s in range(args.warmup + args.steps):
            ctx.synchronize()
            ev.record(0)
            t0 = time.perf_counter()
            for r in range(args.repeats):
                frame(s * args.repeats + r)
            t1 = time.perf_counter()
            ev.record(1)
            ms = ev.ms() / args.repeats
            if s >= args.warmup:
                stream.append(ms * 1e3)
                host.append((t1 - t0) * 1e6 / args.repeats)
        return tuple(np.percentile(x, [50, 25, 75]) for x in (stream, host))

    def report(label, got):
        (sm, s1, s3), (hm, h1, h3) = got
        print("%-78s stream %9.1f us (IQR %.1f)   host %9.1f us (IQR %.1f) per frame" % (label, sm, s3 - s1, hm, h3 - h1), flush=True)

    for n_actors in args.actors:
        shared = capi.Skeleton(ctx, parents, ib)
        clip = shared.add_clip(times, keys)
        crowd = capi.Crowd(shared, n_actors)
        singles = [capi.Skeleton(ctx, parents, ib) for _ in range(0 if args.no_loop else n_actors)]
        for sk in singles:
            sk.add_clip(times, keys)
        handles = [sk.h for sk in singles]
        clips = np.full(n_actors, clip, np.uint32)
        phase = (np.arange(n_actors) * 0.037).astype(np.float32)
        span = float(times[-1])

        def now(f):
            return np.mod(np.float32(0.013 * f) + phase, np.float32(span)).astype(np.float32)

        def crowd_frame(f):
            crowd.set_times(clips, now(f))

        def loop_frame(f):
            t = now(f).tolist()
            set_time = lib.rt_skeleton_set_time
            for h, x in zip(handles, t):
                set_time(h, clip, x)

        head = "%4d actors x %d joints (%d levels): " % (n_actors, n, shared.info()[1])
        if not args.no_loop:
            report(head + "loop of rt_skeleton_set_time (2 launches an actor)", timed(loop_frame))
        report(head + "rt_crowd_set_times (%d-lane blocks)" % (64 if n <= 64 else 128 if n <= 128 else 256), timed(crowd_frame))
        if not args.no_loop:
            report(head + "loop of rt_skeleton_set_time, again (spread)", timed(loop_frame))

        # L layers an actor: packed on the host and uploaded every frame, or a layout set once and times read from device memory
        for n_layers in args.layers:
            layers = np.zeros((n_actors, n_layers), T.SKELETON_LAYER)
            layers["clip"], layers["weight"], layers["mask"] = clip, 0.25, T.SKELETON_NO_MASK
            layers["mode"] = np.where(np.arange(n_layers) % 2 == 0, T.LAYER_BLEND, T.LAYER_ADDITIVE)[None, :]
            layers["mode"][:, :2] = T.LAYER_BLEND
            offsets = (np.arange(n_layers) * 0.21).astype(np.float32)

            def layer_times(f):
                return np.mod(now(f)[:, None] + offsets[None, :], np.float32(span)).astype(np.float32)

            def blend_frame(f):
                layers["time"] = layer_times(f)
                crowd.set_blend(layers)

            if n_layers > 1:
                report(head + "rt_crowd_set_blend, %d layers (packed on the host, one upload)" % n_layers, timed(blend_frame))
            if has_device:
                frames = 64
                table = ctx.upload(np.stack([layer_times(f) for f in range(frames)]))
                stride = 4 * n_actors * n_layers
                crowd.set_layout(layers)
                set_device = lib.rt_crowd_set_blend_device
                handle, base = crowd.h, table.ptr

                def device_frame(f):
                    set_device(handle, base + (f % frames) * stride, None)

                report(head + "rt_crowd_set_blend_device, %d layer%s (layout set once, times on the device)" % (n_layers, "s" if n_layers > 1 else ""), timed(device_frame))
                ctx.synchronize()
                table.close()

        # the scene behind the pose: B boxes an actor, attached to its joints
        if args.boxes and not args.no_loop:
            model = capi.Model(ctx, *cube())
            n_inst = n_actors * args.boxes
            joints = (np.arange(n_inst) * 7 % n).astype(np.uint32)
            actors = (np.arange(n_inst) // args.boxes).astype(np.uint32)
            local = np.tile(np.array([0.5, 0, 0, 0.1, 0, 0.5, 0, 0.2, 0, 0, 0.5, 0.3], np.float32), (n_inst, 1))
            for how in ("crowd", "loop"):
                sc = capi.Scene(ctx)
                for _ in range(n_inst):
                    sc.add_model(model)
                (crowd_frame if how == "crowd" else loop_frame)(0)
                if how == "crowd":
                    sc.attach_crowd(0, crowd, actors, joints, local)
                else:
                    for a in range(n_actors):
                        lo, hi = a * args.boxes, (a + 1) * args.boxes
                        sc.attach(lo, singles[a], joints[lo:hi], local[lo:hi])
                sc.build()
                out = []
                for s in range(args.warmup + args.steps):
                    (crowd_frame if how == "crowd" else loop_frame)(s + 1)
                    sc.update()
                    if s >= args.warmup:
                        out.append(sc.update_ms() * 1e3)
                q1, med, q3 = np.percentile(out, [25, 50, 75])
                print("%s%d instances attached to %s: rt_scene_update_ms %9.1f us (IQR %.1f)" % (head, n_inst, "the crowd" if how == "crowd" else "the skeletons", med, q3 - q1), flush=True)
                sc.close()
            model.close()
        ctx.synchronize()
        crowd.close()
        for sk in singles + [shared]:
            sk.close()
    ev.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
