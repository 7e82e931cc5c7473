#!/usr/bin/env python3
"""What posing a skeleton on the device costs (rt_skeleton_set_time = k_skeleton_sample + k_skeleton_pose; rt_skeleton_set_pose from device
memory = a device-to-device copy of the pose + k_skeleton_pose).

  python3 tools/skeleton_timing.py [--joints N ...] [--steps S] [--warmup W] [--repeats R]

Per joint count (default 64 and 300, a character's range; a random tree, a clip of 4 keys): R back-to-back calls between two events on the
context's stream, per call; the figures include the gaps between back-to-back launches.  Medians and interquartile ranges over S >= 20 samples
after W warm-up samples.  For the kernels alone, run one joint count under `rocprofv3 --kernel-trace --stats -- python3
tools/skeleton_timing.py --joints N`: the trace names k_skeleton_sample and k_skeleton_pose.  Nothing here gates: the figures are recorded
(DESIGN.md section 7)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from dxrexperiments_amd import capi  # noqa: E402


class Events:
    """two events on the context's stream (the HIP runtime the library is linked with)"""

    def __init__(self, ctx):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(ctx.stream)
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def record(self, which):
        assert self.hip.hipEventRecord(self.e[which], self.stream) == 0

    def ms(self):
        out = C.c_float()
        assert self.hip.hipEventSynchronize(self.e[1]) == 0 and self.hip.hipEventElapsedTime(C.byref(out), self.e[0], self.e[1]) == 0
        return out.value

    def close(self):
        for e in self.e:
            self.hip.hipEventDestroy(e)


def character(n, seed):
    """(parents, inverse bind, times, keys): a random tree (depth about log n), unit quaternions, a clip of 4 keys"""
    rng = np.random.default_rng(seed)
    j = np.arange(n)
    parents = np.minimum(np.floor(rng.uniform(size=n) * j).astype(np.int64), j - 1).astype(np.int32)
    parents[0] = -1
    ib = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n, 1))
    ib[:, [3, 7, 11]] = rng.uniform(-1, 1, (n, 3))
    keys = np.zeros((4, n, 10), np.float32)
    keys[:, :, 0:3] = rng.uniform(-0.3, 0.3, (4, n, 3))
    q = rng.normal(size=(4, n, 4))
    keys[:, :, 3:7] = q / np.linalg.norm(q, axis=2, keepdims=True)
    keys[:, :, 7:10] = 1.0
    return parents, ib, np.array([0.0, 0.5, 1.0, 1.5], np.float32), keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--joints", type=int, nargs="+", default=[64, 300])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=100)
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed samples"
    ctx = capi.Context(0)
    ev = Events(ctx)
    for n in args.joints:
        parents, ib, times, keys = character(n, n)
        sk = capi.Skeleton(ctx, parents, ib)
        clip = sk.add_clip(times, keys)
        pose = ctx.upload(keys[1])

        def timed(call):
            out = []
            for s in range(args.warmup + args.steps):
                ctx.synchronize()
                ev.record(0)
                for r in range(args.repeats):
                    call(r)
                ev.record(1)
                ms = ev.ms() / args.repeats
                if s >= args.warmup:
                    out.append(ms * 1e3)
            q1, med, q3 = np.percentile(out, [25, 50, 75])
            return med, q3 - q1
        levels = sk.info()[1]
        for label, call in (("rt_skeleton_set_time (k_skeleton_sample + k_skeleton_pose)", lambda r: sk.set_time(clip, 0.013 * r)),
                            ("rt_skeleton_set_pose, device memory (copy + k_skeleton_pose)", lambda r: sk.set_pose_device(pose.ptr))):
            med, iqr = timed(call)
            print("%5d joints, %2d levels: %-64s %8.2f us per call (IQR %.2f), %d back-to-back calls per sample" % (n, levels, label, med, iqr, args.repeats))
        ctx.synchronize()
        pose.close()
        sk.close()
    ev.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
