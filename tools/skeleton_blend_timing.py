#!/usr/bin/env python3
"""What blending clips on the device costs (rt_skeleton_set_blend = k_skeleton_blend + k_skeleton_pose) beside one clip at one time
(rt_skeleton_set_time = k_skeleton_sample + k_skeleton_pose).

  python3 tools/skeleton_blend_timing.py [--joints N ...] [--layers L ...] [--steps S] [--warmup W] [--repeats R]

Per joint count (default 64, 300 and 65536; the random tree and the 4-key clips of tools/skeleton_timing.py, three clips and a mask) and per
layer count (default 2 and 8; from layer 1 on the layers alternate between RT_LAYER_BLEND and a masked RT_LAYER_ADDITIVE): R back-to-back
calls between two events on the context's stream, per call; the figures include the gaps between back-to-back launches.  Medians and
interquartile ranges over S >= 20 samples after W warm-up samples.  For the kernels alone, run ONE joint count and ONE layer count under
`rocprofv3 --kernel-trace --stats -- python3 tools/skeleton_blend_timing.py --joints N --layers L`: the trace names k_skeleton_blend,
k_skeleton_sample and k_skeleton_pose.  Nothing here gates: the figures are recorded."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from skeleton_timing import Events, character  # noqa: E402
from dxrexperiments_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--joints", type=int, nargs="+", default=[64, 300, 65536])
    ap.add_argument("--layers", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=100)
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 timed samples"
    ctx = capi.Context(0)
    ev = Events(ctx)
    for n in args.joints:
        sk = None
        clips = []
        for c in range(3):
            parents, ib, times, keys = character(n, n + 7 * c)
            if sk is None:
                sk = capi.Skeleton(ctx, parents, ib)
            clips.append(sk.add_clip(times, keys))
        mask = sk.add_mask((np.arange(n) >= n // 2).astype(np.float32))

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
        rows = [("rt_skeleton_set_time (k_skeleton_sample + k_skeleton_pose)", lambda r: sk.set_time(clips[0], 0.013 * r))]
        for n_layers in args.layers:
            layers = capi.Skeleton.layers([(clips[0], 0.0)] + [(clips[k % 3], 0.1 * k, 0.5, mask if k % 2 == 0 else None, "additive" if k % 2 == 0 else "blend")
                                                               for k in range(1, n_layers)])

            def blend(r, layers=layers):
                layers["time"][0] = 0.013 * r
                sk.set_blend(layers)
            rows.append(("rt_skeleton_set_blend, %d layers (k_skeleton_blend + k_skeleton_pose)" % n_layers, blend))
        for label, call in rows:
            med, iqr = timed(call)
            print("%5d joints, %2d levels: %-72s %8.2f us per call (IQR %.2f), %d back-to-back calls per sample" % (n, sk.info()[1], label, med, iqr, args.repeats))
        ctx.synchronize()
        sk.close()
    ev.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
