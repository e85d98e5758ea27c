#!/usr/bin/env python3
"""Time the I-picture step (stages.IFramePipeline) on one GPU: picture 0 of a synthetic clip, the bench's settings.

  python tools/ipicture_probe.py --steps 20 --level 2          # one JSON line: ms per I step, per-stage event times through mark(), us per wave
  rocprofv3 --kernel-trace --stats -d DIR -o i -- python tools/ipicture_probe.py --steps 20     # + tools/rocprof_summary.py kernel-trace DIR/.../i_results.db
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10])
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--qp", type=int, default=27)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    F = importlib.import_module("x265-yuuki-asuna_amd.frames")
    P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
    dev = torch.device("cuda:0")
    qp = a.qp + 12 * (a.depth == 10)
    y, u, v = F.synth_clip(a.width, a.height, 1, depth=a.depth, seed=265)[0]
    cur = P.DevicePicture(y, dev, u, v)
    tabs = HT.load()
    cu_qp = max(qp - 6 * (a.depth - 8), 0)
    cm, ct = HT.sao_contexts(HT.SLICE_I, cu_qp)
    srdo = {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
    pipe = S.IFramePipeline(cur.w64, cur.h64, a.depth, dev, level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                            sao_rdo=srdo)
    for _ in range(a.warmup):
        pipe.run(cur)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        pipe.run(cur)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    # per-stage times: one event after every stage, averaged over the same number of steps
    stages = {}
    for _ in range(a.steps):
        evs = [("start", torch.cuda.Event(enable_timing=True))]
        evs[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append((name, e))
        pipe.run(cur, mark=mark)
        torch.cuda.synchronize()
        for (_, e0), (name, e1) in zip(evs, evs[1:]):
            stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1) / a.steps
    modes = np.bincount(pipe.ip.mode.cpu().numpy(), minlength=35)
    print(json.dumps({"what": "IFramePipeline.run", "width": a.width, "height": a.height, "depth": a.depth, "level": a.level, "steps": a.steps,
                      "ms_per_i_step": round(ms, 4), "stages_ms": {k: round(v, 4) for k, v in stages.items()},
                      "stages_ms_sum": round(sum(stages.values()), 4), "waves": pipe.ip.waves,
                      "us_per_wave": round(1000.0 * stages["intra"] / pipe.ip.waves, 3),
                      "mode_counts": {"dc": int(modes[1]), "planar": int(modes[0]), "angular": int(modes[2:].sum())}, "checksum": pipe.checksum()}))


if __name__ == "__main__":
    main()
