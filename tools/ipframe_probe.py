#!/usr/bin/env python3
"""Time the P step with intra blocks (stages.IntraPFramePipeline) on one GPU, the method of tools/ipicture_probe.py: pictures 0 and 1 of a
synthetic clip, the right `--new` part of picture 1 replaced by a picture of another clip (content the reference lacks), the bench's settings.

  python tools/ipframe_probe.py --steps 20 --level 2          # one JSON line: ms per step, per-stage event times through mark(), share of intra blocks
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
    ap.add_argument("--new", type=float, default=0.3, help="part of the width that shows content the reference lacks")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    F = importlib.import_module("x265-yuuki-asuna_amd.frames")
    P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
    dev = torch.device("cuda:0")
    qp = a.qp + 12 * (a.depth == 10)
    clip = F.synth_clip(a.width, a.height, 2, depth=a.depth, seed=265)
    other = F.synth_clip(a.width, a.height, 1, depth=a.depth, seed=17)[0]
    x0 = int(a.width * (1.0 - a.new)) // 64 * 64 + 24          # the boundary runs through CTUs
    planes = [p.copy() for p in clip[1]]
    for i, p in enumerate(planes):
        p[:, x0 >> (i > 0):] = other[i][:, x0 >> (i > 0):]
    cur, ref = P.DevicePicture(planes[0], dev, planes[1], planes[2]), P.DevicePicture(clip[0][0], dev, clip[0][1], clip[0][2])
    tabs = HT.load()
    cu_qp = max(qp - 6 * (a.depth - 8), 0)
    cm, ct = HT.sao_contexts(HT.SLICE_P, cu_qp)
    srdo = {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
    pipe = S.IntraPFramePipeline(cur.w64, cur.h64, a.depth, dev, level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                                 sao_rdo=srdo)
    for _ in range(a.warmup):
        pipe.run(cur, ref)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        pipe.run(cur, ref)
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
        pipe.run(cur, ref, mark=mark)
        torch.cuda.synchronize()
        for (_, e0), (name, e1) in zip(evs, evs[1:]):
            stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1) / a.steps
    print(json.dumps({"what": "IntraPFramePipeline.run", "width": a.width, "height": a.height, "depth": a.depth, "level": a.level, "steps": a.steps,
                      "new_part_of_width": a.new, "intra_share": round(float(pipe.ii.intra.float().mean().item()), 4),
                      "ms_per_step": round(ms, 4), "stages_ms": {k: round(v, 4) for k, v in stages.items()},
                      "stages_ms_sum": round(sum(stages.values()), 4), "waves": pipe.ii.waves,
                      "us_per_wave": round(1000.0 * stages["intra"] / pipe.ii.waves, 3), "checksum": pipe.checksum()}))


if __name__ == "__main__":
    main()
