#!/usr/bin/env python3
"""Time the P step with merge / skip blocks (stages.MergePFramePipeline) on one GPU, the method of tools/ipframe_probe.py: pictures 0 and 1 of
the synthetic clip at the bench's settings, FramePipeline's step at the same settings beside it, so that the cost of the walk can be read off.

  python tools/merge_probe.py --steps 20 --level 2          # one JSON line: ms per step, per-stage event times through mark(), shares of merged / skipped blocks
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, pipe, cur, ref, steps, warmup):
    """(ms per step, {stage: ms}) of pipe.run(cur, ref): device events around `steps` runs, then one event after every stage."""
    for _ in range(warmup):
        pipe.run(cur, ref)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        pipe.run(cur, ref)
    t1.record()
    torch.cuda.synchronize()
    stages = {}
    for _ in range(steps):
        evs = [("start", torch.cuda.Event(enable_timing=True))]
        evs[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append((name, e))
        pipe.run(cur, ref, mark=mark)
        torch.cuda.synchronize()
        for (_, e0), (name, e1) in zip(evs, evs[1:]):
            stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1) / steps
    return t0.elapsed_time(t1) / steps, stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10])
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--qp", type=int, default=27)
    ap.add_argument("--max-merge", type=int, default=3)
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
    cur, ref = P.DevicePicture(clip[1][0], dev, clip[1][1], clip[1][2]), P.DevicePicture(clip[0][0], dev, clip[0][1], clip[0][2])
    tabs = HT.load()
    cu_qp = max(qp - 6 * (a.depth - 8), 0)
    cm, ct = HT.sao_contexts(HT.SLICE_P, cu_qp)
    srdo = {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
    common = dict(level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True, sao_rdo=srdo)
    pipe = S.MergePFramePipeline(cur.w64, cur.h64, a.depth, dev, max_merge=a.max_merge, **common)
    ms, stages = timed(torch, pipe, cur, ref, a.steps, a.warmup)
    plain = S.FramePipeline(cur.w64, cur.h64, a.depth, dev, want_surf=False, **common)
    ms_plain, stages_plain = timed(torch, plain, cur, ref, a.steps, a.warmup)
    idx = torch.bincount(pipe.md.merge_idx[pipe.md.merge != 0].to(torch.int64), minlength=a.max_merge).tolist()
    print(json.dumps({"what": "MergePFramePipeline.run", "width": a.width, "height": a.height, "depth": a.depth, "level": a.level, "steps": a.steps,
                      "max_merge": a.max_merge, "merge_share": round(float(pipe.md.merge.float().mean().item()), 4),
                      "skip_share": round(float(pipe.skip.float().mean().item()), 4), "merged_by_index": idx,
                      "ms_per_step": round(ms, 4), "stages_ms": {k: round(v, 4) for k, v in stages.items()},
                      "stages_ms_sum": round(sum(stages.values()), 4), "waves": pipe.md.waves,
                      "us_per_wave": round(1000.0 * stages["merge"] / pipe.md.waves, 3),
                      "frame_pipeline_ms_per_step": round(ms_plain, 4), "frame_pipeline_stages_ms": {k: round(v, 4) for k, v in stages_plain.items()},
                      "checksum": pipe.checksum()}))


if __name__ == "__main__":
    main()
