#!/usr/bin/env python3
"""Time the B step with merge / skip blocks (stages.MergeBFramePipeline) on one GPU, the method of tools/merge_probe.py and
tools/bsa8d_probe.py: pictures 0, 1 and 2 of the synthetic clip at the bench's settings (picture 1 is the B picture), per-stage device event
times through mark(), and - timed in the same process on the same pictures - the walk of x265hip_merge_decide (the P slice's, one list)
at the same level, so that the cost of the two-list candidates can be read off as a ratio.

  python tools/bmerge_probe.py --steps 20 --level 2          # one JSON line
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, run, steps, warmup):
    """(ms per step, {stage: ms}) of run(mark): device events around `steps` runs, then one event after every stage."""
    for _ in range(warmup):
        run(None)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        run(None)
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
        run(mark)
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
    clip = F.synth_clip(a.width, a.height, 3, depth=a.depth, seed=265)
    r0, cur, r1 = (P.DevicePicture(y, dev, u, v) for (y, u, v) in clip)
    tabs = HT.load()
    cu_qp = max(qp - 6 * (a.depth - 8), 0)
    cm, ct = HT.sao_contexts(HT.SLICE_B, cu_qp)
    srdo = {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
    common = dict(level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True, sao_rdo=srdo)
    pipe = S.MergeBFramePipeline(cur.w64, cur.h64, a.depth, dev, max_merge=a.max_merge, **common)
    ms, stages = timed(torch, lambda mark: pipe.run(cur, r0, r1, mark=mark), a.steps, a.warmup)
    md = pipe.md
    merged = md.merge != 0
    by_dir = lambda sel: torch.bincount(md.dir[sel].to(torch.int64), minlength=4).tolist()[1:]
    # the P slice's walk on the same current picture and list 0, fed the list-0 records and the same inter costs: only its time is read
    pm = S.MergeDecide(pipe.nctu, cur.w64, cur.h64, a.depth, a.level, dev, max_merge=a.max_merge, qp=qp)

    def p_walk(mark):
        pm.run(cur, r0, pipe.spl[0].out, pipe.bd.cost, inter_cost_stride=4, inter_cost_offset=0)
        if mark:
            mark("p_merge")
    _, p_stages = timed(torch, p_walk, a.steps, a.warmup)
    print(json.dumps({"what": "MergeBFramePipeline.run", "width": a.width, "height": a.height, "depth": a.depth, "level": a.level, "steps": a.steps,
                      "max_merge": a.max_merge, "merge_share": round(float(merged.float().mean().item()), 4),
                      "skip_share": round(float(pipe.skip.float().mean().item()), 4),
                      "merged_by_index": torch.bincount(md.merge_idx[merged].to(torch.int64), minlength=a.max_merge).tolist(),
                      "merged_by_dir_1_2_3": by_dir(merged), "inter_by_dir_1_2_3": by_dir(~merged),
                      "ms_per_step": round(ms, 4), "stages_ms": {k: round(v, 4) for k, v in stages.items()},
                      "stages_ms_sum": round(sum(stages.values()), 4), "waves": md.waves,
                      "us_per_wave": round(1000.0 * stages["merge"] / md.waves, 3),
                      "p_merge_walk_ms": round(p_stages["p_merge"], 4), "p_merge_us_per_wave": round(1000.0 * p_stages["p_merge"] / md.waves, 3),
                      "walk_ratio_b_over_p": round(stages["merge"] / p_stages["p_merge"], 3),
                      "checksum": pipe.checksum()}))


if __name__ == "__main__":
    main()
