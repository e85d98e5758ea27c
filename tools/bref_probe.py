#!/usr/bin/env python3
"""Time the B step with several references per list (stages.MultiRefBFramePipeline) on one GPU: the middle picture of a synthetic clip
with HEVC's default lists - list 0 = the pictures before it, nearest first, list 1 = the picture after it + those - the bench's settings.

  python tools/bref_probe.py --steps 20 --refs 2,2              # one JSON line: ms per step, per-stage event times through mark()
  python tools/bref_probe.py --refs 1,1 --single 1              # the single-reference B step (stages.BFramePipeline) on the same pictures
  python tools/bref_probe.py --refs 1,1 --twin 1                # both steps in every iteration: one kernel trace holds the new kernels with
                                                                # one reference per list AND the kernels they are compared against
  python tools/bref_probe.py --dump-outputs DIR                 # + ref_idx0 / ref_idx1, dir and the coded Y / Cb / Cr planes as DIR/<name>.npy
  rocprofv3 --kernel-trace --stats -d DIR -o b -- python tools/bref_probe.py --steps 20     # + tools/rocprof_summary.py spread DIR/.../b_results.db
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
    ap.add_argument("--range", type=int, default=57)
    ap.add_argument("--subme", type=int, default=3)
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--qp", type=int, default=27)
    ap.add_argument("--refs", default="2,2", help="n0,n1: references in list 0 / list 1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--subpel-planes", type=int, default=1, choices=[0, 1])
    ap.add_argument("--single", type=int, default=0, choices=[0, 1], help="1: stages.BFramePipeline with the first picture of each list instead")
    ap.add_argument("--twin", type=int, default=0, choices=[0, 1], help="1: run stages.BFramePipeline beside the step in every iteration (kernel traces)")
    ap.add_argument("--zero-ref-cost", type=int, default=0, choices=[0, 1], help="1: reference bits 0 (with --refs 1,1 the step computes what BFramePipeline computes)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    F = importlib.import_module("x265-yuuki-asuna_amd.frames")
    P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
    dev = torch.device("cuda:0")
    n0, n1 = (int(v) for v in a.refs.split(","))
    before = max(n0, n1 - 1)
    qp = a.qp + 12 * (a.depth == 10)
    clip = F.synth_clip(a.width, a.height, before + 2, depth=a.depth, seed=265)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    cur = pics[before]
    past = [pics[before - 1 - k] for k in range(before)]
    refs0, refs1 = past[:n0], ([pics[before + 1]] + past)[:n1]
    tabs = HT.load()
    cu_qp = max(qp - 6 * (a.depth - 8), 0)
    cm, ct = HT.sao_contexts(HT.SLICE_B, cu_qp)
    srdo = {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
    common = dict(rng=a.range, subme=a.subme, level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                  subpel_planes=bool(a.subpel_planes), sao_rdo=srdo)
    single = S.BFramePipeline(cur.w64, cur.h64, a.depth, dev, **common) if (a.single or a.twin) else None
    pipe = single
    if not a.single:
        pipe = S.MultiRefBFramePipeline(cur.w64, cur.h64, a.depth, dev, max_refs=(n0, n1), ref_cost=((0,) * n0, (0,) * n1) if a.zero_ref_cost else None, **common)

    def run(mark=None):
        if a.single:
            return single.run(cur, refs0[0], refs1[0], mark=mark)
        pipe.run(cur, refs0, refs1, mark=mark)
        if a.twin:
            single.run(cur, refs0[0], refs1[0])
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        run()
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
        run(mark)
        torch.cuda.synchronize()
        for (_, e0), (name, e1) in zip(evs, evs[1:]):
            stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1) / a.steps
    out = {"what": "BFramePipeline.run" if a.single else ("MultiRefBFramePipeline.run + BFramePipeline.run" if a.twin else "MultiRefBFramePipeline.run"),
           "width": a.width, "height": a.height, "depth": a.depth, "range": a.range, "subme": a.subme, "level": a.level,
           "refs": [1, 1] if a.single else [n0, n1], "subpel_planes": a.subpel_planes, "steps": a.steps, "ms_per_step": round(ms, 4),
           "stages_ms": {k: round(v, 4) for k, v in stages.items()}, "stages_ms_sum": round(sum(stages.values()), 4), "checksum": pipe.checksum()}
    if not a.single:
        out["distinct_pictures"] = 1 + max(max(s) for s in pipe.slots)
        d = pipe.bd.dir.cpu().numpy()
        out["dir_counts"] = [int((d == k).sum()) for k in (1, 2, 3)]
        out["ref_counts"] = [[int((pipe.rs[l].ref_idx.cpu().numpy() == k).sum()) for k in range(n)] for l, n in ((0, n0), (1, n1))]
        if a.twin:
            out["equals_single"] = bool(all(torch.equal(x, y) for x, y in zip(pipe.final_planes(), single.final_planes())))
    if a.dump_outputs:
        os.makedirs(a.dump_outputs, exist_ok=True)
        arrays = dict(zip(("recon_y", "recon_cb", "recon_cr"), (p.cpu().numpy() for p in pipe.final_planes())))
        arrays["dir"] = pipe.bd.dir.cpu().numpy()
        if not a.single:
            arrays.update({"ref_idx0": pipe.rs[0].ref_idx.cpu().numpy(), "ref_idx1": pipe.rs[1].ref_idx.cpu().numpy()})
        for k, v in arrays.items():
            np.save(os.path.join(a.dump_outputs, k + ".npy"), v)
        out["dumped"] = sorted(arrays)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
