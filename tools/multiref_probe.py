#!/usr/bin/env python3
"""Time the P step with several references (stages.MultiRefFramePipeline) on one GPU: picture 4 of a synthetic clip predicted from pictures
3, 2, 1, 0 (nearest first), the bench's settings.

  python tools/multiref_probe.py --steps 20 --refs 4               # one JSON line: ms per step, per-stage event times through mark()
  python tools/multiref_probe.py --refs 1 --single 1               # the single-reference P step (stages.FramePipeline) on the same picture
                                                                   # and reference: the kernels --refs 1 is compared against
  python tools/multiref_probe.py --dump-outputs DIR                # + ref_idx, mv_out and the coded Y / Cb / Cr planes as DIR/<name>.npy
  rocprofv3 --kernel-trace --stats -d DIR -o m -- python tools/multiref_probe.py --steps 20     # + tools/rocprof_summary.py kernel-trace DIR/.../m_results.db
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
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--subpel-planes", type=int, default=1, choices=[0, 1])
    ap.add_argument("--chroma-satd", type=int, default=0, choices=[0, 1])
    ap.add_argument("--single", type=int, default=0, choices=[0, 1], help="1: stages.FramePipeline with the nearest reference instead")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    F = importlib.import_module("x265-yuuki-asuna_amd.frames")
    P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
    dev = torch.device("cuda:0")
    qp = a.qp + 12 * (a.depth == 10)
    clip = F.synth_clip(a.width, a.height, a.refs + 1, depth=a.depth, seed=265)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    cur, refs = pics[a.refs], [pics[a.refs - 1 - k] for k in range(a.refs)]
    tabs = HT.load()
    cu_qp = max(qp - 6 * (a.depth - 8), 0)
    cm, ct = HT.sao_contexts(HT.SLICE_P, cu_qp)
    srdo = {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
    common = dict(rng=a.range, subme=a.subme, level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                  subpel_planes=bool(a.subpel_planes), sao_rdo=srdo, chroma_satd=bool(a.chroma_satd))
    if a.single:
        pipe = S.FramePipeline(cur.w64, cur.h64, a.depth, dev, want_surf=False, **common)
        run = lambda mark=None: pipe.run(cur, refs[0], mark=mark)
    else:
        pipe = S.MultiRefFramePipeline(cur.w64, cur.h64, a.depth, dev, max_refs=a.refs, **common)
        run = lambda mark=None: pipe.run(cur, refs, mark=mark)
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
    out = {"what": "FramePipeline.run" if a.single else "MultiRefFramePipeline.run", "width": a.width, "height": a.height, "depth": a.depth,
           "range": a.range, "subme": a.subme, "level": a.level, "refs": 1 if a.single else a.refs, "subpel_planes": a.subpel_planes,
           "chroma_satd": a.chroma_satd, "steps": a.steps, "ms_per_step": round(ms, 4), "stages_ms": {k: round(v, 4) for k, v in stages.items()},
           "stages_ms_sum": round(sum(stages.values()), 4), "checksum": pipe.checksum()}
    if not a.single:
        idx = pipe.rs.ref_idx.cpu().numpy()
        out["ref_counts"] = [int((idx == k).sum()) for k in range(a.refs)]
    if a.dump_outputs:
        os.makedirs(a.dump_outputs, exist_ok=True)
        arrays = dict(zip(("recon_y", "recon_cb", "recon_cr"), (p.cpu().numpy() for p in pipe.final_planes())))
        if not a.single:
            arrays.update({"ref_idx": pipe.rs.ref_idx.cpu().numpy(), "ref_id": pipe.rs.ref_id.cpu().numpy(), "mv_out": pipe.rs.mv_out.cpu().numpy()})
        for k, v in arrays.items():
            np.save(os.path.join(a.dump_outputs, k + ".npy"), v)
        out["dumped"] = sorted(arrays)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
