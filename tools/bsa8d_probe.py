#!/usr/bin/env python3
"""Time the B step with the sa8d choice (stages.Sa8dBFramePipeline) on one GPU, the method of tools/ipframe_probe.py: pictures 0, 1, 2 of a
synthetic clip, the right `--new` part of picture 1 replaced by a picture of another clip (content both references lack), range 57.

  python tools/bsa8d_probe.py --steps 20 --level 2     # one JSON line: one b_sa8d_decide / bidir_decide / subpel_refine launch on the same
                                                       # pictures (device events), the step without and with b_intra beside BFramePipeline's
                                                       # and IntraPFramePipeline's, per-stage event times through mark(), shares of dir and intra
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
    ap.add_argument("--subme", type=int, default=3)
    ap.add_argument("--qp", type=int, default=27)
    ap.add_argument("--new", type=float, default=0.3, help="part of the width that shows content the references lack")
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
    other = F.synth_clip(a.width, a.height, 1, depth=a.depth, seed=17)[0]
    x0 = int(a.width * (1.0 - a.new)) // 64 * 64 + 24          # the boundary runs through CTUs
    planes = [p.copy() for p in clip[1]]
    for i, p in enumerate(planes):
        p[:, x0 >> (i > 0):] = other[i][:, x0 >> (i > 0):]
    cur = P.DevicePicture(planes[0], dev, planes[1], planes[2])
    r0, r1 = (P.DevicePicture(clip[i][0], dev, clip[i][1], clip[i][2]) for i in (0, 2))
    tabs = HT.load()
    cu_qp = max(qp - 6 * (a.depth - 8), 0)

    def srdo(slice_type):
        cm, ct = HT.sao_contexts(slice_type, cu_qp)
        return {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
    common = dict(subme=a.subme, level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.steps

    def staged(run):
        """per-stage times: one event after every stage, averaged over the steps"""
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
        return {k: round(v, 4) for k, v in stages.items()}

    out = {"what": "Sa8dBFramePipeline.run", "width": a.width, "height": a.height, "depth": a.depth, "level": a.level, "subme": a.subme, "steps": a.steps,
           "new_part_of_width": a.new}
    pipe = S.Sa8dBFramePipeline(cur.w64, cur.h64, a.depth, dev, sao_rdo=srdo(HT.SLICE_B), **common)
    out["sa8d_b_step_ms"] = round(timed(lambda: pipe.run(cur, r0, r1)), 4)
    out["sa8d_b_step_stages_ms"] = staged(lambda mark: pipe.run(cur, r0, r1, mark=mark))
    out["dir_shares"] = [round(float((pipe.bd.dir == d).float().mean().item()), 4) for d in (1, 2, 3)]
    # single launches on the records the step has just left
    mv0, mv1 = pipe.spl[0].out, pipe.spl[1].out
    out["b_sa8d_decide_launch_us"] = round(1000.0 * timed(lambda: pipe.bd.run(cur, r0, r1, mv0, mv1)), 3)
    bd = S.BidirDecide(pipe.nctu, cur.w64, cur.h64, a.depth, a.level, dev)
    out["bidir_decide_launch_us"] = round(1000.0 * timed(lambda: bd.run(cur, r0, r1, mv0, mv1, pipe.spl[0].cost_q, pipe.spl[0].qoff)), 3)
    out["subpel_refine_launch_us"] = round(1000.0 * timed(lambda: pipe.spl[0].run(cur, r0)), 3)
    out["checksum"] = pipe.checksum()
    del pipe, bd
    old = S.BFramePipeline(cur.w64, cur.h64, a.depth, dev, sao_rdo=srdo(HT.SLICE_B), **common)
    out["b_step_ms"] = round(timed(lambda: old.run(cur, r0, r1)), 4)
    del old
    pipe = S.Sa8dBFramePipeline(cur.w64, cur.h64, a.depth, dev, sao_rdo=srdo(HT.SLICE_B), b_intra=True, **common)
    out["sa8d_b_intra_step_ms"] = round(timed(lambda: pipe.run(cur, r0, r1)), 4)
    out["sa8d_b_intra_step_stages_ms"] = staged(lambda mark: pipe.run(cur, r0, r1, mark=mark))
    out["intra_share"] = round(float(pipe.ii.intra.float().mean().item()), 4)
    del pipe
    ip = S.IntraPFramePipeline(cur.w64, cur.h64, a.depth, dev, sao_rdo=srdo(HT.SLICE_P), **common)
    out["intra_p_step_ms"] = round(timed(lambda: ip.run(cur, r0)), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
