"""What chroma SATD costs the sub-pel refinement, the bidirectional decision and the P / B steps: device-event timings with the option off
and on (3840x2160, 8-bit, range 57, subme 3, level 2 by default).  Prints one JSON line.

    python tools/subpel_chroma_probe.py [--width 3840 --height 2160 --depth 8 --range 57 --subme 3 --level 2 --launches 20 --rounds 5]

Per stage and per variant: the median over `rounds` of the mean time of `launches` back-to-back launches between two device events, and the
spread (min, max) of the rounds.  The variants alternate inside a round, so that clock drift touches both alike.  The refinement is timed
in both flavours (luma candidates interpolated / read from phase planes, the planes prepared outside the timed window); the steps are
FramePipeline / BFramePipeline with chroma, deblocking, SAO applied and the luma phase planes."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--range", type=int, default=57)
    ap.add_argument("--subme", type=int, default=3)
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--qp", type=int, default=27)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args()
    import torch
    F = importlib.import_module("x265-yuuki-asuna_amd.frames")
    P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    dev = torch.device("cuda:0")
    qp = a.qp + 6 * (a.depth - 8)
    clip = F.synth_clip(a.width, a.height, 3, depth=a.depth, seed=265)
    r0, cur, r1 = (P.DevicePicture(clip[i][0], dev, clip[i][1], clip[i][2]) for i in range(3))
    w64, h64 = cur.w64, cur.h64

    # the integer stage once per list; the refinements and the decision are then timed on its records
    msl = [P.MotionSearch(w64, h64, a.range, a.depth, dev, want_surf=False) for _ in range(2)]
    for ms, ref in zip(msl, (r0, r1)):
        ms.run(cur, ref)
    stages, launches, moved = {}, {}, {}
    sps = {}
    for planes in (False, True):
        for ch in (False, True):
            sps[planes, ch] = [P.SubpelRefine(ms, a.subme, dev, phase_planes=planes, chroma_satd=ch) for ms in msl]
            for sp, ref in zip(sps[planes, ch], (r0, r1)):
                sp.prepare(ref)
                sp.run(cur, ref, prepared=True)

        def refine(with_chroma, planes=planes):
            sps[planes, with_chroma][0].run(cur, r0, prepared=True)
        name = "subpel_refine_planes" if planes else "subpel_refine_interp"
        stages[name], launches[name] = refine, a.launches
    torch.cuda.synchronize()
    q = [sps[False, ch][0].out.cpu().numpy().reshape(-1, 2)[:, 1] for ch in (False, True)]
    moved["subpel_vectors_changed_by_chroma"] = round(float((q[0] != q[1]).mean()), 4)

    bds = {ch: S.BidirDecide(msl[0].nctu, w64, h64, a.depth, a.level, dev, chroma_satd=ch) for ch in (False, True)}

    def decide(with_chroma):
        sp = sps[False, with_chroma]
        bds[with_chroma].run(cur, r0, r1, sp[0].out, sp[1].out, sp[0].cost_q, sp[0].qoff)
    stages["bidir_decide_interp"], launches["bidir_decide_interp"] = decide, a.launches

    if not a.no_steps:
        HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
        tabs = HT.load()
        cu_qp = max(qp - 6 * (a.depth - 8), 0)

        def srdo(slice_type):
            cm, ct = HT.sao_contexts(slice_type, cu_qp)
            return {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}
        kw = dict(rng=a.range, subme=a.subme, level=a.level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True, subpel_planes=True)
        psteps = {ch: S.FramePipeline(w64, h64, a.depth, dev, want_surf=False, sao_rdo=srdo(HT.SLICE_P), chroma_satd=ch, **kw) for ch in (False, True)}
        bsteps = {ch: S.BFramePipeline(w64, h64, a.depth, dev, sao_rdo=srdo(HT.SLICE_B), chroma_satd=ch, **kw) for ch in (False, True)}
        stages["p_step"], launches["p_step"] = (lambda ch: psteps[ch].run(cur, r0)), max(1, a.launches // 4)
        stages["b_step"], launches["b_step"] = (lambda ch: bsteps[ch].run(cur, r0, r1)), max(1, a.launches // 4)

    out = {"width": w64, "height": h64, "depth": a.depth, "range": a.range, "subme": a.subme, "level": a.level, "device": torch.cuda.get_device_name(0),
           "stages": {}}
    out.update(moved)
    for name, fn in stages.items():
        n = launches[name]
        ms = {False: [], True: []}
        for ch in (False, True):                # warm-up: lazy allocations, kernel loading
            fn(ch)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for ch in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn(ch)
                e1.record()
                torch.cuda.synchronize()
                ms[ch].append(e0.elapsed_time(e1) / n)
        out["stages"][name] = {("chroma_satd" if k else "luma_only"): {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                                                                       "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}
        out["stages"][name]["ratio"] = round(float(np.median(ms[True]) / np.median(ms[False])), 3)
        out["stages"][name]["launches_per_round"] = n
    if not a.no_steps:
        d = [bsteps[ch].bd.dir.cpu().numpy() for ch in (False, True)]
        out["b_step_dir_changed_by_chroma"] = round(float((d[0] != d[1]).mean()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
