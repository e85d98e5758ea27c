#!/usr/bin/env python3
"""Time the P merge walk without and with the AMVP arm on one GPU, the method of tools/tmvp_probe.py: device events around `--steps` runs
of the walk alone, pictures 0, 1, 2 of the synthetic clip at the bench's settings.  Picture 1 is coded by MergePFramePipeline from picture
0; its mv_out is compressed to the collocated field (cur_delta 1); then the walk of picture 2 against picture 1 is timed through
x265hip_merge_decide, x265hip_merge_decide_col with that field, and x265hip_merge_decide_amvp without and with it.

  python tools/amvp_probe.py --steps 20 --level 2                 # one JSON line
  python tools/amvp_probe.py --level 2 --lib path/libx265hip.so   # another build of the library (one without the entry: the old walks only)

Shares, per entry: inter = blocks that keep their searched vector; for the AMVP entry also mvp_idx_1 (blocks whose final predictor is
the second one), mvd_zero (blocks whose vector equals its predictor) and need_sad (blocks whose two predictors differ while the vector's
bits against them tie - an upper bound of the blocks where selectMVP's SADs decide and the kernel spends extra slots, since predictors
that clip to one vector need none)."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


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
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per number")
    ap.add_argument("--lib", default=None, help="another build of libx265hip.so")
    a = ap.parse_args()
    import numpy as np
    import torch
    A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
    if a.lib:
        A.LIB_PATH = os.path.abspath(a.lib)
    F = importlib.import_module("x265-yuuki-asuna_amd.frames")
    P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    dev = torch.device("cuda:0")
    qp = a.qp + 12 * (a.depth == 10)
    clip = F.synth_clip(a.width, a.height, 3, depth=a.depth, seed=265)
    pics = [P.DevicePicture(c[0], dev, c[1], c[2]) for c in clip]
    has_amvp = hasattr(A.lib(), "x265hip_merge_decide_amvp")
    pipe = S.MergePFramePipeline(pics[0].w64, pics[0].h64, a.depth, dev, level=a.level, qp=qp, max_merge=a.max_merge)
    out = {"what": "MergeDecide.run alone", "lib": a.lib or "this tree", "width": a.width, "height": a.height, "depth": a.depth, "level": a.level,
           "steps": a.steps, "max_merge": a.max_merge, "waves": pipe.md.waves}
    pipe.run(pics[1], pics[0])                     # picture 1 from picture 0: its motion is picture 2's collocated field
    col = S.ColField(pipe.nctu, pics[0].w64, pics[0].h64, a.depth, dev).build(pipe.md.mv_out, a.level, 1)
    cur, ref = pics[2], pics[1]
    mv = pipe._search(cur, ref, lambda name: None)
    pipe.ic.run(cur, ref, mv)
    md = pipe.md

    def entry(name, stage, fn):
        ms = [round(timed(torch, fn, a.steps, a.warmup), 4) for _ in range(a.repeats)]
        out[name] = {"ms": ms, "us_per_wave": round(1000.0 * min(ms) / stage.waves, 3), "inter": round(1.0 - float(stage.merge.float().mean().item()), 5),
                     "checksum": stage.checksum()}
        return out[name]
    entry("merge_decide", md, lambda: md.run(cur, ref, mv, pipe.ic.cost))
    entry("merge_decide_col", md, lambda: md.run(cur, ref, mv, pipe.ic.cost, col=col, cur_delta=1))
    if has_amvp:
        ma = S.MergeDecide(pipe.nctu, pics[0].w64, pics[0].h64, a.depth, a.level, dev, max_merge=a.max_merge, lambda8=md.lambda8, qp=qp, amvp=True,
                           base_bits=pipe.ic.base_bits)
        for name, kw in (("merge_decide_amvp", {}), ("merge_decide_amvp_col", dict(col=col, cur_delta=1))):
            e = entry(name, ma, lambda: ma.run(cur, ref, mv, inter_sa8d=pipe.ic.cost, **kw))
            pm = ma.amvp.cpu().numpy().reshape(-1, 2).astype(np.int64)
            bits = ma.bit_sizes.cpu().numpy()
            sl = (np.arange(pipe.nctu * ma.nblk) // ma.nblk) * 85 + (0, 64, 80)[a.level] + np.arange(pipe.nctu * ma.nblk) % ma.nblk
            v = mv.cpu().numpy().reshape(-1, 2)[sl, 1].astype(np.int64)
            s16 = lambda x: ((x & 0xffff) ^ 0x8000) - 0x8000
            cost = lambda p: (bits[np.abs(s16(v) - s16(p))] + bits[np.abs(s16(v >> 16) - s16(p >> 16))] + np.float32(0.5)).astype(np.uint32)
            e.update({"mvp_idx_1": round(float(ma.mvp_idx.float().mean().item()), 5),
                      "mvd_zero": round(float((ma.mvd.reshape(-1, 2) == 0).all(dim=1).float().mean().item()), 5),
                      "need_sad": round(float(((pm[:, 0] != pm[:, 1]) & (cost(pm[:, 0]) == cost(pm[:, 1]))).mean()), 5)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
