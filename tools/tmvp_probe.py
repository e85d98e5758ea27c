#!/usr/bin/env python3
"""Time the P merge walk with and without the temporal candidate on one GPU, the method of tools/merge_probe.py: device events around
`--steps` runs of the walk alone, pictures 0, 1, 2 of the synthetic clip at the bench's settings.  Picture 1 is coded by
MergePFramePipeline from picture 0; its mv_out is compressed to the collocated field (cur_delta 1); then the walk of picture 2 against
picture 1 is timed through x265hip_merge_decide and through x265hip_merge_decide_col with that field.

  python tools/tmvp_probe.py --steps 20 --level 2                 # one JSON line
  python tools/tmvp_probe.py --level 2 --lib path/libx265hip.so   # another build of the library: the walk without the field only
                                                                    (--lib with a library that lacks the _col entry skips the rest)

Shares: temporal_present = blocks whose lookup finds motion (every block after a P picture); merged_on_temporal_vector = merged blocks
whose motion is their temporal vector - an upper bound of the blocks the temporal candidate won, since a spatial candidate may carry
the same vector (the walk does not write which candidate a vector came from)."""
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


def temporal_vectors(np, col_mv, col_delta, cw, ch, level, cur_delta):
    """(found, packed scaled vector) per block, index = ctu * blocks + z: the lookup of csrc/col_field.h restated for the shares."""
    n = 8 << level
    bpc = 64 // n
    found, vec = np.zeros(cw * ch * bpc * bpc, bool), np.zeros(cw * ch * bpc * bpc, np.int64)

    def scale(v):
        if cur_delta == 1:
            return v
        raise SystemExit("the probe codes consecutive pictures: cur_delta and col_delta are 1")
    for ctu in range(cw * ch):
        cx, cy = ctu % cw, ctu // cw
        for z in range(bpc * bpc):
            bx = (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4)
            by = ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)
            lx, ly = bx * n, by * n
            units = []
            if cx * 64 + lx + n < cw * 64 and cy * 64 + ly + n < ch * 64 and ly + n < 64:
                here = lx + n < 64
                units.append((ctu if here else ctu + 1) * 16 + ((ly + n) >> 4) * 4 + (((lx + n) >> 4) if here else 0))
            units.append(ctu * 16 + ((ly + n // 2) >> 4) * 4 + ((lx + n // 2) >> 4))
            for u in units:
                if col_delta[u]:
                    found[ctu * bpc * bpc + z], vec[ctu * bpc * bpc + z] = True, scale(int(col_mv[u]))
                    break
    return found, vec


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
    has_col = hasattr(A.lib(), "x265hip_merge_decide_col")
    pipe = S.MergePFramePipeline(pics[0].w64, pics[0].h64, a.depth, dev, level=a.level, qp=qp, max_merge=a.max_merge)
    out = {"what": "MergeDecide.run alone", "lib": a.lib or "this tree", "width": a.width, "height": a.height, "depth": a.depth, "level": a.level,
           "steps": a.steps, "max_merge": a.max_merge, "waves": pipe.md.waves}
    col = None
    if has_col:                                        # picture 1 from picture 0: its motion is picture 2's collocated field
        pipe.run(pics[1], pics[0])
        col = S.ColField(pipe.nctu, pics[0].w64, pics[0].h64, a.depth, dev).build(pipe.md.mv_out, a.level, 1)
    cur, ref = pics[2], pics[1]
    mv = pipe._search(cur, ref, lambda name: None)
    pipe.ic.run(cur, ref, mv)
    md = pipe.md
    ms = timed(torch, lambda: md.run(cur, ref, mv, pipe.ic.cost), a.steps, a.warmup)
    out.update({"walk_ms": round(ms, 4), "us_per_wave": round(1000.0 * ms / md.waves, 3), "merge_share": round(float(md.merge.float().mean().item()), 4),
                "checksum": md.checksum()})
    if col is not None:
        ms_col = timed(torch, lambda: md.run(cur, ref, mv, pipe.ic.cost, col=col, cur_delta=1), a.steps, a.warmup)
        sl = (torch.arange(pipe.nctu * md.nblk, device=dev) // md.nblk) * 85 + (0, 64, 80)[a.level] + torch.arange(pipe.nctu * md.nblk, device=dev) % md.nblk
        final = md.mv_out.reshape(-1, 2)[sl, 1].cpu().numpy().astype(np.int64)
        merged = md.merge.cpu().numpy() != 0
        found, vec = temporal_vectors(np, col.col_mv.cpu().numpy(), col.col_delta.cpu().numpy(), pics[0].w64 // 64, pics[0].h64 // 64, a.level, 1)
        out.update({"walk_col_ms": round(ms_col, 4), "us_per_wave_col": round(1000.0 * ms_col / md.waves, 3), "ratio": round(ms_col / ms, 4),
                    "merge_share_col": round(float(merged.mean()), 4), "temporal_present": round(float(found.mean()), 4),
                    "merged_on_temporal_vector": round(float((merged & found & (final == vec)).mean()), 4), "checksum_col": md.checksum()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
