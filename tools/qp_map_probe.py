"""What a per-block QP map costs the coding stages: device-event timings of the luma TU stage and of the chroma pair with and without a map
(3840x2160, 8-bit, level 2 by default), and of the level-2 I step with and without maps.  Prints one JSON line.

    python tools/qp_map_probe.py [--width 3840 --height 2160 --depth 8 --level 2 --launches 20 --rounds 5]

Per stage and per variant: the median over `rounds` of the mean time of `launches` back-to-back launches between two device events, and the
spread (min, max) of the rounds.  The variants alternate inside a round, so that clock drift touches both alike."""
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
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-intra", action="store_true")
    a = ap.parse_args()
    import torch
    F = importlib.import_module("x265-yuuki-asuna_amd.frames")
    P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    dev = torch.device("cuda:0")
    clip = F.synth_clip(a.width, a.height, 2, depth=a.depth, seed=5)
    cur, ref = (P.DevicePicture(clip[k][0], dev, clip[k][1], clip[k][2]) for k in (1, 0))
    w64, h64 = cur.w64, cur.h64
    nctu = (w64 // 64) * (h64 // 64)
    qp = 27 + 6 * (a.depth - 8)
    rng = np.random.default_rng(11)
    # vectors of every phase, a few samples long
    q = rng.integers(-32, 33, size=(nctu * 85, 2))
    mv = np.zeros((nctu * 85, 2), np.int32)
    mv[:, 1] = (q[:, 0] & 0xffff) | (q[:, 1] << 16)
    d_mv = torch.from_numpy(mv.reshape(-1)).to(dev)
    # maps: AQ-like QPs around qp, one per block
    offs = rng.normal(0, 2.5, size=(-(-h64 // 16)) * (-(-w64 // 16)))
    maps = S.CuQpMaps(w64, h64, a.depth, a.level, dev).run(qp - 6 * (a.depth - 8), offs)
    rc = S.InterRecon(nctu, w64, h64, a.depth, a.level, qp, dev, intra_slice=2)
    rcc = [S.InterReconChroma(nctu, w64, h64, a.depth, a.level, S.chroma_quant_qp(qp, a.depth), dev, intra_slice=2) for _ in range(2)]
    recon = torch.zeros_like(cur.t)
    recon_c = [torch.zeros_like(p) for p in cur.c]

    def luma(with_map):
        rc.qp_map = maps.tu_qp[0] if with_map else None
        rc.run(cur, ref, recon, d_mv)

    def pair(with_map):
        for i in range(2):
            rcc[i].qp_map = maps.tu_qp[1 + i] if with_map else None
        S.InterReconChroma.run_pair(rcc, cur.c, ref.c, recon_c, cur.stride_c, cur.org_c, d_mv)

    stages = {"inter_recon": luma, "inter_recon_chroma_pair": pair}
    launches = {"inter_recon": a.launches, "inter_recon_chroma_pair": a.launches}
    if not a.no_intra:
        ipipe = S.IFramePipeline(w64, h64, a.depth, dev, level=a.level, qp=qp, deblock=True, chroma=True, sign_hide=True)
        lam = torch.full((52 + 6 * (a.depth - 8),), 1024, dtype=torch.int32, device=dev)

        def istep(with_map):
            ipipe.set_qp_maps(maps if with_map else None, lambda8_by_qp=lam if with_map else None)
            ipipe.run(cur)
        stages["i_step"] = istep
        launches["i_step"] = max(1, a.launches // 10)

    out = {"width": w64, "height": h64, "depth": a.depth, "level": a.level, "map_values": sorted(int(v) for v in np.unique(maps.tu_qp_host[0])),
           "device": torch.cuda.get_device_name(0), "stages": {}}
    for name, fn in stages.items():
        n = launches[name]
        ms = {False: [], True: []}
        for with_map in (False, True):          # warm-up: lazy allocations, kernel loading
            fn(with_map)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for with_map in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn(with_map)
                e1.record()
                torch.cuda.synchronize()
                ms[with_map].append(e0.elapsed_time(e1) / n)
        out["stages"][name] = {("with_map" if k else "without_map"): {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                                                                     "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}
        out["stages"][name]["launches_per_round"] = n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
