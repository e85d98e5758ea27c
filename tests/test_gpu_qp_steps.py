"""GPU parity of the I-picture stage and of the three frame steps under per-block QP maps.

  * x265hip_intra_picture with qp_map + lambda8_by_qp against the coding-order walk with the block's own QPs and lambda
    (qp_map_expect.walk, built from the pieces of tests/intra_expect.py), also with a map and a lambda table at and beyond the ends of their ranges.
  * Closed loop at 256x192 for FramePipeline, BFramePipeline and IFramePipeline: AdaptiveQuant offsets -> CuQpMaps -> set_qp_maps -> one
    step, stage by stage against the oracle chain (qp_map_expect.p_chain / b_chain / i_chain: the TU stages composed from one oracle run
    per QP, deblock_luma / deblock_chroma with qp_map = cu_qp); set_qp_maps(None) afterwards reproduces the uniform step's checksum.
  * MiniGop with an i_step and maps on all three steps, 5 pictures.
Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import intra_cases as IC
import intra_expect as IE
import qp_map_expect as QE

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
H = importlib.import_module("x265-yuuki-asuna_amd.hipabi")

W, HT_ = 256, 192
_walks = {}


def _up(a, dev):
    import torch
    return torch.from_numpy(a if a.dtype in (np.uint8, np.int8, np.int32) else a.view(np.int16 if a.itemsize == 2 else np.int32)).to(dev)


def _intra_case(depth, level, sign_hide):
    """picture, map, lambda table and the walk's expectation: computed once per case and shared (nothing modifies them)"""
    key = (depth, level, sign_hide)
    if key not in _walks:
        yuv = IE.test_picture(depth, W, HT_)
        pl, w64, h64 = IE.padded_planes(yuv)
        nb = (w64 // 64) * (h64 // 64) * (64 >> (2 * level))
        rng = np.random.default_rng([97, depth, level])
        # three planes of block QPs: luma from the tests' map values, chroma maps of their own (the kernel must not derive them from luma)
        qpb = [QE.block_qps(nb, nb, QE.map_values(depth), rng, False) for _ in range(3)]
        QE.coverage(qpb[0], w64, h64, level, depth)
        tu = np.stack([QE.cells_of_blocks(q, w64, h64, level) for q in qpb])
        lam = QE.lambda8_table(depth)
        flags = H.TU_INTRA_SLICE | (H.TU_SIGN_HIDE if sign_hide else 0)
        init = IE.garbage_planes(depth, [np.asarray(p).reshape(-1).shape for p in pl])
        e = QE.walk(depth, pl, w64, h64, level, tu, lambda8_by_qp=lam, flags=flags, recon_init=init)
        e0 = QE.walk(depth, pl, w64, h64, level, tu, lambda8_by_qp=None, lambda8=IE.LAMBDA8, flags=flags, recon_init=init)
        _walks[key] = (yuv, w64, h64, tu, lam, flags, init, e, e0)
    return _walks[key]


@pytest.mark.parametrize("depth,level,sign_hide", [(8, 0, True), (8, 1, False), (8, 2, True), (10, 0, False), (10, 1, True), (10, 2, False)])
def test_intra_picture_with_maps_equals_the_walk(depth, level, sign_hide):
    """256x192, levels 0 - 2 at 8 and 10 bits: mode, cost, levels, num_sig, SSE and the Y / Cb / Cr planes, with the map and the lambda table,
    and with the map alone (lambda8_by_qp NULL: the record's lambda8 prices every block)."""
    import torch
    dev = torch.device("cuda:0")
    yuv, w64, h64, tu, lam, flags, init, e, e0 = _intra_case(depth, level, sign_hide)
    cur = P.DevicePicture(yuv[0], dev, yuv[1], yuv[2])
    dt = cur.host.dtype
    qp = 30 + 6 * (depth - 8)
    ip = S.IntraPicture((w64 // 64) * (h64 // 64), w64, h64, depth, level, qp, dev, flags=flags, chroma=True, qp_c=(qp - 1, qp - 2), lambda8=IE.LAMBDA8,
                        mode_bits=IE.MODE_BITS, want_cost=True)
    ip.qp_map = _up(tu.reshape(-1), dev)
    d_lam = _up(lam.view(np.int32), dev)
    for table, want in ((d_lam, e), (None, e0)):
        ip.lambda8_by_qp = table
        rec = [_up(p.copy(), dev) for p in init]
        ip.run(cur, rec[0], rec[1:])
        torch.cuda.synchronize()
        got = {"mode": ip.mode.cpu().numpy(), "cost": ip.cost.cpu().numpy().reshape(-1, 2), "levels": ip.levels.cpu().numpy(),
               "num_sig": ip.num_sig.cpu().numpy(), "dist": ip.dist.cpu().numpy(), "recon": rec[0].cpu().numpy().view(dt)}
        for c in range(2):
            got.update({"levels_c%d" % c: ip.levels_c[c].cpu().numpy(), "num_sig_c%d" % c: ip.num_sig_c[c].cpu().numpy(),
                        "dist_c%d" % c: ip.dist_c[c].cpu().numpy(), "recon_c%d" % c: rec[1 + c].cpu().numpy().view(dt)})
        bad = BE.compare(got, {k: v for k, v in want.items() if k != "lambda8"})
        assert not bad, (("with" if table is not None else "without") + " lambda8_by_qp", bad)
    # the table matters: blocks are priced with different lambdas, and some decisions differ from those at the record's lambda8
    assert len(np.unique(e["lambda8"])) >= 6 and not np.array_equal(e["cost"], e0["cost"])
    assert not np.array_equal(e["mode"], e0["mode"]), "no block's decision depends on its lambda: the case does not test the table"


@pytest.mark.parametrize("depth", [8, 10])
def test_intra_picture_with_maps_at_the_range_ends(depth):
    """intra_cases' edges picture (192x128) at level 1 under a map whose entries are 0, 1, max - 1, max, two values between and int8 values
    outside the range (-128, -1, 127: they code like 0 and like max), chroma planes with maps of their own, and a lambda table with an entry
    above 2^24 (priced like 2^24) and a 0 - against qp_map_expect.walk, which clamps both the same way (test_intra_cases_cpu shows the map to
    be what this says)."""
    import torch
    dev = torch.device("cuda:0")
    level, flags = 1, H.TU_INTRA_SLICE | H.TU_SIGN_HIDE
    key = ("range ends", depth)
    if key not in _walks:
        yuv = IC.build(depth, "edges")
        pl, w64, h64 = IC.planes(depth, "edges", level)
        tu, lam, _ = IC.range_end_map(depth, level)
        init = IE.garbage_planes(depth, [np.asarray(p).reshape(-1).shape for p in pl])
        _walks[key] = (yuv, w64, h64, tu, lam, init, QE.walk(depth, pl, w64, h64, level, tu, lambda8_by_qp=lam, flags=flags, recon_init=init))
    yuv, w64, h64, tu, lam, init, e = _walks[key]
    cur = P.DevicePicture(yuv[0], dev, yuv[1], yuv[2])
    dt = cur.host.dtype
    qp = 30 + 6 * (depth - 8)
    ip = S.IntraPicture((w64 // 64) * (h64 // 64), w64, h64, depth, level, qp, dev, flags=flags, chroma=True, qp_c=(qp, qp), lambda8=IE.LAMBDA8,
                        mode_bits=IE.MODE_BITS, want_cost=True)
    ip.qp_map, ip.lambda8_by_qp = _up(tu.reshape(-1), dev), _up(lam.view(np.int32), dev)
    rec = [_up(p.copy(), dev) for p in init]
    ip.run(cur, rec[0], rec[1:])
    torch.cuda.synchronize()
    got = {"mode": ip.mode.cpu().numpy(), "cost": ip.cost.cpu().numpy().reshape(-1, 2), "levels": ip.levels.cpu().numpy(),
           "num_sig": ip.num_sig.cpu().numpy(), "dist": ip.dist.cpu().numpy(), "recon": rec[0].cpu().numpy().view(dt)}
    for c in range(2):
        got.update({"levels_c%d" % c: ip.levels_c[c].cpu().numpy(), "num_sig_c%d" % c: ip.num_sig_c[c].cpu().numpy(),
                    "dist_c%d" % c: ip.dist_c[c].cpu().numpy(), "recon_c%d" % c: rec[1 + c].cpu().numpy().view(dt)})
    bad = BE.compare(got, {k: v for k, v in e.items() if k != "lambda8"})
    assert not bad, bad
    assert (e["lambda8"] == 1 << 24).any() and (tu < 0).any() and (tu > 51 + 6 * (depth - 8)).any()


def _aq_maps(pic, depth, level, dev, base_qp):
    """AdaptiveQuant offsets of the picture (the x265 defaults: aq-mode 2, strength 1) -> CuQpMaps"""
    aq = S.AdaptiveQuant(pic.w64, pic.h64, depth, dev, qg_size=16, aq_mode=2, aq_strength=1.0)
    offs, _, _, _ = aq.run(pic, cb=pic.c[0], cr=pic.c[1], stride_c=pic.stride_c, org_c=pic.org_c)
    maps = S.CuQpMaps(pic.w64, pic.h64, depth, level, dev, qg_size=16).run(base_qp, offs)
    assert len(np.unique(maps.cu_qp_host)) >= 3, np.unique(maps.cu_qp_host)
    assert np.array_equal(maps.tu_qp.cpu().numpy().reshape(maps.tu_qp_host.shape), maps.tu_qp_host)
    return maps


def _steps(depth, level, dev, w64, h64, qp):
    kw = dict(level=level, qp=qp, deblock=True, chroma=True, sign_hide=True)
    return (S.FramePipeline(w64, h64, depth, dev, rng=12, subme=3, want_surf=False, **kw), S.BFramePipeline(w64, h64, depth, dev, rng=12, subme=3, **kw),
            S.IFramePipeline(w64, h64, depth, dev, **kw))


@pytest.mark.parametrize("kind", ["p", "b", "i"])
@pytest.mark.parametrize("depth,level", [(8, 2), (10, 1)])
def test_step_with_maps_equals_the_oracle_chain(kind, depth, level):
    import torch
    B = importlib.import_module("bench")
    dev = torch.device("cuda:0")
    qp = 30 + 6 * (depth - 8)
    clip = QE.varied_clip(BE.occluded_clip(W, HT_, 3, depth, 23), depth) if kind != "i" else [IE.test_picture(depth, W, HT_)] * 3
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    cur = pics[1]
    w64, h64 = cur.w64, cur.h64
    pipe = _steps(depth, level, dev, w64, h64, qp)["pbi".index(kind)]
    run = {"p": lambda: pipe.run(cur, pics[0]), "b": lambda: pipe.run(cur, pics[0], pics[2]), "i": lambda: pipe.run(cur)}[kind]
    run()
    torch.cuda.synchronize()
    uniform = pipe.checksum()
    maps = _aq_maps(cur, depth, level, dev, qp - 6 * (depth - 8) + 0.3)
    lam = QE.lambda8_table(depth)
    if kind == "i":
        pipe.set_qp_maps(maps, lambda8_by_qp=_up(lam.view(np.int32), dev))
    else:
        pipe.set_qp_maps(maps)
    run()
    torch.cuda.synchronize()
    assert pipe.checksum() != uniform
    got = QE.step_outputs(pipe, cur.host.dtype, kind)
    hp = [BE.padded_planes(c)[0] for c in clip]
    kw = dict(cores=B.effective_cpus(), avx2=BE.O.host_has_avx2())
    cu, tu = maps.cu_qp_host, maps.tu_qp_host
    if kind == "p":
        want = QE.p_chain(depth, hp[1], hp[0], w64, h64, 12, 3, level, qp, cu, tu, **kw)
    elif kind == "b":
        want = QE.b_chain(depth, hp[1], hp[0], hp[2], w64, h64, 12, 3, level, qp, cu, tu, **kw)
    else:
        want = QE.i_chain(depth, hp[1], w64, h64, level, qp, cu, tu, lambda8_by_qp=lam, avx2=kw["avx2"])
    bad = BE.compare(got, want)
    assert not bad, bad
    assert int(want["num_sig"].sum()) > 0 and (want["bs_ver"] > 0).any()
    # the deblocking stages read cu_qp: with the picture-wide QP instead the filtered picture differs
    pipe.db.qp_map = None
    run()
    torch.cuda.synchronize()
    assert not np.array_equal(pipe.final.cpu().numpy().view(cur.host.dtype).reshape(-1), want["recon"].reshape(-1)), "deblocking does not read the map"
    # cleared: the uniform step again
    pipe.set_qp_maps(None)
    run()
    torch.cuda.synchronize()
    assert pipe.checksum() == uniform


def test_unsupported_run_modes_raise_with_maps_set():
    import torch
    dev = torch.device("cuda:0")
    clip = QE.varied_clip(BE.occluded_clip(W, HT_, 2, 8, 23), 8)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    p, b, i = _steps(8, 2, dev, pics[0].w64, pics[0].h64, 30)
    maps = _aq_maps(pics[1], 8, 2, dev, 30.0)
    with pytest.raises(ValueError):
        p.set_qp_maps(S.CuQpMaps(pics[0].w64, pics[0].h64, 8, 1, dev))          # maps of another level
    p.set_qp_maps(maps)
    p.band_border = (True, False)
    with pytest.raises(ValueError):
        p.run(pics[1], pics[0])
    p.band_border = None
    p.rc.tables = H.tu_tables()
    with pytest.raises(H.X265HipError):                                          # scaling-list tables with a map: refused by the library
        p.run(pics[1], pics[0])


def test_mini_gop_with_maps_on_all_three_steps():
    """MiniGop with an i_step, gop 2, 5 pictures of 256x192, every step under maps of its own: pictures 0 / 2, 4 / 1, 3 are what the I / P / B
    step alone produces from the same references, and differ from the mini-GOP without maps."""
    import torch
    dev = torch.device("cuda:0")
    depth, level, qp, gop = 8, 2, 30, 2
    clip = QE.varied_clip(BE.occluded_clip(W, HT_, 5, depth, 71), depth)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    w64, h64 = pics[0].w64, pics[0].h64
    lam = _up(QE.lambda8_table(depth).view(np.int32), dev)
    maps = [_aq_maps(pics[k], depth, level, dev, 30.0 + k) for k in (0, 2, 1)]

    def gop_steps(with_maps):
        p, b, i = _steps(depth, level, dev, w64, h64, qp)
        if with_maps:
            i.set_qp_maps(maps[0], lambda8_by_qp=lam)
            p.set_qp_maps(maps[1])
            b.set_qp_maps(maps[2])
        return p, b, i
    p, b, i = gop_steps(True)
    order, out = S.MiniGop(p, b, gop, i_step=i).run(pics)
    p0, b0, i0 = gop_steps(False)
    _, out0 = S.MiniGop(p0, b0, gop, i_step=i0).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 2, 1, 4, 3]
    same = lambda a, c: all(torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(a, c))
    assert not any(same(out[k], out0[k]) for k in range(5))
    p, b, i = gop_steps(True)
    i.run(pics[0])
    assert same(i.final_planes(), out[0])
    ref = pics[0].like(out[0])
    for a in (2, 4):
        p.run(pics[a], ref)
        assert same(p.final_planes(), out[a]), f"anchor {a}"
        anchor = pics[a].like(out[a])
        b.run(pics[a - 1], ref, anchor)
        assert same(b.final_planes(), out[a - 1]), f"B picture {a - 1}"
        ref = anchor
