"""Deterministic inputs for the chroma-SATD sub-pel tests (numpy and the oracle only, no torch).

Luma and the integer-stage records are subpel_cases.build's, unchanged.  The 4:2:0 chroma planes are made the same way: a reference
Cb / Cr picture of the case's kind, and a current picture assembled, 16 x 16 chroma quadrant by quadrant (the chroma of a 32 x 32 luma
quadrant), from the reference's own eighth-sample chroma (oracle_api.phase_planes(..., chroma=True)).  About half of the quadrants take
the luma quadrant's vector; the others take a vector of their own a few quarter samples away, so that chroma pulls the refinement
somewhere else than luma alone would.

tests/test_subpel_chroma_cpu.py asserts, with the oracle alone, what these cases reach; tests/test_gpu_subpel_chroma.py feeds them to
the kernels."""
import functools
import importlib
from types import SimpleNamespace

import numpy as np

import subpel_cases as SC

F = importlib.import_module("x265-yuuki-asuna_amd.frames")


@functools.lru_cache(maxsize=None)
def build(depth, width, height, R, kind, seed):
    """subpel_cases.build's case plus, per chroma plane (Cb, Cr): the padded current and reference planes (frames.pad_chroma geometry)
    and the 64 phases of the reference ([64, rows, stride_c], index yf * 8 + xf, phase 0 = the plane itself).  chroma_q[plane] is the
    quarter-sample luma vector (= eighth-sample chroma vector) each chroma quadrant was planted at.  Shared between tests: read only."""
    assert kind in SC.KINDS and not kind.startswith("flat")
    c = SC.build(depth, width, height, R, kind, seed)
    O = SC.oracle()
    maxv = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    rng = np.random.default_rng([seed, depth, R, SC.KINDS.index(kind), 2])
    cw, ch = c.w64 // 2, c.h64 // 2
    assert (R * 4 + 6 + 3) // 8 + 1 + 8 <= F.CHROMA_MARGIN_Y           # chroma phase planes are specified 8 samples in from the buffer edge
    cur_c, ref_c, phases, chroma_q = [], [], [], []
    stride_c = org_c = None
    for plane in range(2):
        if kind == "noise":
            ref_img = rng.integers(0, maxv + 1, size=(ch, cw)).astype(dt)
        else:                                                      # chroma overshoots at both ends whatever the luma kind is
            ref_img = SC.edges_picture(rng, cw, ch, maxv, dt)
        rbuf, stride_c, org_c = F.pad_chroma(ref_img, c.w64, c.h64)
        ph = O.phase_planes(depth, rbuf.reshape(-1), stride_c, rbuf.shape[0], chroma=True)
        ph = np.ascontiguousarray(np.concatenate([rbuf.reshape(1, *rbuf.shape), ph], axis=0))
        qh, qw = c.quad_i.shape[:2]
        cur_img = np.zeros((ch, cw), np.int64)
        cq = np.zeros((qh, qw, 2), np.int64)
        for gy in range(qh):
            for gx in range(qw):
                q = 4 * c.quad_i[gy, gx] + c.quad_f[gy, gx]
                own = rng.random() < 0.5
                if own:                                            # a vector of its own, 1 .. 3 quarter samples away on each axis
                    d = rng.integers(1, 4, size=2) * rng.choice((-1, 1), size=2)
                    q = np.clip(q + d, -4 * R - 3, 4 * R + 3)
                cq[gy, gx] = q
                sy, sx = F.CHROMA_MARGIN_Y + gy * 16 + int(q[1] >> 3), F.CHROMA_MARGIN_X + gx * 16 + int(q[0] >> 3)
                blk = ph[int(q[1] & 7) * 8 + int(q[0] & 7)][sy:sy + 16, sx:sx + 16].astype(np.int64)
                if rng.random() < 0.5:
                    blk = np.clip(blk + rng.integers(-2, 3, size=blk.shape), 0, maxv)
                if kind == "inverse" and rng.random() < 0.5:
                    blk = maxv - blk
                cur_img[gy * 16:gy * 16 + 16, gx * 16:gx * 16 + 16] = blk
        cbuf = F.pad_chroma(cur_img.astype(dt), c.w64, c.h64)[0]
        for a in (cbuf, rbuf, ph, cq):
            a.setflags(write=False)
        cur_c.append(cbuf); ref_c.append(rbuf); phases.append(ph); chroma_q.append(cq)
    return SimpleNamespace(luma=c, depth=depth, R=R, kind=kind, cur_c=cur_c, ref_c=ref_c, phases_c=phases, chroma_q=chroma_q,
                           stride_c=stride_c, org_c=org_c, w64=c.w64, h64=c.h64, nctu=c.nctu)


def chroma_pictures(cc):
    """The unpadded Cb / Cr pictures (current, reference) of a case, as pipeline.DevicePicture takes them."""
    y0, x0, h, w = F.CHROMA_MARGIN_Y, F.CHROMA_MARGIN_X, cc.h64 // 2, cc.w64 // 2
    cut = lambda b: np.ascontiguousarray(b[y0:y0 + h, x0:x0 + w])
    return [cut(b) for b in cc.cur_c], [cut(b) for b in cc.ref_c]


Case = SC.Case

# 192 x 128 = 6 CTUs, every record of every CTU is compared.  (depth, R, kind, seed) x subme; the flavour (phase planes for luma or
# interpolating) is the GPU test's second parameter.
def _cases():
    """Kinds chosen so that in EVERY case chroma moves >= 3 % of the vectors at levels 0 - 2 (tests/test_subpel_chroma_cpu.py): where luma
    matches as sharply as chroma (`edges` / `noise` luma beyond subme 3) its 4 x larger sample count decides alone, so most cases take
    luma that pulls less - `texture` (smooth) or `inverse` (no match) - while Cb / Cr are `edges` planes that clip at both ends throughout."""
    return [Case((8, 192, 128, 8, "edges", 11, 3)), Case((10, 192, 128, 8, "inverse", 12, 3)),
            Case((8, 192, 128, 8, "texture", 11, 4)), Case((10, 192, 128, 8, "inverse", 12, 4)),
            Case((8, 192, 128, 8, "inverse", 11, 5)), Case((10, 192, 128, 8, "texture", 12, 5)),
            Case((8, 192, 128, 8, "texture", 11, 7)), Case((10, 192, 128, 8, "inverse", 12, 7)),
            Case((12, 192, 128, 8, "inverse", 13, 7)),
            Case((8, 192, 128, 57, "inverse", 11, 3))]             # far vectors against the 40-row chroma margin


CHROMA_CASES = _cases()
LUMA_ONLY_CASES = [Case((8, 192, 128, 8, "edges", 11, 2)), Case((10, 192, 128, 8, "edges", 12, 2))]      # subme 2 with chroma operands = the luma-only records


# ---------------------------------------------------------------------------------------------------------------------------------
# The bidirectional decision with chroma: three pictures (list 0, current, list 1) with all three planes.
def six_stripe_yuv(depth, w=384, h=128, seed=21):
    """bidir_expect.six_stripe_lumas' recipe applied to Y, Cb and Cr alike: [list 0, cur, list 1], each (Y, Cb, Cr).  Six vertical stripes:
    (a) plain motion in luma while Cb / Cr match list 0 only (upper half) or list 1 only (lower half), (b) only list 0 matches, (c) only list 1 matches, (d) flat + noise (the zero candidate competes), (e) opposite
    patterns that only the coincident average cancels, (f) three identical pictures."""
    clip = F.synth_clip(w, h, 3, depth=depth, seed=seed)
    other = F.synth_clip(w, h, 3, depth=depth, seed=seed + 1000)
    pics = [[p.copy() for p in f] for f in clip]
    r = np.random.default_rng([seed, depth, 3])
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    for c in range(3):
        ph, pw = pics[0][c].shape
        q = pw // 6
        dt = pics[0][c].dtype
        pics[2][c][:, q:2 * q] = other[0][c][:, q:2 * q]
        pics[0][c][:, 2 * q:3 * q] = other[2][c][:, 2 * q:3 * q]
        for i in range(3):
            pics[i][c][:, 3 * q:4 * q] = np.clip(np.rint(128 * sc + r.normal(0, 3.0 * sc, size=(ph, q))), 0, mx).astype(dt)
        E = np.rint(r.normal(0, 20.0 * sc, size=(ph, q)))
        pics[0][c][:, 4 * q:5 * q] = np.clip(128 * sc + E, 0, mx).astype(dt)
        pics[2][c][:, 4 * q:5 * q] = np.clip(128 * sc - E, 0, mx).astype(dt)
        pics[1][c][:, 4 * q:5 * q] = np.clip(np.rint(128 * sc + r.normal(0, 1.0 * sc, size=(ph, q))), 0, mx).astype(dt)
        pics[0][c][:, 5 * q:] = pics[1][c][:, 5 * q:]
        pics[2][c][:, 5 * q:] = pics[1][c][:, 5 * q:]
        if c:
            # stripe (a) again, chroma only: luma moves plainly in both lists, but Cb / Cr match one list only - list 0 in the upper half
            # of the picture, list 1 in the lower half - so that the chroma term, not the records, turns the list decision
            pics[2][c][:ph // 2, :q] = other[0][c][:ph // 2, :q]
            pics[0][c][ph // 2:, :q] = other[2][c][ph // 2:, :q]
    return [tuple(p) for p in pics]


def refine_inputs(depth, R, cur_pad, ref_pad, w64, h64):
    """A namespace of build()'s shape for subpel_chroma_expect.walk from any pair of pictures: *_pad = padded (Y [rows, stride], Cb, Cr)
    host planes (frames.pad_plane / pad_chroma geometry).  The integer-stage records are the oracle's exhaustive search."""
    O = SC.oracle()
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    stride_c = w64 // 2 + 2 * F.CHROMA_MARGIN_X
    org_c = F.CHROMA_MARGIN_Y * stride_c + F.CHROMA_MARGIN_X
    nctu = (w64 // 64) * (h64 // 64)
    cost = F.mv_cost_table(R)
    cy, ry = cur_pad[0].reshape(rows, stride), ref_pad[0].reshape(rows, stride)
    _, best = O.me_fullsearch(depth, cy, stride, org, ry, stride, org, w64, h64, R, 0, nctu, cost, cost, want_surf=False)
    ph = O.phase_planes(depth, ry.reshape(-1), stride, rows)
    luma = SimpleNamespace(depth=depth, R=R, cur=cy, ref=ry, stride=stride, org=org, w64=w64, h64=h64, nctu=nctu, best=best, planes=[ry] + [ph[k] for k in range(15)])
    rc = [np.ascontiguousarray(p).reshape(-1, stride_c) for p in ref_pad[1:3]]
    phc = [np.ascontiguousarray(np.concatenate([p.reshape(1, *p.shape), O.phase_planes(depth, p.reshape(-1), stride_c, p.shape[0], chroma=True)], axis=0)) for p in rc]
    return SimpleNamespace(luma=luma, depth=depth, R=R, cur_c=[np.ascontiguousarray(p).reshape(-1, stride_c) for p in cur_pad[1:3]], ref_c=rc, phases_c=phc,
                           stride_c=stride_c, org_c=org_c, w64=w64, h64=h64, nctu=nctu)


def b_inputs(depth, R, pad, w64, h64):
    """The B case of three pictures: pad = [list 0, current, list 1], each the padded (Y, Cb, Cr) host planes."""
    lists = [refine_inputs(depth, R, pad[1], pad[l], w64, h64) for l in (0, 2)]
    a = lists[0]
    return SimpleNamespace(depth=depth, R=R, pad=[tuple(np.ascontiguousarray(p) for p in q) for q in pad], lists=lists, stride=a.luma.stride, org=a.luma.org,
                           stride_c=a.stride_c, org_c=a.org_c, w64=w64, h64=h64, nctu=a.nctu)


@functools.lru_cache(maxsize=None)
def build_b(depth, R=12, w=384, h=128, seed=21):
    """The six-stripe B case on the host (shared: read only): b_inputs of its three pictures, which `pics` keeps unpadded."""
    pics = six_stripe_yuv(depth, w, h, seed)
    pad = []
    for y, cb, cr in pics:
        yb, _, _, w64, h64 = F.pad_plane(y)
        pad.append((yb, F.pad_chroma(cb, w64, h64)[0], F.pad_chroma(cr, w64, h64)[0]))
    b = b_inputs(depth, R, pad, w64, h64)
    b.pics = pics
    return b
