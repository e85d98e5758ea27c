"""Expected results of the I-picture stage (x265hip_intra_picture), assembled from the oracle's pieces.

The oracle has no intra-picture function, so the expectation is a coding-order walk in Python: per block the neighbour flags and the
reference samples are a literal restatement of Predict::initIntraNeighbors / fillReferenceSamples (source/common/predict.cpp:664-876, the
I-slice arm) and of Predict::initAdiPattern's ALL_IDX arm (:600-650) - line buffer, over-copy and substitution walk as the reference
writes them, NOT the closed form the kernel uses -, the 35 predictions, the [1 2 1] filter and sa8d are the oracle table's own slots
cu[].intra_pred[mode] / cu[].intra_filter / cu[].sa8d (where the real reference build is present its slots are called beside them and
must agree, and x265ref_pred_intra must reproduce the winning prediction), and the coded block is O.intra_recon, luma and chroma.
What remains here is the integer arithmetic of Search::checkIntraInInter (search.cpp:1344-1446) and of
CUData::getIntraDirLumaPredictor (cudata.cpp:910-953)."""
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_api as O          # noqa: E402
import harness                  # noqa: E402
import step_chain as SC         # noqa: E402

F =importlib.import_module("x265-yuuki-asuna_amd.frames")
H = importlib.import_module("x265-yuuki-asuna_amd.hipabi")

MODE_BITS = (2, 3, 6)
LAMBDA8 = 1024
# constants.cpp:561 g_intraFilterFlags
FILTER_FLAGS = [0x38, 0x00] + [0x38, 0x30, 0x30, 0x30, 0x30, 0x30, 0x30, 0x20, 0x00, 0x20, 0x30, 0x30, 0x30, 0x30, 0x30, 0x30] * 2 + [0x38]
SCAN_ORDER = [1, 0] + list(range(2, 35))          # DC, planar, 2 .. 34 (search.cpp:1357-1444)


def zorder(z):
    return (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4), ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)


def zindex(bx, by):
    z = 0
    for k in range(3):
        z |= ((bx >> k) & 1) << (2 * k) | ((by >> k) & 1) << (2 * k + 1)
    return z


def waves(w64, h64):
    return w64 // 64 + 2 * (h64 // 64 - 1)


def coding_position(x, y, n, w64):
    """(CTU address, z index of the n x n block inside its CTU) of the block that holds luma sample (x, y)."""
    return (y // 64) * (w64 // 64) + x // 64, zindex((x % 64) // n, (y % 64) // n)


def sample_available(x, y, cur, n, w64, h64):
    """A sample is available iff it lies inside the picture and its block precedes the current block (`cur` = its coding position) in
    coding order: CTUs in raster order, blocks in z-order inside a CTU (one slice, no constrained intra prediction)."""
    return 0 <= x < w64 and 0 <= y < h64 and coding_position(x, y, n, w64) < cur


def neighbour_flags(gx, gy, n, w64, h64):
    """bNeighborFlags of Predict::initIntraNeighbors (predict.cpp:664-715, I-slice arm) for the n x n luma block at (gx, gy): one flag per
    4-sample unit (the same flags serve the 2-sample units of its 4:2:0 chroma blocks) - [0, leftUnits) below-left + left from the bottom
    up, [leftUnits] above-left, then above and above-right."""
    cur = coding_position(gx, gy, n, w64)
    units = n // 4                                   # tuWidthInUnits = tuHeightInUnits (:681-682)
    left_units = above_units = 2 * units             # :683-684
    flags = [False] * (left_units + above_units + 1)
    flags[left_units] = sample_available(gx - 1, gy - 1, cur, n, w64, h64)                                          # :691
    for i in range(units):
        flags[left_units + 1 + i] = sample_available(gx + 4 * i, gy - 1, cur, n, w64, h64)                          # :693 above
        flags[left_units + 1 + units + i] = sample_available(gx + n + 4 * i, gy - 1, cur, n, w64, h64)              # :694 above-right
        flags[left_units - 1 - i] = sample_available(gx - 1, gy + 4 * i, cur, n, w64, h64)                          # :695 left, downwards
        flags[units - 1 - i] = sample_available(gx - 1, gy + n + 4 * i, cur, n, w64, h64)                           # :696 below-left, downwards
    return flags


def fill_reference_samples(plane, origin, stride, flags, tu, unit, depth):
    """Predict::fillReferenceSamples (predict.cpp:717-876), line by line.  plane: the flat reconstruction plane, origin: the element of the
    block's top-left sample, tu: the block size in this plane, unit: unitWidth = unitHeight (4 luma, 2 chroma of 4:2:0).  Returns
    dst[4 tu + 1]: [0] corner, [1..2 tu] above + above-right, [2 tu + 1..4 tu] left + below-left."""
    dc_value = 1 << (depth - 1)                                     # :719
    total_units = len(flags)
    above_units = left_units = (total_units - 1) // 2
    num = sum(bool(f) for f in flags)
    ref_size = tu * 2 + 1                                           # :723
    dst = np.zeros(4 * tu + 1, plane.dtype)
    if num == 0:                                                    # :726-735
        dst[:] = dc_value
    elif num == total_units:                                        # :736-749
        t = origin - stride - 1
        dst[:ref_size] = plane[t:t + ref_size]
        t = origin - 1
        for i in range(ref_size - 1):
            dst[i + ref_size] = plane[t]
            t += stride
    else:                                                           # :750-875
        total_samples = left_units * unit + (above_units + 1) * unit
        line = [dc_value] * total_samples                           # :763-764
        t = origin - stride - 1
        adi = left_units * unit                                     # :768
        if flags[left_units]:                                       # :770-775
            for i in range(unit):
                line[adi + i] = int(plane[t])
        t += stride                                                 # :778
        adi -= 1
        for j in range(left_units * unit):                          # :781-784 (over-copy: unavailable units are overwritten below)
            line[adi - j] = int(plane[t + j * stride])
        t = origin - stride                                         # :787
        adi = left_units * unit + unit
        for j in range(above_units * unit):                         # :790 (over-copy)
            line[adi + j] = int(plane[t + j])
        curr, nxt, adi = 0, 1, 0                                    # :793-795
        if not flags[0]:                                            # :797-846
            while nxt < total_units and not flags[nxt]:
                nxt += 1
            # pAdiLineTopRowOffset = leftUnits * (unitHeight - unitWidth) = 0 in 4:2:0 (:796, :803)
            ref_sample = line[nxt * unit]
            while curr < nxt:                                       # :810-827 (left column, then top row: the same stride here)
                for i in range(unit):
                    line[adi + i] = ref_sample
                adi += unit
                curr += 1
        while curr < total_units:                                   # :849-866
            if not flags[curr]:
                ref_sample = line[adi - 1]
                for i in range(unit):
                    line[adi + i] = ref_sample
            adi += unit
            curr += 1
        adi = ref_size + unit - 2                                   # :869-870
        dst[:ref_size] = line[adi:adi + ref_size]
        adi = ref_size - 1                                          # :872-874
        for i in range(ref_size - 1):
            dst[i + ref_size] = line[adi - (i + 1)]
    return dst


class Slots:
    """cu[].intra_pred[mode], cu[].intra_filter and cu[].sa8d of the n x n luma CU from the oracle's table - and from the real reference's
    where it is built: both are called every time and must agree."""

    def __init__(self, depth, n, with_reference=True):
        idx = int(np.log2(n)) - 2
        tabs = [harness.load_oracle(depth, ROOT)]
        ref = harness.load_reference(depth, ROOT) if with_reference else None
        if ref is not None:
            tabs.append(ref)
        self.keep, self.tables = tabs, len(tabs)
        self.pred = [[t.fn(f"cu[{idx}].intra_pred[{m}]") for m in range(35)] for t in tabs]
        self.filt = [t.fn(f"cu[{idx}].intra_filter") for t in tabs]
        self.sa8d = [t.fn(f"cu[{idx}].sa8d") for t in tabs]
        assert all(self.filt) and all(self.sa8d) and all(all(p) for p in self.pred)
        self.n, self.depth, self.dt = n, depth, harness.pix_dtype(depth)
        self.ref_pred_intra = None
        if ref is not None and hasattr(ref._owner, "x265ref_pred_intra"):
            self.ref_pred_intra = ref._owner.x265ref_pred_intra
            self.ref_pred_intra.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]

    def intra_filter(self, ref_buf):
        outs = []
        for f in self.filt:
            d = np.zeros(4 * self.n + 1 + 32, self.dt)
            f(ref_buf.ctypes.data, d.ctypes.data)
            outs.append(d[:4 * self.n + 1].copy())
        assert all(np.array_equal(outs[0], o) for o in outs[1:]), "oracle and reference intra_filter disagree"
        return outs[0]

    def predict(self, mode, buf, b_filter):
        outs = []
        for p in self.pred:
            d = np.zeros((self.n, self.n), self.dt)
            p[mode](d.ctypes.data, self.n, buf.ctypes.data, mode, b_filter)
            outs.append(d)
        assert all(np.array_equal(outs[0], o) for o in outs[1:]), f"oracle and reference intra_pred[{mode}] disagree"
        return outs[0]

    def cost(self, fenc_ptr, fenc_stride, pred):
        out = [s(fenc_ptr, fenc_stride, pred.ctypes.data, self.n) for s in self.sa8d]
        assert len(set(out)) == 1, f"oracle and reference sa8d disagree: {out}"
        return out[0]


def init_adi_pattern(ref_buf, n, depth, strong, slots):
    """Predict::initAdiPattern, the ALL_IDX arm (predict.cpp:611-649): the filtered copy of the reference samples of an n x n luma block
    (n = 8, 16, 32: (8 | 16 | 32) & tuSize always holds).  Returns (filtered, whether the strong form was taken)."""
    tu2 = n << 1
    top_left, top_last, left_last = int(ref_buf[0]), int(ref_buf[tu2]), int(ref_buf[tu2 + tu2])     # :614
    if strong and n == 32:                                                                          # :620
        threshold = 1 << (depth - 5)
        top_middle, left_middle = int(ref_buf[32]), int(ref_buf[tu2 + 32])
        if abs(top_left + top_last - (top_middle << 1)) < threshold and abs(top_left + left_last - (left_middle << 1)) < threshold:   # :626-627
            flt = np.zeros_like(ref_buf)
            shift = 5 + 1
            init = (top_left << shift) + n
            delta_l, delta_r = left_last - top_left, top_last - top_left
            flt[0] = top_left
            for i in range(1, tu2):
                flt[i + tu2] = (init + delta_l * i) >> shift
                flt[i] = (init + delta_r * i) >> shift
            flt[tu2] = top_last
            flt[tu2 + tu2] = left_last
            return flt, True
    return slots.intra_filter(ref_buf), False                                                       # :648


def most_probable_modes(left, above):
    """CUData::getIntraDirLumaPredictor (cudata.cpp:926-952) from the two neighbouring modes (DC where a neighbour does not count)."""
    if left == above:
        if left >= 2:
            return [left, ((left - 2 + 31) & 31) + 2, ((left - 2 + 1) & 31) + 2]
        return [0, 1, 26]
    return [left, above, 0 if (left and above) else (26 if left + above < 2 else 1)]


def garbage_planes(depth, shapes, seed=77):
    """Recon planes pre-filled with a pattern no reconstruction produces by accident."""
    r = np.random.default_rng([seed, depth])
    return [r.integers(0, 1 << depth, size=s).astype(harness.pix_dtype(depth)) for s in shapes]


def expect(depth, planes, w64, h64, level, qp, qp_c=None, flags=H.TU_INTRA_SLICE, lambda8=LAMBDA8, mode_bits=MODE_BITS, strong=True, chroma=True,
           with_reference=True, recon_init=None):
    """The walk.  planes: padded host (Y [rows, stride], Cb, Cr flat or 2-D) source planes in the PicYuv layout; recon_init: the recon
    planes' contents before the walk (default garbage_planes) - the result must not depend on them.  Returns dict: mode uint8, levels /
    num_sig / dist (+ _c0 / _c1), cost int32 [blocks, 2], recon / recon_c0 / recon_c1 (whole padded planes, margins as pre-filled) and
    the boolean coverage masks per block."""
    n = 8 << level
    bpc = 64 // n
    nblk = bpc * bpc
    cw, chh = w64 // 64, h64 // 64
    nctu = cw * chh
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = SC.chroma_geometry(w64)
    src = [np.ascontiguousarray(planes[0]).reshape(-1)] + ([np.ascontiguousarray(p).reshape(-1) for p in planes[1:3]] if chroma else [])
    init = recon_init if recon_init is not None else garbage_planes(depth, [s.shape for s in src])
    rec = [np.array(p, copy=True).reshape(-1) for p in init]
    slots = Slots(depth, n, with_reference)
    log2n = int(np.log2(n))
    es = src[0].itemsize
    nc = n // 2
    qp_c = qp_c if qp_c is not None else (qp, qp)
    tot = nctu * nblk
    max_val = (1 << depth) - 1
    mode_out = np.zeros(tot, np.uint8)
    cost_out = np.zeros((tot, 2), np.int32)
    lev = [np.zeros(tot * n * n, np.int16)] + [np.zeros(tot * nc * nc, np.int16) for _ in range(2)]
    ns = [np.zeros(tot, np.uint32) for _ in range(3)]
    dist = [np.zeros(tot, np.uint64) for _ in range(3)]
    names = ("dc", "planar", "angular_lt18", "angular_ge18", "mpm_priced", "non_mpm", "left_above_differ", "num_sig_0", "num_sig_gt1", "strong_taken",
             "strong_refused", "bits_flip", "edge_clip", "edge_clip_lo", "edge_clip_hi", "cost_tie", "tie_not_p0", "level_sat", "recon_at_limit", "chroma_coded")
    masks = {k: np.zeros(tot, bool) for k in names}
    job = np.zeros(1, dtype=H.job_dtype())
    for ctu in range(nctu):
        cx, cy = (ctu % cw) * 64, (ctu // cw) * 64
        for z in range(nblk):
            bx, by = zorder(z)
            gx, gy = cx + bx * n, cy + by * n
            b = ctu * nblk + z
            flg = neighbour_flags(gx, gy, n, w64, h64)
            off = org + gy * stride + gx
            ref_buf = fill_reference_samples(rec[0], off, stride, flg, n, 4, depth)
            flt_buf, took_strong = init_adi_pattern(ref_buf, n, depth, strong, slots)
            # the three most probable modes (cudata.cpp:917-924): the left block if it is inside the picture, the above block only inside the CTU
            left = int(mode_out[coding_index(gx - 1, gy, n, w64, nblk)]) if gx > 0 else 1
            above = int(mode_out[coding_index(gx, gy - 1, n, w64, nblk)]) if by > 0 else 1
            preds = most_probable_modes(left, above)
            fp = src[0].ctypes.data + off * es
            best = None                     # (cost, sad, mode, bits)
            best_sad = None
            costs = {}
            for mode in SCAN_ORDER:
                buf = ref_buf if mode == 1 else (flt_buf if FILTER_FLAGS[mode] & n else ref_buf)        # search.cpp:1358, :1365-1369, :1394
                p = slots.predict(mode, buf, 1 if (n <= 16 and mode != 0) else 0)
                sad = slots.cost(fp, stride, p)
                bits = mode_bits[0] if mode == preds[0] else (mode_bits[1] if mode in preds[1:] else mode_bits[2])
                cost = sad + ((bits * lambda8 + 128) >> 8)                                              # rdcost.h:148-153
                costs[mode] = cost
                if best is None or cost < best[0]:                                                      # COPY4_IF_LT: strict, in scan order
                    best = (cost, sad, mode, bits, p)
                if best_sad is None or sad < best_sad[0]:
                    best_sad = (sad, mode)
            cost, sad, mode, bits, pwin = best
            if slots.ref_pred_intra is not None:
                want = np.zeros((n, n), slots.dt)
                assert slots.ref_pred_intra(mode, log2n, ref_buf.ctypes.data, flt_buf.ctypes.data, 0, want.ctypes.data) == 0
                assert np.array_equal(want, pwin), f"block {b}: x265ref_pred_intra disagrees with the winning prediction of mode {mode}"
            mode_out[b] = mode
            cost_out[b] = (sad, cost)
            nbs = np.concatenate([ref_buf, flt_buf])
            job["off"][0] = (off, 0, 4 * n + 1, 0)
            job["arg"][0, 0] = mode
            r, l, s_, d = O.intra_recon(depth, n, src[0], stride, nbs, n * n, n, qp, flags, job)
            rec[0].reshape(rows, stride)[F.MARGIN_Y + gy:F.MARGIN_Y + gy + n, F.MARGIN_X + gx:F.MARGIN_X + gx + n] = r.reshape(n, n)
            lev[0][b * n * n:(b + 1) * n * n], ns[0][b], dist[0][b] = l, s_[0], d[0]
            if chroma:
                offc = oc + (gy // 2) * sc + gx // 2
                for c in range(2):
                    cb = fill_reference_samples(rec[1 + c], offc, sc, flg, nc, 2, depth)                # initAdiPatternChroma (:652-662): no filtering in 4:2:0
                    job["off"][0] = (offc, 0, 0, 0)
                    r, l, s_, d = O.intra_recon(depth, nc, src[1 + c], sc, cb, nc * nc, nc, qp_c[c], flags, job, chroma=True)
                    if slots.ref_pred_intra is not None:
                        want = np.zeros((nc, nc), slots.dt)
                        assert slots.ref_pred_intra(mode, log2n - 1, cb.ctypes.data, cb.ctypes.data, 1, want.ctypes.data) == 0
                        if int(s_[0]) == 0:            # nothing coded: the reconstruction IS the prediction
                            assert np.array_equal(want, r.reshape(nc, nc)), f"block {b} plane {1 + c}: x265ref_pred_intra disagrees with the chroma prediction"
                    y0, x0 = F.CHROMA_MARGIN_Y + gy // 2, F.CHROMA_MARGIN_X + gx // 2
                    rec[1 + c].reshape(-1, sc)[y0:y0 + nc, x0:x0 + nc] = r.reshape(nc, nc)
                    lev[1 + c][b * nc * nc:(b + 1) * nc * nc], ns[1 + c][b], dist[1 + c][b] = l, s_[0], d[0]
            masks["dc"][b], masks["planar"][b] = mode == 1, mode == 0
            masks["angular_lt18"][b], masks["angular_ge18"][b] = 2 <= mode < 18, mode >= 18
            masks["mpm_priced"][b], masks["non_mpm"][b] = mode in preds, mode not in preds
            masks["left_above_differ"][b] = left != above
            masks["num_sig_0"][b], masks["num_sig_gt1"][b] = ns[0][b] == 0, ns[0][b] > 1
            masks["strong_taken"][b], masks["strong_refused"][b] = took_strong, (n == 32 and strong and not took_strong)
            masks["bits_flip"][b] = best_sad[1] != mode
            if mode in (10, 26) and n <= 16:
                # the edge filter of the pure directions before its clip (intrapred.cpp:137-142): main = the arm the mode copies, side = the other
                main0, side0 = (1, 2 * n + 1) if mode == 26 else (2 * n + 1, 1)
                edge = int(ref_buf[main0]) + ((ref_buf[side0:side0 + n].astype(np.int64) - int(ref_buf[0])) >> 1)
                masks["edge_clip_lo"][b], masks["edge_clip_hi"][b] = (edge < 0).any(), (edge > max_val).any()
                masks["edge_clip"][b] = masks["edge_clip_lo"][b] or masks["edge_clip_hi"][b]
            tied = [m for m in SCAN_ORDER if costs[m] == cost]
            masks["cost_tie"][b] = len(tied) > 1
            masks["tie_not_p0"][b] = len(tied) > 1 and preds[0] in tied and preds[0] != mode
            lb = lev[0][b * n * n:(b + 1) * n * n]
            masks["level_sat"][b] = ((lb == -32768) | (lb == 32767)).any()
            yb = rec[0].reshape(rows, stride)[F.MARGIN_Y + gy:F.MARGIN_Y + gy + n, F.MARGIN_X + gx:F.MARGIN_X + gx + n]
            masks["recon_at_limit"][b] = ((yb == 0) | (yb == max_val)).any()
            masks["chroma_coded"][b] = chroma and (ns[1][b] > 0 or ns[2][b] > 0)
    out = dict(mode=mode_out, cost=cost_out, levels=lev[0], num_sig=ns[0], dist=dist[0], recon=rec[0], masks=masks, tables=slots.tables)
    if chroma:
        for c in range(2):
            out.update({"levels_c%d" % c: lev[1 + c], "num_sig_c%d" % c: ns[1 + c], "dist_c%d" % c: dist[1 + c], "recon_c%d" % c: rec[1 + c]})
    return out


def coding_index(x, y, n, w64, nblk):
    ctu, z = coding_position(x, y, n, w64)
    return ctu * nblk + z


def reads_of_block(gx, gy, n, w64, h64):
    """Coding positions (CTU address, z) of every block the walk reads reconstructed samples of for the block at (gx, gy): the owners of
    the available units."""
    flg = neighbour_flags(gx, gy, n, w64, h64)
    units = n // 4
    lu = 2 * units
    pos = [(gx - 1, gy + 2 * n - 1 - 4 * i) for i in range(lu)] + [(gx - 1, gy - 1)] + [(gx + 4 * i, gy - 1) for i in range(lu)]
    return sorted({coding_position(x, y, n, w64) for (x, y), f in zip(pos, flg) if f})


def test_picture(depth, w=256, h=192, seed=5):
    """(Y, Cb, Cr) of the picture the tests walk: per 64-column band flat areas, gradients, stripes at several angles, texture and noise
    (see test_ipicture_cpu.test_picture_meets_every_outcome for what the walk finds on it)."""
    r = np.random.default_rng([seed, 8])             # the same 8-bit pattern at every depth, scaled
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    y = np.zeros((h, w))
    angles = (0.0, 90.0, 45.0, 135.0, 22.0, 68.0, 112.0, 158.0, 10.0, 80.0, 30.0, 150.0)
    k = 0
    for by in range(0, h, 32):
        for bx in range(0, w, 32):
            kind = (bx // 32 + 3 * (by // 32)) % 8
            ys, xs = yy[by:by + 32, bx:bx + 32], xx[by:by + 32, bx:bx + 32]
            if kind == 0:
                t = np.full((32, 32), 60.0 + 17 * ((bx // 32 + by // 32) % 7))                          # flat
            elif kind == 1:
                t = 40 + 2.0 * (xs - bx) + 1.5 * (ys - by) + r.normal(0, 0.4, (32, 32))                 # gradient
            elif kind in (2, 3, 4):
                a = np.deg2rad(angles[k % len(angles)])
                k += 1
                t = 128 + 70 * np.sign(np.sin((xs * np.cos(a) + ys * np.sin(a)) * (2 * np.pi / (7 + 2 * kind))))   # stripes
            elif kind == 5:
                # texture of period 16 in both directions: corner, middle and end of a 32x32 block's reference rows agree (the strong
                # smoothing tests pass) while the samples between them swing - the bilinear form and [1 2 1] differ widely
                t = 128 + 35 * np.sin(xs * (2 * np.pi / 16)) + 35 * np.cos(ys * (2 * np.pi / 16)) + r.normal(0, 1.0, (32, 32))
            elif kind == 6:
                t = 128 + r.normal(0, 30, (32, 32))                                                     # noise
            else:
                t = 100 + 0.6 * (xs - bx) + r.normal(0, 1.2, (32, 32))                                  # shallow gradient + fine noise
            y[by:by + 32, bx:bx + 32] = t
    # the last 64 columns: one smooth ramp with fine noise, wider than a 32x32 block and its neighbours - reference rows there pass the
    # strong-smoothing tests, and the bilinear form differs from [1 2 1] by the noise it removes
    y[:, w - 64:] = 90 + 0.5 * (xx[:, w - 64:] - (w - 64)) + 0.3 * yy[:, w - 64:] + r.normal(0, 1.2, (h, 64))
    sc = 1 << (depth - 8)
    dt = harness.pix_dtype(depth)
    mx = (1 << depth) - 1
    yq = np.clip(np.rint(y), 0, 255)
    Y = np.clip(yq * sc + (r.integers(0, sc, size=y.shape) if sc > 1 else 0), 0, mx).astype(dt)
    sub = yq.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    cb = np.clip(np.rint((0.5 * sub + 64 + r.normal(0, 1.5, sub.shape)) * sc), 0, mx).astype(dt)
    cr = np.clip(np.rint((255 - 0.5 * sub - 40 + r.normal(0, 1.5, sub.shape)) * sc), 0, mx).astype(dt)
    return Y, cb, cr


def padded_planes(yuv):
    """(Y, Cb, Cr) pictures -> the padded host planes expect() takes (and w64, h64)."""
    y, stride, org, w64, h64 = F.pad_plane(yuv[0])
    return (y, F.pad_chroma(yuv[1], w64, h64)[0], F.pad_chroma(yuv[2], w64, h64)[0]), w64, h64


def i_chain(depth, planes, w64, h64, level, qp, sao_rdo=None, tu_flags=H.TU_INTRA_SLICE | H.TU_SIGN_HIDE, cores=0, avx2=False, with_reference=False, **kw):
    """One I picture through the oracle, stage by stage (the CPU twin of stages.IFramePipeline.run with chroma, deblocking and SAO
    applied): the walk, the boundary strengths of an all-intra picture, deblocking, SAO, border extension.  Returns every stage output by
    name (bidir_expect.compare takes it)."""
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    nctu = (w64 // 64) * (h64 // 64)
    qpc = S.chroma_quant_qp(qp, depth)
    e = expect(depth, planes, w64, h64, level, qp, qp_c=(qpc, qpc), flags=tu_flags, with_reference=with_reference, **kw)
    out = {k: e[k] for k in ("mode", "levels", "num_sig", "dist", "levels_c0", "levels_c1", "num_sig_c0", "num_sig_c1")}
    nblk = 64 >> (2 * level)
    bv, bh = O.deblock_bs_inter(depth, w64, h64, level, np.zeros((nctu * 85, 2), np.int32), e["num_sig"], avx2=avx2, intra=np.ones(nctu * nblk, np.uint8))
    return SC.filter_tail(out, depth, planes, e["recon"], [e["recon_c0"], e["recon_c1"]], bv, bh, qp, w64, h64, sao_rdo=sao_rdo, cores=cores, avx2=avx2)


def i_device_outputs(pipe, dt):
    """The same names from a stages.IFramePipeline after run() (chroma, deblocking, SAO applied)."""
    out = SC.step_outputs(pipe, dt)
    out["mode"] = pipe.ip.mode.cpu().numpy()
    return out
