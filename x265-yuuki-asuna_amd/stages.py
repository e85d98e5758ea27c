"""Later stages of the frame pipeline (after motion search and sub-pel refinement); see pipeline.py.

  InterRecon  - fused prediction + residual coding round trip (x265hip_inter_recon; reference callers
                predict.cpp:245-265, quant.cpp:397-480,543-605, search.cpp:357-375)
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import hipabi
from .pipeline import PUS_PER_CTU, DevicePicture


def _sum64(t):
    """A checksum word: the sum of a tensor's elements in int64."""
    import torch
    return int(t.to(torch.int64).sum().item())


ReconParams = hipabi.ReconParams          # x265hip_recon_params: the record lives beside ReconRefsParams, which embeds it


def _tu_part(stage, ctu_row0, ctu_rows):
    import copy
    o = copy.copy(stage)
    cw = stage.w64 // 64
    c0, o.nctu, o.h64 = cw * ctu_row0, cw * ctu_rows, ctu_rows * 64
    nb, nn = stage.nblk, stage.n * stage.n
    o.levels = stage.levels[c0 * nb * nn:(c0 + o.nctu) * nb * nn]
    o.num_sig = stage.num_sig[c0 * nb:(c0 + o.nctu) * nb]
    o.dist = stage.dist[c0 * nb:(c0 + o.nctu) * nb]
    if stage.qp_map is not None:          # the part's blocks are looked up from the part's first row: 8 rows of width / 8 cells per CTU row
        o.qp_map = stage.qp_map[ctu_row0 * 8 * (stage.w64 // 8):(ctu_row0 + ctu_rows) * 8 * (stage.w64 // 8)]
    return o


class InterRecon:
    """Stage 3: for every NxN block (N = 8 << level) predict with the refined mv, transform / quantise the
    residual, reconstruct, measure SSE.  Outputs: recon plane, levels, num_sig, dist."""

    def __init__(self, nctu, w64, h64, depth, level, qp, device, intra_slice=0):
        import torch
        self.nctu, self.w64, self.h64, self.depth, self.level, self.qp, self.intra = nctu, w64, h64, depth, level, qp, intra_slice
        self.n = 8 << level
        self.nblk = (64 // self.n) ** 2
        self.levels = torch.zeros(nctu * self.nblk * self.n * self.n, dtype=torch.int16, device=device)
        self.num_sig = torch.zeros(nctu * self.nblk, dtype=torch.int32, device=device)
        self.dist = torch.zeros(nctu * self.nblk, dtype=torch.int64, device=device)
        self.tables = None          # hipabi.tu_tables(...): scaling-list coefficients / denoiser tables of this block size, or None
        self.qp_map = None          # device int8 [h64 / 8 * w64 / 8]: the luma plane of CuQpMaps.tu_qp (per-block quantiser QP), or None = qp

    def part(self, ctu_row0, ctu_rows):
        """The stage for `ctu_rows` CTU rows from `ctu_row0` (outputs = the matching slices; see pipeline.MotionSearch.part)."""
        return _tu_part(self, ctu_row0, ctu_rows)

    def algorithmic_bytes(self, bpp=1):
        """per block: source N^2 + reference patch (N+7)^2 + recon N^2 pixels, levels 2*N^2, 16 B of results"""
        n = self.n
        return self.nctu * self.nblk * ((2 * n * n + (n + 7) * (n + 7)) * bpp + 2 * n * n + 16)

    def run(self, cur: DevicePicture, ref: DevicePicture, recon_plane, mv, stream=None):
        es = 1 if self.depth == 8 else 2
        p = ReconParams()
        p.depth, p.width, p.height, p.level, p.qp, p.intra_slice = self.depth, self.w64, self.h64, self.level, self.qp, self.intra
        p.fenc, p.fenc_stride = cur.t.data_ptr() + cur.org * es, cur.stride
        p.fref, p.fref_stride = ref.t.data_ptr() + ref.org * es, ref.stride
        p.recon, p.recon_stride = recon_plane.data_ptr() + cur.org * es, cur.stride
        p.mv, p.levels, p.num_sig, p.dist = mv.data_ptr(), self.levels.data_ptr(), self.num_sig.data_ptr(), self.dist.data_ptr()
        p.tables = ctypes.addressof(self.tables) if self.tables is not None else None
        p.qp_map = hipabi._p(self.qp_map)
        s = hipabi.current_stream() if stream is None else stream
        f = hipabi.lib().x265hip_inter_recon
        f.argtypes = [ctypes.POINTER(ReconParams), ctypes.c_void_p]
        hipabi.check(f(ctypes.byref(p), s), "x265hip_inter_recon")

    def checksum(self):
        return {"levels": _sum64(self.levels), "num_sig": int(self.num_sig.sum().item()), "dist": int(self.dist.sum().item())}


PredWeight = hipabi.PredWeight            # x265hip_pred_weight and x265hip_recon_bi_params: the records live beside ReconBiRefsParams, which embeds them
ReconBiParams = hipabi.ReconBiParams


class InterReconBi(InterRecon):
    """The inter TU stage for B pictures (x265hip_inter_recon_bi): per block list 0, list 1 or the average of both
    (predInterLumaShort + addAvg, predict.cpp:168-304)."""

    def run(self, cur: DevicePicture, ref0: DevicePicture, ref1: DevicePicture, recon_plane, mv0, mv1, dir_flags=None, stream=None, weights=None):
        """weights: (list 0, list 1), each None (the list has no weight table) or (present, weight, offset, log2_denom) - explicit
        weighted prediction (addWeightUni / addWeightBi); a P picture with weights is `dir` all 1 with ref1 = ref0."""
        es = 1 if self.depth == 8 else 2
        q = ReconBiParams()
        keep = []
        for name, w in zip(("weight0", "weight1"), weights or (None, None)):
            if w is not None:
                keep.append(PredWeight(*[int(v) for v in w]))
                setattr(q, name, ctypes.pointer(keep[-1]))
        p = q.base
        p.depth, p.width, p.height, p.level, p.qp, p.intra_slice = self.depth, self.w64, self.h64, self.level, self.qp, self.intra
        p.fenc, p.fenc_stride = cur.t.data_ptr() + cur.org * es, cur.stride
        p.fref, p.fref_stride = ref0.t.data_ptr() + ref0.org * es, ref0.stride
        p.recon, p.recon_stride = recon_plane.data_ptr() + cur.org * es, cur.stride
        p.mv, p.levels, p.num_sig, p.dist = mv0.data_ptr(), self.levels.data_ptr(), self.num_sig.data_ptr(), self.dist.data_ptr()
        p.tables = ctypes.addressof(self.tables) if self.tables is not None else None
        p.qp_map = hipabi._p(self.qp_map)
        q.fref1, q.mv1 = ref1.t.data_ptr() + ref1.org * es, mv1.data_ptr()
        q.dir = None if dir_flags is None else dir_flags.data_ptr()
        s = hipabi.current_stream() if stream is None else stream
        f = hipabi.lib().x265hip_inter_recon_bi
        f.argtypes = [ctypes.POINTER(ReconBiParams), ctypes.c_void_p]
        hipabi.check(f(ctypes.byref(q), s), "x265hip_inter_recon_bi")


class InterReconChroma:
    """The same stage for one chroma plane of a 4:2:0 picture (x265hip_inter_recon_chroma; reference predInterChromaPixel,
    predict.cpp:304-351, + the residual round trip on half-size blocks).  Planes are flat device tensors with `stride` samples per
    row and sample (0,0) at element `org`; `qp` is the plane's quantiser QP (chroma mapping / offsets applied by the caller)."""

    def __init__(self, nctu, w64, h64, depth, level, qp, device, intra_slice=0):
        import torch
        self.nctu, self.w64, self.h64, self.depth, self.level, self.qp, self.intra = nctu, w64, h64, depth, level, qp, intra_slice
        self.n = 4 << level
        self.nblk = (32 // self.n) ** 2
        self.levels = torch.zeros(nctu * self.nblk * self.n * self.n, dtype=torch.int16, device=device)
        self.num_sig = torch.zeros(nctu * self.nblk, dtype=torch.int32, device=device)
        self.dist = torch.zeros(nctu * self.nblk, dtype=torch.int64, device=device)
        self.tables = None
        self.qp_map = None          # device int8 [h64 / 8 * w64 / 8] over the LUMA grid: this plane's (Cb or Cr) part of CuQpMaps.tu_qp, or None = qp

    def part(self, ctu_row0, ctu_rows):
        return _tu_part(self, ctu_row0, ctu_rows)

    def params(self, fenc, fref, recon, stride, org, mv):
        es = 1 if self.depth == 8 else 2
        p = ReconParams()
        p.depth, p.width, p.height, p.level, p.qp, p.intra_slice = self.depth, self.w64, self.h64, self.level, self.qp, self.intra
        p.fenc, p.fenc_stride = fenc.data_ptr() + org * es, stride
        p.fref, p.fref_stride = fref.data_ptr() + org * es, stride
        p.recon, p.recon_stride = recon.data_ptr() + org * es, stride
        p.mv, p.levels, p.num_sig, p.dist = mv.data_ptr(), self.levels.data_ptr(), self.num_sig.data_ptr(), self.dist.data_ptr()
        p.tables = ctypes.addressof(self.tables) if self.tables is not None else None
        p.qp_map = hipabi._p(self.qp_map)
        return p

    def run(self, fenc, fref, recon, stride, org, mv, stream=None):
        p = self.params(fenc, fref, recon, stride, org, mv)
        s = hipabi.current_stream() if stream is None else stream
        f = hipabi.lib().x265hip_inter_recon_chroma
        f.argtypes = [ctypes.POINTER(ReconParams), ctypes.c_void_p]
        hipabi.check(f(ctypes.byref(p), s), "x265hip_inter_recon_chroma")

    @staticmethod
    def run_pair(stages, fencs, frefs, recons, stride, org, mv, stream=None):
        """Cb and Cr (stages = the two planes' InterReconChroma objects) in one launch: x265hip_inter_recon_chroma_pair."""
        ps = [st.params(fenc, fref, recon, stride, org, mv) for st, fenc, fref, recon in zip(stages, fencs, frefs, recons)]
        s = hipabi.current_stream() if stream is None else stream
        f = hipabi.lib().x265hip_inter_recon_chroma_pair
        f.argtypes = [ctypes.POINTER(ReconParams), ctypes.POINTER(ReconParams), ctypes.c_void_p]
        hipabi.check(f(ctypes.byref(ps[0]), ctypes.byref(ps[1]), s), "x265hip_inter_recon_chroma_pair")


class InterReconRefs(InterRecon):
    """The inter TU stage of a P picture with several references (x265hip_inter_recon_refs): block blk is predicted from
    refs[ref_idx[blk]]; everything else is InterRecon's contract.  No scaling-list / denoiser tables."""

    def run(self, cur: DevicePicture, refs, recon_plane, mv, ref_idx, stream=None):
        """refs: the reference pictures in list order (one geometry); ref_idx: int8 [ctu][blocks] (RefSelect.ref_idx)."""
        es = 1 if self.depth == 8 else 2
        assert all(r.stride == refs[0].stride and r.org == refs[0].org for r in refs)
        p = ReconParams()
        p.depth, p.width, p.height, p.level, p.qp, p.intra_slice = self.depth, self.w64, self.h64, self.level, self.qp, self.intra
        p.fenc, p.fenc_stride = cur.t.data_ptr() + cur.org * es, cur.stride
        p.fref, p.fref_stride = None, refs[0].stride
        p.recon, p.recon_stride = recon_plane.data_ptr() + cur.org * es, cur.stride
        p.mv, p.levels, p.num_sig, p.dist = mv.data_ptr(), self.levels.data_ptr(), self.num_sig.data_ptr(), self.dist.data_ptr()
        p.tables = ctypes.addressof(self.tables) if self.tables is not None else None          # refused by the entry
        p.qp_map = hipabi._p(self.qp_map)
        hipabi.inter_recon_refs(hipabi.recon_refs_params(p, [r.t.data_ptr() + r.org * es for r in refs], ref_idx), stream)


class InterReconChromaRefs(InterReconChroma):
    """One chroma plane of a P picture with several references (x265hip_inter_recon_chroma_refs), run_pair: Cb and Cr in one launch."""

    def params_refs(self, fenc, frefs, recon, stride, org, mv, ref_idx):
        es = 1 if self.depth == 8 else 2
        p = self.params(fenc, frefs[0], recon, stride, org, mv)
        p.fref = None
        return hipabi.recon_refs_params(p, [f.data_ptr() + org * es for f in frefs], ref_idx)

    def run(self, fenc, frefs, recon, stride, org, mv, ref_idx, stream=None):
        """frefs: this plane (Cb or Cr) of every reference picture, list order."""
        hipabi.inter_recon_chroma_refs(self.params_refs(fenc, frefs, recon, stride, org, mv, ref_idx), stream)

    @staticmethod
    def run_pair(stages, fencs, frefs, recons, stride, org, mv, ref_idx, stream=None):
        """stages = the two planes' objects; frefs = ([Cb of every reference], [Cr of every reference])."""
        qs = [st.params_refs(fenc, fr, recon, stride, org, mv, ref_idx) for st, fenc, fr, recon in zip(stages, fencs, frefs, recons)]
        hipabi.inter_recon_chroma_pair_refs(qs[0], qs[1], stream)


class InterReconChromaBi(InterReconChroma):
    """One chroma plane of a B picture (or of a P picture with explicit weights): x265hip_inter_recon_chroma_bi - per block list 0,
    list 1 or both, with the plane's own weights (Predict::motionCompensation's chroma half, predict.cpp:77-243, 304-409)."""

    def run(self, fenc, fref0, fref1, recon, stride, org, mv0, mv1, dir_flags=None, stream=None, weights=None):
        q = ReconBiParams()
        q.base = self.params(fenc, fref0, recon, stride, org, mv0)          # copied into the record
        es = 1 if self.depth == 8 else 2
        q.fref1, q.mv1 = fref1.data_ptr() + org * es, mv1.data_ptr()
        q.dir = None if dir_flags is None else dir_flags.data_ptr()
        keep = []
        for name, w in zip(("weight0", "weight1"), weights or (None, None)):
            if w is not None:
                keep.append(PredWeight(*[int(v) for v in w]))
                setattr(q, name, ctypes.pointer(keep[-1]))
        s = hipabi.current_stream() if stream is None else stream
        f = hipabi.lib().x265hip_inter_recon_chroma_bi
        f.argtypes = [ctypes.POINTER(ReconBiParams), ctypes.c_void_p]
        hipabi.check(f(ctypes.byref(q), s), "x265hip_inter_recon_chroma_bi")


class InterReconBiRefs(InterRecon):
    """The bi-predictive TU stage of a B picture with several references per list (x265hip_inter_recon_bi_refs): block blk takes list
    l's prediction from refs_l[ref_idx_l[blk]]; everything else is InterReconBi's contract.  No tables, no weights."""

    def run(self, cur: DevicePicture, refs0, refs1, recon_plane, mv0, mv1, ref_idx0, ref_idx1, dir_flags=None, stream=None):
        """refs0 / refs1: each list's reference pictures in list order (one geometry); ref_idx0 / ref_idx1: int8 [ctu][blocks] (the two
        RefSelect.ref_idx); mv0 / mv1, dir_flags: BidirDecideRefs' outputs."""
        es = 1 if self.depth == 8 else 2
        first = refs0[0]
        assert all(r.stride == first.stride and r.org == first.org for r in list(refs0) + list(refs1))
        q = ReconBiParams()
        p = q.base
        p.depth, p.width, p.height, p.level, p.qp, p.intra_slice = self.depth, self.w64, self.h64, self.level, self.qp, self.intra
        p.fenc, p.fenc_stride = cur.t.data_ptr() + cur.org * es, cur.stride
        p.fref, p.fref_stride = None, first.stride
        p.recon, p.recon_stride = recon_plane.data_ptr() + cur.org * es, cur.stride
        p.mv, p.levels, p.num_sig, p.dist = mv0.data_ptr(), self.levels.data_ptr(), self.num_sig.data_ptr(), self.dist.data_ptr()
        p.tables = ctypes.addressof(self.tables) if self.tables is not None else None          # refused by the entry
        p.qp_map = hipabi._p(self.qp_map)
        q.mv1 = mv1.data_ptr()
        q.dir = None if dir_flags is None else dir_flags.data_ptr()
        addr = lambda refs: [r.t.data_ptr() + r.org * es for r in refs]
        hipabi.inter_recon_bi_refs(hipabi.recon_bi_refs_params(q, addr(refs0), addr(refs1), ref_idx0, ref_idx1), stream)


class InterReconChromaBiRefs(InterReconChroma):
    """One chroma plane of a B picture with several references per list (x265hip_inter_recon_chroma_bi_refs)."""

    def run(self, fenc, frefs0, frefs1, recon, stride, org, mv0, mv1, ref_idx0, ref_idx1, dir_flags=None, stream=None):
        """frefs0 / frefs1: this plane (Cb or Cr) of every reference picture of each list, list order."""
        es = 1 if self.depth == 8 else 2
        q = ReconBiParams()
        q.base = self.params(fenc, frefs0[0], recon, stride, org, mv0)          # copied into the record
        q.base.fref = None
        q.mv1 = mv1.data_ptr()
        q.dir = None if dir_flags is None else dir_flags.data_ptr()
        addr = lambda frefs: [f.data_ptr() + org * es for f in frefs]
        hipabi.inter_recon_chroma_bi_refs(hipabi.recon_bi_refs_params(q, addr(frefs0), addr(frefs1), ref_idx0, ref_idx1), stream)


def extend_border_rows(plane, pic: DevicePicture, top: bool, bottom: bool, stream=None, chroma=False):
    """Row-wise border extension of the band `pic` is a view of (x265hip_extend_border_rows): left / right margins of the band's rows, the
    picture's top margin when the band is its first, the bottom margin when it is its last."""
    from . import frames as F
    es = 1 if pic.depth == 8 else 2
    s = hipabi.current_stream() if stream is None else stream
    f = hipabi.lib().x265hip_extend_border_rows
    f.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    if chroma:
        my = F.CHROMA_MARGIN_Y
        hipabi.check(f(plane.data_ptr() + pic.org_c * es, pic.stride_c, pic.w64 // 2, pic.h64 // 2, F.CHROMA_MARGIN_X, my if top else 0, my if bottom else 0,
                       pic.depth, s), "x265hip_extend_border_rows")
        return
    my = F.MARGIN_Y
    hipabi.check(f(plane.data_ptr() + pic.org * es, pic.stride, pic.w64, pic.h64, F.MARGIN_X, my if top else 0, my if bottom else 0, pic.depth, s),
                 "x265hip_extend_border_rows")


def extend_border(plane, pic: DevicePicture, stream=None, chroma=False):
    """Replicate the picture edges into the margins of `plane` (same geometry as `pic`; chroma: one of its 4:2:0 planes), on device."""
    from . import frames as F
    es = 1 if pic.depth == 8 else 2
    s = hipabi.current_stream() if stream is None else stream
    f = hipabi.lib().x265hip_extend_border
    f.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    if chroma:
        hipabi.check(f(plane.data_ptr() + pic.org_c * es, pic.stride_c, pic.w64 // 2, pic.h64 // 2, F.CHROMA_MARGIN_X, F.CHROMA_MARGIN_Y, pic.depth, s),
                     "x265hip_extend_border")
        return
    hipabi.check(f(plane.data_ptr() + pic.org * es, pic.stride, pic.w64, pic.h64, F.MARGIN_X, F.MARGIN_Y, pic.depth, s),
                 "x265hip_extend_border")


class BorderPlane(ctypes.Structure):
    _fields_ = [("pic", ctypes.c_void_p), ("stride", ctypes.c_ssize_t), ("width", ctypes.c_int), ("height", ctypes.c_int), ("margin_x", ctypes.c_int),
                ("margin_top", ctypes.c_int), ("margin_bottom", ctypes.c_int)]


def extend_border_picture(planes, pic: DevicePicture, stream=None, top=True, bottom=True):
    """extend_border of [Y, Cb, Cr] (or [Y]) of one picture as ONE launch (x265hip_extend_border_planes); `pic` a band view with top / bottom =
    whether it is the picture's first / last band: the row-wise form (extend_border_rows) of all planes at once."""
    from . import frames as F
    es = 1 if pic.depth == 8 else 2
    s = hipabi.current_stream() if stream is None else stream
    arr = (BorderPlane * len(planes))()
    arr[0] = BorderPlane(planes[0].data_ptr() + pic.org * es, pic.stride, pic.w64, pic.h64, F.MARGIN_X, F.MARGIN_Y if top else 0, F.MARGIN_Y if bottom else 0)
    for i in range(1, len(planes)):
        arr[i] = BorderPlane(planes[i].data_ptr() + pic.org_c * es, pic.stride_c, pic.w64 // 2, pic.h64 // 2, F.CHROMA_MARGIN_X,
                             F.CHROMA_MARGIN_Y if top else 0, F.CHROMA_MARGIN_Y if bottom else 0)
    f = hipabi.lib().x265hip_extend_border_planes
    f.argtypes = [ctypes.POINTER(BorderPlane), ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    hipabi.check(f(arr, len(planes), pic.depth, s), "x265hip_extend_border_planes")


SUBPEL_DEFER_DEFAULT = "after"       # FramePipeline._run_parallel2: where the PU levels the reconstruction does not read are refined

# g_chromaScale (constants.cpp:346-350) as Quant::setChromaQP applies it to 4:2:0 pictures (quant.cpp:233-244)
_CHROMA_SCALE = list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37] + list(range(38, 52)) + [51] * 12


def chroma_quant_qp(qp, depth, offset=0):
    """The chroma quantiser's QP for a CU whose luma quantiser runs at `qp` (= CU QP + QP_BD_OFFSET)."""
    bd = 6 * (depth - 8)
    q = min(max(qp - bd + offset, -bd), 57)
    if q >= 30:
        q = _CHROMA_SCALE[q]
    return q + bd


class CuQpMaps:
    """The step between the lookahead's QP offsets and the coding stages (x265hip_cu_qp_maps; reference Analysis::calculateQpforCuSize,
    analysis.cpp:3679-3713, + Quant::setQPforQuant / setChromaQP, quant.cpp:221-244): offsets -> host maps -> device tensors.  After
    run(): cu_qp int8 [h/8 * w/8] (the CUs' m_qp: what the deblocking entries take) and tu_qp int8 [3][h/8 * w/8] (the quantiser QPs of
    Y, Cb, Cr: what the TU stages take), on the device; cu_qp_host / tu_qp_host the numpy arrays they were uploaded from."""

    def __init__(self, w64, h64, depth, level, device, qg_size=16, qp_min=0, qp_max=51, cb_qp_offset=0, cr_qp_offset=0):
        import torch
        self.w64, self.h64, self.depth, self.level, self.qg_size = w64, h64, depth, level, qg_size
        self.qp_min, self.qp_max, self.cb_qp_offset, self.cr_qp_offset = qp_min, qp_max, cb_qp_offset, cr_qp_offset
        cells = (h64 // 8) * (w64 // 8)
        self.cu_qp = torch.zeros(cells, dtype=torch.int8, device=device)
        self.tu_qp = torch.zeros(3 * cells, dtype=torch.int8, device=device).view(3, cells)
        self.cu_qp_host = self.tu_qp_host = None

    def run(self, base_qp, qp_offsets=None):
        """base_qp: the picture's QP as rate control hands it to the CTUs (a double; CU QP domain, without QP_BD_OFFSET); qp_offsets: the
        picture's qpAqOffset or qpCuTreeOffset (AdaptiveQuant.qp_aq_offset / .qp_cutree_offset, a cuTree finish), or None."""
        import torch
        cu, tu = hipabi.cu_qp_maps(self.depth, self.w64, self.h64, self.level, self.qg_size, base_qp, qp_offsets, self.qp_min, self.qp_max,
                                   self.cb_qp_offset, self.cr_qp_offset)
        return self.load(cu, tu)

    def load(self, cu, tu):
        """Maps made elsewhere (numpy int8 [h/8, w/8] and [3, h/8, w/8], every 8x8 cell of a block holding the block's value)."""
        import torch
        self.cu_qp_host, self.tu_qp_host = np.ascontiguousarray(cu, dtype=np.int8), np.ascontiguousarray(tu, dtype=np.int8)
        self.cu_qp.copy_(torch.from_numpy(self.cu_qp_host.reshape(-1)))
        self.tu_qp.copy_(torch.from_numpy(self.tu_qp_host.reshape(3, -1)))
        return self


class Deblock:
    """In-loop deblocking of the luma reconstruction on device (x265hip_deblock_bs_inter + x265hip_deblock_luma; reference
    Deblock::getBoundaryStrength / edgeFilterLuma, deblock.cpp:191-215, 317-415) for the reconstruction stage's block grid."""

    def __init__(self, w64, h64, depth, level, qp, device):
        import torch
        self.w64, self.h64, self.depth, self.level, self.qp = w64, h64, depth, level, qp
        self.qp_map = None          # device int8 [h64 / 8 * w64 / 8]: CuQpMaps.cu_qp (the CUs' m_qp), or None = qp; the pipelines' chroma pass reads it too
        self.bs_ver = torch.zeros((h64 // 4) * (w64 // 8), dtype=torch.uint8, device=device)
        self.bs_hor = torch.zeros((h64 // 8) * (w64 // 4), dtype=torch.uint8, device=device)

    def _luma(self, plane, pic: DevicePicture):
        """The luma edge filter with the boundary strengths a run* method has just left."""
        hipabi.deblock_luma(self.depth, plane, pic.stride, pic.org, self.w64, self.h64, self.bs_ver, self.bs_hor, self.qp, qp_map=self.qp_map)

    def run(self, plane, pic: DevicePicture, mv, num_sig, intra=None):
        """intra: optional device uint8 [ctu][blocks] (IntraInInter.intra) - the edges of its non-zero blocks get Bs 2 (deblock.cpp:198-199)."""
        hipabi.deblock_bs_inter(self.w64, self.h64, self.level, mv, num_sig, self.bs_ver, self.bs_hor, intra=intra)
        self._luma(plane, pic)

    def run_b(self, plane, pic: DevicePicture, mv0, mv1, ref0, ref1, num_sig, intra=None):
        """A B picture: the boundary strengths compare (ref0, ref1) x (mv0, mv1) per block (deblock.cpp:217-247); ref0 / ref1 = int8 picture
        ids per block, -1 = list unused (what BidirDecide leaves).  intra: as in run() - Bs 2 on an intra block's edges comes before the B
        rules (deblock.cpp:198-199)."""
        hipabi.deblock_bs_inter(self.w64, self.h64, self.level, mv0, num_sig, self.bs_ver, self.bs_hor, slice_b=True, mv1=mv1, ref0=ref0, ref1=ref1,
                                intra=intra)
        self._luma(plane, pic)

    def run_refs(self, plane, pic: DevicePicture, mv, ref_id, num_sig):
        """A P picture with several references: two blocks predicted from different pictures get Bs 1 whatever their vectors
        (deblock.cpp:217-247 in a P slice); ref_id = int8 picture ids per block (what RefSelect leaves)."""
        hipabi.deblock_bs_inter(self.w64, self.h64, self.level, mv, num_sig, self.bs_ver, self.bs_hor, slice_b=False, ref0=ref_id)
        self._luma(plane, pic)

    def prepare_intra(self):
        """Allocates what run_intra passes beside num_sig (IFramePipeline calls it in its constructor, so that run() allocates nothing)."""
        import torch
        if getattr(self, "_intra_flags", None) is None:
            nctu = (self.w64 // 64) * (self.h64 // 64)
            self._intra_flags = torch.ones(nctu * (64 >> (2 * self.level)), dtype=torch.uint8, device=self.bs_ver.device)
            self._intra_mv = torch.zeros(nctu * PUS_PER_CTU * 2, dtype=torch.int32, device=self.bs_ver.device)

    def run_intra(self, plane, pic: DevicePicture, num_sig):
        """An I picture: every block is an intra CU, so every block edge gets Bs 2 (deblock.cpp:198-199) - all-ones intra flags; the
        vector records are not looked at on such edges (zeros are passed)."""
        self.prepare_intra()
        hipabi.deblock_bs_inter(self.w64, self.h64, self.level, self._intra_mv, num_sig, self.bs_ver, self.bs_hor, intra=self._intra_flags)
        self._luma(plane, pic)


class Sao:
    """Sample adaptive offset of the deblocked luma picture: the two pixel passes on device (x265hip_sao_stats /
    x265hip_sao_apply; reference SAO::calcSaoStatsCTU sao.cpp:735-917 and generateLumaOffsets / applyPixelOffsets :572-630,
    :274-570).  The parameter choice between them (rdoSaoUnitCu, entropy-coder bit counts) is host work: `stats()` fills
    count / offset_org [numCtu, 5, 32]; `apply(params)` takes int32 [numCtu, 7] = typeIdx, bandPos, offset[4], mergeLeft."""

    def __init__(self, width, height, depth, device, ctu=(64, 64), plane_offset=0):
        """width / height: the PLANE's size; ctu: the CTU's footprint in it (4:2:0 chroma: (32, 32) with plane_offset 2)."""
        import torch
        self.width, self.height, self.depth, self.ctu, self.plane_offset = width, height, depth, ctu, plane_offset
        self.nctu = ((width + ctu[0] - 1) // ctu[0]) * ((height + ctu[1] - 1) // ctu[1])
        self.count = torch.zeros(self.nctu * 160, dtype=torch.int32, device=device)
        self.offset_org = torch.zeros(self.nctu * 160, dtype=torch.int32, device=device)
        self.params = torch.zeros(self.nctu * 7, dtype=torch.int32, device=device)

    def stats(self, src, rec, rec_stride, rec_org, src_plane=None):
        """src: a DevicePicture (its luma plane) or, with src_plane, any plane of the same stride / origin as the reconstruction."""
        if src_plane is not None:
            hipabi.sao_stats(self.depth, src_plane, rec_stride, rec_org, rec, rec_stride, rec_org, self.width, self.height, self.count, self.offset_org,
                             ctu=self.ctu, plane_offset=self.plane_offset)
            return
        hipabi.sao_stats(self.depth, src.t, src.stride, src.org, rec, rec_stride, rec_org, self.width, self.height, self.count, self.offset_org,
                         ctu=self.ctu, plane_offset=self.plane_offset)

    def plane(self, src, src_stride, src_org, rec, rec_stride, rec_org, out=None):
        """This plane's record for hipabi.sao_planes (several planes, one launch per SAO step)."""
        return dict(src=src, src_stride=src_stride, src_org=src_org, rec=rec, rec_stride=rec_stride, rec_org=rec_org, out=out, width=self.width,
                    height=self.height, count=self.count, offset_org=self.offset_org, params=self.params, ctu=self.ctu, plane_offset=self.plane_offset)

    def decide(self):
        """saoStatsInitialOffset + the distortion-only type choice of x265hip_sao_decide -> self.params (stays on the device)."""
        hipabi.sao_decide(self.depth, self.count, self.offset_org, self.nctu, self.params)

    def apply(self, rec, rec_stride, rec_org, out, params=None):
        hipabi.sao_apply(self.depth, rec, rec_stride, rec_org, out, rec_stride, rec_org, self.width, self.height,
                         self.params if params is None else params, ctu=self.ctu)


class Lookahead:
    """Lookahead picture preparation + intra cost estimate on device (x265hip_lowres_init / x265hip_lowres_intra; reference
    Lowres::init lowres.cpp:294-306 and LookaheadTLD::lowresIntraEstimate slicetype.cpp:696-772).  Geometry follows
    Lowres::create (lowres.cpp:50-72): half resolution rounded up to whole 8x8 blocks, the full-resolution margins; the
    row stride is sized for the ROUNDED width so the right margin never runs into the next row (the reference sizes it
    from the unrounded width - a layout choice, not a result)."""

    def __init__(self, width, height, depth, device, intra_penalty=5):
        import torch
        from . import frames as F
        self.depth, self.penalty = depth, intra_penalty
        self.wcu, self.hcu = (width // 2 + 7) >> 3, (height // 2 + 7) >> 3
        self.width, self.lines = self.wcu * 8, self.hcu * 8
        self.mx, self.my = F.MARGIN_X, F.MARGIN_Y
        self.stride = (self.width + 2 * self.mx + 31) & ~31
        self.org = self.stride * self.my + self.mx
        dt = torch.uint8 if depth == 8 else torch.int16
        self.planes = [torch.zeros(self.stride * (self.lines + 2 * self.my), dtype=dt, device=device) for _ in range(4)]
        n = self.wcu * self.hcu
        self.intra_cost = torch.zeros(n, dtype=torch.int32, device=device)
        self.intra_mode = torch.zeros(n, dtype=torch.uint8, device=device)
        self.lowres_costs = torch.zeros(n, dtype=torch.int16, device=device)

    def run(self, pic: DevicePicture):
        hipabi.lowres_init(self.depth, pic.t, pic.stride, pic.org, self.planes, self.stride, self.org,
                           self.width, self.lines, self.mx, self.my)
        hipabi.lowres_intra(self.depth, self.planes[0], self.stride, self.org, self.wcu, self.hcu, self.penalty,
                            self.intra_cost, self.intra_mode, self.lowres_costs)

    def checksum(self):
        import torch
        return {"intra_cost": int(self.intra_cost.sum(dtype=torch.int64).item()), "intra_mode": int(self.intra_mode.sum(dtype=torch.int64).item())}


class AdaptiveQuant:
    """The adaptive-quantisation pass of the lookahead - LookaheadTLD::calcAdaptiveQuantFrame (slicetype.cpp:439-694; AQ modes 0-3,
    no hevcAq / edge mode / HDR10 / per-block quant offsets).  The pixel work (every block's AC energy through the var primitive, the
    picture's wp_sum / wp_ssd totals) is one device launch (x265hip_aq_energy); the QP offsets are the reference's double-precision
    expressions, evaluated by the library's host-side x265hip_aq_offsets through the C library's pow / log2 like the reference."""

    def __init__(self, width, height, depth, device, qg_size=16, aq_mode=2, aq_strength=1.0, weightp=True):
        import torch
        self.width, self.height, self.depth, self.qg = width, height, depth, qg_size
        self.mode, self.strength, self.weightp = aq_mode, float(aq_strength), bool(weightp)
        self.bw, self.bh = (width + qg_size - 1) // qg_size, (height + qg_size - 1) // qg_size
        self.energy = torch.zeros(self.bw * self.bh, dtype=torch.int32, device=device)
        self.wp = torch.zeros(6, dtype=torch.int64, device=device)

    def run(self, y: DevicePicture, cb=None, cr=None, stride_c=0, org_c=0):
        """y: the source luma picture; cb / cr: device chroma planes (4:2:0) or None.  Returns (qp_aq_offset float64 [blocks],
        inv_qscale int32 [blocks], wp_sum [3], wp_ssd [3]) as Lowres holds them afterwards."""
        import numpy as np
        hipabi.aq_energy(self.depth, y.t, y.stride, y.org, self.width, self.height, self.qg, self.energy, self.wp, cb, cr, stride_c, org_c)
        energy = self.energy.cpu().numpy().view(np.uint32)
        wp = self.wp.cpu().numpy().view(np.uint64)
        qp, inv = hipabi.aq_offsets(self.depth, self.qg, self.mode, self.strength, energy, hipabi.aq_average_blocks(self.width, self.height, self.qg))
        wp_sum = [int(v) for v in wp[:3]]
        wp_ssd = [int(v) for v in wp[3:]]
        if self.weightp:                                             # the final normalisation, slicetype.cpp:662-675
            col, row = ((self.width + 8) >> 4) << 4, ((self.height + 8) >> 4) << 4
            dims = [col * row, (col >> 1) * (row >> 1), (col >> 1) * (row >> 1)]
            m64 = 0xffffffffffffffff                                 # `sum * sum` wraps in uint64_t in the reference (bright 4K 10/12-bit)
            wp_ssd = [(wp_ssd[i] - ((wp_sum[i] * wp_sum[i] + dims[i] // 2) & m64) // dims[i]) & m64 for i in range(3)]
        return qp, inv, wp_sum, wp_ssd


class HevcAq:
    """--hevc-aq: the pass calcAdaptiveQuantFrame runs instead of the AQ modes - LookaheadTLD::xPreanalyze / xPreanalyzeQp
    (slicetype.cpp:293-441).  Per enabled layer (lowres.h:123-129, 64x64 CTUs) one launch produces the quadrant sums of every partition
    (x265hip_aq_hevc_quadrants); activities, the layer's average and the QP offsets are the reference's double-precision expressions in
    the library's host-side x265hip_aq_hevc_offsets; the wp_sum / wp_ssd statistics of the same loop come from x265hip_aq_energy."""
    LAYERS = {64: (1, 0, 1, 0), 32: (1, 1, 1, 0), 16: (1, 1, 1, 0), 8: (1, 1, 1, 1)}

    def __init__(self, width, height, depth, device, qg_size=16, qp_adaptation_range=1.0, weightp=True):
        import torch
        self.width, self.height, self.depth, self.qg, self.range = width, height, depth, qg_size, float(qp_adaptation_range)
        self.parts = [64 >> d for d in range(4) if self.LAYERS[qg_size][d]]
        self.sums = [torch.zeros(8 * ((width + p - 1) // p) * ((height + p - 1) // p), dtype=torch.int64, device=device) for p in self.parts]
        self.wp_pass = AdaptiveQuant(width, height, depth, device, qg_size=8 if qg_size == 8 else 16, aq_mode=0, weightp=weightp)

    def run(self, y: DevicePicture, cb=None, cr=None, stride_c=0, org_c=0):
        """Returns ({partition size: (activity, qp_offset, avg_activity)}, inv_qscale of the deepest layer, wp_sum [3], wp_ssd [3])."""
        import numpy as np
        for p, sm in zip(self.parts, self.sums):
            hipabi.aq_hevc_quadrants(self.depth, y.t, y.stride, y.org, self.width, self.height, p, sm)
        _, _, wp_sum, wp_ssd = self.wp_pass.run(y, cb, cr, stride_c, org_c)
        layers, inv = {}, None
        for p, sm in zip(self.parts, self.sums):
            act, qp, avg, inv = hipabi.aq_hevc_offsets(self.width, self.height, p, self.range, sm.cpu().numpy().view(np.uint64).reshape(-1, 4, 2))
            layers[p] = (act, qp, avg)
        return layers, inv, wp_sum, wp_ssd


class WeightAnalysis:
    """Weighted-reference analysis of a prepared picture against a prepared reference - LookaheadTLD::weightsAnalyse
    (slicetype.cpp:860-957).  The pixel work runs on the device (x265hip_lowres_weight_cost scores the unweighted reference and the
    offset candidate in ONE launch - the second candidate does not depend on the first score -, x265hip_lowres_weight_apply weights
    the four planes); the float guess in between is evaluated here in single precision, operation by operation as the reference
    writes it.  wp_ssd / wp_sum are the pictures' luma statistics (Lowres::wp_ssd[0] / wp_sum[0], left there by the reference's
    adaptive-quantisation pass)."""

    def __init__(self, la: Lookahead, device):
        import torch
        self.la, self.depth = la, la.depth
        self.cost = torch.zeros(4, dtype=torch.int32, device=device)
        self.weighted = [torch.zeros_like(p) for p in la.planes]          # the reference's wbuffer[0..3]

    @property
    def weighted_ref(self):
        """The weighted planes in the shape LookaheadCost takes a reference in: estimateFrameCost searches them instead of the
        reference's own planes once a weight is accepted (wfref0, slicetype.cpp:3222,3267; P pictures - the bi-directional
        candidates of B pictures keep the unweighted planes, :3328)."""
        from types import SimpleNamespace
        return SimpleNamespace(planes=self.weighted)

    def analyse(self, cur: Lookahead, ref: Lookahead, wp_ssd, wp_sum):
        """wp_ssd / wp_sum: (current, reference).  Returns (weight or None, minscore, origscore); with a weight, self.weighted holds
        the weighted reference planes (weightedRef.isWeighted)."""
        import numpy as np
        f32 = np.float32
        depth = self.depth
        guess = np.sqrt(f32(int(wp_ssd[0])) / f32(int(wp_ssd[1]))) if (wp_ssd[0] and wp_ssd[1]) else f32(1.0)
        npx = f32(cur.lines * cur.width)
        fenc_mean = f32(int(wp_sum[0])) / npx / f32(1 << (depth - 8))
        ref_mean = f32(int(wp_sum[1])) / npx / f32(1 << (depth - 8))
        if abs(ref_mean - fenc_mean) < f32(0.5) and abs(f32(1.0) - guess) < f32(1.0 / 128.0):
            return None, 0, 0
        # WeightParam::setFromWeightAndOffset(w, 0, 7, true), slice.h:304-316
        w, mindenom = int(guess * f32(128) + f32(0.5)), 7
        while mindenom > 0 and w > 127:
            mindenom -= 1
            w >>= 1
        minscale, minoff, found = min(w, 127), 0, False
        cur_scale = minscale
        cur_off = int(fenc_mean - ref_mean * f32(cur_scale) / f32(1 << mindenom) + f32(0.5))
        if cur_off < -128 or cur_off > 127:
            cur_off = max(-128, min(127, cur_off))
            cur_scale = int(f32(1 << mindenom) * (fenc_mean - f32(cur_off)) / ref_mean + f32(0.5))
            cur_scale = max(0, min(127, cur_scale))
        # origscore: wp.wtPresent is still 0 at :907 - the UNWEIGHTED cost; then the offset candidate (:925)
        hipabi.lowres_weight_cost(depth, cur.planes[0], ref.planes[0], cur.stride, cur.org, cur.width, cur.lines, cur.intra_cost,
                                  [None, (cur_scale, mindenom, cur_off)], self.cost)
        scores = self.cost[:2].cpu().numpy().view(np.uint32)
        origscore = minscore = int(scores[0])
        if not minscore:
            return None, minscore, origscore
        s = int(scores[1])
        if s < minscore:
            minscore, minscale, minoff, found = s, cur_scale, cur_off, True
        if mindenom > 0 and not (minscale & 1):
            idx = 32 if not minscale else (minscale & -minscale).bit_length() - 1        # CTZ
            shift = min(idx, mindenom)
            mindenom -= shift
            minscale >>= shift
        if (not found) or (minscale == 1 << mindenom and minoff == 0) or f32(minscore) / f32(origscore) > f32(0.998):
            return None, minscore, origscore
        weight = (minscale, mindenom, minoff)
        rows = cur.lines + 2 * cur.my
        hipabi.lowres_weight_apply(depth, ref.planes, self.weighted, cur.stride, rows, weight)
        return weight, minscore, origscore


class LookaheadCost:
    """The lookahead's frame cost estimate of a prepared picture against one (P) or two (B) prepared references
    (x265hip_lowres_cost; reference CostEstimateGroup::estimateFrameCost / estimateCUCost, slicetype.cpp:3115-3388).  `lam` is
    x265_lambda_tab[X265_LOOKAHEAD_QP] (1.0 for 8-bit, 16.0 for 10-bit); the mv cost table is built on the host like BitCost's
    (bitcost.cpp:51-55,103-118)."""

    def __init__(self, la: Lookahead, device, lam=None, bidir=False):
        import numpy as np
        import torch
        from . import frames as F
        self.depth, self.bidir = la.depth, bidir
        lam = (1.0 if la.depth == 8 else (16.0 if la.depth == 10 else 64.0)) if lam is None else lam
        cq, self.qoff = F.qpel_cost_table(16, lam=lam, qmax=4 * (max(la.width, la.lines) + 64))
        self.cost_q = torch.from_numpy(cq.view(np.int16)).to(device)
        n = la.wcu * la.hcu
        self.mvs = torch.zeros(n * 2, dtype=torch.int32, device=device)
        self.mv_costs = torch.zeros(n, dtype=torch.int32, device=device)
        self.mvs1 = torch.zeros(n * 2, dtype=torch.int32, device=device) if bidir else None
        self.mv_costs1 = torch.zeros(n, dtype=torch.int32, device=device) if bidir else None
        self.lowres_costs = torch.zeros(n, dtype=torch.int16, device=device)
        self.row_satds = torch.zeros(la.hcu, dtype=torch.int32, device=device)
        self.frame = torch.zeros(4, dtype=torch.int64, device=device)

    def pair(self, cur: Lookahead, ref: Lookahead, ref1: Lookahead = None, do_search=(1, 1), ref_bi: Lookahead = None):
        """ref_bi: --weightp on a B picture - `ref` then carries the weighted list-0 planes (WeightAnalysis.weighted_ref) and ref_bi the
        reference's own planes, which the bi-directional candidates keep (slicetype.cpp:3328)."""
        return hipabi.lowres_cost_pair(self.depth, cur.org, cur.planes[0], ref.planes, cur.intra_cost, self.mvs, self.mv_costs,
                                       self.lowres_costs, self.row_satds, self.frame,
                                       ref1_planes=None if ref1 is None else ref1.planes, mvs1=self.mvs1, mv_costs1=self.mv_costs1,
                                       do_search=do_search, ref_bi_planes=None if ref_bi is None else ref_bi.planes)

    def run(self, cur: Lookahead, ref: Lookahead, ref1: Lookahead = None, do_search=(1, 1), bframe_bias=0, stream=None, ref_bi: Lookahead = None):
        hipabi.lowres_cost(self.depth, cur.stride, cur.wcu, cur.hcu, self.cost_q, self.qoff, [self.pair(cur, ref, ref1, do_search, ref_bi)],
                           bframe_bias=bframe_bias, stream=stream)

    @staticmethod
    def run_batch(stages, curs, refs, refs1=None, bframe_bias=0, stream=None, device_table=None):
        """One launch for many independent pictures of one geometry and kind (one workgroup each).  device_table: a table made by
        `table()` for exactly these operands - the launch then involves no host-to-device copy."""
        s0, c0 = stages[0], curs[0]
        refs1 = [None] * len(stages) if refs1 is None else refs1
        pairs = None if device_table is not None else [s.pair(c, r, r1) for s, c, r, r1 in zip(stages, curs, refs, refs1)]
        hipabi.lowres_cost(s0.depth, c0.stride, c0.wcu, c0.hcu, s0.cost_q, s0.qoff, pairs, bframe_bias=bframe_bias, stream=stream,
                           device_table=device_table)

    @staticmethod
    def table(stages, curs, refs, device, refs1=None, stream=None):
        refs1 = [None] * len(stages) if refs1 is None else refs1
        return hipabi.lowres_cost_table([s.pair(c, r, r1) for s, c, r, r1 in zip(stages, curs, refs, refs1)], device, stream=stream)


class PatternSearch:
    """Motion search drivers for every 8x8..64x64 PU of every CTU (x265hip_me_search; reference
    MotionEstimate::motionEstimate, motion.cpp:739-1561) with predictor (0,0): integer pattern + sub-pel refinement in
    one launch.  Output has SubpelRefine's layout: int32 [ctu*85][2] = {cost, qmvx | qmvy << 16}."""

    def __init__(self, w64, h64, depth, method, subme, merange, device, lam=4.0):
        import numpy as np
        import torch
        from . import frames as F
        self.depth, self.method, self.subme, self.merange = depth, method, subme, merange
        jobs = []
        for cy in range(0, h64, 64):
            for cx in range(0, w64, 64):
                for n in (8, 16, 32, 64):
                    npu = (64 // n) ** 2
                    for z in range(npu):
                        bx = (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4)
                        by = ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)
                        jobs.append((cx + bx * n, cy + by * n, n, n, 0, 0, 0, 0, 0))
        self.njobs = len(jobs)
        arr = np.array(jobs, dtype=hipabi.me_search_job_dtype())
        self.jobs = torch.from_numpy(arr.view(np.int32).reshape(-1, 9).copy()).to(device)
        cq, self.qoff = F.qpel_cost_table(merange, lam, qmax=8 * (merange + 8) + 64)
        self.cost_q = torch.from_numpy(cq.view(np.int16)).to(device)
        self.out = torch.zeros(self.njobs * 2, dtype=torch.int32, device=device)
        self.w64, self.h64, self.planes = w64, h64, None

    def run(self, cur: DevicePicture, ref: DevicePicture):
        from . import frames as F
        r = self.merange
        integral = None
        if self.method == hipabi.ME_SEA:
            # the reference picture's block-sum planes, rebuilt per reference like FrameFilter does after reconstruction
            integral = hipabi.sea_integral(self.depth, ref.t, ref.stride, ref.org, self.w64, self.h64, F.MARGIN_X, F.MARGIN_Y, planes=self.planes)
            self.planes = integral[0]
        hipabi.me_search(self.depth, cur.t, cur.stride, cur.org, ref.t, ref.stride, ref.org, self.method, self.subme, r,
                         self.cost_q, self.qoff, (-r, -r), (r, r), self.jobs, self.njobs, integral=integral)
        o = self.out.view(-1, 2)
        o[:, 0] = self.jobs[:, 8]
        o[:, 1] = (self.jobs[:, 6] & 0xffff) | (self.jobs[:, 7] << 16)

    def checksum(self):
        import torch
        return {"subpel": int(self.out.to(dtype=torch.int64).sum().item())}


class _PictureStep:
    """What the whole-picture steps (FramePipeline, BFramePipeline, MultiRefFramePipeline, IFramePipeline) share: the picture's geometry,
    the loop-filter stages, the planes they work on and everything behind the luma deblocking - chroma deblocking, SAO (statistics,
    x265hip_sao_rdo or the distortion-only stand-in, application), border extension."""

    fuse_sao = False            # FramePipeline: the stand-in SAO of Y, Cb, Cr as ONE launch per step (X265HIP_FUSE_SAO)
    band_border = None          # FramePipeline as a band of a picture: (is_first_band, is_last_band) -> row-wise border extension
    border_switch = None        # FramePipeline: the environment switch whose "0" means one border launch per plane instead of one per picture

    def __init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo):
        import torch
        self.w64, self.h64, self.nctu, self.depth, self.qp, self.chroma = w64, h64, (w64 // 64) * (h64 // 64), depth, qp, chroma
        # `qp` is the quantiser's QP (qp + QP_BD_OFFSET, what transformNxN works with); the deblocking tables are indexed with the
        # CU's own QP (m_qp, 0..51)
        self.db = Deblock(w64, h64, depth, level, max(qp - 6 * (depth - 8), 0), device) if deblock else None
        # SAO statistics of the deblocked reconstruction (what rdoSaoUnitCu reads), 4:2:0 chroma on 32x32 footprints
        self.sao = Sao(w64, h64, depth, device) if sao else None
        self.sao_c = [Sao(w64 // 2, h64 // 2, depth, device, ctu=(32, 32), plane_offset=2) for _ in range(2)] if (sao and chroma) else None
        # SAO applied in the loop: the picture handed on is deblocked AND offset like a decoder's.  sao_rdo: dict(lambdas=(luma, chroma),
        # ctx_merge, ctx_type, entropy_bits) - the parameters come from x265hip_sao_rdo, the reference's own rate-distortion decision
        # (SAO::rdoSaoUnitCu) on all planes' statistics; None - from x265hip_sao_decide (initial offsets + distortion-only choice)
        self.sao_apply = bool(sao and sao_apply)
        self.sao_rdo = sao_rdo if (sao and sao_apply) else None
        if self.sao_rdo is not None:
            self.sao_scratch = torch.zeros(hipabi.sao_rdo_scratch_bytes(w64 // 64, h64 // 64), dtype=torch.uint8, device=device)
            self.sao_no = torch.zeros(2, dtype=torch.int32, device=device)
        self.recon, self.recon_c, self.out, self.out_c = None, None, None, None          # _alloc_planes, or whoever owns the step
        self.qp_maps = None

    def _alloc_planes(self, cur):
        """The reconstruction and, where SAO is applied, the planes it is applied into: on first use, with cur's geometry."""
        import torch
        if self.recon is None:
            self.recon = torch.zeros_like(cur.t)
        if self.chroma and self.recon_c is None:
            self.recon_c = [torch.zeros_like(p) for p in cur.c]
        if self.sao_apply and self.out is None:
            self.out = torch.zeros_like(cur.t)
            self.out_c = [torch.zeros_like(p) for p in cur.c] if self.chroma else None

    def _set_qp_maps(self, maps, tu_luma, tu_chroma):
        """The maps' planes go to the TU stages (tu_qp) and to the deblocking stage (cu_qp), which the luma and chroma deblocking calls
        both read.  maps: a CuQpMaps of the step's geometry, depth and level, or None."""
        if maps is not None:
            geo = (self.w64, self.h64, self.depth, tu_luma.level)
            if (maps.w64, maps.h64, maps.depth, maps.level) != geo:
                raise ValueError(f"set_qp_maps: maps of (w, h, depth, level) = {(maps.w64, maps.h64, maps.depth, maps.level)} for a pipeline of {geo}")
        self.qp_maps = maps
        tu_luma.qp_map = None if maps is None else maps.tu_qp[0]
        for i, st in enumerate(tu_chroma):
            st.qp_map = None if maps is None else maps.tu_qp[1 + i]
        if self.db is not None:
            self.db.qp_map = None if maps is None else maps.cu_qp

    def set_qp_maps(self, maps):
        """Per-block QPs (adaptive quantisation) for the following run() calls: maps = a CuQpMaps of this geometry, depth and level, or None
        = the picture-wide qp again.  Not for bands (BandedFramePipeline), captured graphs or scaling-list tables: run() raises there."""
        self._set_qp_maps(maps, self.rc, self.rc_c if self.chroma else [])

    def _set_decision_qp_maps(self, maps, lambda8_by_qp, luma, planes3):
        """set_qp_maps of a step with decision stages: the maps reach the TU stages and the deblocking stage as above, the stages of `luma`
        (they price a block by its luma QP) get maps.tu_qp[0], those of `planes3` (the intra walks, which also code) all of maps.tu_qp, and
        both get lambda8_by_qp: device int32 tensor [52 + 6 (depth - 8)] - 256 x lambda of a CU per luma quantiser QP, for the rate term
        of every candidate - or None = the constructor's lambda8 for every block."""
        self._set_qp_maps(maps, self.rc, self.rc_c if self.chroma else [])
        for st in luma:
            st.qp_map = None if maps is None else maps.tu_qp[0]
        for st in planes3:
            st.qp_map = None if maps is None else maps.tu_qp
        for st in list(luma) + list(planes3):
            st.lambda8_by_qp = None if maps is None else lambda8_by_qp

    def _temporal_mvp_run_check(self, col, what, deltas):
        """run() of a merge step: a field or POC distances (`what` names the argument) without temporal_mvp, or temporal_mvp without them."""
        name = type(self).__name__
        if not self.temporal_mvp and (col is not None or deltas is not None):
            raise ValueError(f"{name}.run: col / {what} need temporal_mvp=True")
        if self.temporal_mvp and deltas is None:
            raise ValueError(f"{name}.run: temporal_mvp needs {what}")

    def _qp_maps_run_check(self):
        """run() with maps set, in a mode that would not honour them: raise instead of coding with other QPs than asked for."""
        if self.qp_maps is None:
            return
        import torch
        name = type(self).__name__
        if self.band_border is not None:
            raise ValueError(f"{name}: QP maps are set, but a band of a picture does not take its rows of them")
        if torch.cuda.is_current_stream_capturing():
            raise ValueError(f"{name}: QP maps are set, but a captured step would go on replaying the maps it was captured with")

    def _deblock_chroma(self, cur):
        """Both chroma planes with the boundary strengths of the luma pass (in an all-inter picture no edge has Bs 2: the pass still runs
        like the reference's)."""
        hipabi.deblock_chroma(self.depth, self.recon_c[0], self.recon_c[1], cur.stride_c, cur.org_c, cur.w64, cur.h64,
                              self.db.bs_ver, self.db.bs_hor, self.db.qp, qp_map=self.db.qp_map)

    def _sao_planes(self, cur):
        """The planes' records for hipabi.sao_planes / sao_apply_planes: [Y, Cb, Cr] or [Y]."""
        return [self.sao.plane(cur.t, cur.stride, cur.org, self.recon, cur.stride, cur.org, self.out)] + \
               ([self.sao_c[i].plane(cur.c[i], cur.stride_c, cur.org_c, self.recon_c[i], cur.stride_c, cur.org_c, self.out_c[i]) for i in range(2)] if self.chroma else [])

    def _sao_rdo(self):
        """x265hip_sao_rdo on the statistics of all planes -> every plane's Sao.params."""
        st = [self.sao] + (list(self.sao_c) if self.chroma else [])
        q = self.sao_rdo
        hipabi.sao_rdo(self.depth, [x.count for x in st], [x.offset_org for x in st], self.w64 // 64, self.h64 // 64, q["lambdas"], q["ctx_merge"], q["ctx_type"],
                       q["entropy_bits"], [x.params for x in st], self.sao_scratch, sao_flag=(1, 1 if self.chroma else 0), num_no_sao=self.sao_no)

    def _extend_border(self, plane, cur, chroma=False):
        """One plane: the whole picture's margins, or a band's (side margins, top / bottom margin only at the picture's edge)."""
        if self.band_border is not None:
            extend_border_rows(plane, cur, self.band_border[0], self.band_border[1], chroma=chroma)
        else:
            extend_border(plane, cur, chroma=chroma)

    def _extend_borders(self, cur, planes):
        """planes = [Y, Cb, Cr] or [Y] in one launch, or plane by plane where the step's switch asks for it."""
        if self.border_switch is None or os.environ.get(self.border_switch, "1") != "0":
            top, bottom = self.band_border or (True, True)
            extend_border_picture(planes, cur, top=top, bottom=bottom)
        else:
            for i, plane in enumerate(planes):
                self._extend_border(plane, cur, chroma=i > 0)

    def _filter_tail(self, cur, mark):
        """Everything behind the luma deblocking, serially on the caller's stream; sets final / final_c and returns final."""
        if self.db is not None:
            if self.chroma:
                self._deblock_chroma(cur)
            mark("deblock")
        final, final_c = (self.out, self.out_c) if self.sao_apply else (self.recon, self.recon_c)
        if self.sao_rdo is not None:
            # statistics of all planes (one launch) -> the reference's rate-distortion decision (x265hip_sao_rdo: it needs every plane's
            # statistics, Cb / Cr share a type) -> application of all planes (one launch)
            planes = self._sao_planes(cur)
            hipabi.sao_planes(self.depth, [dict(q, out=None) for q in planes])
            mark("sao_stats")
            self._sao_rdo()
            mark("sao_rdo")
            hipabi.sao_apply_planes(self.depth, planes)
            mark("sao_apply")
        elif self.sao_apply and self.chroma and self.fuse_sao:
            hipabi.sao_planes(self.depth, self._sao_planes(cur))
            mark("sao")                      # statistics + parameters + application of the three planes: three launches
        elif self.sao is not None:
            self.sao.stats(cur, self.recon, cur.stride, cur.org)
            if self.chroma:
                for i in range(2):
                    self.sao_c[i].stats(None, self.recon_c[i], cur.stride_c, cur.org_c, src_plane=cur.c[i])
            mark("sao_stats")
            if self.sao_apply:
                self.sao.decide()
                self.sao.apply(self.recon, cur.stride, cur.org, self.out)
                if self.chroma:
                    for i in range(2):
                        self.sao_c[i].decide()
                        self.sao_c[i].apply(self.recon_c[i], cur.stride_c, cur.org_c, self.out_c[i])
                mark("sao_apply")
        self._extend_borders(cur, [final] + (list(final_c) if self.chroma else []))
        mark("border")
        self.final, self.final_c = final, final_c
        return final

    def final_planes(self):
        """[Y, Cb, Cr] (or [Y]) of the picture the last run() produced."""
        return [self.final] + (list(self.final_c) if self.chroma else [])


class _RefListStep(_PictureStep):
    """The part BFramePipeline and MultiRefFramePipeline share: one exhaustive search + sub-pel refinement per reference picture."""

    def _build_lists(self, n, w64, h64, depth, device, rng, subme, subpel_planes, chroma_satd):
        from .pipeline import MotionSearch, SubpelRefine
        self.msl = [MotionSearch(w64, h64, rng, depth, device, want_surf=False, want_best=True) for _ in range(n)]
        self.spl = [SubpelRefine(m, subme, device, phase_planes=subpel_planes, chroma_satd=chroma_satd) for m in self.msl]

    def _search_lists(self, cur, refs, mark):
        for l, ref in enumerate(refs):
            self.msl[l].reset()
            self.msl[l].search(cur, ref)
            mark("me%d" % l)
            self.spl[l].run(cur, ref)
            mark("subpel%d" % l)

    def _checksum(self, choice):
        """choice: the stage that chose between the lists (BidirDecide / RefSelect)."""
        out = {}
        for l in range(len(self.msl)):
            out.update({"%s%d" % (k, l): v for k, v in self.msl[l].checksum().items()})
            out.update({"%s%d" % (k, l): v for k, v in self.spl[l].checksum().items()})
        out.update(choice.checksum())
        out.update(self.rc.checksum())
        if self.chroma:
            for i in range(2):
                out.update({"%s_c%d" % (k, i): v for k, v in InterRecon.checksum(self.rc_c[i]).items()})
        out["recon"] = _sum64(self.final)
        return out


class FramePipeline(_PictureStep):
    """Closed-loop frame pipeline: every frame is searched in, predicted from and reconstructed against the
    RECONSTRUCTION of the previous frame (like the reference's P-frame chain), all on device:
        ME (exhaustive, SAD surfaces and/or best mv) -> sub-pel refinement -> prediction + residual round trip
        (NxN blocks) -> border extension -> the reconstruction becomes the next reference.
    With lookahead=(width, height) the source picture also goes through the lookahead stage (half-resolution planes + intra
    cost estimate per 8x8 block), which only depends on the source."""

    border_switch = "X265HIP_BORDER_PLANES"          # 0 (A/B runs): the picture's (band's) planes in three border launches instead of one

    def __init__(self, w64, h64, depth, device, rng=57, subme=2, level=2, qp=27, want_surf=True, packed=False, lookahead=None,
                 search="full", deblock=False, sao=False, lookahead_cost_batch=0, chroma=False, sao_apply=False, sign_hide=False,
                 subpel_planes=False, parallel_planes=False, split=1, sao_rdo=None, chroma_satd=False):
        """chroma_satd (with chroma): the sub-pel refinement adds the SATD of Cb and Cr to every comparison, as the reference does at
        subme >= 3 (x265hip_subpel_refine_chroma); every run mode honours it.  Exhaustive search only: x265hip_me_search is luma only.
        split (with parallel_planes): the picture goes through search -> sub-pel refinement -> reconstruction in `split` parts of whole
        CTU rows; while the search of part k + 1 runs on the caller's stream, part k is refined and reconstructed on a side stream.  No
        CTU's result depends on another CTU before the loop filters, which still run on the whole picture: same outputs, and only the last
        part's refinement + reconstruction stay behind the search on the critical path.  Measured at 4K 8-bit (profiles/r02_split.txt):
        2.94 ms per picture with 2 parts against 2.29 ms in one piece - the record-per-lane search kernel wants every CU's LDS and both of
        its workgroup slots, and workgroups of other kernels resident next to it cost it more than the overlap hides.  Off by default."""
        import torch
        from .pipeline import MotionSearch, SubpelRefine
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        # parallel_planes: after the sub-pel stage the three planes are independent chains (reconstruction -> deblocking -> SAO ->
        # border) of small, latency-bound launches: Cb and Cr run on their own HIP streams next to Y, the lookahead (source picture
        # only) next to the search; everything joins the caller's stream before run() returns
        self.parallel = bool(parallel_planes)
        self.pstreams = None
        self._spare_ready = None
        self.schedule2 = os.environ.get("X265HIP_PAR_SCHEDULE", "2") != "1"          # 1: the round-2 schedule (A/B runs)
        self.split = max(1, min(int(split), h64 // 64))
        self.parts = None
        # the three planes' SAO passes as one launch per step: on by default where every launch is on one stream (0.144 vs 0.187 ms at 4K);
        # with the planes' chains on side streams the per-plane passes already overlap and fusing them costs 0.07 ms ("2" forces it there too)
        self.fuse_sao = os.environ.get("X265HIP_FUSE_SAO", "1") != "0"
        self.fuse_sao_parallel = os.environ.get("X265HIP_FUSE_SAO", "1") == "2"
        # experiment switches of the parallel-planes launch structure (read once): where the lookahead and the phase planes run
        self.la_after_search = os.environ.get("X265HIP_LA_AFTER_ME", "1") == "1"
        self.prep_next_to_search = os.environ.get("X265HIP_PREP_OVERLAP", "0") == "1"
        # the default parallel schedule refines only the PU level the reconstruction codes in front of it and the other three levels on the
        # side stream, next to the SAO decision (x265hip_subpel_refine_levels).  0: one launch of all four levels (A/B runs);
        # "before" / "after" / "mv": where the three levels go - in front of the lookahead, behind it, or on a stream of their own right
        # behind the first launch (1 = the default placement)
        defer = os.environ.get("X265HIP_SUBPEL_DEFER", "1")
        if defer not in ("0", "1", "before", "after", "mv"):
            raise ValueError(f"X265HIP_SUBPEL_DEFER={defer}: 0, 1, before, after or mv")
        self.subpel_defer = {"0": None, "1": SUBPEL_DEFER_DEFAULT}.get(defer, defer)
        self.ms = MotionSearch(w64, h64, rng, depth, device, want_surf=want_surf and search == "full", want_best=True, packed=packed)
        # subpel_planes: sub-pel candidates read from the reference picture's phase planes (one x265hip_phase_planes launch per frame)
        if chroma_satd and search != "full":
            raise ValueError("FramePipeline: chroma_satd needs search='full' (the pattern-search step is luma only)")
        if chroma_satd and not chroma:
            raise ValueError("FramePipeline: chroma_satd needs chroma=True")
        self.sp = SubpelRefine(self.ms, subme, device, phase_planes=subpel_planes, chroma_satd=chroma_satd)
        # search != "full": the pattern-search drivers replace the exhaustive search + sub-pel pair
        self.ps = None
        if search != "full":
            method = {"dia": hipabi.ME_DIA, "hex": hipabi.ME_HEX, "umh": hipabi.ME_UMH, "star": hipabi.ME_STAR, "sea": hipabi.ME_SEA}[search]
            self.ps = PatternSearch(w64, h64, depth, method, subme, rng, device)
        # sign_hide: Quant::signBitHidingHDQ after the quantiser (pps.bSignHideEnabled, the x265 default)
        self.tu_flags = hipabi.TU_SIGN_HIDE if sign_hide else 0
        self.rc = InterRecon(self.nctu, w64, h64, depth, level, qp, device, intra_slice=self.tu_flags)
        self.la = Lookahead(lookahead[0], lookahead[1], depth, device) if lookahead else None
        # The lookahead's P-frame cost estimate runs AHEAD of the encode like the reference's lookahead thread: every
        # `lookahead_cost_batch` frames one launch on a side stream scores that many (picture, previous picture) pairs.  The
        # prepared pictures live in a ring so that a slot is only rewritten after the launches that read it.
        self.lcb = lookahead_cost_batch if lookahead else 0
        if self.lcb:
            self.ring = [self.la] + [Lookahead(lookahead[0], lookahead[1], depth, device) for _ in range(2 * self.lcb)]
            self.lc = [LookaheadCost(self.la, device) for _ in range(self.lcb)]
            self.side = torch.cuda.Stream(device=device)
            self.frame_no, self.pending, self.read_done = 0, [], {}
            # the operand tables of the launches repeat with the ring: upload each once, up front for the full batches
            self.device, self.tables = device, {}
            nring = len(self.ring)
            for j in range(nring):
                self._table(tuple(((j * self.lcb + 1 + i) % nring, (j * self.lcb + i) % nring) for i in range(self.lcb)))
            torch.cuda.synchronize()
        # 4:2:0 chroma through the same closed loop (predInterChromaPixel + residual round trip, edgeFilterChroma)
        if chroma:
            qpc = chroma_quant_qp(qp, depth)
            self.rc_c = [InterReconChroma(self.nctu, w64, h64, depth, level, qpc, device, intra_slice=self.tu_flags) for _ in range(2)]

    def set_qp_maps(self, maps):
        """Per-block QPs (adaptive quantisation) for the following run() calls: maps = a CuQpMaps of this geometry, depth and level, or None
        = the picture-wide qp again.  Every run mode reads the maps from the stages; the parts of `split` are rebuilt with their rows of
        the maps.  Not for bands (BandedFramePipeline), captured graphs or scaling-list tables: run() raises there."""
        _PictureStep.set_qp_maps(self, maps)
        self.parts = None

    def run(self, cur: DevicePicture, ref: DevicePicture, mark=None):
        """ref: the current reference picture (extended borders; with chroma=True also its Cb / Cr planes); returns the luma plane of
        the picture for the next frame's reference list (final_planes() has all three).  mark(name), if given, is called after every
        stage (bench.py records an event there)."""
        import torch
        self._qp_maps_run_check()
        self._alloc_planes(cur)
        par = self.parallel and mark is None and self.chroma and not self.lcb and self.ps is None and self.db is not None and self.sao is not None \
            and self.sao_apply
        if par:
            return self._run_parallel(cur, ref)
        mark = mark or (lambda name: None)
        if self.lcb:
            slot = self.frame_no % len(self.ring)
            if slot in self.read_done:                       # the cost launches that read this slot must be through
                torch.cuda.current_stream().wait_event(self.read_done.pop(slot))
            self.la = self.ring[slot]
            self.la.run(cur)
            if self.frame_no:
                self.pending.append((slot, (self.frame_no - 1) % len(self.ring)))
            self.frame_no += 1
            if len(self.pending) == self.lcb:
                self.launch_lookahead_costs()
        elif self.la is not None:
            self.la.run(cur)
        if self.ps is None:
            self.ms.reset()                                  # 4 us fill of best[]: kept out of the search kernel's interval
        mark("lookahead")
        if self.ps is not None:
            self.ps.run(cur, ref)
            mv = self.ps.out
            mark("me")
        else:
            self.ms.search(cur, ref)                         # ONE fused launch: SAD surfaces + best mv
            mark("me")
            self.sp.run(cur, ref)
            mv = self.sp.out
        mark("subpel")
        self.rc.run(cur, ref, self.recon, mv)
        mark("recon")
        if self.chroma:
            if self.rc_c[0].tables is None and self.rc_c[1].tables is None:
                InterReconChroma.run_pair(self.rc_c, cur.c, ref.c, self.recon_c, cur.stride_c, cur.org_c, mv)      # Cb + Cr: one launch
            else:
                for i in range(2):
                    self.rc_c[i].run(cur.c[i], ref.c[i], self.recon_c[i], cur.stride_c, cur.org_c, mv)
            mark("recon_chroma")
        if self.db is not None:
            self.db.run(self.recon, cur, mv, self.rc.num_sig)
        return self._filter_tail(cur, mark)

    def _run_parallel(self, cur: DevicePicture, ref: DevicePicture):
        """The same launches as run(), Y on the caller's stream, Cb / Cr on two side streams from the reconstruction on, the lookahead on
        a third; all joined before returning (stage outputs are identical: no stage shares an output buffer with another plane)."""
        import torch
        main = torch.cuda.current_stream()
        if self.pstreams is None:
            # (a higher HIP priority for the stream that carries the chroma chain - it ends after the luma chain - moved nothing: 2.189 ms
            # against 2.163 without, profiles/r03_step_timeline.txt)
            self.pstreams = [torch.cuda.Stream() for _ in range(4)]
        sCb, sCr, sLa = self.pstreams[:3]
        if self.sao_rdo is not None and self.split == 1 and self.la_after_search and self.schedule2 and self.band_border is None:
            return self._run_parallel2(cur, ref, main, sCb)
        start = torch.cuda.Event(); start.record(main)
        # The lookahead of the source picture only depends on the source, but it does not run next to the search: the record-per-lane search
        # kernel loses more to any co-resident kernel than that kernel takes (see split below); next to the latency-bound stages behind the
        # search it is free - 2.20 against 2.25 ms per 4K picture (X265HIP_LA_AFTER_ME=0: the old placement)
        la_after_me = self.la is not None and self.split == 1 and self.la_after_search
        if self.la is not None and not la_after_me:
            sLa.wait_event(start)
            with torch.cuda.stream(sLa):
                self.la.run(cur)
        # the reference's phase planes need only the reference and could run next to the search (X265HIP_PREP_OVERLAP=1), but their 141 MB
        # of plane writes compete with the search's record stream: measured 2.34 ms per step against 2.30 with the planes after the search
        overlap_prep = self.prep_next_to_search
        if overlap_prep:
            sCb.wait_event(start)
            with torch.cuda.stream(sCb):
                self.sp.prepare(ref)
                ev_pl = torch.cuda.Event(); ev_pl.record(sCb)
        self.ms.reset()
        mv = self.sp.out
        if self.split > 1:
            ev_rec = self._search_to_recon_in_parts(cur, ref, main, sCb, sCr, start)
        else:
            self.ms.search(cur, ref)
            if la_after_me:                  # the lookahead next to the stages behind the search instead of next to the search
                ev_me = torch.cuda.Event(); ev_me.record(main)
                sLa.wait_event(ev_me)
                with torch.cuda.stream(sLa):
                    self.la.run(cur)
            if overlap_prep:
                main.wait_event(ev_pl)
            self.sp.run(cur, ref, prepared=overlap_prep)
            ev_mv = torch.cuda.Event(); ev_mv.record(main)
            # reconstruction: one plane per stream
            self.rc.run(cur, ref, self.recon, mv)
            ev_rec = []
            for i, st in enumerate((sCb, sCr)):
                st.wait_event(ev_mv)
                with torch.cuda.stream(st):
                    self.rc_c[i].run(cur.c[i], ref.c[i], self.recon_c[i], cur.stride_c, cur.org_c, mv)
                    e = torch.cuda.Event(); e.record(st); ev_rec.append(e)
        # deblocking: boundary strengths + luma on the caller's stream; the chroma pass (both planes, one entry point) on Cb's stream
        self.db.run(self.recon, cur, mv, self.rc.num_sig)
        ev_bs = torch.cuda.Event(); ev_bs.record(main)
        sCb.wait_event(ev_bs); sCb.wait_event(ev_rec[1])
        with torch.cuda.stream(sCb):
            self._deblock_chroma(cur)
            ev_dbc = torch.cuda.Event(); ev_dbc.record(sCb)
        sCr.wait_event(ev_dbc)
        if self.sao_rdo is not None:
            # the decision couples the planes: statistics of Y on the caller's stream and of Cb / Cr on theirs, the decision + the application
            # of all three on the caller's stream, the border extensions back on the side streams
            self.sao.stats(cur, self.recon, cur.stride, cur.org)
            evs = []
            for i, st in enumerate((sCb, sCr)):
                with torch.cuda.stream(st):
                    self.sao_c[i].stats(None, self.recon_c[i], cur.stride_c, cur.org_c, src_plane=cur.c[i])
                    e = torch.cuda.Event(); e.record(st); evs.append(e)
            for e in evs:
                main.wait_event(e)
            self._sao_rdo()
            hipabi.sao_apply_planes(self.depth, self._sao_planes(cur))
            ev_sao = torch.cuda.Event(); ev_sao.record(main)
        elif self.fuse_sao_parallel:
            # SAO of the three planes: one launch per step on the caller's stream; only the border extensions go back to the side streams
            main.wait_event(ev_dbc)
            hipabi.sao_planes(self.depth, self._sao_planes(cur))
            ev_sao = torch.cuda.Event(); ev_sao.record(main)
        else:
            # SAO + border extension per plane
            self.sao.stats(cur, self.recon, cur.stride, cur.org)
            self.sao.decide()
            self.sao.apply(self.recon, cur.stride, cur.org, self.out)
        self._extend_border(self.out, cur)
        done = []
        for i, st in enumerate((sCb, sCr)):
            if self.fuse_sao_parallel or self.sao_rdo is not None:
                st.wait_event(ev_sao)
            with torch.cuda.stream(st):
                if not self.fuse_sao_parallel and self.sao_rdo is None:
                    self.sao_c[i].stats(None, self.recon_c[i], cur.stride_c, cur.org_c, src_plane=cur.c[i])
                    self.sao_c[i].decide()
                    self.sao_c[i].apply(self.recon_c[i], cur.stride_c, cur.org_c, self.out_c[i])
                self._extend_border(self.out_c[i], cur, chroma=True)
                e = torch.cuda.Event(); e.record(st); done.append(e)
        if self.la is not None:
            e = torch.cuda.Event(); e.record(sLa); done.append(e)
        for e in done:
            main.wait_event(e)
        self.final, self.final_c = self.out, self.out_c
        return self.final

    def _run_parallel2(self, cur, ref, main, sC):
        """The launch schedule of the default bench step since round 3, read off the dispatch timeline of one step
        (tools/gpu_visit.sh timeline, profiles/r03_step_timeline.txt).  Same launches and outputs as run(); what moved:
          * Cb + Cr are ONE chain of pair launches on one side stream (reconstruction pair, deblocking of both planes, statistics of both
            planes): two chains of half-size launches next to the luma chain each ran 1.8x their stand-alone time and ended 50 us after it;
          * the lookahead of the source picture runs on that stream BEHIND the chroma statistics, i.e. next to the SAO decision - a serial
            pass on ONE compute unit (115 us with the other 255 idle) - instead of next to the phase planes / sub-pel refinement, which it
            slowed; the minima of the NEXT picture's search are cleared there too (MotionSearch.reset_spare);
          * the sub-pel launch in front of the reconstruction refines the PU level the reconstruction codes and nothing else (25 instead of
            96 us at 4K); the other three levels' records are refined on the side stream behind the lookahead, next to the SAO decision
            (profiles/subpel_levels_kernel_trace.txt; X265HIP_SUBPEL_DEFER=0: all four in the one launch again);
          * ONE side stream: every cross-stream dependency costs the waiting stream ~8 us on this runtime, and a step on three side streams
            had eight of them on the caller's stream - now three records and two waits."""
        import torch
        ms = self.ms
        if self._spare_ready:                             # cleared next to the previous picture's stages, on the stream the caller joined last
            ms.swap_best()
        else:
            ms.reset()
        if self.prep_next_to_search:                      # X265HIP_PREP_OVERLAP=1 (experiment): the reference's phase planes next to the search, late in it
            ev0 = torch.cuda.Event(); ev0.record(main)
            sC.wait_event(ev0)
            with torch.cuda.stream(sC):
                self.sp.prepare(ref)
                ev_pl = torch.cuda.Event(); ev_pl.record(sC)
        ms.search(cur, ref)
        if self.prep_next_to_search:
            main.wait_event(ev_pl)
        # only the level the reconstruction codes is refined in front of it; the records of the other three are products of the step that
        # nothing in it reads: they are refined next to the SAO decision (below), or all four here in one launch (X265HIP_SUBPEL_DEFER=0)
        defer = self.subpel_defer
        rest = [l for l in range(4) if l != self.rc.level]
        self.sp.run(cur, ref, prepared=self.prep_next_to_search, levels=(self.rc.level,) if defer else None)
        mv = self.sp.out
        ev_mv = torch.cuda.Event(); ev_mv.record(main)
        ev_rest = None
        if defer == "mv":                                 # a stream of their own: the chroma chain on sC is on the critical path
            sD = self.pstreams[1]
            sD.wait_event(ev_mv)
            with torch.cuda.stream(sD):
                self.sp.run(cur, ref, prepared=True, levels=rest)
                ev_rest = torch.cuda.Event(); ev_rest.record(sD)
        self.rc.run(cur, ref, self.recon, mv)
        sC.wait_event(ev_mv)
        with torch.cuda.stream(sC):
            InterReconChroma.run_pair(self.rc_c, cur.c, ref.c, self.recon_c, cur.stride_c, cur.org_c, mv)
        self.db.run(self.recon, cur, mv, self.rc.num_sig)
        ev_bs = torch.cuda.Event(); ev_bs.record(main)
        planes = self._sao_planes(cur)
        sC.wait_event(ev_bs)
        with torch.cuda.stream(sC):
            self._deblock_chroma(cur)
            hipabi.sao_planes(self.depth, [dict(q, out=None) for q in planes[1:3]])
            ev_cstats = torch.cuda.Event(); ev_cstats.record(sC)
            ms.reset_spare()                              # the sub-pel stage has long read this picture's minima: the other buffer may be cleared
            self._spare_ready = True
            # behind the record the caller's stream waits for, in front of the one the step ends with: every record of sp.out is written
            # when run() returns, and the next step's phase planes are not rewritten while these launches read them
            if defer == "before":
                self.sp.run(cur, ref, prepared=True, levels=rest)
            if self.la is not None:
                self.la.run(cur)
            if defer == "after":
                self.sp.run(cur, ref, prepared=True, levels=rest)
            ev_side = torch.cuda.Event(); ev_side.record(sC)
        hipabi.sao_planes(self.depth, [dict(planes[0], out=None)])
        main.wait_event(ev_cstats)
        self._sao_rdo()
        hipabi.sao_apply_planes(self.depth, planes)
        self._extend_borders(cur, [self.out] + list(self.out_c))          # one launch; three back to back (15 us) with the switch at 0
        main.wait_event(ev_side)                          # the lookahead and the cleared minima (long done: next to the SAO decision)
        if ev_rest is not None:
            main.wait_event(ev_rest)
        self.final, self.final_c = self.out, self.out_c
        return self.final

    def swap_output(self, spare):
        """Ping-pong of the decoded picture: hands out the planes the last run() wrote (the next reference) and takes `spare` - [Y, Cb, Cr]
        planes the host no longer needs, e.g. the reference that has just been replaced - as the destination of the next run().  What a
        decoded-picture buffer does instead of copying a picture per frame.  None when the last output is not a plane set of its own."""
        if self.final is not self.out or self.out is None or (self.chroma and self.final_c is not self.out_c):
            return None
        outs = self.final_planes()
        self.out = spare[0]
        if self.chroma:
            self.out_c = list(spare[1:3])
        return outs

    def _search_to_recon_in_parts(self, cur, ref, main, sCb, sCr, start):
        """Search on `main`, part after part; a part's sub-pel refinement + luma reconstruction follow on a fourth stream, its chroma
        reconstructions on the Cb / Cr streams - except the last part's luma chain, which continues on `main` (the loop filters wait for it
        there anyway).  Returns the events after which Cb / Cr are reconstructed; `main` has waited for every luma part."""
        import torch
        if self.parts is None:
            rows = self.h64 // 64
            cuts = [rows * k // self.split for k in range(self.split + 1)]
            self.parts = []
            for r0, r1 in zip(cuts[:-1], cuts[1:]):
                msp = self.ms.part(r0, r1 - r0)
                self.parts.append((r0, r1 - r0, msp, self.sp.part(msp, r0), self.rc.part(r0, r1 - r0), [q.part(r0, r1 - r0) for q in self.rc_c]))
        sY = self.pstreams[3]
        sY.wait_event(start)
        with torch.cuda.stream(sY):                       # the reference's phase planes: next to the first part's search
            self.sp.prepare(ref)
        last = len(self.parts) - 1
        for k, (r0, n, msp, spp, rcp, rcc) in enumerate(self.parts):
            c, r = cur.band_view(r0, n), ref.band_view(r0, n)
            msp.search(c, r)
            ev_me = torch.cuda.Event(); ev_me.record(main)
            st = main if k == last else sY
            if k == last:
                main.wait_stream(sY)                      # the phase planes (and the earlier parts' luma chains)
            else:
                sY.wait_event(ev_me)
            with torch.cuda.stream(st):
                spp.run(c, r, prepared=True)
                ev_mv = torch.cuda.Event(); ev_mv.record(st)
                rcp.run(c, r, self.recon, spp.out)
            for i, sc in enumerate((sCb, sCr)):
                sc.wait_event(ev_mv)
                with torch.cuda.stream(sc):
                    rcc[i].run(cur.c[i], ref.c[i], self.recon_c[i], cur.stride_c, c.org_c, spp.out)
        ev_rec = []
        for sc in (sCb, sCr):
            e = torch.cuda.Event(); e.record(sc); ev_rec.append(e)
        return ev_rec

    def _table(self, key):
        if key not in self.tables:
            n = len(key)
            self.tables[key] = LookaheadCost.table(self.lc[:n], [self.ring[c] for c, _ in key], [self.ring[r] for _, r in key], self.device)
        return self.tables[key]

    def launch_lookahead_costs(self):
        """Score the pending (picture, previous picture) pairs in one launch on the side stream."""
        import torch
        if not self.lcb or not self.pending:
            return
        ready = torch.cuda.Event()
        ready.record()                                       # the pictures were prepared on the current stream
        self.side.wait_event(ready)
        n = len(self.pending)
        LookaheadCost.run_batch(self.lc[:n], [self.ring[c] for c, _ in self.pending], [self.ring[r] for _, r in self.pending],
                                stream=self.side.cuda_stream, device_table=self._table(tuple(self.pending)))
        done = torch.cuda.Event()
        done.record(self.side)
        for c, r in self.pending:
            self.read_done[c] = done
            self.read_done[r] = done
        self.pending = []

    def checksum(self):
        import torch
        out = {}
        if self.lcb:
            out["lookahead_cost"] = int(sum(int(s.frame[0].item()) for s in self.lc))
        out.update(self.ps.checksum() if self.ps is not None else self.sp.checksum())
        out.update(self.rc.checksum())
        if self.la is not None:
            out.update(self.la.checksum())
        if self.sao is not None:
            out["sao_count"] = int(self.sao.count.sum(dtype=torch.int64).item())
            out["sao_offset_org"] = int(self.sao.offset_org.sum(dtype=torch.int64).item())
        out["recon"] = _sum64(self.final.view(torch.uint8))
        if self.chroma:
            out["recon_cb"] = _sum64(self.final_c[0].view(torch.uint8))
            out["recon_cr"] = _sum64(self.final_c[1].view(torch.uint8))
            out["levels_c"] = sum(_sum64(r.levels) for r in self.rc_c)
        if self.sao_apply:
            out["sao_types"] = int((self.sao.params.view(-1, 7)[:, 0] >= 0).sum().item())
        return out


class BandedFramePipeline:
    """The frame pipeline band by band - the reference's `--slices` picture: bands of `band_rows` CTU rows, each searched, reconstructed
    and loop-filtered as a slice of its own (deblocking and SAO stop at the band boundary like the reference's slices: m_cuAbove is NULL
    for the first row of a slice, cudata.cpp:319; SAO's firstRowInSlice / lastRowInSlice, sao.cpp:286-287), while the exhaustive search,
    sub-pel refinement and prediction read the whole reference picture around the band.  A finished band (filtered, side margins
    extended) can be handed to the rank that searches it next while the following bands are still in flight - the granularity of the
    reference's m_reconRowFlag (framefilter.cpp:664).  band_ready(b, row0, rows), if given, is called after band b's launches."""

    def __init__(self, w64, h64, depth, device, band_rows=4, lookahead=None, graphs=False, streams=1, **kw):
        """graphs: a band's ~25 launches are captured once per (band, source picture, reference picture) into a HIP graph and replayed with
        one launch - a band is 240 workgroups per kernel, so enqueueing its launches one by one from the host costs more than running them
        (3.9 ms per 4K frame of 9 bands against 2.2 ms for the frame in one piece).  The buffers must then stay where they are between frames."""
        self.w64, self.h64, self.depth, self.device = w64, h64, depth, device
        self.use_graphs, self.graphs, self.warm = bool(graphs), {}, set()
        rows = h64 // 64
        self.bands = [(r, min(band_rows, rows - r)) for r in range(0, rows, band_rows)]
        kw.pop("lookahead_cost_batch", None)
        # options that make a stage read or write WHOLE pictures per call have no banded meaning: every band would recompute the whole
        # reference's phase planes, and in ring mode read reference rows that have not arrived yet (round-2 advisor finding)
        # (parallel_planes - the Cb / Cr chains of a band on their own streams - IS a per-band option: tests/test_gpu_banded.py)
        for opt in ("subpel_planes", "split"):
            if kw.get(opt):
                raise ValueError(f"BandedFramePipeline: {opt} is a whole-picture option and cannot be forwarded to the band pipelines")
        if kw.get("chroma_satd"):
            raise ValueError("BandedFramePipeline: chroma_satd is not supported in band mode")
        # streams > 1: band b runs on HIP stream b % streams with its own set of stage buffers.  The bands of one picture do not depend on
        # each other (each is a slice), so the exhaustive search of band b + 1 - the one launch that fills the chip - overlaps the
        # reconstruction / deblocking / SAO launches of band b, which at band size are a few dozen workgroups each and bound by their own
        # latency.  begin_frame() forks the band streams from the caller's stream, end_frame() joins them.
        self.nstreams = max(1, int(streams))
        self.pipe_sets = [{n: FramePipeline(w64, n * 64, depth, device, lookahead=None, **kw) for n in sorted({n for _, n in self.bands})}
                          for _ in range(self.nstreams)]
        self.pipes = self.pipe_sets[0]
        self.streams = None
        self.la = Lookahead(lookahead[0], lookahead[1], depth, device) if lookahead else None
        self.planes = None          # [Y, Cb, Cr] the bands are written into: reconstruction and filtered picture
        self.chroma = bool(kw.get("chroma"))
        self.sao_apply = bool(kw.get("sao") and kw.get("sao_apply"))

    def _alloc(self, cur):
        import torch
        if self.planes is None:
            self.recon = [torch.zeros_like(p) for p in cur.planes()]
            self.final = [torch.zeros_like(p) for p in cur.planes()] if self.sao_apply else self.recon
        for pipe in [q for ps in self.pipe_sets for q in ps.values()]:
            pipe.recon = self.recon[0]
            pipe.recon_c = self.recon[1:3] if self.chroma else None
            if self.sao_apply:
                pipe.out = self.final[0]
                pipe.out_c = self.final[1:3] if self.chroma else None
        self.planes = self.final

    def begin_frame(self, cur):
        """Per-frame work that does not depend on the reference: output planes, the lookahead stage of the source picture."""
        self._alloc(cur)
        if self.nstreams > 1:
            import torch
            if self.streams is None:
                self.streams = [torch.cuda.Stream(device=self.device) for _ in range(self.nstreams)]
            ev = torch.cuda.Event()
            ev.record()
            for st in self.streams:          # whatever the caller queued before (the hand-off of the previous picture) comes first
                st.wait_event(ev)
        if self.la is not None:
            self.la.run(cur)

    def band_context(self, b):
        """Context manager under which band b's launches (and the transfers that wait for / follow them) are issued."""
        import contextlib
        if self.nstreams == 1 or self.streams is None:
            return contextlib.nullcontext()
        import torch
        return torch.cuda.stream(self.streams[b % self.nstreams])

    def end_frame(self):
        """The caller's stream continues after every band of the picture."""
        if self.nstreams > 1 and self.streams is not None:
            import torch
            main = torch.cuda.current_stream()
            for st in self.streams:
                main.wait_stream(st)

    def _launch_band(self, b, cur, ref):
        row0, n = self.bands[b]
        pipe = self.pipe_sets[b % self.nstreams][n]
        pipe.band_border = (b == 0, b == len(self.bands) - 1)
        pipe.run(cur.band_view(row0, n), ref.band_view(row0, n))

    def run_band(self, b, cur, ref):
        if not self.use_graphs:
            return self._launch_band(b, cur, ref)
        import torch
        n = (self.bands[b][1], b % self.nstreams)
        if n not in self.warm:                     # the first band of this height runs launch by launch: lazy allocations, kernel attributes
            self.warm.add(n)
            return self._launch_band(b, cur, ref)
        key = (b,) + tuple(p.data_ptr() for p in cur.planes()) + tuple(p.data_ptr() for p in ref.planes())
        g = self.graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):       # other threads (RCCL's watchdog) keep working during the capture
                self._launch_band(b, cur, ref)
            self.graphs[key] = g
        g.replay()

    def capture(self, cur, ref):
        """Record every band of (cur, ref) ahead of time (set-up, outside any timed region).  Executes the bands once."""
        self.begin_frame(cur)
        for _ in range(2):
            for b in range(len(self.bands)):
                with self.band_context(b):
                    self.run_band(b, cur, ref)
        self.end_frame()

    def run(self, cur, ref, band_ready=None, before_band=None):
        self.begin_frame(cur)
        for b, (row0, n) in enumerate(self.bands):
            with self.band_context(b):
                if before_band is not None:
                    before_band(b, row0, n)                 # e.g. wait until the reference rows this band reads have arrived
                self.run_band(b, cur, ref)
                if band_ready is not None:
                    band_ready(b, row0, n)
        self.end_frame()
        return self.planes[0]

    def final_planes(self):
        return list(self.planes)


class BidirDecide:
    """The bidirectional decision of a B picture (x265hip_bidir_decide; reference Search::predInterSearch, search.cpp:2473-2640): from the
    two lists' refined records, per block of the TU stages' grid, list 0 / list 1 / both.  Owns dir uint8 [ctu][blocks] (what InterReconBi
    takes), ref0 / ref1 int8 [ctu][blocks] (what Deblock.run_b takes), mv0_out / mv1_out int32 [ctu*85][2] (the level's entries) and,
    with want_cost, cost_out int32 [ctu][blocks][4]."""

    def __init__(self, nctu, w64, h64, depth, level, device, dir_cost=(12, 12, 20), ref_ids=(0, 1), want_cost=False, chroma_satd=False):
        """dir_cost: lambda x the list-selection bits of a B slice's 2Nx2N (3, 3, 5; search.cpp:2649-2656) - (12, 12, 20) at the pipeline's lambda 4.
        chroma_satd: the records come from the chroma refinement and the bidirectional candidate is the motion compensation of all three
        planes (x265hip_bidir_decide_chroma); the pictures must carry chroma planes and no phase planes are passed."""
        import torch
        self.chroma_satd = bool(chroma_satd)
        self.nctu, self.w64, self.h64, self.depth, self.level = nctu, w64, h64, depth, level
        self.nblk = (64 // (8 << level)) ** 2
        self.dir_cost, self.ref_ids = tuple(int(c) for c in dir_cost), tuple(ref_ids)
        self.dir = torch.zeros(nctu * self.nblk, dtype=torch.uint8, device=device)
        self.ref0 = torch.zeros(nctu * self.nblk, dtype=torch.int8, device=device)
        self.ref1 = torch.zeros(nctu * self.nblk, dtype=torch.int8, device=device)
        self.mv0_out = torch.zeros(nctu * PUS_PER_CTU * 2, dtype=torch.int32, device=device)
        self.mv1_out = torch.zeros(nctu * PUS_PER_CTU * 2, dtype=torch.int32, device=device)
        self.cost_out = torch.zeros(nctu * self.nblk * 4, dtype=torch.int32, device=device) if want_cost else None

    def run(self, cur: DevicePicture, ref0: DevicePicture, ref1: DevicePicture, mv0, mv1, cost_q, qoff, phase_planes=None, stream=None):
        """mv0 / mv1: the two SubpelRefine outputs; phase_planes: (list 0, list 1) planes of x265hip_phase_planes or None (interpolate)."""
        assert ref0.stride == ref1.stride and ref0.org == ref1.org
        chroma = None
        if self.chroma_satd:
            if cur.c is None or ref0.c is None or ref1.c is None:
                raise ValueError("BidirDecide(chroma_satd=True) needs pictures with chroma planes")
            assert ref0.stride_c == ref1.stride_c and ref0.org_c == ref1.org_c
            chroma = dict(fenc=cur.c, fenc_stride=cur.stride_c, fenc_org=cur.org_c, fref0=ref0.c, fref1=ref1.c, fref_stride=ref0.stride_c, fref_org=ref0.org_c)
            phase_planes = None              # rounded pixels: they cannot serve the 14-bit motion compensation
        hipabi.bidir_decide(self.depth, self.w64, self.h64, self.level, cur.t, cur.stride, ref0.t, ref1.t, ref0.stride, mv0, mv1, cost_q, qoff,
                            self.dir_cost, self.dir, self.mv0_out, self.mv1_out, ref0=self.ref0, ref1=self.ref1, cost_out=self.cost_out,
                            ref_ids=self.ref_ids, fenc_off=cur.org, fref_off=ref0.org, phase_planes=phase_planes, stream=stream, chroma=chroma)

    def checksum(self):
        return {"dir": _sum64(self.dir), "mv0_out": _sum64(self.mv0_out), "mv1_out": _sum64(self.mv1_out)}


class BFramePipeline(_RefListStep):
    """One B picture on the device, the stages of FramePipeline.run with two reference lists:
        per list: exhaustive search (best mv) -> sub-pel refinement;  bidirectional decision (BidirDecide);  bi-predictive luma + 4:2:0
        chroma reconstruction with the decided dir / vectors;  B-picture boundary strengths + luma / chroma deblocking;  SAO (statistics,
        x265hip_sao_rdo or the distortion-only stand-in, application);  border extension.
    The constructor switches mean what they mean in FramePipeline.  A B picture is not referenced here; final_planes() are its output."""

    def __init__(self, w64, h64, depth, device, rng=57, subme=2, level=2, qp=27, deblock=False, sao=False, chroma=False, sao_apply=False,
                 sign_hide=False, subpel_planes=False, sao_rdo=None, dir_cost=(12, 12, 20), want_cost=False, chroma_satd=False):
        """chroma_satd (with chroma): both refinements and the decision measure chroma as the reference does at subme >= 3
        (x265hip_subpel_refine_chroma, x265hip_bidir_decide_chroma)."""
        if chroma_satd and not chroma:
            raise ValueError("BFramePipeline: chroma_satd needs chroma=True")
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        self._build_lists(2, w64, h64, depth, device, rng, subme, subpel_planes, chroma_satd)
        self.bd = BidirDecide(self.nctu, w64, h64, depth, level, device, dir_cost=dir_cost, want_cost=want_cost,
                              chroma_satd=chroma_satd and subme >= 3)      # bChromaSATD is off at subme <= 2 (motion.cpp:212): luma-only decision there
        self.tu_flags = hipabi.TU_SIGN_HIDE if sign_hide else 0
        self.rc = InterReconBi(self.nctu, w64, h64, depth, level, qp, device, intra_slice=self.tu_flags)
        if chroma:
            qpc = chroma_quant_qp(qp, depth)
            self.rc_c = [InterReconChromaBi(self.nctu, w64, h64, depth, level, qpc, device, intra_slice=self.tu_flags) for _ in range(2)]

    def run(self, cur: DevicePicture, ref0: DevicePicture, ref1: DevicePicture, mark=None):
        """ref0 / ref1: the list-0 / list-1 reference pictures (extended borders; with chroma=True also their Cb / Cr planes).  Returns the
        luma plane of the coded picture; mark(name), if given, is called after every stage."""
        self._qp_maps_run_check()
        mark = mark or (lambda name: None)
        self._alloc_planes(cur)
        self._search_lists(cur, (ref0, ref1), mark)
        phases = (self.spl[0].planes, self.spl[1].planes) if self.spl[0].use_planes else None      # what the two refinements just prepared
        self.bd.run(cur, ref0, ref1, self.spl[0].out, self.spl[1].out, self.spl[0].cost_q, self.spl[0].qoff, phase_planes=phases)
        mark("bidir")
        mv0, mv1, dirs = self.bd.mv0_out, self.bd.mv1_out, self.bd.dir
        self.rc.run(cur, ref0, ref1, self.recon, mv0, mv1, dir_flags=dirs)
        mark("recon")
        if self.chroma:
            for i in range(2):
                self.rc_c[i].run(cur.c[i], ref0.c[i], ref1.c[i], self.recon_c[i], cur.stride_c, cur.org_c, mv0, mv1, dir_flags=dirs)
            mark("recon_chroma")
        if self.db is not None:
            self.db.run_b(self.recon, cur, mv0, mv1, self.bd.ref0, self.bd.ref1, self.rc.num_sig)
        return self._filter_tail(cur, mark)

    def checksum(self):
        return self._checksum(self.bd)


class RefSelect:
    """The reference of every block of a P picture with several references (x265hip_ref_select; reference Search::predInterSearch's
    uni-directional loop, search.cpp:2386-2471): from the records of the per-reference refinements, per block of the TU stages' grid,
    the list index with the smallest cost + ref_cost, the lowest index on a tie.  Owns ref_idx int8 [ctu][blocks] (what InterReconRefs
    takes), ref_id int8 [ctu][blocks] (what Deblock.run_refs takes), mv_out int32 [ctu*85][2] (the level's entries) and, with want_cost,
    cost_out int32 [ctu][blocks][max_refs] (the first nrefs * blocks entries hold [ctu][blocks][nrefs] of a run with nrefs references)."""

    def __init__(self, nctu, w64, h64, depth, level, device, max_refs=4, want_cost=False):
        import torch
        if not 1 <= max_refs <= hipabi.MAX_REFS:
            raise ValueError(f"RefSelect: max_refs {max_refs} out of [1, {hipabi.MAX_REFS}]")
        self.nctu, self.w64, self.h64, self.depth, self.level, self.max_refs = nctu, w64, h64, depth, level, max_refs
        self.nblk = (64 // (8 << level)) ** 2
        self.ref_idx = torch.zeros(nctu * self.nblk, dtype=torch.int8, device=device)
        self.ref_id = torch.zeros(nctu * self.nblk, dtype=torch.int8, device=device)
        self.mv_out = torch.zeros(nctu * PUS_PER_CTU * 2, dtype=torch.int32, device=device)
        self.cost_out = torch.zeros(nctu * self.nblk * max_refs, dtype=torch.int32, device=device) if want_cost else None

    def run(self, mvs, ref_cost=None, ref_ids=None, stream=None):
        """mvs: the SubpelRefine outputs, list order (1 .. max_refs of them); ref_cost: one int per reference, None = lambda 4 x the bits of
        the index (hipabi.ref_cost_bits); ref_ids: the picture ids ref_id gets, None = the list indices."""
        n = len(mvs)
        if not 1 <= n <= self.max_refs:
            raise ValueError(f"RefSelect: {n} references for max_refs {self.max_refs}")
        cost = hipabi.ref_cost_bits(n) if ref_cost is None else tuple(int(c) for c in ref_cost)
        if len(cost) != n or (ref_ids is not None and len(ref_ids) != n):
            raise ValueError("RefSelect: ref_cost / ref_ids need one entry per reference")
        hipabi.ref_select(self.depth, self.w64, self.h64, self.level, mvs, cost, self.ref_idx, self.mv_out, ref_id=self.ref_id,
                          cost_out=self.cost_out, ref_ids=ref_ids, stream=stream)

    def checksum(self):
        return {"ref_idx": _sum64(self.ref_idx), "mv_out": _sum64(self.mv_out)}


class MultiRefFramePipeline(_RefListStep):
    """One P picture with several references on the device, the stages of FramePipeline.run with a reference list:
        per reference: exhaustive search (best mv) -> sub-pel refinement;  reference selection (RefSelect);  luma + 4:2:0 chroma
        reconstruction of every block from its chosen picture;  boundary strengths that compare the blocks' pictures + luma / chroma
        deblocking;  SAO (statistics, x265hip_sao_rdo or the distortion-only stand-in, application);  border extension.
    The constructor switches mean what they mean in BFramePipeline.  Everything runs serially on the caller's stream."""

    def __init__(self, w64, h64, depth, device, max_refs=4, rng=57, subme=2, level=2, qp=27, deblock=False, sao=False, chroma=False,
                 sao_apply=False, sign_hide=False, subpel_planes=False, sao_rdo=None, chroma_satd=False, ref_cost=None, want_cost=False):
        """ref_cost: one int per reference of every run() (lambda x the bits of the reference index), None = hipabi.ref_cost_bits of the
        number of references a run() is given."""
        if chroma_satd and not chroma:
            raise ValueError("MultiRefFramePipeline: chroma_satd needs chroma=True")
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        self.max_refs = max_refs
        self.ref_cost = None if ref_cost is None else tuple(int(c) for c in ref_cost)
        self._build_lists(max_refs, w64, h64, depth, device, rng, subme, subpel_planes, chroma_satd)
        self.rs = RefSelect(self.nctu, w64, h64, depth, level, device, max_refs=max_refs, want_cost=want_cost)
        self.tu_flags = hipabi.TU_SIGN_HIDE if sign_hide else 0
        self.rc = InterReconRefs(self.nctu, w64, h64, depth, level, qp, device, intra_slice=self.tu_flags)
        if chroma:
            qpc = chroma_quant_qp(qp, depth)
            self.rc_c = [InterReconChromaRefs(self.nctu, w64, h64, depth, level, qpc, device, intra_slice=self.tu_flags) for _ in range(2)]

    def run(self, cur: DevicePicture, refs, mark=None):
        """refs: 1 .. max_refs reference pictures, nearest first = list order (extended borders; with chroma=True also their Cb / Cr
        planes).  Returns the luma plane of the coded picture; mark(name), if given, is called after every stage."""
        self._qp_maps_run_check()
        mark = mark or (lambda name: None)
        refs = list(refs)
        if not 1 <= len(refs) <= self.max_refs:
            raise ValueError(f"MultiRefFramePipeline: {len(refs)} references for max_refs {self.max_refs}")
        if self.ref_cost is not None and len(self.ref_cost) != len(refs):
            raise ValueError(f"MultiRefFramePipeline: ref_cost has {len(self.ref_cost)} entries for {len(refs)} references")
        self._alloc_planes(cur)
        self._search_lists(cur, refs, mark)
        self.rs.run([self.spl[r].out for r in range(len(refs))], ref_cost=self.ref_cost)
        mark("ref_select")
        mv, idx = self.rs.mv_out, self.rs.ref_idx
        self.rc.run(cur, refs, self.recon, mv, idx)
        mark("recon")
        if self.chroma:
            InterReconChromaRefs.run_pair(self.rc_c, cur.c, [[ref.c[i] for ref in refs] for i in range(2)], self.recon_c, cur.stride_c, cur.org_c, mv, idx)
            mark("recon_chroma")
        if self.db is not None:
            self.db.run_refs(self.recon, cur, mv, self.rs.ref_id, self.rc.num_sig)
        return self._filter_tail(cur, mark)

    def checksum(self):
        return self._checksum(self.rs)


class BidirDecideRefs(BidirDecide):
    """The bidirectional decision of a B picture with several references per list (x265hip_bidir_decide_refs): every block is measured
    against the two pictures it chose - the two RefSelect outputs - with the reference bits of both lists in the bidirectional and the zero
    candidate.  Owns what BidirDecide owns; ref0 / ref1 hold the PICTURE ids of the blocks' references (or -1)."""

    def __init__(self, nctu, w64, h64, depth, level, device, dir_cost=(12, 12, 20), want_cost=False):
        BidirDecide.__init__(self, nctu, w64, h64, depth, level, device, dir_cost=dir_cost, want_cost=want_cost)

    def run(self, cur: DevicePicture, refs0, refs1, mv0, mv1, ref_idx0, ref_idx1, ref_cost0, ref_cost1, cost_q, qoff, ref_ids0=None, ref_ids1=None,
            phase_planes0=None, phase_planes1=None, stream=None):
        """refs0 / refs1: each list's pictures in list order; mv0 / mv1, ref_idx0 / ref_idx1: mv_out and ref_idx of the two RefSelect
        passes; ref_cost0 / ref_cost1: what those passes were given; phase_planes0 / phase_planes1: per reference the planes of
        x265hip_phase_planes, or None (interpolate)."""
        first = refs0[0]
        assert all(r.stride == first.stride and r.org == first.org for r in list(refs0) + list(refs1))
        hipabi.bidir_decide_refs(self.depth, self.w64, self.h64, self.level, cur.t, cur.stride, [r.t for r in refs0], [r.t for r in refs1], first.stride,
                                 mv0, mv1, ref_idx0, ref_idx1, ref_cost0, ref_cost1, cost_q, qoff, self.dir_cost, self.dir, self.mv0_out, self.mv1_out,
                                 ref0=self.ref0, ref1=self.ref1, cost_out=self.cost_out, ref_ids0=ref_ids0, ref_ids1=ref_ids1, fenc_off=cur.org,
                                 fref_off=first.org, phase_planes0=phase_planes0, phase_planes1=phase_planes1, stream=stream)


class MultiRefBFramePipeline(_RefListStep):
    """One B picture with several references per list on the device, the stages of BFramePipeline.run with two reference lists of pictures:
        per DISTINCT reference picture: exhaustive search (best mv) -> sub-pel refinement;  per list: reference selection (RefSelect);
        bidirectional decision against the two pictures every block chose (BidirDecideRefs);  bi-predictive luma + 4:2:0 chroma
        reconstruction from those pictures;  B-picture boundary strengths on picture ids + luma / chroma deblocking;  SAO;  border extension.
    The constructor switches mean what they mean in BFramePipeline.  Everything runs serially on the caller's stream."""

    def __init__(self, w64, h64, depth, device, max_refs=(2, 2), rng=57, subme=2, level=2, qp=27, deblock=False, sao=False, chroma=False, sao_apply=False,
                 sign_hide=False, subpel_planes=False, sao_rdo=None, dir_cost=(12, 12, 20), want_cost=False, chroma_satd=False, ref_cost=None):
        """max_refs: (list 0, list 1), the most references a run() is given per list.  ref_cost: (list 0, list 1), one int per reference
        of every run() (lambda x the bits of the reference index), None = hipabi.b_ref_cost_bits of each list's length."""
        if chroma_satd:
            raise ValueError("MultiRefBFramePipeline: chroma SATD is not part of the decision with several references per list")
        n0, n1 = (int(n) for n in max_refs)
        if not (1 <= n0 <= hipabi.MAX_REFS and 1 <= n1 <= hipabi.MAX_REFS):
            raise ValueError(f"MultiRefBFramePipeline: max_refs {max_refs} out of [1, {hipabi.MAX_REFS}]")
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        self.max_refs = (n0, n1)
        self.ref_cost = None if ref_cost is None else tuple(tuple(int(c) for c in l) for l in ref_cost)
        self._build_lists(n0 + n1, w64, h64, depth, device, rng, subme, subpel_planes, False)      # one slot per distinct picture
        self.rs = [RefSelect(self.nctu, w64, h64, depth, level, device, max_refs=n, want_cost=want_cost) for n in (n0, n1)]
        self.bd = BidirDecideRefs(self.nctu, w64, h64, depth, level, device, dir_cost=dir_cost, want_cost=want_cost)
        self.tu_flags = hipabi.TU_SIGN_HIDE if sign_hide else 0
        self.rc = InterReconBiRefs(self.nctu, w64, h64, depth, level, qp, device, intra_slice=self.tu_flags)
        if chroma:
            qpc = chroma_quant_qp(qp, depth)
            self.rc_c = [InterReconChromaBiRefs(self.nctu, w64, h64, depth, level, qpc, device, intra_slice=self.tu_flags) for _ in range(2)]
        self.slots = ([], [])

    def run(self, cur: DevicePicture, refs0, refs1, mark=None, ref_ids=None):
        """refs0 / refs1: the list-0 / list-1 reference pictures in list order (extended borders; with chroma=True also their Cb / Cr
        planes).  A picture that sits in both lists - the same object - is searched and refined once; its records and phase planes serve
        both lists.  ref_ids: (list 0, list 1) picture ids within int8, equal for the same picture and distinct otherwise (two objects
        may carry one id: copies of one picture); None = derived here (the picture's place among the distinct objects).  Returns the luma plane of the coded picture; mark(name), if given, is
        called after every stage."""
        self._qp_maps_run_check()
        mark = mark or (lambda name: None)
        lists = (list(refs0), list(refs1))
        for l in range(2):
            if not 1 <= len(lists[l]) <= self.max_refs[l]:
                raise ValueError(f"MultiRefBFramePipeline: {len(lists[l])} references in list {l} for max_refs {self.max_refs}")
            if self.ref_cost is not None and len(self.ref_cost[l]) != len(lists[l]):
                raise ValueError(f"MultiRefBFramePipeline: ref_cost has {len(self.ref_cost[l])} entries for {len(lists[l])} references in list {l}")
        distinct = []
        for ref in lists[0] + lists[1]:
            if not any(ref is d for d in distinct):
                distinct.append(ref)
        slot_of = lambda ref: next(i for i, d in enumerate(distinct) if d is ref)
        self.slots = tuple([slot_of(ref) for ref in lists[l]] for l in range(2))
        if ref_ids is None:
            ids = self.slots
        else:
            ids = tuple([int(i) for i in ref_ids[l]] for l in range(2))
            by_slot = {}
            for l in range(2):
                if len(ids[l]) != len(lists[l]) or any(not -128 <= i <= 127 for i in ids[l]):
                    raise ValueError("MultiRefBFramePipeline: ref_ids need one int8 per reference")
                for sl, i in zip(self.slots[l], ids[l]):
                    if by_slot.setdefault(sl, i) != i:
                        raise ValueError("MultiRefBFramePipeline: one picture with two ids")
        self._alloc_planes(cur)
        self._search_lists(cur, distinct, mark)
        cost = tuple(hipabi.b_ref_cost_bits(len(lists[l])) if self.ref_cost is None else self.ref_cost[l] for l in range(2))
        for l in range(2):
            self.rs[l].run([self.spl[sl].out for sl in self.slots[l]], ref_cost=cost[l], ref_ids=ids[l])
        mark("ref_select")
        phases = [[self.spl[sl].planes for sl in self.slots[l]] if self.spl[0].use_planes else None for l in range(2)]
        self.bd.run(cur, lists[0], lists[1], self.rs[0].mv_out, self.rs[1].mv_out, self.rs[0].ref_idx, self.rs[1].ref_idx, cost[0], cost[1],
                    self.spl[0].cost_q, self.spl[0].qoff, ref_ids0=ids[0], ref_ids1=ids[1], phase_planes0=phases[0], phase_planes1=phases[1])
        mark("bidir")
        mv0, mv1, dirs, i0, i1 = self.bd.mv0_out, self.bd.mv1_out, self.bd.dir, self.rs[0].ref_idx, self.rs[1].ref_idx
        self.rc.run(cur, lists[0], lists[1], self.recon, mv0, mv1, i0, i1, dir_flags=dirs)
        mark("recon")
        if self.chroma:
            for i in range(2):
                self.rc_c[i].run(cur.c[i], [r.c[i] for r in lists[0]], [r.c[i] for r in lists[1]], self.recon_c[i], cur.stride_c, cur.org_c, mv0, mv1, i0, i1,
                                 dir_flags=dirs)
            mark("recon_chroma")
        if self.db is not None:
            self.db.run_b(self.recon, cur, mv0, mv1, self.bd.ref0, self.bd.ref1, self.rc.num_sig)
        return self._filter_tail(cur, mark)

    def checksum(self):
        out = self._checksum(self.bd)
        for l in range(2):
            out["ref_idx%d" % l] = self.rs[l].checksum()["ref_idx"]
        return out


class IntraPicture:
    """One I picture on the TU stages' block grid (x265hip_intra_picture; reference Predict::initIntraNeighbors / fillReferenceSamples /
    initAdiPattern, predict.cpp:600-876, Search::checkIntraInInter, search.cpp:1344-1446, and the coding contract of
    x265hip_intra_recon_batch): per block the neighbours from the reconstruction, the 35-mode sa8d decision and the winner's transform
    round trip, CTUs wave by wave (wave = cx + 2 cy, one launch each).  Owns mode uint8 [ctu][blocks], levels / num_sig / dist as
    InterRecon lays them out, with chroma the Cb / Cr twins (levels_c / num_sig_c / dist_c, (N/2)^2 levels per block) and, with
    want_cost, cost int32 [ctu][blocks][2] = {winning sad, winning cost}."""

    def __init__(self, nctu, w64, h64, depth, level, qp, device, flags=hipabi.TU_INTRA_SLICE, chroma=False, qp_c=None, lambda8=1024,
                 mode_bits=(2, 3, 6), strong_intra_smoothing=True, want_cost=False):
        """lambda8: 256 x lambda (RDCost::m_lambda; 1024 at the pipeline's lambda 4).  mode_bits: bitsIntraModeMPM of preds[0], of
        preds[1] / preds[2] and bitsIntraModeNonMPM at the host's context state - (2, 3, 6) prices both bin values at one bit."""
        import torch
        self.nctu, self.w64, self.h64, self.depth, self.level, self.qp, self.flags = nctu, w64, h64, depth, level, qp, flags
        self.chroma, self.qp_c = chroma, (qp_c if qp_c is not None else (qp, qp))
        self.lambda8, self.mode_bits, self.strong = int(lambda8), tuple(int(b) for b in mode_bits), bool(strong_intra_smoothing)
        self.n = 8 << level
        self.nblk = (64 // self.n) ** 2
        self.waves = hipabi.intra_picture_waves(w64, h64)
        nb = nctu * self.nblk

        def outs(nn):
            return (torch.zeros(nb * nn, dtype=torch.int16, device=device), torch.zeros(nb, dtype=torch.int32, device=device),
                    torch.zeros(nb, dtype=torch.int64, device=device))
        self.mode = torch.zeros(nb, dtype=torch.uint8, device=device)
        self.levels, self.num_sig, self.dist = outs(self.n * self.n)
        self.cost = torch.zeros(nb * 2, dtype=torch.int32, device=device) if want_cost else None
        if chroma:
            c = [outs(self.n * self.n // 4) for _ in range(2)]
            self.levels_c, self.num_sig_c, self.dist_c = ([c[i][k] for i in range(2)] for k in range(3))
        # per-block QPs: qp_map = the whole CuQpMaps.tu_qp (device int8 [3][h64 / 8 * w64 / 8]); lambda8_by_qp = device int32 [52 + 6 (depth - 8)],
        # 256 x lambda of a CU at that luma quantiser QP (None = lambda8 for every block)
        self.qp_map, self.lambda8_by_qp = None, None

    def run(self, cur: DevicePicture, recon_plane, recon_c=None, stream=None):
        """recon_plane (and recon_c = [Cb, Cr] with chroma): planes of cur's geometry the reconstruction is written into - and read from,
        block after block; their contents before the call do not matter."""
        ch = None
        if self.chroma:
            ch = dict(fenc=cur.c, recon=recon_c, stride=cur.stride_c, org=cur.org_c, qp=self.qp_c, levels=self.levels_c, num_sig=self.num_sig_c,
                      dist=self.dist_c)
        hipabi.intra_picture(self.depth, self.w64, self.h64, self.level, self.qp, self.flags, self.lambda8, self.mode_bits, cur.t, cur.stride, cur.org,
                             recon_plane, self.mode, self.levels, self.num_sig, self.dist, chroma=ch, cost=self.cost,
                             strong_intra_smoothing=self.strong, stream=stream, qp_map=self.qp_map, lambda8_by_qp=self.lambda8_by_qp)

    def checksum(self):
        out = {"mode": _sum64(self.mode), "levels": _sum64(self.levels), "num_sig": int(self.num_sig.sum().item()), "dist": int(self.dist.sum().item())}
        if self.chroma:
            for i in range(2):
                out["levels_c%d" % i] = _sum64(self.levels_c[i])
                out["num_sig_c%d" % i] = int(self.num_sig_c[i].sum().item())
        return out


class IFramePipeline(_PictureStep):
    """One I picture on the device: intra picture (IntraPicture: mode decision + coding, luma and 4:2:0 chroma) -> boundary strengths of
    an all-intra picture + luma / chroma deblocking -> SAO (statistics, x265hip_sao_rdo or the distortion-only stand-in, application)
    -> border extension.  The constructor switches mean what they mean in BFramePipeline; X265HIP_TU_INTRA_SLICE is always set.
    final_planes() are the coded picture - the first reference of a GOP (MiniGop's i_step).  Every buffer is allocated in the constructor: run()
    only launches, so it can be captured into a graph without a warm-up."""

    def __init__(self, w64, h64, depth, device, level=2, qp=27, deblock=False, sao=False, chroma=False, sao_apply=False, sign_hide=False,
                 sao_rdo=None, lambda8=1024, mode_bits=(2, 3, 6), strong_intra_smoothing=True, want_cost=False):
        import torch
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        self.tu_flags = hipabi.TU_INTRA_SLICE | (hipabi.TU_SIGN_HIDE if sign_hide else 0)
        qpc = chroma_quant_qp(qp, depth)
        self.ip = IntraPicture(self.nctu, w64, h64, depth, level, qp, device, flags=self.tu_flags, chroma=chroma, qp_c=(qpc, qpc), lambda8=lambda8,
                               mode_bits=mode_bits, strong_intra_smoothing=strong_intra_smoothing, want_cost=want_cost)
        if self.db is not None:
            self.db.prepare_intra()
        # the planes of the picture (PicYuv geometry of a DevicePicture), allocated here: run() allocates nothing and can be captured without a warm-up
        from . import frames as F
        _, _, stride, rows, _ = F.padded_dims(w64, h64)
        dt = torch.uint8 if depth == 8 else torch.int16
        nc = (h64 // 2 + 2 * F.CHROMA_MARGIN_Y) * (w64 // 2 + 2 * F.CHROMA_MARGIN_X)

        def planes():
            return torch.zeros((rows, stride), dtype=dt, device=device), ([torch.zeros(nc, dtype=dt, device=device) for _ in range(2)] if chroma else None)
        self.recon, self.recon_c = planes()
        self.out, self.out_c = planes() if self.sao_apply else (None, None)

    def set_qp_maps(self, maps, lambda8_by_qp=None):
        """Per-block QPs for the following run() calls (see FramePipeline.set_qp_maps); None = the picture-wide qp again.  lambda8_by_qp: device
        int32 tensor [52 + 6 (depth - 8)] - 256 x lambda of a CU per luma quantiser QP - or None = the constructor's lambda8 for every block."""
        self._set_qp_maps(maps, self.ip, [])
        self.ip.qp_map = None if maps is None else maps.tu_qp
        self.ip.lambda8_by_qp = None if maps is None else lambda8_by_qp

    def run(self, cur: DevicePicture, mark=None):
        """Returns the luma plane of the coded picture; mark(name), if given, is called after every stage."""
        mark = mark or (lambda name: None)
        self._qp_maps_run_check()
        assert cur.t.shape == self.recon.shape and cur.t.dtype == self.recon.dtype
        self.ip.run(cur, self.recon, self.recon_c)
        mark("intra")
        if self.db is not None:
            self.db.run_intra(self.recon, cur, self.ip.num_sig)
        return self._filter_tail(cur, mark)

    def checksum(self):
        out = self.ip.checksum()
        out["recon"] = _sum64(self.final)
        return out


class InterSa8dCost:
    """The inter candidate's cost per block of a P picture (x265hip_inter_sa8d_cost; reference Analysis::checkInter_rd0_4 at RD level <= 2,
    analysis.cpp:3023-3071): sa8d of the luma prediction at the block's vector + the rate of base_bits and the vector.  Owns cost int32
    [ctu][blocks][2] = {sa8d, cost} and the float bit-size table (BitCost::s_bitsizes) sized from the search range."""

    def __init__(self, nctu, w64, h64, depth, level, device, rng=57, base_bits=2, lambda8=1024, qp=0):
        """base_bits: m_listSelBits[0] of a P 2Nx2N + MVP_IDX_BITS + getTUBits(0, 1) = hipabi.ref_cost_bits(1, lam=1)[0] = 2 for one
        reference.  rng: the search range in full samples; a longer vector is priced with the table's last entry."""
        import torch
        self.nctu, self.w64, self.h64, self.depth, self.level, self.qp = nctu, w64, h64, depth, level, qp
        self.base_bits, self.lambda8 = int(base_bits), int(lambda8)
        self.nblk = (64 >> (3 + level)) ** 2
        self.cost = torch.zeros(nctu * self.nblk * 2, dtype=torch.int32, device=device)
        self.bit_sizes = torch.from_numpy(hipabi.mv_bit_sizes(4 * int(rng) + 4)).to(device)
        # per-block lambda: qp_map = the LUMA plane of CuQpMaps.tu_qp, lambda8_by_qp = device int32 [52 + 6 (depth - 8)] (None = lambda8)
        self.qp_map, self.lambda8_by_qp = None, None

    def run(self, cur: DevicePicture, ref: DevicePicture, mv, stream=None):
        hipabi.inter_sa8d_cost(self.depth, self.w64, self.h64, self.level, cur.t, cur.stride, cur.org, ref.t, ref.stride, ref.org, mv, self.base_bits,
                               self.lambda8, self.bit_sizes, self.cost, qp=self.qp, qp_map=self.qp_map, lambda8_by_qp=self.lambda8_by_qp, stream=stream)

    def checksum(self):
        return {"inter_cost": _sum64(self.cost)}


class IntraInInter:
    """The intra candidates of a P picture's blocks (x265hip_intra_in_inter; reference Search::checkIntraInInter and the choice of
    Analysis::compressInterCU_rd0_4, analysis.cpp:1649-1671): per block, in coding order, the 35-mode sa8d decision from the reconstruction
    around it; where the intra cost is strictly below the inter candidate's the block is recoded as intra IN the inter stages' outputs.
    Owns mode uint8 and intra uint8 [ctu][blocks] (and, with want_cost, the intra candidates' cost int32 [ctu][blocks][2]); levels /
    num_sig / dist and the recon planes belong to the inter TU stages it is run behind."""

    def __init__(self, nctu, w64, h64, depth, level, qp, device, flags=0, chroma=False, qp_c=None, lambda8=1024, mode_bits=(2, 3, 6),
                 strong_intra_smoothing=True, want_cost=False):
        import torch
        if flags & hipabi.TU_INTRA_SLICE:
            raise ValueError("IntraInInter: TU_INTRA_SLICE in the flags of a P slice")
        self.nctu, self.w64, self.h64, self.depth, self.level, self.qp, self.flags = nctu, w64, h64, depth, level, qp, flags
        self.chroma, self.qp_c = chroma, (qp_c if qp_c is not None else (qp, qp))
        self.lambda8, self.mode_bits, self.strong = int(lambda8), tuple(int(b) for b in mode_bits), bool(strong_intra_smoothing)
        self.n = 8 << level
        self.nblk = (64 // self.n) ** 2
        self.waves = hipabi.intra_picture_waves(w64, h64)
        nb = nctu * self.nblk
        self.mode = torch.zeros(nb, dtype=torch.uint8, device=device)
        self.intra = torch.zeros(nb, dtype=torch.uint8, device=device)
        self.cost = torch.zeros(nb * 2, dtype=torch.int32, device=device) if want_cost else None
        self.qp_map, self.lambda8_by_qp = None, None          # as IntraPicture's

    def run(self, cur: DevicePicture, recon_plane, rc, inter_cost, recon_c=None, rc_c=None, stream=None, inter_cost_stride=2, inter_cost_offset=1):
        """recon_plane (and recon_c = [Cb, Cr]): the inter reconstruction, rc (and rc_c = [Cb, Cr]): the inter TU stages whose levels / num_sig /
        dist the intra winners overwrite; inter_cost: InterSa8dCost.cost (the pairs; the defaults read their cost word), or BSa8dDecide.cost
        with inter_cost_stride = 4, inter_cost_offset = 0."""
        ch = None
        if self.chroma:
            ch = dict(fenc=cur.c, recon=recon_c, stride=cur.stride_c, org=cur.org_c, qp=self.qp_c, levels=[r.levels for r in rc_c],
                      num_sig=[r.num_sig for r in rc_c], dist=[r.dist for r in rc_c])
        hipabi.intra_in_inter(self.depth, self.w64, self.h64, self.level, self.qp, self.flags, self.lambda8, self.mode_bits, cur.t, cur.stride, cur.org,
                              recon_plane, self.mode, rc.levels, rc.num_sig, rc.dist, inter_cost, self.intra, inter_cost_stride=inter_cost_stride,
                              inter_cost_offset=inter_cost_offset, chroma=ch, cost=self.cost,
                              strong_intra_smoothing=self.strong, stream=stream, qp_map=self.qp_map, lambda8_by_qp=self.lambda8_by_qp)

    def checksum(self):
        return {"mode": _sum64(self.mode), "intra": _sum64(self.intra)}


class _Sa8dPStep(_PictureStep):
    """What the P steps with an sa8d decision share: search -> sub-pel refinement, the inter TU stages (luma + chroma pair) and InterSa8dCost.
    A step adds its decision stage and orders coding and deciding in run()."""

    def __init__(self, w64, h64, depth, device, rng, subme, level, qp, deblock, sao, chroma, sao_apply, sign_hide, sao_rdo, lambda8, base_bits):
        from .pipeline import MotionSearch, SubpelRefine
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        self.tu_flags = hipabi.TU_SIGN_HIDE if sign_hide else 0
        self.ms = MotionSearch(w64, h64, rng, depth, device, want_surf=False, want_best=True)
        self.sp = SubpelRefine(self.ms, subme, device)
        self.rc = InterRecon(self.nctu, w64, h64, depth, level, qp, device, intra_slice=self.tu_flags)
        if chroma:
            qpc = chroma_quant_qp(qp, depth)
            self.rc_c = [InterReconChroma(self.nctu, w64, h64, depth, level, qpc, device, intra_slice=self.tu_flags) for _ in range(2)]
        self.ic = InterSa8dCost(self.nctu, w64, h64, depth, level, device, rng=rng, base_bits=base_bits, lambda8=lambda8, qp=qp)

    def _search(self, cur, ref, mark):
        """The head of run(): checks, planes, search and sub-pel refinement; returns the refined records."""
        self._qp_maps_run_check()
        self._alloc_planes(cur)
        self.ms.reset()
        self.ms.search(cur, ref)
        mark("me")
        self.sp.run(cur, ref)
        mark("subpel")
        return self.sp.out

    def _code(self, cur, ref, mv, mark):
        """The inter TU stages on the records mv: luma, then the chroma pair."""
        self.rc.run(cur, ref, self.recon, mv)
        mark("recon")
        if self.chroma:
            InterReconChroma.run_pair(self.rc_c, cur.c, ref.c, self.recon_c, cur.stride_c, cur.org_c, mv)
            mark("recon_chroma")

    def _checksum(self, decision, **more):
        out = {}
        for st in (self.ms, self.sp, self.ic, decision, self.rc):
            out.update(st.checksum())
        out.update(more, recon=_sum64(self.final))
        return out


class IntraPFramePipeline(_Sa8dPStep):
    """One P picture whose blocks may be intra: search -> sub-pel refinement -> inter TU stage (luma + chroma) -> InterSa8dCost ->
    IntraInInter -> boundary strengths with the intra flags + luma / chroma deblocking -> the shared loop-filter tail.  Inter
    reconstruction does not depend on neighbours, so coding every block as inter first and overwriting the intra winners in coding order
    is the reference's result.  run(cur, ref) / final_planes() as FramePipeline's: MiniGop(p_step=...) takes it.
    The constructor switches mean what they mean in BFramePipeline / IFramePipeline; base_bits: see InterSa8dCost."""

    def __init__(self, w64, h64, depth, device, rng=57, subme=2, level=2, qp=27, deblock=False, sao=False, chroma=False, sao_apply=False,
                 sign_hide=False, sao_rdo=None, lambda8=1024, mode_bits=(2, 3, 6), strong_intra_smoothing=True, base_bits=2):
        _Sa8dPStep.__init__(self, w64, h64, depth, device, rng, subme, level, qp, deblock, sao, chroma, sao_apply, sign_hide, sao_rdo, lambda8, base_bits)
        qpc = chroma_quant_qp(qp, depth)
        self.ii = IntraInInter(self.nctu, w64, h64, depth, level, qp, device, flags=self.tu_flags, chroma=chroma, qp_c=(qpc, qpc), lambda8=lambda8,
                               mode_bits=mode_bits, strong_intra_smoothing=strong_intra_smoothing)

    def set_qp_maps(self, maps, lambda8_by_qp=None):
        """Per-block QPs for the following run() calls (see FramePipeline.set_qp_maps); None = the picture-wide qp again.  lambda8_by_qp
        prices both candidates' rate terms per block (see _set_decision_qp_maps)."""
        self._set_decision_qp_maps(maps, lambda8_by_qp, [self.ic], [self.ii])

    def run(self, cur: DevicePicture, ref: DevicePicture, mark=None):
        """ref: the reference picture (extended borders, with chroma its Cb / Cr planes); returns the luma plane of the coded picture.
        mark(name), if given, is called after every stage."""
        mark = mark or (lambda name: None)
        mv = self._search(cur, ref, mark)
        self._code(cur, ref, mv, mark)
        self.ic.run(cur, ref, mv)
        mark("inter_cost")
        self.ii.run(cur, self.recon, self.rc, self.ic.cost, self.recon_c, self.rc_c if self.chroma else None)
        mark("intra")
        if self.db is not None:
            self.db.run(self.recon, cur, mv, self.rc.num_sig, intra=self.ii.intra)
        return self._filter_tail(cur, mark)

    def checksum(self):
        return self._checksum(self.ii)


class ColField:
    """The collocated motion field of a coded picture (x265hip_col_field_build; what CUData::getColMVP, cudata.cpp:1968-2000, can see of
    it): one entry per 16x16 luma unit.  Owns col_mv int32 and col_delta int16 [ctu][16]; a col_delta of 0 is "no motion here", so a new
    field is the field of an I picture.  Only list 0 of the picture is modelled: collocated pictures here are P or I anchors."""

    def __init__(self, nctu, w64, h64, depth, device):
        import torch
        self.nctu, self.w64, self.h64, self.depth = nctu, w64, h64, depth
        self.col_mv = torch.zeros(nctu * 16, dtype=torch.int32, device=device)
        self.col_delta = torch.zeros(nctu * 16, dtype=torch.int16, device=device)

    def build(self, mv_out, level, poc_delta, intra=None, ref_idx=None, stream=None):
        """mv_out: the picture's final motion (MergeDecide.mv_out-style records); poc_delta: colPOC - colRefPOC, one int or one per
        reference index; intra uint8 / ref_idx int8 [ctu][blocks], optional."""
        hipabi.col_field_build(self.depth, self.w64, self.h64, level, mv_out, poc_delta, self.col_mv, self.col_delta, intra=intra, ref_idx=ref_idx,
                               stream=stream)
        return self

    def clear(self):
        """The field of a picture without motion (an I picture, or an anchor taken as it is)."""
        self.col_mv.zero_()
        self.col_delta.zero_()
        return self

    def checksum(self):
        return {"col_mv": _sum64(self.col_mv), "col_delta": _sum64(self.col_delta)}


class _MergeStage:
    """What MergeDecide and BMergeDecide share: the operating point, the grid, merge / merge_idx uint8 [ctu][blocks], cost and best int32
    [ctu][blocks][2], the optional per-block QP inputs and the skip flags."""

    def __init__(self, nctu, w64, h64, depth, level, device, max_merge, lambda8, qp):
        import torch
        if not 1 <= int(max_merge) <= 5:
            raise ValueError("%s: max_merge %r outside 1..5" % (type(self).__name__, max_merge))
        self.nctu, self.w64, self.h64, self.depth, self.level, self.qp = nctu, w64, h64, depth, level, qp
        self.max_merge, self.lambda8 = int(max_merge), int(lambda8)
        self.nblk = (64 >> (3 + level)) ** 2
        self.waves = hipabi.intra_picture_waves(w64, h64)
        nb = nctu * self.nblk
        self.merge = torch.zeros(nb, dtype=torch.uint8, device=device)
        self.merge_idx = torch.zeros(nb, dtype=torch.uint8, device=device)
        self.cost = torch.zeros(nb * 2, dtype=torch.int32, device=device)
        self.best = torch.zeros(nb * 2, dtype=torch.int32, device=device)
        self.qp_map, self.lambda8_by_qp = None, None          # as InterSa8dCost's

    def _records(self, count, device):
        import torch
        return (torch.zeros(self.nctu * PUS_PER_CTU * 2, dtype=torch.int32, device=device) for _ in range(count))

    def skip_flags(self, rc, rc_c=None):
        """uint8 [ctu][blocks]: a merged block none of whose planes has a coded coefficient (encodeResidue sets MODE_SKIP there,
        analysis.cpp:3358-3359).  rc (and rc_c = [Cb, Cr]): the TU stages that coded the picture from mv_pred."""
        import torch
        skip = (self.merge != 0) & (rc.num_sig == 0)
        for r in (rc_c or ()):
            skip = skip & (r.num_sig == 0)
        return skip.to(torch.uint8)


class MergeDecide(_MergeStage):
    """The merge arm of a P picture's sa8d choice (x265hip_merge_decide; reference Analysis::checkMerge2Nx2N_rd0_4 at RD level 0,
    analysis.cpp:2787-2838, CUData::getInterMergeCandidates, cudata.cpp:1458-1712, and the comparison of compressInterCU_rd0_4,
    analysis.cpp:1650): per block, in coding order, the candidates its neighbours' final motion gives, priced by sa8d; the block merges
    unless its inter candidate is strictly cheaper.  Owns merge / merge_idx uint8 [ctu][blocks], mv_out (the CUs' motion, unclipped) and
    mv_pred (what the TU stages predict from) int32 [ctu*85][2], cost and best int32 [ctu][blocks][2]."""

    def __init__(self, nctu, w64, h64, depth, level, device, max_merge=3, lambda8=1024, qp=0, amvp=False, base_bits=2, rng=57):
        """amvp: the inter candidate is priced against its AMVP predictor (x265hip_merge_decide_amvp; CUData::getPMV, Search::selectMVP,
        Search::checkBestMVP).  The stage then also owns mvp_idx uint8 [ctu][blocks], mvd, amvp and inter int32
        [ctu][blocks][2] and the float bit-size table of 2 * BC_MAX_MV + 1 = 65537 entries, which holds every difference of two vectors
        (rng, the search range, does not bound the table: a predictor may lie anywhere).  base_bits: see InterSa8dCost."""
        import torch
        _MergeStage.__init__(self, nctu, w64, h64, depth, level, device, max_merge, lambda8, qp)
        self.mv_out, self.mv_pred = self._records(2, device)
        self.amvp_on, self.base_bits, self.rng = bool(amvp), int(base_bits), int(rng)
        if self.amvp_on:
            nb = nctu * self.nblk
            self.mvp_idx = torch.zeros(nb, dtype=torch.uint8, device=device)
            self.mvd, self.amvp, self.inter = (torch.zeros(nb * 2, dtype=torch.int32, device=device) for _ in range(3))
            self.bit_sizes = torch.from_numpy(hipabi.mv_bit_sizes(65537)).to(device)

    def run(self, cur: DevicePicture, ref: DevicePicture, mv, inter_cost=None, stream=None, inter_cost_stride=2, inter_cost_offset=1, col=None, cur_delta=None,
            inter_sa8d=None, inter_sa8d_stride=2, inter_sa8d_offset=0):
        """mv: the searched records; inter_cost: InterSa8dCost.cost (the pairs; the defaults read their cost word).  col: a ColField of
        the collocated picture - the list then has the temporal candidate (x265hip_merge_decide_col) - with cur_delta = curPOC - refPOC.
        A stage built with amvp takes inter_sa8d instead of inter_cost: InterSa8dCost.cost again (the defaults read the sa8d word)."""
        if col is not None and cur_delta is None:
            raise ValueError("MergeDecide.run: a collocated field needs cur_delta")
        if self.amvp_on != (inter_sa8d is not None) or self.amvp_on != (inter_cost is None):
            raise ValueError("MergeDecide.run: inter_sa8d goes with amvp=True, inter_cost with amvp=False")
        if self.amvp_on:
            hipabi.merge_decide_amvp(self.depth, self.w64, self.h64, self.level, cur.t, cur.stride, cur.org, ref.t, ref.stride, ref.org, mv, inter_sa8d,
                                     self.base_bits, self.bit_sizes, self.lambda8, self.max_merge, self.merge, self.merge_idx, self.mv_out, self.mv_pred,
                                     self.cost, self.mvp_idx, self.mvd, self.inter, amvp=self.amvp, col_mv=None if col is None else col.col_mv,
                                     col_delta=None if col is None else col.col_delta, cur_delta=1 if cur_delta is None else cur_delta, best=self.best,
                                     inter_sa8d_stride=inter_sa8d_stride, inter_sa8d_offset=inter_sa8d_offset, qp=self.qp, qp_map=self.qp_map,
                                     lambda8_by_qp=self.lambda8_by_qp, stream=stream)
            return
        args = (self.depth, self.w64, self.h64, self.level, cur.t, cur.stride, cur.org, ref.t, ref.stride, ref.org, mv, inter_cost, self.lambda8,
                self.max_merge, self.merge, self.merge_idx, self.mv_out, self.mv_pred, self.cost)
        kw = dict(best=self.best, inter_cost_stride=inter_cost_stride, inter_cost_offset=inter_cost_offset, qp=self.qp, qp_map=self.qp_map,
                  lambda8_by_qp=self.lambda8_by_qp, stream=stream)
        if col is None:
            hipabi.merge_decide(*args, **kw)
        else:
            hipabi.merge_decide_col(*args, col.col_mv, col.col_delta, cur_delta, **kw)

    def checksum(self):
        out = {"merge": _sum64(self.merge), "merge_idx": _sum64(self.merge_idx), "mv_out": _sum64(self.mv_out), "mv_pred": _sum64(self.mv_pred),
               "merge_cost": _sum64(self.cost)}
        if self.amvp_on:
            out.update(mvp_idx=_sum64(self.mvp_idx), mvd=_sum64(self.mvd), amvp=_sum64(self.amvp), inter=_sum64(self.inter))
        return out


class MergePFramePipeline(_Sa8dPStep):
    """One P picture whose blocks may merge: search -> sub-pel refinement -> InterSa8dCost on the searched vectors -> MergeDecide -> inter TU
    stage (luma + chroma) on mv_pred -> skip flags -> boundary strengths from mv_out + luma / chroma deblocking -> the shared loop-filter
    tail.  The candidate list reads motion only, so one walk in coding order before the coding is the reference's result (DESIGN.md
    section 19).  run(cur, ref) / final_planes() as FramePipeline's: MiniGop(p_step=...) takes it.  The constructor switches mean what they
    mean in IntraPFramePipeline; max_merge: --max-merge (the reference's default 3, param.cpp:199)."""

    def __init__(self, w64, h64, depth, device, rng=57, subme=2, level=2, qp=27, deblock=False, sao=False, chroma=False, sao_apply=False,
                 sign_hide=False, sao_rdo=None, lambda8=1024, base_bits=2, max_merge=3, temporal_mvp=False, amvp=False):
        _Sa8dPStep.__init__(self, w64, h64, depth, device, rng, subme, level, qp, deblock, sao, chroma, sao_apply, sign_hide, sao_rdo, lambda8, base_bits)
        # amvp: the walk prices the inter candidate against its AMVP predictor and puts out mvp_idx / mvd; with
        # temporal_mvp the predictor list has the temporal candidate too, without it neither list has
        self.amvp = bool(amvp)
        self.md = MergeDecide(self.nctu, w64, h64, depth, level, device, max_merge=max_merge, lambda8=lambda8, qp=qp, amvp=self.amvp, base_bits=base_bits, rng=rng)
        self.skip = None
        # temporal_mvp: the merge list has the temporal candidate; self.col is then this picture's own field
        self.temporal_mvp = bool(temporal_mvp)
        self.col = ColField(self.nctu, w64, h64, depth, device) if self.temporal_mvp else None

    def set_qp_maps(self, maps, lambda8_by_qp=None):
        """As IntraPFramePipeline.set_qp_maps: the maps reach the TU stages, the deblocking stage and both candidates' rate terms."""
        self._set_decision_qp_maps(maps, lambda8_by_qp, [self.ic, self.md], [])

    def run(self, cur: DevicePicture, ref: DevicePicture, mark=None, col=None, cur_delta=None):
        """ref: the reference picture (extended borders, with chroma its Cb / Cr planes); returns the luma plane of the coded picture.
        mark(name), if given, is called after every stage.  With temporal_mvp: col = the ColField of the collocated picture (the
        reference; None = a picture without motion) and cur_delta = curPOC - refPOC; after the walk self.col is this picture's field."""
        mark = mark or (lambda name: None)
        self._temporal_mvp_run_check(col, "cur_delta", cur_delta)
        mv = self._search(cur, ref, mark)
        self.ic.run(cur, ref, mv)
        mark("inter_cost")
        cost = dict(inter_sa8d=self.ic.cost) if self.amvp else dict(inter_cost=self.ic.cost)      # the pairs: the walk reads word 0 / word 1
        if self.temporal_mvp:
            if col is self.col:
                raise ValueError("MergePFramePipeline.run: col is this step's own field, which the run overwrites: hand a copy")
            self.md.run(cur, ref, mv, col=col if col is not None else self.col.clear(), cur_delta=cur_delta, **cost)
            self.col.build(self.md.mv_out, self.md.level, cur_delta)
        else:
            self.md.run(cur, ref, mv, **cost)
        mark("merge")
        self._code(cur, ref, self.md.mv_pred, mark)
        self.skip = self.md.skip_flags(self.rc, self.rc_c if self.chroma else None)
        mark("skip")
        if self.db is not None:
            self.db.run(self.recon, cur, self.md.mv_out, self.rc.num_sig)
        return self._filter_tail(cur, mark)

    def checksum(self):
        return self._checksum(self.md, skip=_sum64(self.skip))


class BSa8dDecide:
    """The sa8d choice of a B picture's blocks between the cheaper single list and both (x265hip_b_sa8d_decide; reference
    Analysis::compressInterCU_rd0_4 with checkInter_rd0_4 and checkBidir2Nx2N, analysis.cpp:1649-1655, 3059-3071, 3145-3270).  Owns what
    BidirDecide owns - dir uint8, ref0 / ref1 int8 [ctu][blocks], mv0_out / mv1_out int32 [ctu*85][2] - plus cost int32 [ctu][blocks][4] =
    {winning inter sa8d cost, single list, both lists after the zero pair, flags} and the float bit-size table sized from the search range."""

    def __init__(self, nctu, w64, h64, depth, level, device, dir_cost=(12, 12, 20), ref_ids=(0, 1), rng=57, base_bits=None, bi_bits_delta=None,
                 lambda8=1024, qp=0):
        """dir_cost: what the two records' costs are compared with, as in BidirDecide.  base_bits / bi_bits_delta: hipabi.b_sa8d_bits() -
        (4, 4) and -1 for one reference per list - where None."""
        import torch
        self.nctu, self.w64, self.h64, self.depth, self.level, self.qp = nctu, w64, h64, depth, level, qp
        self.nblk = (64 >> (3 + level)) ** 2
        self.dir_cost, self.ref_ids, self.lambda8 = tuple(int(c) for c in dir_cost), tuple(ref_ids), int(lambda8)
        bb, delta = hipabi.b_sa8d_bits()
        self.base_bits = bb if base_bits is None else tuple(int(b) for b in base_bits)
        self.bi_bits_delta = delta if bi_bits_delta is None else int(bi_bits_delta)
        self.dir = torch.zeros(nctu * self.nblk, dtype=torch.uint8, device=device)
        self.ref0 = torch.zeros(nctu * self.nblk, dtype=torch.int8, device=device)
        self.ref1 = torch.zeros(nctu * self.nblk, dtype=torch.int8, device=device)
        self.mv0_out = torch.zeros(nctu * PUS_PER_CTU * 2, dtype=torch.int32, device=device)
        self.mv1_out = torch.zeros(nctu * PUS_PER_CTU * 2, dtype=torch.int32, device=device)
        self.cost = torch.zeros(nctu * self.nblk * 4, dtype=torch.int32, device=device)
        self.bit_sizes = torch.from_numpy(hipabi.mv_bit_sizes(4 * int(rng) + 4)).to(device)
        self.qp_map, self.lambda8_by_qp = None, None          # as InterSa8dCost's

    def run(self, cur: DevicePicture, ref0: DevicePicture, ref1: DevicePicture, mv0, mv1, stream=None):
        """mv0 / mv1: the two SubpelRefine outputs."""
        assert ref0.stride == ref1.stride and ref0.org == ref1.org
        hipabi.b_sa8d_decide(self.depth, self.w64, self.h64, self.level, cur.t, cur.stride, ref0.t, ref1.t, ref0.stride, mv0, mv1, self.dir_cost,
                             self.base_bits, self.bi_bits_delta, self.lambda8, self.bit_sizes, self.dir, self.mv0_out, self.mv1_out, self.cost,
                             ref0=self.ref0, ref1=self.ref1, ref_ids=self.ref_ids, fenc_off=cur.org, fref_off=ref0.org, qp=self.qp, qp_map=self.qp_map,
                             lambda8_by_qp=self.lambda8_by_qp, stream=stream)

    def checksum(self):
        return {"dir": _sum64(self.dir), "mv0_out": _sum64(self.mv0_out), "mv1_out": _sum64(self.mv1_out), "b_cost": _sum64(self.cost)}


class Sa8dBFramePipeline(_RefListStep):
    """One B picture whose decision is the reference's own for the 2Nx2N CUs this pipeline codes: per list search -> sub-pel refinement;
    BSa8dDecide; bi-predictive luma + 4:2:0 chroma reconstruction; with b_intra (--b-intra, bIntraInBFrames) IntraInInter against word 0 of
    the decision's cost, with the B slice's flags; B-picture boundary strengths with the intra flags + luma / chroma deblocking; the shared
    loop-filter tail.  Overwriting the intra winners in coding order is the reference's result as in IntraPFramePipeline: an inter block's
    reconstruction never depends on a neighbour, whichever lists it uses.  run(cur, ref0, ref1) / final_planes() as
    BFramePipeline's: MiniGop(b_step=...) takes it.  The constructor switches mean what they mean in BFramePipeline / IntraPFramePipeline."""

    def __init__(self, w64, h64, depth, device, rng=57, subme=2, level=2, qp=27, deblock=False, sao=False, chroma=False, sao_apply=False,
                 sign_hide=False, sao_rdo=None, dir_cost=(12, 12, 20), b_intra=False, lambda8=1024, mode_bits=(2, 3, 6), strong_intra_smoothing=True,
                 base_bits=None, bi_bits_delta=None):
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        self._build_lists(2, w64, h64, depth, device, rng, subme, False, False)
        self.bd = BSa8dDecide(self.nctu, w64, h64, depth, level, device, dir_cost=dir_cost, rng=rng, base_bits=base_bits, bi_bits_delta=bi_bits_delta,
                              lambda8=lambda8, qp=qp)
        self.tu_flags = hipabi.TU_SIGN_HIDE if sign_hide else 0
        self.rc = InterReconBi(self.nctu, w64, h64, depth, level, qp, device, intra_slice=self.tu_flags)
        qpc = chroma_quant_qp(qp, depth)
        if chroma:
            self.rc_c = [InterReconChromaBi(self.nctu, w64, h64, depth, level, qpc, device, intra_slice=self.tu_flags) for _ in range(2)]
        self.b_intra = bool(b_intra)
        self.ii = IntraInInter(self.nctu, w64, h64, depth, level, qp, device, flags=self.tu_flags, chroma=chroma, qp_c=(qpc, qpc), lambda8=lambda8,
                               mode_bits=mode_bits, strong_intra_smoothing=strong_intra_smoothing) if b_intra else None

    def set_qp_maps(self, maps, lambda8_by_qp=None):
        """As IntraPFramePipeline.set_qp_maps: the maps reach the TU stages, the deblocking stage, the decision and (with b_intra) the intra
        walk; lambda8_by_qp prices the rate terms of all candidates per block."""
        self._set_decision_qp_maps(maps, lambda8_by_qp, [self.bd], [] if self.ii is None else [self.ii])

    def run(self, cur: DevicePicture, ref0: DevicePicture, ref1: DevicePicture, mark=None):
        """ref0 / ref1: the list-0 / list-1 reference pictures (extended borders; with chroma=True also their Cb / Cr planes).  Returns the
        luma plane of the coded picture; mark(name), if given, is called after every stage."""
        self._qp_maps_run_check()
        mark = mark or (lambda name: None)
        self._alloc_planes(cur)
        self._search_lists(cur, (ref0, ref1), mark)
        self.bd.run(cur, ref0, ref1, self.spl[0].out, self.spl[1].out)
        mark("b_sa8d")
        mv0, mv1, dirs = self.bd.mv0_out, self.bd.mv1_out, self.bd.dir
        self.rc.run(cur, ref0, ref1, self.recon, mv0, mv1, dir_flags=dirs)
        mark("recon")
        if self.chroma:
            for i in range(2):
                self.rc_c[i].run(cur.c[i], ref0.c[i], ref1.c[i], self.recon_c[i], cur.stride_c, cur.org_c, mv0, mv1, dir_flags=dirs)
            mark("recon_chroma")
        if self.ii is not None:
            self.ii.run(cur, self.recon, self.rc, self.bd.cost, self.recon_c, self.rc_c if self.chroma else None, inter_cost_stride=4, inter_cost_offset=0)
            mark("intra")
        if self.db is not None:
            self.db.run_b(self.recon, cur, mv0, mv1, self.bd.ref0, self.bd.ref1, self.rc.num_sig, intra=None if self.ii is None else self.ii.intra)
        return self._filter_tail(cur, mark)

    def checksum(self):
        out = self._checksum(self.bd)
        if self.ii is not None:
            out.update(self.ii.checksum())
        return out


class BMergeDecide(_MergeStage):
    """The merge arm of a B picture's sa8d choice (x265hip_b_merge_decide; reference Analysis::checkMerge2Nx2N_rd0_4 at RD level 0,
    analysis.cpp:2787-2838, CUData::getInterMergeCandidates with isInterB, cudata.cpp:1458-1712, and the comparisons of
    compressInterCU_rd0_4, analysis.cpp:1650-1655): per block, in coding order, the two-list candidates its neighbours' final motion gives
    - spatial, combined bi-predictive, zero -, priced by sa8d; the block merges unless its inter winner is strictly cheaper.  Owns merge /
    merge_idx / dir uint8 and ref0 / ref1 int8 [ctu][blocks], mv0_out / mv1_out (the CUs' motion, unclipped) and mv0_pred / mv1_pred (what
    the two-list TU stages predict from, with dir) int32 [ctu*85][2], cost and best int32 [ctu][blocks][2]."""

    def __init__(self, nctu, w64, h64, depth, level, device, max_merge=3, lambda8=1024, qp=0, ref_ids=(0, 1)):
        import torch
        _MergeStage.__init__(self, nctu, w64, h64, depth, level, device, max_merge, lambda8, qp)
        self.ref_ids = tuple(ref_ids)
        nb = nctu * self.nblk
        self.dir = torch.zeros(nb, dtype=torch.uint8, device=device)
        self.ref0 = torch.zeros(nb, dtype=torch.int8, device=device)
        self.ref1 = torch.zeros(nb, dtype=torch.int8, device=device)
        self.mv0_out, self.mv1_out, self.mv0_pred, self.mv1_pred = self._records(4, device)

    def run(self, cur: DevicePicture, ref0: DevicePicture, ref1: DevicePicture, dir_in, mv0, mv1, inter_cost, stream=None, inter_cost_stride=4,
            inter_cost_offset=0, col=None, cur_deltas=None):
        """dir_in / mv0 / mv1: the inter winner (BSa8dDecide.dir / mv0_out / mv1_out); inter_cost: BSa8dDecide.cost (the defaults read its
        word 0).  col: the ColField of the collocated picture (L1[0]) - the list then has the temporal candidate
        (x265hip_b_merge_decide_col) - with cur_deltas = (curPOC - POC(L0[0]), curPOC - POC(L1[0]))."""
        assert ref0.stride == ref1.stride and ref0.org == ref1.org
        if col is not None and cur_deltas is None:
            raise ValueError("BMergeDecide.run: a collocated field needs cur_deltas")
        args = (self.depth, self.w64, self.h64, self.level, cur.t, cur.stride, ref0.t, ref1.t, ref0.stride, dir_in, mv0, mv1, inter_cost, self.lambda8,
                self.max_merge, self.merge, self.merge_idx, self.dir, self.mv0_out, self.mv1_out, self.mv0_pred, self.mv1_pred, self.cost)
        kw = dict(best=self.best, ref0=self.ref0, ref1=self.ref1, ref_ids=self.ref_ids, fenc_off=cur.org, fref_off=ref0.org,
                  inter_cost_stride=inter_cost_stride, inter_cost_offset=inter_cost_offset, qp=self.qp, qp_map=self.qp_map,
                  lambda8_by_qp=self.lambda8_by_qp, stream=stream)
        if col is None:
            hipabi.b_merge_decide(*args, **kw)
        else:
            hipabi.b_merge_decide_col(*args, col.col_mv, col.col_delta, cur_deltas, **kw)

    def checksum(self):
        return {"merge": _sum64(self.merge), "merge_idx": _sum64(self.merge_idx), "merge_dir": _sum64(self.dir), "mv0_out": _sum64(self.mv0_out),
                "mv1_out": _sum64(self.mv1_out), "mv0_pred": _sum64(self.mv0_pred), "mv1_pred": _sum64(self.mv1_pred), "merge_cost": _sum64(self.cost)}


class MergeBFramePipeline(_RefListStep):
    """One B picture whose blocks may merge: per list search -> sub-pel refinement; BSa8dDecide (the inter winner); BMergeDecide against word
    0 of its cost; bi-predictive luma + 4:2:0 chroma coding from the merge stage's dir / mv0_pred / mv1_pred; skip flags; B-picture boundary
    strengths from mv0_out / mv1_out / ref0 / ref1 + luma / chroma deblocking; the shared loop-filter tail.  The candidate list reads motion
    only, so one walk in coding order before the coding is the reference's result for two lists as for one.
    run(cur, ref0, ref1) / final_planes() as BFramePipeline's: MiniGop(b_step=...) takes it.  The constructor switches mean what they mean in
    Sa8dBFramePipeline; max_merge: --max-merge.  b_intra is refused: the intra and merge decisions interleave in coding order (one walk, not
    built)."""

    def __init__(self, w64, h64, depth, device, rng=57, subme=2, level=2, qp=27, deblock=False, sao=False, chroma=False, sao_apply=False,
                 sign_hide=False, sao_rdo=None, dir_cost=(12, 12, 20), b_intra=False, lambda8=1024, base_bits=None, bi_bits_delta=None, max_merge=3,
                 temporal_mvp=False):
        self.temporal_mvp = bool(temporal_mvp)     # the merge list has the temporal candidate
        if b_intra:
            raise ValueError("MergeBFramePipeline: b_intra together with merge is one walk in coding order and is not built")
        _PictureStep.__init__(self, w64, h64, depth, level, qp, device, deblock, sao, chroma, sao_apply, sao_rdo)
        self._build_lists(2, w64, h64, depth, device, rng, subme, False, False)
        self.bd = BSa8dDecide(self.nctu, w64, h64, depth, level, device, dir_cost=dir_cost, rng=rng, base_bits=base_bits, bi_bits_delta=bi_bits_delta,
                              lambda8=lambda8, qp=qp)
        self.md = BMergeDecide(self.nctu, w64, h64, depth, level, device, max_merge=max_merge, lambda8=lambda8, qp=qp, ref_ids=self.bd.ref_ids)
        self.tu_flags = hipabi.TU_SIGN_HIDE if sign_hide else 0
        self.rc = InterReconBi(self.nctu, w64, h64, depth, level, qp, device, intra_slice=self.tu_flags)
        if chroma:
            qpc = chroma_quant_qp(qp, depth)
            self.rc_c = [InterReconChromaBi(self.nctu, w64, h64, depth, level, qpc, device, intra_slice=self.tu_flags) for _ in range(2)]
        self.skip = None

    def set_qp_maps(self, maps, lambda8_by_qp=None):
        """As Sa8dBFramePipeline.set_qp_maps: the maps reach the TU stages, the deblocking stage and the rate terms of the inter winner and
        of every merge candidate."""
        self._set_decision_qp_maps(maps, lambda8_by_qp, [self.bd, self.md], [])

    def run(self, cur: DevicePicture, ref0: DevicePicture, ref1: DevicePicture, mark=None, col=None, cur_deltas=None):
        """ref0 / ref1: the list-0 / list-1 reference pictures (extended borders; with chroma=True also their Cb / Cr planes).  Returns the
        luma plane of the coded picture; mark(name), if given, is called after every stage.  With temporal_mvp: col = the ColField of
        the collocated picture ref1 (None = a picture without motion: no temporal candidate) and cur_deltas = (curPOC - POC(ref0),
        curPOC - POC(ref1))."""
        self._temporal_mvp_run_check(col, "cur_deltas", cur_deltas)
        self._qp_maps_run_check()
        mark = mark or (lambda name: None)
        self._alloc_planes(cur)
        self._search_lists(cur, (ref0, ref1), mark)
        self.bd.run(cur, ref0, ref1, self.spl[0].out, self.spl[1].out)
        mark("b_sa8d")
        md = self.md
        md.run(cur, ref0, ref1, self.bd.dir, self.bd.mv0_out, self.bd.mv1_out, self.bd.cost, col=col, cur_deltas=cur_deltas if col is not None else None)
        mark("merge")
        self.rc.run(cur, ref0, ref1, self.recon, md.mv0_pred, md.mv1_pred, dir_flags=md.dir)
        mark("recon")
        if self.chroma:
            for i in range(2):
                self.rc_c[i].run(cur.c[i], ref0.c[i], ref1.c[i], self.recon_c[i], cur.stride_c, cur.org_c, md.mv0_pred, md.mv1_pred, dir_flags=md.dir)
            mark("recon_chroma")
        self.skip = md.skip_flags(self.rc, self.rc_c if self.chroma else None)
        mark("skip")
        if self.db is not None:
            self.db.run_b(self.recon, cur, md.mv0_out, md.mv1_out, md.ref0, md.ref1, self.rc.num_sig)
        return self._filter_tail(cur, mark)

    def checksum(self):
        out = self._checksum(self.bd)
        out.update(self.md.checksum())
        out["skip"] = _sum64(self.skip)
        return out


class MiniGop:
    """Display order in, coding order inside: anchor pictures 0, gop, 2 gop, ... form the P chain (each coded by p_step.run from the
    previous anchor's OUTPUT), and the pictures between two anchors are B pictures coded by b_step.run(cur, previous anchor, this
    anchor) once the later anchor is done.  B pictures are not referenced.  p_step: a FramePipeline, b_step: a BFramePipeline of the same
    geometry and chroma setting; i_step: an IFramePipeline of that geometry that codes picture 0, or None.
    p_refs > 1: p_step is a MultiRefFramePipeline and every anchor is coded by p_step.run(cur, [up to p_refs previous coded anchors,
    newest first]); B pictures keep using the two anchors around them unless
    b_refs = (n0, n1) != (1, 1): b_step is a MultiRefBFramePipeline and a B picture between two anchors is coded by b_step.run(cur, list 0,
    list 1) with list 0 = the coded anchors before it, newest first, [:n0], and list 1 = ([the later anchor] + those)[:n1] - HEVC's default
    list order, so with n1 > 1 a picture sits in both lists."""

    def __init__(self, p_step, b_step, gop, i_step=None, p_refs=1, b_refs=(1, 1), temporal_mvp=False):
        """temporal_mvp: p_step / b_step are a MergePFramePipeline / MergeBFramePipeline built with temporal_mvp=True; POC = display index.
        An anchor coded by i_step or taken as it is leaves a field without motion; a P anchor hands its own field (a copy) to the next
        anchor (cur_delta = gop) and to the B pictures before it (cur_deltas = (k - (a - gop), k - a))."""
        assert gop >= 1 and p_refs >= 1 and len(b_refs) == 2 and min(b_refs) >= 1
        self.p, self.b, self.gop, self.i, self.p_refs = p_step, b_step, int(gop), i_step, int(p_refs)
        self.b_refs = (int(b_refs[0]), int(b_refs[1]))
        self.temporal_mvp = bool(temporal_mvp)
        if self.temporal_mvp:
            if self.p_refs > 1 or self.b_refs != (1, 1):
                raise ValueError("MiniGop: temporal_mvp with several references per list (p_refs > 1 or b_refs != (1, 1)) is not built")
            for name, step in (("p_step", p_step), ("b_step", b_step)):
                if step is not None and not getattr(step, "temporal_mvp", False):
                    raise ValueError("MiniGop: temporal_mvp=True needs a %s built with temporal_mvp=True" % name)

    def run(self, pictures):
        """pictures: DevicePictures in display order; picture 0 is the first anchor - coded by i_step where there is one (its output is
        the first reference), otherwise taken as it is.  Pictures behind the last anchor are left out.  Returns (coding order as display
        indices, {display index: [Y, Cb, Cr] planes of the coded picture (clones)})."""
        def keep(planes):
            return [p.clone() for p in planes]
        prev = pictures[0]
        out, order = {0: keep(prev.planes())}, [0]
        if self.i is not None:
            self.i.run(pictures[0])
            out[0] = keep(self.i.final_planes())
            prev = pictures[0].like(out[0])
        anchors = [prev]                 # coded anchors, newest first (p_refs > 1)
        col = None                       # temporal_mvp: the previous anchor's collocated field (None: an anchor without motion)
        for a in range(self.gop, len(pictures), self.gop):
            if self.temporal_mvp:
                self.p.run(pictures[a], prev, col=col, cur_delta=self.gop)
                if col is None:
                    col = ColField(self.p.nctu, self.p.col.w64, self.p.col.h64, self.p.col.depth, self.p.col.col_mv.device)
                col.col_mv.copy_(self.p.col.col_mv)
                col.col_delta.copy_(self.p.col.col_delta)
            elif self.p_refs > 1:
                self.p.run(pictures[a], anchors[:self.p_refs])
            else:
                self.p.run(pictures[a], prev)
            out[a] = keep(self.p.final_planes())
            order.append(a)
            anchor = pictures[a].like(out[a])
            for k in range(a - self.gop + 1, a):
                if self.temporal_mvp:            # the collocated picture is L1[0] = anchor a, whose field col now holds
                    self.b.run(pictures[k], prev, anchor, col=col, cur_deltas=(k - (a - self.gop), k - a))
                elif self.b_refs != (1, 1):
                    self.b.run(pictures[k], anchors[:self.b_refs[0]], ([anchor] + anchors)[:self.b_refs[1]])
                else:
                    self.b.run(pictures[k], prev, anchor)
                out[k] = keep(self.b.final_planes())
                order.append(k)
            prev = anchor
            anchors.insert(0, anchor)
        return order, out
