"""GPU parity, BATCH LAYER, EVERY KIND: each kind of each job-list entry point of include/x265hip.h (x265hip_*_batch) at the launch shapes
the batch layer exists for - many jobs per launch, enough for at least three full workgroups of the kernel that packs several jobs into one
workgroup plus a partial one, a second pass of the persistent MFMA loops - compared JOB BY JOB with the oracle's slot of the same operation
called on host copies.  What every case here does:
  * depths 8, 10 and 12 (the quantiser family has no depth: full int16 / int32 operands instead);
  * full-range random operands, and TestBench extremes (job 0 all-min, job 1 all-max);
  * per-job arguments that vary inside one launch (filter index, shifts, weights, counts, offsets, tc / masks, ...);
  * row strides that differ from the block width, job offsets that are not multiples of the block size;
  * every output buffer pre-filled with a sentinel and compared WHOLE, so a write outside a job's footprint fails;
  * jobs whose reference carries state (SAO sign buffers, deblocked edges, integral rows, accumulated statistics, RDOQ totals) work on disjoint
    state - or, for the RDOQ totals, on state the header says they may share.
COVERAGE names the test of every enumerator of the kind enums; tests/test_abi_cpu.py checks it against the header."""
import bisect
import importlib

import numpy as np
import pytest

import harness as H

pytestmark = pytest.mark.gpu

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
spec = H.spec
ptr = H.ptr
DEPTHS = [8, 10, 12]
I16 = (-32768, 32767)
HERE = "test_gpu_batch_kinds.py"

# enumerator -> the test that drives it at batch level (tests/test_abi_cpu.py: every enumerator of the kind enums is here, every test named exists)
COVERAGE = {}
COVERAGE.update({f"X265HIP_CMP_{k}": "test_gpu_pixelcmp.py::test_pixelcmp_batch_matches_oracle" for k in ("SAD", "SATD", "SA8D", "SSE_PP", "PSY_COST")})
COVERAGE.update({f"X265HIP_IP_{k}": f"{HERE}::test_interp_every_kind" for k in ("HPP", "HPS", "VPP", "VPS", "VSP", "VSS", "HVPP", "P2S")})
COVERAGE.update({f"X265HIP_TR_{k}": f"{HERE}::test_transform_every_kind" for k in ("DCT", "IDCT", "DST4", "IDST4", "LOWPASS_DCT")})
COVERAGE.update({f"X265HIP_Q_{k}": f"{HERE}::test_quant_every_kind"
                 for k in ("QUANT", "NQUANT", "DEQUANT_NORMAL", "DEQUANT_SCALING", "DENOISE", "COUNT_NONZERO", "COPY_CNT")})
COVERAGE.update({f"X265HIP_INTRA_{k}": f"{HERE}::test_intra_every_kind" for k in ("PRED", "FILTER", "ALLANGS")})
COVERAGE.update({f"X265HIP_OP_{k}": f"{HERE}::test_blockop_every_op"
                 for k in ("COPY_PP", "COPY_PS", "COPY_SP", "COPY_SS", "SUB_PS", "ADD_PS", "ADDAVG", "PIXELAVG", "BLOCKFILL", "CPY2DTO1D_SHL",
                           "CPY2DTO1D_SHR", "CPY1DTO2D_SHL", "CPY1DTO2D_SHR", "TRANSPOSE", "WEIGHT_PP", "WEIGHT_SP", "SCALE1D_128TO64",
                           "SCALE2D_64TO32", "SSE_SS", "SSD_S", "VAR", "SSIM_DIST", "NORM_FACT")})
COVERAGE.update({f"X265HIP_LF_{k}": f"{HERE}::test_loopfilter_every_kind"
                 for k in ("SIGN", "SAO_E0", "SAO_E1", "SAO_E1_2ROWS", "SAO_E2", "SAO_E3", "SAO_B0", "STATS_BO", "STATS_E0", "STATS_E1", "STATS_E2",
                           "STATS_E3", "DEBLOCK_LUMA_STRONG", "DEBLOCK_CHROMA", "INTEGRAL_H", "INTEGRAL_V", "ADS")})
COVERAGE.update({f"X265HIP_FR_{k}": "test_gpu_frame_coeff.py::test_whole_plane_copies"
                 for k in ("PLANECOPY_CP", "PLANECOPY_SP", "PLANECOPY_SP_SHL", "PLANECOPY_PP_SHR", "PLANE_CLIP_MAX")})
COVERAGE.update({f"X265HIP_FR_{k}": "test_gpu_frame_coeff.py::test_ssim_rows_lowres_and_cutree_rows" for k in ("SSIM_CORE", "SSIM_END4", "FIX8_PACK", "FIX8_UNPACK")})
COVERAGE.update({"X265HIP_CF_SCAN_POS_LAST": "test_gpu_frame_coeff.py::test_scan_pos_last_batch"})
COVERAGE.update({f"X265HIP_CF_{k}": "test_gpu_frame_coeff.py::test_cabac_estimators_batch"
                 for k in ("FIND_POS_FIRST_LAST", "COST_COEFF_NXN", "COST_COEFF_REMAIN", "COST_C1C2")})
COVERAGE.update({f"X265HIP_CF_{k}": f"{HERE}::test_rdoq_prepass_groups_of_a_tu_share_its_totals" for k in ("RDOQ_NONPSY", "RDOQ_PSY", "RDOQ_PSY_1P", "RDOQ_PSY_2P")})


# ----------------------------------------------------------------------------- helpers
def dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to("cuda:0")


def back(t, dtype):
    return t.cpu().numpy().view(dtype)


def pl(t, stride=0):
    return A.Plane(t.data_ptr(), stride) if t is not None else None


def jobs_of(entries):
    return A.make_jobs(entries, "cuda:0")


def packed(jpw):
    """a job count of three full workgroups of `jpw` jobs plus a partial one (7 when every job has a workgroup of its own)"""
    return 3 * jpw + max(1, jpw // 2) if jpw > 1 else 7


def rand(rng, lo, hi, n, dtype):
    return rng.integers(lo, hi + 1, size=n, dtype=np.int64).astype(dtype)


class Blocks:
    """One w x h block per job in one allocation: block j's sample (0, 0) at off[j], row stride `stride` (wider than the block unless
    given), `apron` readable samples around it, origins skewed so that no offset is a multiple of the block size.  Inputs are random in
    [lo, hi] with block 0 all-lo and block 1 all-hi (TestBench extremes); outputs (sentinel given) hold the sentinel everywhere."""

    def __init__(self, rng, nj, w, h, dtype, lo=0, hi=0, stride=None, apron=0, sentinel=None, extremes=True):
        self.w, self.h = w, h
        self.stride = stride if stride is not None else w + 2 * apron + int(rng.integers(1, 9))
        self.pitch = self.stride * (h + 2 * apron + 1) + 3
        self.off = [j * self.pitch + apron * (self.stride + 1) + 1 + j % 3 for j in range(nj)]
        n = nj * self.pitch + 64
        if sentinel is not None:
            self.a = np.full(n, sentinel, dtype=dtype)
        else:
            self.a = rand(rng, lo, hi, n, dtype)
            if extremes and nj > 2:
                self.a[:self.pitch] = lo
                self.a[self.pitch:2 * self.pitch] = hi
        self.exp = self.a.copy()

    def p(self, j, exp=False):
        return ptr(self.exp if exp else self.a, self.off[j])


def check(got, exp, offs, what):
    """whole-buffer equality; on failure name the first differing element and the job whose region holds it"""
    bad = np.flatnonzero(got != exp)
    if bad.size:
        i = int(bad[0])
        j = max(0, bisect.bisect_right(list(offs), i) - 1)
        pytest.fail(f"{what}: {bad.size} elements differ, first at {i} (job {j}): got {got[i]}, expected {exp[i]}")


# ----------------------------------------------------------------------------- blockop
QUAD_OPS = (A.OP_COPY_PP, A.OP_COPY_PS, A.OP_COPY_SP, A.OP_COPY_SS, A.OP_SUB_PS, A.OP_ADD_PS, A.OP_ADDAVG, A.OP_PIXELAVG)


def blockop_jpw(op, w, h):
    """jobs per workgroup of x265hip_blockop_batch's launcher (quant_blockop_kernels.hip launch_quad): the streaming ops with w % 4 == 0
    share a workgroup, groups of 16 samples per thread when w % 16 == 0; every other op / width has a workgroup per job"""
    if op not in QUAD_OPS or w & 3:
        return 1
    wide = (w & 15) == 0
    ng = (w >> 2) * h // (4 if wide else 1)
    tpj = 1
    while tpj < ng and tpj < 256:
        tpj <<= 1
    return 256 // tpj


def pu_path(w, h):
    for i in range(25):
        if spec.pu_dims(i) == (w, h):
            return f"pu[{i}]"
        if spec.chroma_pu_dims(spec.CSP_I420, i) == (w, h):
            return f"chroma[1].pu[{i}]"
    raise KeyError((w, h))


def cu_path(n):
    return f"cu[{spec.LUMA_CU.index(n)}]" if n >= 4 else "chroma[1].cu[0]"          # 2x2: the 4:2:0 chroma block of a 4x4 CU


PU_QUAD = [(4, 4), (8, 8), (12, 16), (16, 4), (16, 16), (48, 64), (64, 64), (2, 4), (6, 8), (2, 8)]   # quad / wide quad / generic widths
CU_ALL = [(n, n) for n in (2, 4, 8, 16, 32, 64)]
CU_LUMA = [(n, n) for n in (4, 8, 16, 32, 64)]

# op -> (slot field (with the size's path in front), sizes, operand roles p0..p2, argument draw, oracle call)
#   role: (direction, type, layout): "o"/"i"; "P" pixel, "S" int16 full range, "s" int16 in [0, max], "r" int16 in [-max, max]; "2" strided, "1" contiguous
BLOCKOPS = {
    A.OP_COPY_PP: (lambda w, h: pu_path(w, h) + ".copy_pp", PU_QUAD, ["oP2", "iP2"], None,
                   lambda f, d, a, b, x: f(d.p, d.s, a.p, a.s)),
    A.OP_COPY_PS: (lambda w, h: cu_path(w) + ".copy_ps", CU_ALL, ["oS2", "iP2"], None, lambda f, d, a, b, x: f(d.p, d.s, a.p, a.s)),
    A.OP_COPY_SP: (lambda w, h: cu_path(w) + ".copy_sp", CU_ALL, ["oP2", "is2"], None, lambda f, d, a, b, x: f(d.p, d.s, a.p, a.s)),
    A.OP_COPY_SS: (lambda w, h: cu_path(w) + ".copy_ss", CU_ALL, ["oS2", "iS2"], None, lambda f, d, a, b, x: f(d.p, d.s, a.p, a.s)),
    A.OP_SUB_PS: (lambda w, h: cu_path(w) + ".sub_ps", CU_ALL, ["oS2", "iP2", "iP2"], None, lambda f, d, a, b, x: f(d.p, d.s, a.p, b.p, a.s, b.s)),
    A.OP_ADD_PS: (lambda w, h: cu_path(w) + ".add_ps[0]", CU_ALL, ["oP2", "iP2", "iS2"], None, lambda f, d, a, b, x: f(d.p, d.s, a.p, b.p, a.s, b.s)),
    A.OP_ADDAVG: (lambda w, h: pu_path(w, h) + ".addAvg[0]", [(4, 4), (4, 8), (12, 16), (16, 16), (64, 64), (6, 8), (2, 4)],
                  ["oP2", "iS2", "iS2"], None, lambda f, d, a, b, x: f(a.p, b.p, d.p, a.s, b.s, d.s)),
    A.OP_PIXELAVG: (lambda w, h: pu_path(w, h) + ".pixelavg_pp[0]", [(4, 4), (8, 4), (12, 16), (16, 16), (64, 64)],
                    ["oP2", "iP2", "iP2"], None, lambda f, d, a, b, x: f(d.p, d.s, a.p, a.s, b.p, b.s, 32)),
    A.OP_BLOCKFILL: (lambda w, h: cu_path(w) + ".blockfill_s[0]", CU_LUMA, ["oS2"], lambda rng, depth: [int(rng.integers(-32768, 32768))],
                     lambda f, d, a, b, x: f(d.p, d.s, x[0])),
    A.OP_CPY2DTO1D_SHL: (lambda w, h: cu_path(w) + ".cpy2Dto1D_shl", CU_LUMA, ["oS1", "iS2"], lambda rng, depth: [int(rng.integers(0, 8))],
                         lambda f, d, a, b, x: f(d.p, a.p, a.s, x[0])),
    A.OP_CPY2DTO1D_SHR: (lambda w, h: cu_path(w) + ".cpy2Dto1D_shr", CU_LUMA, ["oS1", "iS2"], lambda rng, depth: [int(rng.integers(1, 8))],
                         lambda f, d, a, b, x: f(d.p, a.p, a.s, x[0])),
    A.OP_CPY1DTO2D_SHL: (lambda w, h: cu_path(w) + ".cpy1Dto2D_shl[0]", CU_LUMA, ["oS2", "iS1"], lambda rng, depth: [int(rng.integers(0, 8))],
                         lambda f, d, a, b, x: f(d.p, a.p, d.s, x[0])),
    A.OP_CPY1DTO2D_SHR: (lambda w, h: cu_path(w) + ".cpy1Dto2D_shr", CU_LUMA, ["oS2", "iS1"], lambda rng, depth: [int(rng.integers(1, 8))],
                         lambda f, d, a, b, x: f(d.p, a.p, d.s, x[0])),
    A.OP_TRANSPOSE: (lambda w, h: cu_path(w) + ".transpose", CU_LUMA, ["oP1", "iP2"], None, lambda f, d, a, b, x: f(d.p, a.p, a.s)),
    A.OP_SSE_SS: (lambda w, h: cu_path(w) + ".sse_ss", CU_LUMA, ["ir2", "ir2"], None, lambda f, d, a, b, x: f(a.p, a.s, b.p, b.s)),
    A.OP_SSD_S: (lambda w, h: cu_path(w) + ".ssd_s[0]", CU_LUMA, ["ir2"], None, lambda f, d, a, b, x: f(a.p, a.s)),
    A.OP_VAR: (lambda w, h: cu_path(w) + ".var", CU_LUMA, ["iP2"], None, lambda f, d, a, b, x: f(a.p, a.s)),
    A.OP_NORM_FACT: (lambda w, h: cu_path(w) + ".normFact", CU_LUMA[1:],                     # 8x8 .. 64x64: the slots the reference fills
                   ["iP1"], lambda rng, depth: [int(rng.integers(0, depth - 6))], None),
    A.OP_SSIM_DIST: (lambda w, h: cu_path(w) + ".ssimDist", CU_LUMA, ["iP2", "iP2"], lambda rng, depth: [int(rng.integers(0, depth - 6))], None),
}


def _weight_args(rng, depth, pp):
    corr = 14 - depth
    w0, shift = int(rng.integers(0, 128)), int(rng.integers(corr, corr + 7))
    rnd = (1 << (shift - 1)) if shift else 0
    if pp:
        rnd &= ~((1 << corr) - 1)
    return [w0, rnd, shift, int(rng.integers(-128, 128))]


class _Op:
    """an operand of one blockop launch: the Blocks, its stride and job j's pointer, for the oracle call"""

    def __init__(self, blocks, j, exp):
        self.p, self.s = blocks.p(j, exp), blocks.stride


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("op", list(range(23)))
def test_blockop_every_op(op, depth, repo_root):
    import torch
    orc = H.load_oracle(depth, repo_root)
    rng = np.random.default_rng([31, op, depth])
    pd, m = H.pix_dtype(depth), H.pixel_max(depth)
    if op in (A.OP_WEIGHT_PP, A.OP_WEIGHT_SP, A.OP_SCALE1D_128TO64, A.OP_SCALE2D_64TO32):
        return _blockop_special(op, depth, orc, rng)
    field, sizes, roles, argf, call = BLOCKOPS[op]
    for w, h in sizes:
        fn = orc.fn(field(w, h))
        assert fn is not None, field(w, h)
        nj = packed(blockop_jpw(op, w, h))
        bl = []
        for r in roles:
            d, t, lay = r
            dt, lo, hi = {"P": (pd, 0, m), "S": (np.int16, *I16), "s": (np.int16, 0, m), "r": (np.int16, -m, m)}[t]
            stride = w if lay == "1" else None
            bl.append(Blocks(rng, nj, w, h, dt, lo, hi, stride=stride, sentinel=(0x5A if d == "o" else None)))
        args = [argf(rng, depth) if argf else [] for _ in range(nj)]
        red = op in (A.OP_SSE_SS, A.OP_SSD_S, A.OP_VAR, A.OP_NORM_FACT, A.OP_SSIM_DIST)
        per = 2 if op == A.OP_SSIM_DIST else 1
        res_exp = np.full(per * nj + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        for j in range(nj):
            ops = [_Op(b, j, True) for b in bl] + [None, None]
            if op == A.OP_NORM_FACT:
                z = np.zeros(1, np.uint64)
                fn(ops[0].p, w, args[j][0], ptr(z))
                res_exp[j] = z[0]
            elif op == A.OP_SSIM_DIST:
                ss, ac = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
                fn(ops[0].p, ops[0].s, ops[1].p, ops[1].s, ptr(ss), args[j][0], ptr(ac))
                res_exp[2 * j], res_exp[2 * j + 1] = ss[0], ac[0]
            elif red:
                res_exp[j] = np.uint64(call(fn, None, ops[0], ops[1], args[j]) & 0xFFFFFFFFFFFFFFFF)
            else:
                call(fn, ops[0], ops[1], ops[2], args[j])
        tens = [dev(b.a) for b in bl]
        planes = [A.Plane(t.data_ptr(), b.stride) for t, b in zip(tens, bl)]
        if red:
            planes = planes + [None] * (3 - len(planes))
        jobs = jobs_of([([b.off[j] for b in bl], args[j]) for j in range(nj)])
        res = None
        if red:
            res = torch.from_numpy(np.full(per * nj + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64)).to("cuda:0")
        A.blockop_batch(op, depth, w, h, planes, jobs, nj, res)
        torch.cuda.synchronize()
        what = f"blockop {op} ({field(w, h)}) {w}x{h} depth {depth}, {nj} jobs"
        if red:
            check(back(res, np.uint64), res_exp, [per * j for j in range(nj)], what + " result")
        for k, (b, t) in enumerate(zip(bl, tens)):
            if roles[k][0] == "o":
                check(back(t, b.a.dtype), b.exp, b.off, what + f" plane {k}")


def _blockop_special(op, depth, orc, rng):
    import torch
    pd, m = H.pix_dtype(depth), H.pixel_max(depth)
    if op in (A.OP_WEIGHT_PP, A.OP_WEIGHT_SP):
        pp = op == A.OP_WEIGHT_PP
        fn = orc.fn("weight_pp" if pp else "weight_sp")
        sizes = [(16, 4), (32, 7), (48, 1), (64, 64)] if pp else [(2, 3), (6, 8), (13, 5), (16, 16), (64, 64)]
        for w, h in sizes:
            nj = packed(1)
            src = Blocks(rng, nj, w, h, pd, 0, m) if pp else Blocks(rng, nj, w, h, np.int16, *I16)
            dst = Blocks(rng, nj, w, h, pd, stride=src.stride if pp else None, sentinel=0x5A)    # weight_pp: one stride for both
            args = [_weight_args(rng, depth, pp) for _ in range(nj)]
            for j in range(nj):
                if pp:
                    fn(src.p(j), dst.p(j, True), src.stride, w, h, *args[j])
                else:
                    fn(src.p(j), dst.p(j, True), src.stride, dst.stride, w, h, *args[j])
            ts, td = dev(src.a), dev(dst.a)
            A.blockop_batch(op, depth, w, h, [pl(td, dst.stride), pl(ts, src.stride), None],
                            jobs_of([([dst.off[j], src.off[j]], args[j]) for j in range(nj)]), nj)
            torch.cuda.synchronize()
            check(back(td, pd), dst.exp, dst.off, f"weight_{'pp' if pp else 'sp'} {w}x{h} depth {depth}")
        return
    nj = 37
    if op == A.OP_SCALE1D_128TO64:
        src, dst, fn = Blocks(rng, nj, 256, 1, pd, 0, m, stride=256), Blocks(rng, nj, 128, 1, pd, stride=128, sentinel=0x5A), orc.fn("scale1D_128to64[0]")
        for j in range(nj):
            fn(dst.p(j, True), src.p(j))
    else:
        src, dst, fn = Blocks(rng, nj, 64, 64, pd, 0, m), Blocks(rng, nj, 32, 32, pd, stride=32, sentinel=0x5A), orc.fn("scale2D_64to32")
        for j in range(nj):
            fn(dst.p(j, True), src.p(j), src.stride)
    ts, td = dev(src.a), dev(dst.a)
    A.blockop_batch(op, depth, 0, 0, [pl(td, dst.stride), pl(ts, src.stride), None], jobs_of([([dst.off[j], src.off[j]], []) for j in range(nj)]), nj)
    torch.cuda.synchronize()
    check(back(td, pd), dst.exp, dst.off, f"blockop {op} depth {depth}")


# ----------------------------------------------------------------------------- quant
def test_quant_every_kind(repo_root):
    """All seven kinds, 37 jobs of mixed sizes per launch (one workgroup per job), int16 coefficients over their full range; the int32
    scaling factors up to where the reference's int products still hold (|coef| * quantCoeff + add < 2^31).  result[] per job."""
    import torch
    orc = H.load_oracle(8, repo_root)
    rng = np.random.default_rng(32)
    nj = 37
    for kind in range(7):
        sizes = [int(rng.choice([4, 8, 16, 32])) for _ in range(nj)]
        sizes[0], sizes[1], sizes[2] = 32, 32, 4
        counts = [n * n for n in sizes]
        if kind in (A.Q_QUANT, A.Q_NQUANT, A.Q_DEQUANT_NORMAL, A.Q_DEQUANT_SCALING, A.Q_DENOISE):
            counts[3], counts[4] = 13, 1023                            # counts that are not multiples of 4: the one-coefficient-per-step path
        offs = np.cumsum([0] + [c + 3 for c in counts]).tolist()
        offs = [o + 1 for o in offs]
        n = offs[-1] + 64
        coef = rand(rng, *I16, n, np.int16)
        coef[offs[0]:offs[1]] = -32768
        coef[offs[1]:offs[2]] = 32767
        if kind in (A.Q_COUNT_NONZERO, A.Q_COPY_CNT):
            coef[rng.random(n) < 0.6] = 0
        qc = rand(rng, 0, 57000, n, np.int32)
        qc[offs[0]:offs[2]] = 57000
        out16 = np.full(n, 0x4D4D, np.int16)
        out32 = np.full(n, 0x4D4D4D4D, np.int32)
        res_exp = np.full(nj + 4, 0xDEADBEEF, np.uint32)
        jobs, inputs = [], None
        if kind in (A.Q_QUANT, A.Q_NQUANT):
            e16, e32 = out16.copy(), out32.copy()
            for j in range(nj):
                o, c = offs[j], counts[j]
                bits = int(rng.integers(9, 29))
                add = int(rng.integers(0, 1 << bits)) if j % 2 else (171 if j & 2 else 85) << (bits - 9)
                if kind == A.Q_QUANT:
                    res_exp[j] = orc.fn("quant")(ptr(coef, o), ptr(qc, o), ptr(e32, o), ptr(e16, o), bits, add, c)
                else:
                    res_exp[j] = orc.fn("nquant")(ptr(coef, o), ptr(qc, o), ptr(e16, o), bits, add, c)
                jobs.append(([o, o, o, o], [bits, add, c]))
            bufs = [coef, qc, out32, out16]
            outs = [(3, e16), (2, e32)] if kind == A.Q_QUANT else [(3, e16)]
        elif kind == A.Q_DEQUANT_NORMAL:
            e16 = out16.copy()
            for j in range(nj):
                o, c = offs[j], counts[j]
                per, shift = int(rng.integers(0, 9)), int(rng.integers(1, 11))
                scale = [40, 45, 51, 57, 64, 72][int(rng.integers(0, 6))] << per
                orc.fn("dequant_normal")(ptr(coef, o), ptr(e16, o), c, scale, shift)
                jobs.append(([o, o, o, o], [c, scale, shift]))
            bufs, outs, res_exp = [coef, coef, out16, out16], [(3, e16)], None
        elif kind == A.Q_DEQUANT_SCALING:
            e16 = out16.copy()
            dq = rand(rng, 16, 16 * 255, n, np.int32)
            for j in range(nj):
                o, c = offs[j], counts[j]
                per, shift = int(rng.integers(0, 12)), int(rng.integers(1, 11))
                orc.fn("dequant_scaling")(ptr(coef, o), ptr(dq, o), ptr(e16, o), c, per, shift)
                jobs.append(([o, o, o, o], [c, per, shift]))
            bufs, outs, res_exp = [coef, dq, out16, out16], [(3, e16)], None
        elif kind == A.Q_DENOISE:
            rs = rand(rng, 0, (1 << 32) - 1, n, np.uint32)
            off = rand(rng, 0, 65535, n, np.uint16)
            off[rng.random(n) < 0.3] = 0
            ec, er = coef.copy(), rs.copy()
            for j in range(nj):
                o, c = offs[j], counts[j]
                orc.fn("denoiseDct")(ptr(ec, o), ptr(er, o), ptr(off, o), c)
                jobs.append(([o, o, o, o], [c]))
            bufs, outs, res_exp = [coef, rs, off, off], [(0, ec), (1, er)], None
        elif kind == A.Q_COUNT_NONZERO:
            for j in range(nj):
                o, s = offs[j], sizes[j]
                res_exp[j] = orc.fn(f"{cu_path(s)}.count_nonzero")(ptr(coef, o))
                jobs.append(([o, o, o, o], [s * s]))
            bufs, outs = [coef, coef, coef, coef], []
        else:                                                            # COPY_CNT: strided residual (one stride for the launch), dense copy out
            st = 37
            resid = rand(rng, *I16, nj * st * 33 + 64, np.int16)
            resid[rng.random(resid.size) < 0.6] = 0
            resid[:st * 32] = -32768
            e16 = out16.copy()
            for j in range(nj):
                s = sizes[j]
                ro = j * st * 33 + 1 + j % 3
                res_exp[j] = orc.fn(f"{cu_path(s)}.copy_cnt")(ptr(e16, offs[j]), ptr(resid, ro), st)
                jobs.append(([ro, 0, 0, offs[j]], [s]))
            tr, to = dev(resid), dev(out16)
            res = torch.from_numpy(np.full(nj + 4, 0xDEADBEEF, np.uint32).view(np.int32)).to("cuda:0")
            A.quant_batch(kind, [A.Plane(tr.data_ptr(), st), A.Plane(tr.data_ptr(), 0), A.Plane(tr.data_ptr(), 0), A.Plane(to.data_ptr(), 0)],
                          jobs_of(jobs), nj, res)
            torch.cuda.synchronize()
            check(back(res, np.uint32), res_exp, list(range(nj)), "copy_cnt result")
            check(back(to, np.int16), e16, offs, "copy_cnt coefficients")
            continue
        ts = [dev(b) for b in bufs]
        res = None
        if res_exp is not None:
            res = torch.from_numpy(np.full(nj + 4, 0xDEADBEEF, np.uint32).view(np.int32)).to("cuda:0")
        A.quant_batch(kind, [A.Plane(t.data_ptr(), 0) for t in ts], jobs_of(jobs), nj, res)
        torch.cuda.synchronize()
        if res_exp is not None:
            check(back(res, np.uint32), res_exp, list(range(nj)), f"quant kind {kind} result")
        for k, e in outs:
            check(back(ts[k], e.dtype), e, offs, f"quant kind {kind} plane {k}")


# ----------------------------------------------------------------------------- intra
def intra_jpw(n):
    """jobs per workgroup of intra_quad_kernel (intra_kernels.hip x265hip_intra_batch)"""
    log2n = n.bit_length() - 1
    return 256 >> (2 * log2n - 2 - (2 if n >= 16 else 0))


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", [A.INTRA_PRED, A.INTRA_FILTER, A.INTRA_ALLANGS])
def test_intra_every_kind(kind, depth, repo_root):
    import torch
    orc = H.load_oracle(depth, repo_root)
    rng = np.random.default_rng([33, kind, depth])
    pd, m = H.pix_dtype(depth), H.pixel_max(depth)
    for ci, n in enumerate(spec.LUMA_CU[:4]):
        nj = packed(intra_jpw(n) if kind != A.INTRA_FILTER else 1)
        nb = Blocks(rng, 2 * nj, 4 * n + 1, 1, pd, 0, m)             # block j: the job's neighbours, block nj + j: its filtered neighbours (ALLANGS)
        if kind == A.INTRA_PRED:
            dst = Blocks(rng, nj, n, n, pd, sentinel=0x5A)
            args = [[int(rng.integers(0, 35)), int(rng.integers(0, 2))] for _ in range(nj)]
            for j in range(nj):
                orc.fn(f"cu[{ci}].intra_pred[{args[j][0]}]")(dst.p(j, True), dst.stride, nb.p(j), *args[j])
            offs = [[nb.off[j], dst.off[j]] for j in range(nj)]
        elif kind == A.INTRA_FILTER:
            dst = Blocks(rng, nj, 4 * n + 1, 1, pd, sentinel=0x5A)
            args = [[] for _ in range(nj)]
            for j in range(nj):
                orc.fn(f"cu[{ci}].intra_filter")(nb.p(j), dst.p(j, True))
            offs = [[nb.off[j], dst.off[j]] for j in range(nj)]
        else:
            dst = Blocks(rng, nj, 33 * n * n, 1, pd, stride=33 * n * n, sentinel=0x5A)
            args = [[j % 2] for j in range(nj)]
            for j in range(nj):
                orc.fn(f"cu[{ci}].intra_pred_allangs")(dst.p(j, True), nb.p(j), nb.p(nj + j), args[j][0])
            offs = [[nb.off[j], dst.off[j], nb.off[nj + j]] for j in range(nj)]
        tn, td = dev(nb.a), dev(dst.a)
        A.intra_batch(kind, depth, n, pl(tn, 0), pl(td, dst.stride), jobs_of(zip(offs, args)), nj)
        torch.cuda.synchronize()
        check(back(td, pd), dst.exp, dst.off, f"intra kind {kind} {n}x{n} depth {depth}, {nj} jobs")


# ----------------------------------------------------------------------------- interp
INTERP = [("hpp", A.IP_HPP), ("hps", A.IP_HPS), ("vpp", A.IP_VPP), ("vps", A.IP_VPS), ("vsp", A.IP_VSP), ("vss", A.IP_VSS),
          ("hvpp", A.IP_HVPP), ("p2s", A.IP_P2S)]


def interp_jpw(kind, taps, w, h):
    """jobs per workgroup of interp_strip_kernel (interp_kernels.hip launch_strip, STRIP_ROWS = 8); P2S and widths that are not multiples
    of 4 take the one-workgroup-per-job kernel"""
    if w & 3 or kind == A.IP_P2S:
        return 1
    spj = (w >> 2) * ((h + (taps - 1 if kind == A.IP_HPS else 0) + 7) // 8)
    return max(1, 256 // spj)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name,kind,luma", [(n, k, lu) for n, k in INTERP for lu in (True, False) if lu or n != "hvpp"])   # no chroma hvpp slot
def test_interp_every_kind(name, kind, luma, depth, repo_root):
    import torch
    orc = H.load_oracle(depth, repo_root)
    rng = np.random.default_rng([34, kind, int(luma), depth])
    pd, m = H.pix_dtype(depth), H.pixel_max(depth)
    taps = 8 if luma else 4
    sizes = [(4, 4), (8, 4), (12, 16), (16, 16), (64, 64)] if luma else [(2, 4), (4, 4), (2, 8), (6, 8), (8, 2), (32, 32)]
    src_short, dst_short = name in ("vsp", "vss"), name in ("hps", "vps", "vss", "p2s")
    for w, h in sizes:
        path = pu_path(w, h) if luma else f"pu[{[spec.chroma_pu_dims(spec.CSP_I420, i) for i in range(25)].index((w, h))}]"
        if name == "p2s":
            field = f"{path}.convert_p2s[0]" if luma else f"chroma[1].{path}.p2s[0]"
        else:
            field = f"{path}.luma_{name}" if luma else f"chroma[1].{path}.filter_{name}"
        fn = orc.fn(field)
        assert fn is not None, field
        nj = packed(interp_jpw(kind, taps, w, h))
        src = Blocks(rng, nj, w, h, np.int16, *I16, apron=8) if src_short else Blocks(rng, nj, w, h, pd, 0, m, apron=8)
        ddt = np.int16 if dst_short else pd
        dst = Blocks(rng, nj, w, h + 8, ddt, sentinel=0x5A)
        args = []
        for j in range(nj):
            idx = int(rng.integers(0, 4 if luma else 8))
            a = [idx, int(rng.integers(0, 2))] if name == "hps" else ([idx, int(rng.integers(0, 4))] if name == "hvpp" else [idx])
            if name == "p2s":
                a = []
            args.append(a)
            fn(src.p(j), src.stride, dst.p(j, True), dst.stride, *a)
        ts, td = dev(src.a), dev(dst.a)
        A.interp_batch(kind, depth, taps, w, h, pl(ts, src.stride), pl(td, dst.stride), jobs_of([([src.off[j], dst.off[j]], args[j]) for j in range(nj)]), nj)
        torch.cuda.synchronize()
        check(back(td, ddt), dst.exp, dst.off, f"{field} depth {depth}, {nj} jobs")


# ----------------------------------------------------------------------------- transform
def _transform_launch(orc, rng, kind, name, n, depth, nj, use_mfma):
    import torch
    m = H.pixel_max(depth)
    field = name if name.endswith("4x4") else f"cu[{spec.LUMA_CU.index(n)}].{name}"
    fn = orc.fn(field)
    inverse = kind in (A.TR_IDCT, A.TR_IDST4)
    if inverse:                                                          # dense coefficients in, strided residual out
        src = Blocks(rng, nj, n, n, np.int16, *I16, stride=n)
        dst = Blocks(rng, nj, n, n, np.int16, sentinel=0x5A5)
        for j in range(nj):
            fn(src.p(j), dst.p(j, True), dst.stride)
    else:                                                                # strided residual in (TestBench range), dense coefficients out
        src = Blocks(rng, nj, n, n, np.int16, -m, m)
        dst = Blocks(rng, nj, n, n, np.int16, stride=n, sentinel=0x5A5)
        for j in range(nj):
            fn(src.p(j), dst.p(j, True), src.stride)
    ts, td = dev(src.a), dev(dst.a)
    A.transform_batch(kind, depth, n, pl(ts, src.stride), pl(td, dst.stride), jobs_of([([src.off[j], dst.off[j]], []) for j in range(nj)]), nj, use_mfma)
    torch.cuda.synchronize()
    check(back(td, np.int16), dst.exp, dst.off, f"{field} depth {depth} mfma={use_mfma}, {nj} jobs")


TRANSFORMS = ([("dct", A.TR_DCT, n) for n in (4, 8, 16, 32)] + [("idct", A.TR_IDCT, n) for n in (4, 8, 16, 32)]
              + [("dst4x4", A.TR_DST4, 4), ("idst4x4", A.TR_IDST4, 4)] + [("lowpass_dct", A.TR_LOWPASS_DCT, n) for n in (8, 16, 32)])


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("use_mfma", [0, 1])
def test_transform_every_kind(depth, use_mfma, repo_root):
    orc = H.load_oracle(depth, repo_root)
    rng = np.random.default_rng([35, depth, use_mfma])
    for name, kind, n in TRANSFORMS:
        _transform_launch(orc, rng, kind, name, n, depth, 203, use_mfma)


@pytest.mark.parametrize("depth", DEPTHS)
def test_transform_persistent_loop_second_pass(depth, repo_root):
    """The MFMA transforms are persistent kernels with the grid capped at 2048 workgroups (transform_kernels.hip launch_mfma): 16x16 TUs go
    four to a wavefront quad, 4 wavefronts x 2048 workgroups x 4 TUs = 32768 per pass; 32x32 TUs one per wavefront, 8192 per pass.  One
    launch each past a pass, with a partial last quad (njobs % 4 != 0); every job checked."""
    orc = H.load_oracle(depth, repo_root)
    rng = np.random.default_rng([36, depth])
    for name, kind, n, nj in (("dct", A.TR_DCT, 16, 40001), ("idct", A.TR_IDCT, 16, 32771), ("dct", A.TR_DCT, 32, 9001), ("idct", A.TR_IDCT, 32, 8194)):
        _transform_launch(orc, rng, kind, name, n, depth, nj, 1)


# ----------------------------------------------------------------------------- loopfilter
ADS_SUMS = {(4, 4): 1, (8, 8): 1, (8, 4): 2, (4, 8): 2, (16, 8): 2, (8, 16): 2, (16, 12): 1, (12, 16): 1, (16, 4): 1, (4, 16): 1,
            (32, 16): 2, (16, 32): 2, (64, 32): 2, (32, 64): 2}          # the sums each PU's ads slot compares (pixel.cpp ads_x1 / x2 / x4); others 4


def _smooth(b, rng, m, jobs):
    """jobs' regions of an input as a flat area plus small noise: equal neighbours (edge class 0) and filters that change samples"""
    for j in jobs:
        lo = j * b.pitch
        base = int(rng.integers(8, m - 8))
        b.a[lo:lo + b.pitch] = np.clip(base + rng.integers(-3, 4, size=b.pitch), 0, m)
    b.exp = b.a.copy()


def _signs(rng, nj, w, apron=0):
    return Blocks(rng, nj, w, 1, np.int8, -1, 1, apron=apron, extremes=False)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", list(range(17)))
def test_loopfilter_every_kind(kind, depth, repo_root):
    """Operand conventions: csrc/loopfilter_kernels.hip:13-29.  Every job has its own samples and its own carried buffers; the deblocking
    kinds pack 64 edge segments per workgroup, everything else has a workgroup per job."""
    import torch
    orc = H.load_oracle(depth, repo_root)
    rng = np.random.default_rng([37, kind, depth])
    pd, m = H.pix_dtype(depth), H.pixel_max(depth)
    nj = packed(64) if kind in (A.LF_DEBLOCK_LUMA_STRONG, A.LF_DEBLOCK_CHROMA) else 37
    result, res_exp, outs = None, None, []
    if kind == A.LF_SIGN:
        a, b = Blocks(rng, nj, 300, 1, pd, 0, m, stride=301), Blocks(rng, nj, 300, 1, pd, 0, m, stride=301)
        b.a[::3] = a.a[::3]
        d = Blocks(rng, nj, 300, 1, np.int8, sentinel=9)
        args = [[int(rng.integers(1, 301))] for _ in range(nj)]
        for j in range(nj):
            orc.fn("sign")(d.p(j, True), a.p(j), b.p(j), args[j][0])
        bufs, offs, outs = [d, a, b], [[d.off[j], a.off[j], b.off[j]] for j in range(nj)], [0]
    elif kind in (A.LF_SAO_E0, A.LF_SAO_E1, A.LF_SAO_E1_2ROWS, A.LF_SAO_E2, A.LF_SAO_E3, A.LF_SAO_B0):
        rows = {A.LF_SAO_E0: 2, A.LF_SAO_E1: 2, A.LF_SAO_E1_2ROWS: 3, A.LF_SAO_E2: 2, A.LF_SAO_E3: 2, A.LF_SAO_B0: 64}[kind]
        rec = Blocks(rng, nj, 65, rows, pd, 0, m, apron=1)
        _smooth(rec, rng, m, range(3, nj, 2))
        off = Blocks(rng, nj, 32, 1, np.int8, -128, 127)
        up, upt = _signs(rng, nj, 66, apron=1), Blocks(rng, nj, 66, 1, np.int8, sentinel=0x55)
        args, offs = [], []
        for j in range(nj):
            width = int(rng.integers(1, 65))
            if kind == A.LF_SAO_E0:
                sl = up.p(j)                                         # two signLeft entries, read only
                orc.fn("saoCuOrgE0")(rec.p(j, True), off.p(j), width, sl, rec.stride)
                args.append([width]); offs.append([rec.off[j], off.off[j], up.off[j]])
            elif kind in (A.LF_SAO_E1, A.LF_SAO_E1_2ROWS):
                orc.fn("saoCuOrgE1" if kind == A.LF_SAO_E1 else "saoCuOrgE1_2Rows")(rec.p(j, True), up.p(j, True), off.p(j), rec.stride, width)
                args.append([width]); offs.append([rec.off[j], off.off[j], up.off[j]])
            elif kind == A.LF_SAO_E2:
                orc.fn(f"saoCuOrgE2[{j % 2}]")(rec.p(j, True), upt.p(j, True), up.p(j), off.p(j), width, rec.stride)
                args.append([width]); offs.append([rec.off[j], off.off[j], up.off[j], upt.off[j]])
            elif kind == A.LF_SAO_E3:
                sx = int(rng.integers(0, 2))
                ex = int(rng.integers(sx + 2, 65))
                orc.fn(f"saoCuOrgE3[{j % 2}]")(rec.p(j, True), up.p(j, True), off.p(j), rec.stride, sx, ex)
                args.append([sx, ex]); offs.append([rec.off[j], off.off[j], up.off[j]])
            else:
                width = [13, 16, 64, 6, 32, 1][j % 6]
                hh = int(rng.integers(1, 65))
                orc.fn("saoCuOrgB0")(rec.p(j, True), off.p(j), width, hh, rec.stride)
                args.append([width, hh]); offs.append([rec.off[j], off.off[j]])
        bufs, outs = [rec, off, up, upt], [0, 2, 3]
    elif kind in (A.LF_STATS_BO, A.LF_STATS_E0, A.LF_STATS_E1, A.LF_STATS_E2, A.LF_STATS_E3):
        name = ["BO", "E0", "E1", "E2", "E3"][kind - A.LF_STATS_BO]
        diff = Blocks(rng, nj, 64, 64, np.int16, *I16, stride=64)          # the reference's diff stride is MAX_CU_SIZE
        rec = Blocks(rng, nj, 64, 65, pd, 0, m, apron=1)
        _smooth(rec, rng, m, range(3, nj, 2))
        up, upt = _signs(rng, nj, 66, apron=1), _signs(rng, nj, 66, apron=1)
        bins = 32 if name == "BO" else 5
        res0 = rng.integers(-100000, 100000, size=nj * 64 + 64).astype(np.int32)     # statistics are ADDED to what is there
        res_exp = res0.copy()
        f = orc.fn(f"saoCuStats{name}")
        args, offs = [], []
        for j in range(nj):
            hi = 65 if name in ("BO", "E0", "E1") else 64
            ex, ey = int(rng.integers(1, hi)), int(rng.integers(1, hi))
            if j < 3:
                ex, ey = hi - 1, hi - 1
            s, c = res_exp[j * 64:j * 64 + bins].copy(), res_exp[j * 64 + 32:j * 64 + 32 + bins].copy()
            if name in ("BO", "E0"):
                f(diff.p(j), rec.p(j), rec.stride, ex, ey, ptr(s), ptr(c))
            elif name in ("E1", "E3"):
                f(diff.p(j), rec.p(j), rec.stride, up.p(j, True), ex, ey, ptr(s), ptr(c))
            else:
                f(diff.p(j), rec.p(j), rec.stride, up.p(j, True), upt.p(j, True), ex, ey, ptr(s), ptr(c))
            res_exp[j * 64:j * 64 + bins], res_exp[j * 64 + 32:j * 64 + 32 + bins] = s, c
            args.append([ex, ey]); offs.append([diff.off[j], rec.off[j], up.off[j], upt.off[j]])
        result = torch.from_numpy(res0.copy()).to("cuda:0")
        bufs, outs = [diff, rec, up, upt], [2, 3]
    elif kind in (A.LF_DEBLOCK_LUMA_STRONG, A.LF_DEBLOCK_CHROMA):
        chroma = kind == A.LF_DEBLOCK_CHROMA
        rec = Blocks(rng, nj, 16, 16, pd, 0, m)
        _smooth(rec, rng, m, range(2, nj, 3))
        args, offs = [], []
        for j in range(nj):
            vert = j % 2 == 0                                         # EDGE_VER: across columns, lines down the rows; EDGE_HOR the other way
            offset, step = (1, rec.stride) if vert else (rec.stride, 1)
            o = rec.off[j] + 8 * rec.stride + 8
            tc = int(rng.integers(0, (25 << (depth - 8)) + 1)) if j % 5 else int(rng.integers(0, m + 1))
            if chroma:
                mp, mq = [int(x) for x in rng.integers(-1, 1, size=2)]
                orc.fn(f"pelFilterChroma[{0 if vert else 1}]")(ptr(rec.exp, o), step, offset, tc, mp, mq)
                args.append([step, offset, tc]); offs.append([o, 0, mp, mq])
            else:
                tq = int(rng.integers(0, tc + 1))
                orc.fn(f"pelFilterLumaStrong[{0 if vert else 1}]")(ptr(rec.exp, o), step, offset, tc, tq)
                args.append([step, offset, tc, tq]); offs.append([o])
        bufs, outs = [rec], [0]
    elif kind in (A.LF_INTEGRAL_H, A.LF_INTEGRAL_V):
        strides = [int(rng.integers(40, 200)) for _ in range(nj)]
        ks = [int(rng.integers(0, 6)) for _ in range(nj)]
        sizes = [(2 if kind == A.LF_INTEGRAL_H else spec.INTEGRAL_SIZES[k] + 1) * s + 5 for k, s in zip(ks, strides)]
        base = np.cumsum([3] + sizes).tolist()
        sums = Blocks(rng, 1, base[-1], 1, np.uint32, 0, (1 << 32) - 1, stride=base[-1] + 1, extremes=False)
        pix = Blocks(rng, nj, 200, 1, pd, 0, m)
        args, offs = [], []
        for j in range(nj):
            n, s = spec.INTEGRAL_SIZES[ks[j]], strides[j]
            if kind == A.LF_INTEGRAL_H:
                so = sums.off[0] + base[j] + s                                # the row; the row above sits one stride before it
                orc.fn(f"integral_inith[{ks[j]}]")(ptr(sums.exp, so), pix.p(j), s)
                args.append([s, n, s - n]); offs.append([so, pix.off[j]])
            else:
                so = sums.off[0] + base[j]
                orc.fn(f"integral_initv[{ks[j]}]")(ptr(sums.exp, so), s)
                args.append([s, n, s]); offs.append([so])
        bufs, outs = [sums, pix], [0]
    else:                                                                # ADS
        nsum_of = lambda w, h: ADS_SUMS.get((w, h), 4)
        pus = [spec.pu_dims(i) for i in range(25)]
        sums = Blocks(rng, nj, 400, 1, np.uint32, 0, 4000, extremes=False)
        cost = Blocks(rng, nj, 128, 1, np.uint16, 0, 4000, extremes=False)
        enc = Blocks(rng, nj, 4, 1, np.int32, 0, 4000, extremes=False)
        mvs = Blocks(rng, nj, 128, 1, np.int16, sentinel=-7)
        res_exp = np.full(nj + 4, 0xDEADBEEF, np.uint32)
        args, offs = [], []
        for j in range(nj):
            i = j % 25
            w, h = pus[i]
            width, delta = int(rng.integers(8, 121)), int(rng.integers(130, 200))
            thresh = int(rng.integers(1000, 12000))
            res_exp[j] = orc.fn(f"pu[{i}].ads")(enc.p(j), sums.p(j), delta, cost.p(j), mvs.p(j, True), width, thresh)
            args.append([delta, width, thresh, w | (nsum_of(w, h) << 16)]); offs.append([sums.off[j], cost.off[j], mvs.off[j], enc.off[j]])
        assert 0 < int(res_exp[:nj].sum()) < sum(a[1] for a in args)
        result = torch.from_numpy(np.full(nj + 4, 0xDEADBEEF, np.uint32).view(np.int32)).to("cuda:0")
        bufs, outs = [sums, cost, mvs, enc], [2]
    ts = [dev(b.a) for b in bufs]
    planes = [A.Plane(t.data_ptr(), b.stride) for t, b in zip(ts, bufs)]
    if kind in (A.LF_STATS_BO, A.LF_STATS_E0, A.LF_STATS_E1, A.LF_STATS_E2, A.LF_STATS_E3):
        planes[0] = A.Plane(ts[0].data_ptr(), 64)
    A.loopfilter_batch(kind, depth, planes, jobs_of(zip(offs, args)), nj, result)
    torch.cuda.synchronize()
    what = f"loopfilter kind {kind} depth {depth}, {nj} jobs"
    if result is not None:
        check(back(result, res_exp.dtype), res_exp, [64 * j if kind != A.LF_ADS else j for j in range(nj)], what + " result")
    for k in outs:
        check(back(ts[k], bufs[k].a.dtype), bufs[k].exp, [o[k] if k < len(o) else 0 for o in offs], what + f" plane {k}")


# ----------------------------------------------------------------------------- RDOQ pre-pass: a TU's groups share its totals
@pytest.mark.parametrize("depth", DEPTHS)
def test_rdoq_prepass_groups_of_a_tu_share_its_totals(depth, repo_root):
    """Quant::rdoQuant adds every coefficient group of a TU into ONE {totalUncodedCost, totalRdCost} pair; the batch form of the four
    pre-pass slots must give the serial sums however its jobs are ordered or packed.  Several TUs per launch at every size, groups shuffled."""
    import torch
    orc = H.load_oracle(depth, repo_root, host=True)
    rng = np.random.default_rng([38, depth])
    for kind, name, has_fenc in ((A.CF_RDOQ_NONPSY, "nonPsyRdoQuant", False), (A.CF_RDOQ_PSY, "psyRdoQuant", True),
                                 (A.CF_RDOQ_PSY_1P, "psyRdoQuant_1p", False), (A.CF_RDOQ_PSY_2P, "psyRdoQuant_2p", True)):
        for log2 in (2, 3, 4, 5):
            f = orc.fn(f"cu[{log2 - 2}].{name}")
            tr, nb = 1 << log2, 6
            resi = rng.integers(-32768, 32768, size=(nb, tr * tr)).astype(np.int16)
            resi[0], resi[1] = -32768, 32767
            fenc = rng.integers(-32768, 32768, size=(nb, tr * tr)).astype(np.int16)
            cost0 = rng.integers(-(1 << 40), 1 << 40, size=(nb, tr * tr)).astype(np.int64)
            psy = rng.integers(0, 1 << 16, size=nb).astype(np.int64)
            tot0 = rng.integers(0, 1 << 40, size=(nb + 1, 2)).astype(np.int64)          # one pair per TU, one more that nobody touches
            groups = [(b, (g // (tr // 4)) * 4 * tr + (g % (tr // 4)) * 4) for b in range(nb) for g in range((tr // 4) ** 2)]
            want_cost, want_tot, jobs = cost0.copy(), tot0.copy(), []
            for b, blk in groups:
                if has_fenc:
                    f(ptr(resi[b]), ptr(fenc[b]), ptr(want_cost[b]), ptr(want_tot[b], 0), ptr(want_tot[b], 1), ptr(psy, b), blk)
                else:
                    f(ptr(resi[b]), ptr(want_cost[b]), ptr(want_tot[b], 0), ptr(want_tot[b], 1), blk)
            for k in rng.permutation(len(groups)):
                b, blk = groups[k]
                jobs.append(([b * tr * tr, b * tr * tr, b * tr * tr, 2 * b, b], [blk, log2]))
            d_cost, d_tot = dev(cost0), dev(tot0)
            A.coeff_batch(kind, depth, [dev(fenc), dev(resi), d_cost, d_tot, dev(psy)], A.make_coeff_jobs(jobs, "cuda:0"), len(jobs))
            torch.cuda.synchronize()
            assert np.array_equal(back(d_cost, np.int64).reshape(nb, -1), want_cost), (name, log2, depth)
            got = back(d_tot, np.int64).reshape(-1, 2)
            bad = [b for b in range(nb + 1) if not np.array_equal(got[b], want_tot[b])]
            assert not bad, f"{name} {tr}x{tr} depth {depth}: totals of TUs {bad} differ (got {got[bad[0]].tolist()}, expected {want_tot[bad[0]].tolist()})"
