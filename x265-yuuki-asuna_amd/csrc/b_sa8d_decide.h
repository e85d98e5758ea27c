// b_sa8d_decide.h - the sa8d choice of a B picture's 2Nx2N blocks between one list and both, on gfx950 (included at the end of
// tu_kernels.hip behind inter_sa8d_cost.h: the same luma taps, sa8d_tile_sums and block geometry).
//
// Analysis::compressInterCU_rd0_4 at RD level <= 2 for a B slice (source/encoder/analysis.cpp:1649-1671), per N x N block (N = 8 << level):
//   l    = the cheaper list of Search::predInterSearch: c0 <= c1 ? 0 : 1 with c_l = rec_l.cost + dir_cost[l]          (search.cpp:2611)
//   uni  = sa8d(fenc, predInterLumaPixel(ref_l, mv_l)) + getCost(base_bits[l] + bitcost(mv_l))            (checkInter_rd0_4, :3059-3071)
//   bi   = sa8d(fenc, addAvg(predInterLumaShort(ref0, mv0), predInterLumaShort(ref1, mv1)))
//          + getCost(bits0 + bits1 + bi_bits_delta)                                                        (checkBidir2Nx2N, :3180-3198)
//   z    = sa8d(fenc, pixelavg_pp(ref0, ref1) at the block's own position) + getCost(the same bits with bitcost(0)), tried when mv0 or
//          mv1 is not zero; the candidate becomes the zero pair when z < bi                                             (:3200-3269)
//   dir  = bi < uni ? 3 : 1 + l                                                                                       (:1653-1655)
// bitcost, getCost and sa8d are those of inter_sa8d_cost.h.  The predictor of both lists is (0, 0): the range check of :3205-3213 always
// passes and checkBestMVP (:3246-3247) has one candidate.
//
// Mapping: one workgroup of 256 threads per 32x32 quarter of a CTU (16 / 4 / 1 blocks).  The two lists are staged ONE AT A TIME through the
// same patch and `immed` buffers: list 0's 14-bit prediction waits in LDS, list 1's is combined with it where it is formed.  Each filter
// sum gives the 14-bit intermediate and the rounded pixel of the single-list candidate (they share the sum), so the chosen list's
// prediction costs no second pass.  Three difference planes (single list, both lists, zero pair) go to LDS, and all four wavefronts run
// the 3 x 16 8x8 Hadamard transforms.  Blocks are independent: one launch per picture, no atomics.  The staging steps (patches, 14-bit rows,
// the sample's intermediate and pixel, addAvg) are __device__ functions that b_merge_decide_kernel (b_merge_decide.h) calls too, so the two
// price a two-list prediction alike.
#pragma once

namespace x265hip {

struct BSa8dArgs
{
    const uint8_t* fenc; long fencStrideB;
    const uint8_t* fref[2]; long frefStrideB;
    const int2* mv[2];                  // [ctu*85] {cost, qx | qy << 16}
    const float* bitSizes; int bitSizesLen;
    int ctusW, ctusH, depth, qp, lambda8;
    int dirCost[2], baseBits[2], biBitsDelta, refId[2];
    uint8_t* dir;                       // [ctu][blocks]
    int8_t* ref[2];                     // optional [ctu][blocks]
    int2* mvOut[2];                     // [ctu*85]
    int* cost;                          // [ctu][blocks][4] {winner, uni, bi after the zero twin, flags}
    const int8_t* qpMap;                // optional: the luma plane of tu_qp
    const uint32_t* lambdaByQp;         // optional, indexed by the block's luma quantiser QP
};

// ---- the staging steps of one list's prediction, which b_merge_decide_kernel (b_merge_decide.h) runs too: slot b of nAct predicts the N x N
// block at pos(b) (int2, its first luma sample) from fref displaced by mvOf(b) (qx | qy << 16); use(b) = the slot takes part in this
// list.  All 256 threads call each step; a barrier belongs between two steps. --------------------------------------------------------------

// the slots' reference patches: N + 7 rows and columns around the full-sample position
template <typename Px, int N, class Use, class Mv, class Pos>
__device__ __forceinline__ void luma_stage_patches(int16_t* patch, const int nAct, const Use use, const Mv mvOf, const Pos pos, const Px* fref, const long rst)
{
    constexpr int APRON = 3, PW = N + 7, PP = PW + 1;
    for (int i = threadIdx.x; i < nAct * PW * PW; i += 256)
    {
        const int b = i / (PW * PW), r = i - b * (PW * PW), y = r / PW, x = r - y * PW;
        if (!use(b)) continue;
        const int w = mvOf(b);
        const int qx = (int16_t)(w & 0xffff), qy = (int16_t)(w >> 16);
        const int2 o = pos(b);
        const int px = o.x + (qx >> 2) - APRON + x, py = o.y + (qy >> 2) - APRON + y;
        patch[b * (PW * PP) + y * PP + x] = (int16_t)fref[(long)py * rst + px];
    }
}

// where both phases are set, the horizontal pass at 14-bit precision first (luma_hps with row extension)
template <int N, class Use, class Mv>
__device__ __forceinline__ void luma_stage_rows(const int16_t* patch, int16_t* immed, const int nAct, const Use use, const Mv mvOf, const int headRoom)
{
    constexpr int LOG2N = N == 8 ? 3 : (N == 16 ? 4 : 5), PW = N + 7, PP = PW + 1;
    const int shiftPS = 6 - headRoom, offPS = -(8192 << shiftPS);
    for (int i = threadIdx.x; i < nAct * PW * N; i += 256)
    {
        const int b = i / (PW * N), r = i - b * (PW * N), y = r >> LOG2N, x = r & (N - 1);
        if (!use(b)) continue;
        const int w = mvOf(b);
        const int xf = w & 3, yf = (w >> 16) & 3;
        if (xf && yf)
        {
            int s = 0;
#pragma unroll
            for (int t = 0; t < 8; t++) s += (int)patch[b * (PW * PP) + y * PP + x + t] * (int)kTuTaps[xf][t];
            immed[i] = (int16_t)((s + offPS) >> shiftPS);
        }
    }
}

// sample (x, y) of a slot whose patch is pt and whose rows are im: the 14-bit intermediate (predInterLumaShort) and, from the same sum,
// the rounded pixel (predInterLumaPixel)
template <int N>
__device__ __forceinline__ void luma_short_and_pixel(const int16_t* pt, const int16_t* im, const int w, const int x, const int y, const int headRoom,
                                                     const int maxVal, int& sh, int& px)
{
    constexpr int APRON = 3, PP = N + 8;
    const int xf = w & 3, yf = (w >> 16) & 3;
    const int shiftPS = 6 - headRoom, offPS = -(8192 << shiftPS);
    if (xf && yf)
    {
        const int shiftSP = 6 + headRoom, offSP = (1 << (shiftSP - 1)) + (8192 << 6);
        int s = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) s += (int)im[(y + t) * N + x] * (int)kTuTaps[yf][t];
        sh = (int16_t)(s >> 6);                                                                     // luma_vss
        px = tu_clip16((s + offSP) >> shiftSP, maxVal);                                            // luma_vsp
    }
    else if (!(xf | yf))
    {
        px = pt[(y + APRON) * PP + x + APRON];
        sh = (int16_t)((px << headRoom) - 8192);                                                    // convert_p2s
    }
    else
    {
        int s = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) s += (int)(xf ? pt[(y + APRON) * PP + x + t] : pt[(y + t) * PP + x + APRON]) * (int)kTuTaps[xf ? xf : yf][t];
        sh = (int16_t)((s + offPS) >> shiftPS);                                                     // luma_hps / vps
        px = tu_clip16((s + 32) >> 6, maxVal);                                                      // luma_hpp / vpp
    }
}

// addAvg (pixel.cpp) of two 14-bit intermediates
__device__ __forceinline__ int luma_add_avg(const int s0, const int s1, const int depth, const int maxVal)
{
    const int shiftAvg = 15 - depth, offAvg = (1 << (shiftAvg - 1)) + 2 * 8192;
    return clip3(0, maxVal, (s0 + s1 + offAvg) >> shiftAvg);
}

template <typename Px, int N>
__global__ void __launch_bounds__(256) b_sa8d_decide_kernel(BSa8dArgs a)
{
    constexpr int LOG2N = N == 8 ? 3 : (N == 16 ? 4 : 5), BPR = 32 / N, NB = BPR * BPR, BPC = 64 / N, NPU = BPC * BPC;
    constexpr int PW = N + 7, PP = PW + 1, BPP = sizeof(Px);
    __shared__ int16_t patch[NB * PW * PP];
    __shared__ int16_t immed[NB * PW * N];
    __shared__ int16_t fe[32 * 32], ps0[32 * 32];
    __shared__ int16_t diff[3][32 * 32];                // 0: the single list, 1: both lists, 2: the zero pair
    __shared__ int2 sRec[2][NB];
    __shared__ int sSum[3][16];

    const int tid = threadIdx.x, lane = tid & 63;
    const int ctu = (int)blockIdx.x >> 2, quarter = (int)blockIdx.x & 3;
    const int cx = ctu % a.ctusW, cy = ctu / a.ctusW;
    const int rx0 = cx * 64 + (quarter & 1) * 32, ry0 = cy * 64 + (quarter >> 1) * 32;         // the quarter's first luma sample
    const int maxVal = (1 << a.depth) - 1, headRoom = 14 - a.depth;
    const int lbase = level_record_base<N>();
    // block b of the quarter (raster order inside it) -> its z index inside the CTU
    auto zof = [&](const int b) { return ip_zidx((quarter & 1) * BPR + (b & (BPR - 1)), (quarter >> 1) * BPR + (b / BPR)); };
    if (tid < 2 * NB) sRec[tid / NB][tid % NB] = a.mv[tid / NB][(size_t)ctu * 85 + lbase + zof(tid % NB)];
    const long rst = a.frefStrideB / BPP, fst = a.fencStrideB / BPP;
    {
        const Px* fenc = reinterpret_cast<const Px*>(a.fenc);
        for (int i = tid; i < 32 * 32; i += 256) fe[i] = (int16_t)fenc[(long)(ry0 + (i >> 5)) * fst + rx0 + (i & 31)];
    }
    __syncthreads();
    // the list predInterSearch leaves for block b: list 0 on a tie
    auto single_list = [&](const int b) { return sRec[0][b].x + a.dirCost[0] <= sRec[1][b].x + a.dirCost[1] ? 0 : 1; };
#pragma unroll 1
    for (int l = 0; l < 2; l++)
    {
        const Px* fref = reinterpret_cast<const Px*>(a.fref[l]);
        const int2* rec = sRec[l];
        auto all = [](const int) { return true; };
        auto mvOf = [&](const int b) { return rec[b].y; };
        luma_stage_patches<Px, N>(patch, NB, all, mvOf, [&](const int b) { return make_int2(rx0 + (b & (BPR - 1)) * N, ry0 + (b / BPR) * N); }, fref, rst);
        __syncthreads();
        luma_stage_rows<N>(patch, immed, NB, all, mvOf, headRoom);
        __syncthreads();
        // ---- per sample: the 14-bit intermediate (predInterLumaShort) and, from the same sum, the rounded pixel (predInterLumaPixel) ----
        for (int i = tid; i < 32 * 32; i += 256)
        {
            const int ry = i >> 5, rx = i & 31, b = (ry >> LOG2N) * BPR + (rx >> LOG2N), y = ry & (N - 1), x = rx & (N - 1);
            int sh, px;
            luma_short_and_pixel<N>(patch + b * (PW * PP), immed + b * (PW * N), rec[b].y, x, y, headRoom, maxVal, sh, px);
            const int f = fe[i];
            const int co = (int)fref[(long)(ry0 + ry) * rst + rx0 + rx];                                    // the coincident sample
            if (single_list(b) == l) diff[0][i] = (int16_t)(f - px);
            if (l == 0) { ps0[i] = (int16_t)sh; diff[2][i] = (int16_t)co; }
            else
            {
                diff[1][i] = (int16_t)(f - luma_add_avg((int)ps0[i], sh, a.depth, maxVal));                 // addAvg
                diff[2][i] = (int16_t)(f - (((int)diff[2][i] + co + 1) >> 1));                              // pixelavg_pp
            }
        }
        __syncthreads();                                        // patch / immed are free for list 1; after list 1 the planes are complete
    }
    // ---- 3 x 16 8x8 Hadamard transforms: plane 0 and 2 on wavefronts 0 and 1, plane 1 on wavefronts 2 and 3 ----------------------------
    for (int k = tid >> 7; k < 3; k += 2) sa8d_tile_sums<N>(diff[k], sSum[k], tid & 127, lane);
    __syncthreads();
    if (tid < NB)
    {
        const int b = tid;
        int sad[3];
#pragma unroll
        for (int k = 0; k < 3; k++) sad[k] = sa8d_slot_sum<N>(sSum[k], b);
        auto bitcost = [&](const int w) { return mv_bitcost(a.bitSizes, a.bitSizesLen, w); };
        const int lambda8 = block_lambda8(a.lambda8, a.lambdaByQp, a.qpMap, a.qp, a.depth, a.ctusW, (rx0 + (b & (BPR - 1)) * N) >> 3, (ry0 + (b / BPR) * N) >> 3);
        auto rate = [&](const int bits) { return rd_sad_rate(bits, lambda8); };
        const int2 r0 = sRec[0][b], r1 = sRec[1][b];
        const int l = single_list(b);
        const int uni = (int)(sad[0] + rate(a.baseBits[l] + bitcost(l ? r1.y : r0.y)));
        int bi = (int)(sad[1] + rate(a.baseBits[0] + bitcost(r0.y) + a.baseBits[1] + bitcost(r1.y) + a.biBitsDelta));
        int m0 = r0.y, m1 = r1.y, flags = l;
        if (m0 != 0 || m1 != 0)                                      // bTryZero
        {
            const int z = (int)(sad[2] + rate(a.baseBits[0] + a.baseBits[1] + 2 * bitcost(0) + a.biBitsDelta));
            flags |= 4;
            if (z < bi) { bi = z; m0 = 0; m1 = 0; flags |= 2; }
        }
        const int dir = bi < uni ? 3 : 1 + l;
        const int c0 = r0.x + a.dirCost[0], c1 = r1.x + a.dirCost[1];
        const size_t blk = (size_t)ctu * NPU + zof(b), rec = (size_t)ctu * 85 + lbase + zof(b);
        a.dir[blk] = (uint8_t)dir;
        if (a.ref[0]) a.ref[0][blk] = (int8_t)((dir & 1) ? a.refId[0] : -1);
        if (a.ref[1]) a.ref[1][blk] = (int8_t)((dir & 2) ? a.refId[1] : -1);
        const int win = dir == 3 ? bi : uni;
        a.mvOut[0][rec] = (dir & 1) ? make_int2(win, dir == 3 ? m0 : r0.y) : make_int2(c0, 0);
        a.mvOut[1][rec] = (dir & 2) ? make_int2(win, dir == 3 ? m1 : r1.y) : make_int2(c1, 0);
        int* co = a.cost + blk * 4;
        co[0] = win; co[1] = uni; co[2] = bi; co[3] = flags;
    }
}

static bool b_sa8d_records_alias(const int nctu, const void* mv0, const void* mv1, const void* mv0Out, const void* mv1Out)
{
    const uintptr_t len = (uintptr_t)nctu * 85 * 8;
    const uintptr_t in[2] = { (uintptr_t)mv0, (uintptr_t)mv1 }, out[2] = { (uintptr_t)mv0Out, (uintptr_t)mv1Out };
    bool alias = out[0] < out[1] + len && out[1] < out[0] + len;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) alias = alias || (out[i] < in[j] + len && in[j] < out[i] + len);
    return alias;
}

} // namespace x265hip

extern "C" int x265hip_b_sa8d_decide(const x265hip_b_sa8d_params* p, void* stream)
{
    using namespace x265hip;
    // argument checks first: they need no device
    if (decision_record_refused("b_sa8d_decide", p, !p || !p->fenc || !p->fref0 || !p->fref1 || !p->mv0 || !p->mv1 || !p->bit_sizes || !p->dir || !p->mv0_out ||
                                !p->mv1_out || !p->cost)) return X265HIP_EINVAL;
    // base_bits[l] <= 4096, |bi_bits_delta| <= 4096 (+ at most 4 * 33 bits of two vectors) and lambda8 <= 2^24 keep every rate term below
    // 2^30 and every cost inside int32
    for (int l = 0; l < 2; l++)
        if (p->base_bits[l] < 0 || p->base_bits[l] > 4096) { set_error("b_sa8d_decide: base_bits[%d] %d out of [0, 4096]", l, p->base_bits[l]); return X265HIP_EINVAL; }
    if (p->bi_bits_delta < -4096 || p->bi_bits_delta > 4096 || p->base_bits[0] + p->base_bits[1] + p->bi_bits_delta < 0)
    { set_error("b_sa8d_decide: bi_bits_delta %d out of [-4096, 4096] or below -(base_bits[0] + base_bits[1])", p->bi_bits_delta); return X265HIP_EINVAL; }
    if (bit_sizes_len_refused("b_sa8d_decide", p->bit_sizes_len)) return X265HIP_EINVAL;
    const int nctu = (p->width / 64) * (p->height / 64);
    if (b_sa8d_records_alias(nctu, p->mv0, p->mv1, p->mv0_out, p->mv1_out))
    { set_error("b_sa8d_decide: mv0_out / mv1_out must not alias mv0 / mv1 or each other"); return X265HIP_EINVAL; }
    int rc = ensure_device();
    if (rc) return rc;

    const int bpp = p->depth == 8 ? 1 : 2;
    BSa8dArgs a = {};
    a.fenc = (const uint8_t*)p->fenc; a.fencStrideB = (long)p->fenc_stride * bpp;
    a.fref[0] = (const uint8_t*)p->fref0; a.fref[1] = (const uint8_t*)p->fref1; a.frefStrideB = (long)p->fref_stride * bpp;
    a.mv[0] = (const int2*)p->mv0; a.mv[1] = (const int2*)p->mv1;
    a.bitSizes = p->bit_sizes; a.bitSizesLen = p->bit_sizes_len;
    a.ctusW = p->width / 64; a.ctusH = p->height / 64; a.depth = p->depth; a.qp = p->qp; a.lambda8 = p->lambda8;
    for (int l = 0; l < 2; l++) { a.dirCost[l] = p->dir_cost[l]; a.baseBits[l] = p->base_bits[l]; }
    a.biBitsDelta = p->bi_bits_delta; a.refId[0] = p->ref_id0; a.refId[1] = p->ref_id1;
    a.dir = p->dir; a.ref[0] = p->ref0; a.ref[1] = p->ref1;
    a.mvOut[0] = (int2*)p->mv0_out; a.mvOut[1] = (int2*)p->mv1_out; a.cost = p->cost;
    a.qpMap = p->qp_map; a.lambdaByQp = p->lambda8_by_qp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a.ctusW * a.ctusH * 4);
    for_depth_level(p->depth, p->level, [&](auto px, auto size)
    { hipLaunchKernelGGL((b_sa8d_decide_kernel<decltype(px), decltype(size)::value>), grid, dim3(256), 0, s, a); });
    X265HIP_TRY(hipGetLastError());
    return 0;
}
