// b_merge_decide.h - the merge arm of the sa8d choice of a B picture's blocks, on gfx950 (included at the end of tu_kernels.hip behind
// merge_decide.h: the candidate walk of merge_walk.h, the staging steps of b_sa8d_decide.h, the Hadamard stage of decision_common.h).
//
// Analysis::checkMerge2Nx2N_rd0_4 at RD level 0 (source/encoder/analysis.cpp:2787-2838) and the comparisons of
// Analysis::compressInterCU_rd0_4 (analysis.cpp:1650-1655), per N x N block (N = 8 << level) of the TU stages' grid - one 2Nx2N CU each, CTUs
// in raster order, blocks in z-order, one slice, a B slice with one reference per list; the COL instances (x265hip_b_merge_decide_col with
// a field) have the temporal candidate of col_field.h, the others none:
//   list   CUData::getInterMergeCandidates (common/cudata.cpp:1458-1712) with isInterB: a candidate is (dir, mv[0], mv[1]), an unused
//          list's vector is 0.  The spatial candidates of merge_walk.h, pruned by hasEqualMotion (cudata.cpp:1439-1455): equal directions
//          first, then the vectors of the used lists; the temporal one, never pruned (:1594-1650).  Combined candidates (:1652-1683):
//          cutoff = count * (count - 1) once, pairs in the order of 0xEDC984 / 0xB73621, {3, cand[i].mv[0], cand[j].mv[1]} where cand[i]
//          uses list 0 and cand[j] list 1, unless both lists name one picture and the two vectors are equal.  The rest {3, (0, 0), (0, 0)}
//          (:1684-1709, one reference per list).  Returned once count == max_merge, at every increment.  A neighbour's motion is what it
//          ENDED UP with.
//   price  Predict::motionCompensation (predict.cpp:168-215) after clipMv of every used vector (the limits of merge_walk.h, per list):
//          dir 3 = addAvg of the two lists' 14-bit intermediates, dir 1 / 2 = predInterLumaPixel of that list; dist = cu[].sa8d, bits =
//          getTUBits(i, max_merge), cost = dist + ((bits * lambda8 + 128) >> 8); the best with strict <.
//   choice the block keeps its inter winner iff inter_cost < merge cost, inter_cost = the cost of b_sa8d_decide.h's winner.  The reference
//          (analysis.cpp:1650-1655) starts with bestMode = merge, replaces it by the single list when uni < merge, then by the
//          bidirectional candidate when bi < what stands.  With b_sa8d_decide.h's dir = bi < uni ? 3 : 1 + l and inter_cost = min(uni, bi):
//            bi < uni:   inter_cost = bi.  Whether or not uni < merge, the last comparison is bi < min(uni, merge), and bi < uni: bi wins
//                        iff bi < merge.
//            bi >= uni:  inter_cost = uni.  uni wins the first comparison iff uni < merge; then bi < uni fails.  If uni >= merge, bi >= uni
//                        >= merge fails too: merge stays.
//            so in both cases an inter mode stands iff inter_cost < merge, and it is the one dir names; a tie stays merge.
//
// Mapping: the schedule of merge_decide_kernel - wave = cx + 2 cy, one launch per wave, one workgroup of 256 threads per CTU of the wave,
// the CTU's blocks in z-order.  The CTU's motion field (dir, mv0, mv1 per block) sits in LDS with its border (read from dir / mv0_out /
// mv1_out, which earlier waves wrote); the blocks' inter winners, inter costs and lambdas are fetched into LDS once, off the serial chain.
// Thread 0 builds the list, clips it and keeps one slot per distinct (dir, clipped mv0, clipped mv1) - pricing equal candidates once is
// exact.  The slots are priced side by side (16 / 4 / 1 per pass): the two lists are staged one after the other through one patch and one
// `immed` buffer, as in b_sa8d_decide_kernel; a slot takes part in the lists its dir names.  A dir-3 slot's 14-bit prediction of list 0
// waits in LDS and is combined with list 1's where that is formed; a single-list slot takes the rounded pixel of the same filter sum
// (sa8d_slots() predicts from one plane only, so the single-list slots of two planes share this path instead).  One Hadamard stage per pass.
#pragma once

namespace x265hip {

struct BMergeArgs
{
    const uint8_t* fenc; long fencStrideB;
    const uint8_t* fref[2]; long frefStrideB;
    const uint8_t* dirIn;               // [ctu][blocks]: the inter winner's direction
    const int2* mv[2];                  // [ctu*85] {cost, qx | qy << 16}: the inter winner's records
    const int32_t* interCost; long interCostStride;
    int ctusW, ctusH, depth, qp, lambda8, maxMerge, refId[2];
    uint8_t* merge; uint8_t* mergeIdx; uint8_t* dir;    // [ctu][blocks]
    int8_t* ref[2];                     // optional [ctu][blocks]
    int2* mvOut[2]; int2* mvPred[2];    // [ctu*85], the level's slots
    int2* cost;                         // [ctu][blocks] {sa8d, cost} of the best merge candidate
    int2* best;                         // optional [ctu][blocks]
    const int8_t* qpMap;                // optional: the luma plane of tu_qp
    const uint32_t* lambdaByQp;         // optional
    const int32_t* colMv; const int16_t* colDelta; int curDelta[2];   // the COL instances only: the collocated field (col_field.h)
};

struct BMotion { int dir, mv0, mv1; };  // an unused list's vector is 0, so hasEqualMotion is equality of the three words

__device__ __forceinline__ bool b_equal_motion(const BMotion& p, const BMotion& q) { return p.dir == q.dir && p.mv0 == q.mv0 && p.mv1 == q.mv1; }

// COL: the list has the temporal candidate of col_field.h - {3, the collocated vector scaled for list 0, for list 1} - between B2 and the
// combined candidates, which count it and pair it like any other entry (x265hip_b_merge_decide_col with a field)
template <typename Px, int N, bool COL>
__global__ void __launch_bounds__(256) b_merge_decide_kernel(BMergeArgs a, const int wave, const int cyLo)
{
    constexpr int BPC = 64 / N, NPU = BPC * BPC, NB = Sa8dLds<N>::NB, BPR = 32 / N, BPP = sizeof(Px), FW = BPC + 2, FH = BPC + 1, FS = FH * FW;
    constexpr int LOG2N = N == 8 ? 3 : (N == 16 ? 4 : 5), PW = N + 7, PP = PW + 1;
    __shared__ Sa8dLds<N> s;
    __shared__ int16_t ps0[32 * 32];              // list 0's 14-bit prediction of the dir-3 slots
    __shared__ int sField[3][FS];                 // dir, mv0, mv1 at block (bx, by) of the CTU: [(by + 1) * FW + bx + 1]; row 0 / column 0 = the border
    __shared__ int sCand[3][5], sSlotOf[5], sSlot[3][5], sSlotSad[5], sSlots;
    __shared__ int2 sWinner[2][NPU];
    __shared__ int sWinnerDir[NPU], sInter[NPU], sLambda[NPU];
    __shared__ int sTemporal[2][COL ? NPU : 1], sTemporalOk[COL ? NPU : 1];  // the block's collocated vector scaled per list / whether it has one

    const int tid = threadIdx.x, lane = tid & 63;
    const int cyb = cyLo + (int)blockIdx.x, cxb = wave - 2 * cyb;
    const int ctu = cyb * a.ctusW + cxb;
    const int blocksW = a.ctusW * BPC, blocksH = a.ctusH * BPC;
    const int width = a.ctusW * 64, height = a.ctusH * 64;
    const int lbase = level_record_base<N>();
    const int maxVal = (1 << a.depth) - 1, headRoom = 14 - a.depth;
    const Px* fenc = reinterpret_cast<const Px*>(a.fenc);
    const long rst = a.frefStrideB / BPP, fst = a.fencStrideB / BPP;

    // ---- the border of the motion field: the final motion of the blocks around the CTU that earlier waves left in dir / mv0_out / mv1_out --
    merge_field_border<N, BMotion>(tid, cxb, cyb, a.ctusW, [&](const size_t nctu, const int nz)
    {
        return BMotion{ a.dir[nctu * NPU + nz], a.mvOut[0][nctu * 85 + lbase + nz].y, a.mvOut[1][nctu * 85 + lbase + nz].y };
    }, [&](const int f, const BMotion& m) { sField[0][f] = m.dir; sField[1][f] = m.mv0; sField[2][f] = m.mv1; });
    // ---- what the decisions read of the CTU's own blocks, off the serial chain: the inter winner, its cost, the block's lambda ------------
    if (tid < NPU)
    {
        const int z = tid;
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        sWinnerDir[z] = a.dirIn[(size_t)ctu * NPU + z];
        sWinner[0][z] = a.mv[0][(size_t)ctu * 85 + lbase + z];
        sWinner[1][z] = a.mv[1][(size_t)ctu * 85 + lbase + z];
        merge_prefetch_block<N>(a, ctu, cxb, cyb, z, sInter, sLambda);
        if constexpr (COL)                                                  // another picture's finished field: off the chain as well
        {
            // m_bCheckLDC and m_colFromL0Flag are false (dpb.cpp:193-195): both lists read list 0 of the collocated picture, so the
            // availability (bottom-right, then centre) falls out equal for both
            int cmv = 0, cd = 0;
            const bool ok = tmvp_collocated<N>(a.colMv, a.colDelta, ctu, cxb, cyb, a.ctusW, a.ctusH, bxz * N, byz * N, cmv, cd);
            sTemporalOk[z] = ok ? 1 : 0;
            sTemporal[0][z] = ok ? tmvp_scale_mv(cmv, a.curDelta[0], cd) : 0;
            sTemporal[1][z] = ok ? tmvp_scale_mv(cmv, a.curDelta[1], cd) : 0;
        }
    }
    __syncthreads();

    // thread 0: the candidate list of block z from the motion field, clipped, one slot per distinct clipped candidate
    auto build = [&](const int z)
    {
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        const int gbx = cxb * BPC + bxz, gby = cyb * BPC + byz;
        const int x0 = gbx * N, y0 = gby * N;
        const int num = a.maxMerge;
        int count = 0;
        auto put = [&](const BMotion& m) { sCand[0][count] = m.dir; sCand[1][count] = m.mv0; sCand[2][count] = m.mv1; count++; };
        merge_spatial_candidates<BMotion>(gbx, gby, num, count, merge_available<N>(cxb, cyb, ctu, a.ctusW, blocksW, blocksH, z), [&](const int dx, const int dy)
        {
            const int f = (byz + dy + 1) * FW + bxz + dx + 1;
            return BMotion{ sField[0][f], sField[1][f], sField[2][f] };
        }, b_equal_motion, put);
        if constexpr (COL) { if (count < num && sTemporalOk[z]) put(BMotion{ 3, sTemporal[0][z], sTemporal[1][z] }); }   // :1594-1650: never pruned
        if (count < num)                                                                                             // :1652-1683
        {
            const int cutoff = count * (count - 1);                   // from the count in front of the combined candidates, once
            unsigned p0 = 0xEDC984u, p1 = 0xB73621u;
            for (int k = 0; k < cutoff && count < num; k++, p0 >>= 2, p1 >>= 2)
            {
                const int i = p0 & 3, j = p1 & 3;
                if ((sCand[0][i] & 1) && (sCand[0][j] & 2))
                {
                    const BMotion m = { 3, sCand[1][i], sCand[2][j] };
                    if (!(a.refId[0] == a.refId[1] && m.mv0 == m.mv1)) put(m);                                       // :1670
                }
            }
        }
        const BMotion zero = { 3, 0, 0 };
        while (count < num) put(zero);                                                                               // :1684-1709
        const auto clip = merge_clip(x0, y0, width, height);               // of every used vector
        int slots = 0;
        for (int i = 0; i < num; i++)
        {
            const int d = sCand[0][i];
            const int c0 = (d & 1) ? clip(sCand[1][i]) : 0, c1 = (d & 2) ? clip(sCand[2][i]) : 0;
            int k = 0;
            while (k < slots && !(sSlot[0][k] == d && sSlot[1][k] == c0 && sSlot[2][k] == c1)) k++;
            if (k == slots) { sSlot[0][k] = d; sSlot[1][k] = c0; sSlot[2][k] = c1; slots++; }
            sSlotOf[i] = k;
        }
        sSlots = slots;
    };
    if (tid == 0) build(0);
    __syncthreads();

    for (int z = 0; z < NPU; z++)
    {
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        const int x0 = (cxb * BPC + bxz) * N, y0 = (cyb * BPC + byz) * N;
        const int slots = sSlots;
        auto pos = [&](const int) { return make_int2(x0, y0); };
        for (int base = 0; base < slots; base += NB)
        {
            const int nAct = min(NB, slots - base);
#pragma unroll 1
            for (int l = 0; l < 2; l++)
            {
                bool any = false;                                                  // the same for every thread: the barriers below are uniform
                for (int b = 0; b < nAct; b++) any = any || (sSlot[0][base + b] & (1 << l));
                if (!any) continue;
                const Px* fref = reinterpret_cast<const Px*>(a.fref[l]);
                auto use = [&](const int b) { return (sSlot[0][base + b] & (1 << l)) != 0; };
                auto mvOf = [&](const int b) { return sSlot[1 + l][base + b]; };
                luma_stage_patches<Px, N>(s.patch, nAct, use, mvOf, pos, fref, rst);
                __syncthreads();
                luma_stage_rows<N>(s.patch, s.immed, nAct, use, mvOf, headRoom);
                __syncthreads();
                for (int i = tid; i < 32 * 32; i += 256)
                {
                    const int ry = i >> 5, rx = i & 31, b = (ry >> LOG2N) * BPR + (rx >> LOG2N), y = ry & (N - 1), x = rx & (N - 1);
                    if (b >= nAct || !use(b)) continue;
                    int sh, px;
                    luma_short_and_pixel<N>(s.patch + b * (PW * PP), s.immed + b * (PW * N), mvOf(b), x, y, headRoom, maxVal, sh, px);
                    if (sSlot[0][base + b] != 3) s.diff[i] = (int16_t)((int)fenc[(long)(y0 + y) * fst + x0 + x] - px);
                    else if (l == 0) ps0[i] = (int16_t)sh;
                    else s.diff[i] = (int16_t)((int)fenc[(long)(y0 + y) * fst + x0 + x] - luma_add_avg((int)ps0[i], sh, a.depth, maxVal));
                }
                __syncthreads();                                    // patch / immed are free for list 1; after list 1 the plane is complete
            }
            // (the tiles of a slot at or beyond nAct transform whatever the difference array holds; nothing reads their sums)
            if (tid < 128) sa8d_tile_sums<N>(s.diff, s.sum, tid, lane);
            __syncthreads();
            if (tid < nAct) sSlotSad[base + tid] = sa8d_slot_sum<N>(s.sum, tid);
            __syncthreads();
        }
        if (tid == 0)
        {
            const MergeBest won = merge_price(a.maxMerge, sLambda[z], sSlotSad, sSlotOf);
            const int bestI = won.i, bestSad = won.sad;
            const long long bestCost = won.cost;
            const size_t blk = (size_t)ctu * NPU + z, rec = (size_t)ctu * 85 + lbase + z;
            const int2 w0 = sWinner[0][z], w1 = sWinner[1][z];
            const int ic = sInter[z];
            const bool inter = (long long)ic < bestCost;                                                     // analysis.cpp:1650-1655: a tie stays merge
            const int k = sSlotOf[bestI];
            const int dir = inter ? sWinnerDir[z] : sCand[0][bestI];
            const int f0 = (dir & 1) ? (inter ? w0.y : sCand[1][bestI]) : 0, f1 = (dir & 2) ? (inter ? w1.y : sCand[2][bestI]) : 0;
            // a merged block's used lists carry the merge cost; every other cost word is the input record's
            const int c0 = (!inter && (dir & 1)) ? (int)bestCost : w0.x, c1 = (!inter && (dir & 2)) ? (int)bestCost : w1.x;
            a.merge[blk] = inter ? 0 : 1;
            a.mergeIdx[blk] = inter ? 0 : (uint8_t)bestI;
            a.dir[blk] = (uint8_t)dir;
            if (a.ref[0]) a.ref[0][blk] = (int8_t)((dir & 1) ? a.refId[0] : -1);
            if (a.ref[1]) a.ref[1][blk] = (int8_t)((dir & 2) ? a.refId[1] : -1);
            a.mvOut[0][rec] = make_int2(c0, f0);
            a.mvOut[1][rec] = make_int2(c1, f1);
            a.mvPred[0][rec] = inter ? w0 : make_int2(c0, sSlot[1][k]);
            a.mvPred[1][rec] = inter ? w1 : make_int2(c1, sSlot[2][k]);
            a.cost[blk] = make_int2(bestSad, (int)bestCost);
            if (a.best) a.best[blk] = inter ? make_int2(-1, ic) : make_int2(bestSad, (int)bestCost);
            const int f = (byz + 1) * FW + bxz + 1;
            sField[0][f] = dir; sField[1][f] = f0; sField[2][f] = f1;
            if (z + 1 < NPU) build(z + 1);                                                                   // the next block's list: no barrier in between
        }
        __syncthreads();
    }
}

// true where two of the six record arrays overlap, or dir is dir_in
static bool b_merge_records_alias(const int nctu, const x265hip_b_merge_decide_params* p)
{
    const uintptr_t len = (uintptr_t)nctu * 85 * 8;
    const uintptr_t r[6] = { (uintptr_t)p->mv0_out, (uintptr_t)p->mv1_out, (uintptr_t)p->mv0_pred, (uintptr_t)p->mv1_pred, (uintptr_t)p->mv0, (uintptr_t)p->mv1 };
    bool alias = (const void*)p->dir == (const void*)p->dir_in;
    for (int i = 0; i < 4; i++)                                                  // every output against every later array; mv0 may be mv1
        for (int j = i + 1; j < 6; j++) alias = alias || (r[i] < r[j] + len && r[j] < r[i] + len);
    return alias;
}

} // namespace x265hip

namespace x265hip {

// both entries: colMv / colDelta NULL = the list without a temporal candidate
static int b_merge_decide_run(const char* who, const x265hip_b_merge_decide_params* p, const int32_t* colMv, const int16_t* colDelta, const int curDelta0,
                              const int curDelta1, void* stream)
{
    // argument checks first: they need no device
    if (merge_operands_refused(who, p, !p || !p->fenc || !p->fref0 || !p->fref1 || !p->dir_in || !p->mv0 || !p->mv1 || !p->inter_cost || !p->merge ||
                               !p->merge_idx || !p->dir || !p->mv0_out || !p->mv1_out || !p->mv0_pred || !p->mv1_pred || !p->cost)) return X265HIP_EINVAL;
    // the walk reads a block's inter winner from dir_in / mv0 / mv1 and its neighbours' final motion from dir / mv*_out: shared arrays would
    // change what a second run sees
    if (b_merge_records_alias((p->width / 64) * (p->height / 64), p))
    { set_error("%s: mv*_out / mv*_pred must not alias mv0 / mv1 or each other, nor dir dir_in", who); return X265HIP_EINVAL; }
    int rc = ensure_device();
    if (rc) return rc;

    const int bpp = p->depth == 8 ? 1 : 2;
    BMergeArgs a = {};
    a.fenc = (const uint8_t*)p->fenc; a.fencStrideB = (long)p->fenc_stride * bpp;
    a.fref[0] = (const uint8_t*)p->fref0; a.fref[1] = (const uint8_t*)p->fref1; a.frefStrideB = (long)p->fref_stride * bpp;
    a.dirIn = p->dir_in; a.mv[0] = (const int2*)p->mv0; a.mv[1] = (const int2*)p->mv1;
    a.interCost = p->inter_cost; a.interCostStride = (long)p->inter_cost_stride;
    a.ctusW = p->width / 64; a.ctusH = p->height / 64; a.depth = p->depth; a.qp = p->qp; a.lambda8 = p->lambda8; a.maxMerge = p->max_merge;
    a.refId[0] = p->ref_id0; a.refId[1] = p->ref_id1;
    a.merge = p->merge; a.mergeIdx = p->merge_idx; a.dir = p->dir; a.ref[0] = p->ref0; a.ref[1] = p->ref1;
    a.mvOut[0] = (int2*)p->mv0_out; a.mvOut[1] = (int2*)p->mv1_out; a.mvPred[0] = (int2*)p->mv0_pred; a.mvPred[1] = (int2*)p->mv1_pred;
    a.cost = (int2*)p->cost; a.best = (int2*)p->best; a.qpMap = p->qp_map; a.lambdaByQp = p->lambda8_by_qp;
    a.colMv = colMv; a.colDelta = colDelta; a.curDelta[0] = curDelta0; a.curDelta[1] = curDelta1;
    hipStream_t s = (hipStream_t)stream;
    merge_launch_waves(a.ctusW, a.ctusH, p->depth, p->level, colMv != nullptr, [&](auto px, auto size, auto col, const int n, const int w, const int cyLo)
    {
        hipLaunchKernelGGL((b_merge_decide_kernel<decltype(px), decltype(size)::value, decltype(col)::value>), dim3(n), dim3(256), 0, s, a, w, cyLo);
    });
    X265HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace x265hip

extern "C" int x265hip_b_merge_decide(const x265hip_b_merge_decide_params* p, void* stream)
{
    return x265hip::b_merge_decide_run("b_merge_decide", p, nullptr, nullptr, 0, 0, stream);
}

extern "C" int x265hip_b_merge_decide_col(const x265hip_b_merge_decide_col_params* p, void* stream)
{
    using namespace x265hip;
    if (!p) { set_error("b_merge_decide_col: NULL operand"); return X265HIP_EINVAL; }
    if (col_operands_refused("b_merge_decide_col", p->col_mv, p->col_delta) || tmvp_delta_refused("b_merge_decide_col", "cur_delta0", p->cur_delta0) ||
        tmvp_delta_refused("b_merge_decide_col", "cur_delta1", p->cur_delta1)) return X265HIP_EINVAL;
    return b_merge_decide_run("b_merge_decide_col", &p->base, p->col_mv, p->col_delta, p->cur_delta0, p->cur_delta1, stream);
}
