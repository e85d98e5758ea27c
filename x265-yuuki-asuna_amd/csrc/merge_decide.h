// merge_decide.h - the merge arm of the sa8d choice of a P picture's blocks, on gfx950 (included at the end of tu_kernels.hip behind
// inter_sa8d_cost.h and merge_walk.h: it prices every candidate with the former's sa8d_slots() and walks the list of the latter).
//
// Analysis::checkMerge2Nx2N_rd0_4 at RD level 0 (source/encoder/analysis.cpp:2787-2838, 2870-2871) and the comparison of
// Analysis::compressInterCU_rd0_4 (analysis.cpp:1650), per N x N block (N = 8 << level) of the TU stages' grid - one 2Nx2N CU each, CTUs
// in raster order, blocks in z-order, one slice, a P slice with one reference; the COL instances (x265hip_merge_decide_col with a field)
// have the temporal candidate of col_field.h, the others none:
//   list   CUData::getInterMergeCandidates (common/cudata.cpp:1458-1712): the spatial candidates of merge_walk.h, the temporal one, never
//          pruned (:1594-1650), returned once count == max_merge; the rest (0, 0).  A neighbour's motion is what it ENDED UP with (its
//          candidate where it merged, its searched vector where it did not).
//   price  dist = cu[].sa8d(fenc, predInterLumaPixel(fref, clipMv(mv_i))), rate and comparison of merge_walk.h
//   choice the block keeps its searched vector iff inter_cost < merge cost (analysis.cpp:1650; a tie stays merge)
//
// Mapping: the candidate list reads motion only, never reconstruction, so the walk is the wave schedule of intra_picture.h without its
// coding chain: wave = cx + 2 cy, one launch per wave, one workgroup of 256 threads per CTU of the wave, the CTU's blocks in z-order.
// The CTU's motion field sits in LDS with its border (read from mv_out, which the earlier waves wrote); the blocks' searched records,
// inter costs and lambdas are fetched into LDS once, off the serial chain.  Thread 0 builds the list, clips it and keeps one slot per
// distinct clipped vector - evaluating equal vectors once is exact; the slots go through sa8d_slots() side by side (16 / 4 / 1 per pass
// at 8x8 / 16x16 / 32x32), thread 0 prices the candidates and decides.
#pragma once

namespace x265hip {

struct MergeArgs
{
    const uint8_t* fenc; long fencStrideB;
    const uint8_t* fref; long frefStrideB;
    const int2* mv;                     // [ctu*85] {cost, qx | qy << 16}: the searched records
    const int32_t* interCost; long interCostStride;
    int ctusW, ctusH, depth, qp, lambda8, maxMerge;
    uint8_t* merge; uint8_t* mergeIdx;  // [ctu][blocks]
    int2* mvOut; int2* mvPred;          // [ctu*85], the level's slots
    int2* cost;                         // [ctu][blocks] {sa8d, cost} of the best merge candidate
    int2* best;                         // optional [ctu][blocks]
    const int8_t* qpMap;                // optional: the luma plane of tu_qp
    const uint32_t* lambdaByQp;         // optional
    const int32_t* colMv; const int16_t* colDelta; int curDelta;   // the COL instances only: the collocated field (col_field.h)
};

// COL: the list has the temporal candidate of col_field.h between B2 and the zero candidates (x265hip_merge_decide_col with a field)
template <typename Px, int N, bool COL>
__global__ void __launch_bounds__(256) merge_decide_kernel(MergeArgs a, const int wave, const int cyLo)
{
    constexpr int BPC = 64 / N, NPU = BPC * BPC, NB = Sa8dLds<N>::NB, BPP = sizeof(Px), FW = BPC + 2, FH = BPC + 1;
    __shared__ Sa8dLds<N> s;
    __shared__ int sField[FH * FW];               // motion at block (bx, by) of the CTU: [(by + 1) * FW + bx + 1]; row 0 / column 0 = the border
    __shared__ int sCand[5], sSlotOf[5], sSlotMv[5], sSlotSad[5], sSlots;
    __shared__ int2 sSearched[NPU];
    __shared__ int sInter[NPU], sLambda[NPU];
    __shared__ int sTemporal[COL ? NPU : 1], sTemporalOk[COL ? NPU : 1];     // the block's scaled collocated vector / whether it has one

    const int tid = threadIdx.x;
    const int cyb = cyLo + (int)blockIdx.x, cxb = wave - 2 * cyb;
    const int ctu = cyb * a.ctusW + cxb;
    const int blocksW = a.ctusW * BPC, blocksH = a.ctusH * BPC;
    const int width = a.ctusW * 64, height = a.ctusH * 64;
    const int lbase = level_record_base<N>();
    const Px* fref = reinterpret_cast<const Px*>(a.fref);
    const Px* fenc = reinterpret_cast<const Px*>(a.fenc);
    const long rst = a.frefStrideB / BPP, fst = a.fencStrideB / BPP;

    // ---- the border of the motion field: the final motion of the blocks around the CTU that earlier waves left in mv_out ----------------
    merge_field_border<N, int>(tid, cxb, cyb, a.ctusW, [&](const size_t nctu, const int nz) { return a.mvOut[nctu * 85 + lbase + nz].y; },
                               [&](const int slot, const int m) { sField[slot] = m; });
    // ---- what the decisions read of the CTU's own blocks, off the serial chain: the searched record, the inter cost, the block's lambda ---
    if (tid < NPU)
    {
        const int z = tid;
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        sSearched[z] = a.mv[(size_t)ctu * 85 + lbase + z];
        merge_prefetch_block<N>(a, ctu, cxb, cyb, z, sInter, sLambda);
        if constexpr (COL)                                                  // another picture's finished field: off the chain as well
        {
            int cmv = 0, cd = 0;
            const bool ok = tmvp_collocated<N>(a.colMv, a.colDelta, ctu, cxb, cyb, a.ctusW, a.ctusH, bxz * N, byz * N, cmv, cd);
            sTemporalOk[z] = ok ? 1 : 0;
            sTemporal[z] = ok ? tmvp_scale_mv(cmv, a.curDelta, cd) : 0;
        }
    }
    __syncthreads();

    // thread 0: the candidate list of block z from the motion field, clipped, one slot per distinct clipped vector
    auto build = [&](const int z)
    {
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        const int gbx = cxb * BPC + bxz, gby = cyb * BPC + byz;
        const int x0 = gbx * N, y0 = gby * N;
        const int num = a.maxMerge;
        int count = 0;
        merge_spatial_candidates<int>(gbx, gby, num, count, merge_available<N>(cxb, cyb, ctu, a.ctusW, blocksW, blocksH, z),
                                      [&](const int dx, const int dy) { return sField[(byz + dy + 1) * FW + bxz + dx + 1]; },
                                      [](const int p, const int q) { return p == q; }, [&](const int m) { sCand[count++] = m; });
        if constexpr (COL) { if (count < num && sTemporalOk[z]) sCand[count++] = sTemporal[z]; }          // :1594-1650: never pruned
        while (count < num) sCand[count++] = 0;                                                          // the zero candidates, refIdx 0
        // clipMv: merge_clip() of merge_walk.h, written out
        const int xmin = -((64 + 8 + x0 - 1) << 2), xmax = (width + 8 - x0 - 1) << 2;
        const int ymin = -((64 + 8 + y0 - 1) << 2), ymax = (height + 8 - y0 - 1) << 2;
        int slots = 0;
        for (int i = 0; i < num; i++)
        {
            const int c = sCand[i];
            const int qx = min(xmax, max(xmin, (int)(int16_t)(c & 0xffff))), qy = min(ymax, max(ymin, (int)(int16_t)(c >> 16)));
            const int cl = merge_pack(qx, qy);
            int k = 0;
            while (k < slots && sSlotMv[k] != cl) k++;
            if (k == slots) sSlotMv[slots++] = cl;
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
        for (int base = 0; base < slots; base += NB)
        {
            const int nAct = min(NB, slots - base);
            if (tid < nAct) s.mv[tid] = sSlotMv[base + tid];
            __syncthreads();
            sa8d_slots<Px, N>(s, nAct, [&](const int) { return make_int2(x0, y0); }, fref, rst, fenc, fst, a.depth);
            if (tid < nAct) sSlotSad[base + tid] = sa8d_slot_sum<N>(s.sum, tid);
            __syncthreads();
        }
        if (tid == 0)
        {
            const MergeBest won = merge_price(a.maxMerge, sLambda[z], sSlotSad, sSlotOf);
            const int bestI = won.i, bestSad = won.sad;
            const long long bestCost = won.cost;
            const size_t blk = (size_t)ctu * NPU + z, rec = (size_t)ctu * 85 + lbase + z;
            const int2 searched = sSearched[z];
            const int ic = sInter[z];
            const bool inter = (long long)ic < bestCost;                                                     // analysis.cpp:1650: a tie stays merge
            const int finalMv = inter ? searched.y : sCand[bestI];
            a.merge[blk] = inter ? 0 : 1;
            a.mergeIdx[blk] = inter ? 0 : (uint8_t)bestI;
            a.mvOut[rec] = make_int2(inter ? searched.x : (int)bestCost, finalMv);
            a.mvPred[rec] = make_int2(inter ? searched.x : (int)bestCost, inter ? searched.y : sSlotMv[sSlotOf[bestI]]);
            a.cost[blk] = make_int2(bestSad, (int)bestCost);
            if (a.best) a.best[blk] = inter ? make_int2(-1, ic) : make_int2(bestSad, (int)bestCost);
            sField[(byz + 1) * FW + bxz + 1] = finalMv;
            if (z + 1 < NPU) build(z + 1);                                                                   // the next block's list: no barrier in between
        }
        __syncthreads();
    }
}

// What the AMVP instances take besides MergeArgs (x265hip_merge_decide_amvp); MergeArgs::interCost is then the inter candidate's sa8d
struct MergeAmvpArgs
{
    const float* bitSizes; int bitSizesLen, baseBits;
    uint8_t* mvpIdx;                    // [ctu][blocks]
    int2* mvd;                          // [ctu][blocks] {dx, dy}
    int2* amvp;                         // optional [ctu][blocks]: the two candidates, packed
    int2* inter;                        // [ctu][blocks] {bits, cost} of the inter candidate
};

// merge_decide_kernel with the AMVP arm (x265hip_merge_decide_amvp; see the entry's comment at the end of this file): the same walk over
// the same pieces - the statements of merge_decide_kernel are repeated here, not shared through a common body, because with a common
// body the instances x265hip_merge_decide / _col launch came out as other code (profiles/amvp_kernel_resources.txt).  What is added:
// thread 0's build() makes the predictor list beside the merge list, from the same field and temporal vector; the block's inter cost is
// a.interCost's sa8d plus the rate against the chosen predictor; where selectMVP's SADs decide, the two predictors take slots of the
// sa8d passes and their plain SADs are summed from the passes' difference tile.
template <typename Px, int N, bool COL>
__global__ void __launch_bounds__(256) merge_decide_amvp_kernel(MergeArgs a, MergeAmvpArgs v, const int wave, const int cyLo)
{
    constexpr int BPC = 64 / N, NPU = BPC * BPC, NB = Sa8dLds<N>::NB, BPP = sizeof(Px), FW = BPC + 2, FH = BPC + 1;
    __shared__ Sa8dLds<N> s;
    __shared__ int sField[FH * FW];               // motion at block (bx, by) of the CTU: [(by + 1) * FW + bx + 1]; row 0 / column 0 = the border
    __shared__ int sCand[5], sSlotOf[5], sSlotMv[7], sSlotSad[7], sSlots;   // five merge slots and up to two for the predictors
    __shared__ int2 sSearched[NPU];
    __shared__ int sInter[NPU], sLambda[NPU];
    __shared__ int sTemporal[COL ? NPU : 1], sTemporalOk[COL ? NPU : 1];     // the block's scaled collocated vector / whether it has one
    // the head of the bit-size table (the lookups sit on the serial chain), the block's two predictors, the vector's bits against each,
    // the index where the bits decide it (-1: selectMVP's SADs do), the predictors' slots and the slots' plain SADs
    constexpr int HEAD = 256;
    __shared__ float sBitHead[HEAD];
    __shared__ int sMvp[2], sMvpBits[2], sMvpSlot[2], sMvpIdx, sSlotPlain[7];

    const int tid = threadIdx.x;
    const int cyb = cyLo + (int)blockIdx.x, cxb = wave - 2 * cyb;
    const int ctu = cyb * a.ctusW + cxb;
    const int blocksW = a.ctusW * BPC, blocksH = a.ctusH * BPC;
    const int width = a.ctusW * 64, height = a.ctusH * 64;
    const int lbase = level_record_base<N>();
    const Px* fref = reinterpret_cast<const Px*>(a.fref);
    const Px* fenc = reinterpret_cast<const Px*>(a.fenc);
    const long rst = a.frefStrideB / BPP, fst = a.fencStrideB / BPP;

    for (int i = tid; i < HEAD; i += 256) sBitHead[i] = v.bitSizes[min(i, v.bitSizesLen - 1)];
    // ---- the border of the motion field: the final motion of the blocks around the CTU that earlier waves left in mv_out ----------------
    merge_field_border<N, int>(tid, cxb, cyb, a.ctusW, [&](const size_t nctu, const int nz) { return a.mvOut[nctu * 85 + lbase + nz].y; },
                               [&](const int slot, const int m) { sField[slot] = m; });
    // ---- what the decisions read of the CTU's own blocks, off the serial chain: the searched record, the inter cost, the block's lambda ---
    if (tid < NPU)
    {
        const int z = tid;
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        sSearched[z] = a.mv[(size_t)ctu * 85 + lbase + z];
        merge_prefetch_block<N>(a, ctu, cxb, cyb, z, sInter, sLambda);
        if constexpr (COL)                                                  // another picture's finished field: off the chain as well
        {
            int cmv = 0, cd = 0;
            const bool ok = tmvp_collocated<N>(a.colMv, a.colDelta, ctu, cxb, cyb, a.ctusW, a.ctusH, bxz * N, byz * N, cmv, cd);
            sTemporalOk[z] = ok ? 1 : 0;
            sTemporal[z] = ok ? tmvp_scale_mv(cmv, a.curDelta, cd) : 0;
        }
    }
    __syncthreads();

    // thread 0: the candidate list of block z from the motion field, clipped, one slot per distinct clipped vector
    auto build = [&](const int z)
    {
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        const int gbx = cxb * BPC + bxz, gby = cyb * BPC + byz;
        const int x0 = gbx * N, y0 = gby * N;
        const int num = a.maxMerge;
        int count = 0;
        merge_spatial_candidates<int>(gbx, gby, num, count, merge_available<N>(cxb, cyb, ctu, a.ctusW, blocksW, blocksH, z),
                                      [&](const int dx, const int dy) { return sField[(byz + dy + 1) * FW + bxz + dx + 1]; },
                                      [](const int p, const int q) { return p == q; }, [&](const int m) { sCand[count++] = m; });
        if constexpr (COL) { if (count < num && sTemporalOk[z]) sCand[count++] = sTemporal[z]; }          // :1594-1650: never pruned
        while (count < num) sCand[count++] = 0;                                                          // the zero candidates, refIdx 0
        // clipMv: merge_clip() of merge_walk.h, written out
        const int xmin = -((64 + 8 + x0 - 1) << 2), xmax = (width + 8 - x0 - 1) << 2;
        const int ymin = -((64 + 8 + y0 - 1) << 2), ymax = (height + 8 - y0 - 1) << 2;
        int slots = 0;
        for (int i = 0; i < num; i++)
        {
            const int c = sCand[i];
            const int qx = min(xmax, max(xmin, (int)(int16_t)(c & 0xffff))), qy = min(ymax, max(ymin, (int)(int16_t)(c >> 16)));
            const int cl = merge_pack(qx, qy);
            int k = 0;
            while (k < slots && sSlotMv[k] != cl) k++;
            if (k == slots) sSlotMv[slots++] = cl;
            sSlotOf[i] = k;
        }
        {
            // CUData::getPMV (cudata.cpp:1715-1807) over the same field.  Every block is inter with refIdx 0, so getDirectPMV (:1931-1944)
            // is true exactly where the neighbour is available and getIndirectPMV never decides anything; with several references the
            // POC comparison of getDirectPMV and the scaled indirect candidates would come in here.
            const auto available = merge_available<N>(cxb, cyb, ctu, a.ctusW, blocksW, blocksH, z);
            const auto motion = [&](const int dx, const int dy) { return sField[(byz + dy + 1) * FW + bxz + dx + 1]; };
            int c0 = 0, c1 = 0, n = 0;
            if (available(gbx - 1, gby + 1)) { c0 = motion(-1, 1); n = 1; }                                // left: A0, else A1 (:1740-1743)
            else if (available(gbx - 1, gby)) { c0 = motion(-1, 0); n = 1; }
            bool above = true;
            int m = 0;
            if (available(gbx + 1, gby - 1)) m = motion(1, -1);                                            // above: B0, else B1, else B2 (:1752-1757)
            else if (available(gbx, gby - 1)) m = motion(0, -1);
            else if (available(gbx - 1, gby - 1)) m = motion(-1, -1);
            else above = false;
            if (above) { if (n) c1 = m; else c0 = m; n++; }
            if (n == 2 && c0 == c1) { n = 1; c1 = 0; }                                                     // :1779-1780
            if constexpr (COL) { if (n < 2 && sTemporalOk[z]) { if (n) c1 = sTemporal[z]; else c0 = sTemporal[z]; n++; } }   // :1784-1801
            // the rest stays (0, 0) (:1803-1804)
            const int mvx = (int16_t)(sSearched[z].y & 0xffff), mvy = (int16_t)(sSearched[z].y >> 16);
            const auto size = [&](const int d) { return d < HEAD ? sBitHead[d] : v.bitSizes[min(d, v.bitSizesLen - 1)]; };
            const auto bitcost = [&](const int c)                                                          // bitcost.h:54-58
            { return (int)(uint32_t)(size(abs(mvx - (int)(int16_t)(c & 0xffff))) + size(abs(mvy - (int)(int16_t)(c >> 16))) + 0.5f); };
            const int b0 = bitcost(c0), b1 = c0 == c1 ? b0 : bitcost(c1);
            // Search::checkBestMVP (search.cpp:2702-2713) leaves the candidate that is cheaper in bits; on a tie what Search::selectMVP
            // (:1992-2023) chose: index 0 where the candidates, or their clipped vectors, are equal, else the smaller SAD
            int idx = b1 < b0 ? 1 : 0;
            if (c0 != c1 && b0 == b1)
            {
                const int cl[2] = { merge_pack(min(xmax, max(xmin, (int)(int16_t)(c0 & 0xffff))), min(ymax, max(ymin, (int)(int16_t)(c0 >> 16)))),
                                    merge_pack(min(xmax, max(xmin, (int)(int16_t)(c1 & 0xffff))), min(ymax, max(ymin, (int)(int16_t)(c1 >> 16)))) };
                if (cl[0] != cl[1])
                {
                    idx = -1;
#pragma unroll
                    for (int i = 0; i < 2; i++)
                    {
                        int k = 0;
                        while (k < slots && sSlotMv[k] != cl[i]) k++;
                        if (k == slots) sSlotMv[slots++] = cl[i];
                        sMvpSlot[i] = k;
                    }
                }
            }
            sMvp[0] = c0; sMvp[1] = c1; sMvpBits[0] = b0; sMvpBits[1] = b1; sMvpIdx = idx;
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
        const bool wantSad = sMvpIdx < 0;                                       // uniform over the workgroup
        for (int base = 0; base < slots; base += NB)
        {
            const int nAct = min(NB, slots - base);
            if (tid < nAct) s.mv[tid] = sSlotMv[base + tid];
            __syncthreads();
            sa8d_slots<Px, N>(s, nAct, [&](const int) { return make_int2(x0, y0); }, fref, rst, fenc, fst, a.depth);
            if (tid < nAct) sSlotSad[base + tid] = sa8d_slot_sum<N>(s.sum, tid);
            {
                // bufSAD of the pass's slots from the difference tile: four samples of a row per thread
                if (wantSad)
                {
                    if (tid < nAct) sSlotPlain[base + tid] = 0;
                    __syncthreads();
                    constexpr int LOG2N = N == 8 ? 3 : (N == 16 ? 4 : 5), BPR = 32 / N;
                    const int ry = tid >> 3, rx = (tid & 7) * 4, b = (ry >> LOG2N) * BPR + (rx >> LOG2N);
                    if (b < nAct)
                    {
                        const int16_t* d = s.diff + ry * 32 + rx;
                        atomicAdd(&sSlotPlain[base + b], abs((int)d[0]) + abs((int)d[1]) + abs((int)d[2]) + abs((int)d[3]));
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0)
        {
            const MergeBest won = merge_price(a.maxMerge, sLambda[z], sSlotSad, sSlotOf);
            const int bestI = won.i, bestSad = won.sad;
            const long long bestCost = won.cost;
            const size_t blk = (size_t)ctu * NPU + z, rec = (size_t)ctu * 85 + lbase + z;
            const int2 searched = sSearched[z];
            long long icl = sInter[z];
            {
                // the inter candidate: sInter holds its sa8d; bits = base_bits + bitcost(mv, amvp[mvp_idx]) (search.cpp:2455)
                int idx = sMvpIdx;
                if (idx < 0) idx = sSlotPlain[sMvpSlot[0]] <= sSlotPlain[sMvpSlot[1]] ? 0 : 1;               // search.cpp:2022
                const int bits = v.baseBits + sMvpBits[idx], pred = sMvp[idx];
                icl += rd_sad_rate(bits, sLambda[z]);
                v.mvpIdx[blk] = (uint8_t)idx;
                v.mvd[blk] = make_int2((int)(int16_t)(searched.y & 0xffff) - (int)(int16_t)(pred & 0xffff), (int)(int16_t)(searched.y >> 16) - (int)(int16_t)(pred >> 16));
                if (v.amvp) v.amvp[blk] = make_int2(sMvp[0], sMvp[1]);
                v.inter[blk] = make_int2(bits, (int)icl);
            }
            const int ic = (int)icl;
            const bool inter = icl < bestCost;                                                               // analysis.cpp:1650: a tie stays merge
            const int finalMv = inter ? searched.y : sCand[bestI];
            a.merge[blk] = inter ? 0 : 1;
            a.mergeIdx[blk] = inter ? 0 : (uint8_t)bestI;
            a.mvOut[rec] = make_int2(inter ? searched.x : (int)bestCost, finalMv);
            a.mvPred[rec] = make_int2(inter ? searched.x : (int)bestCost, inter ? searched.y : sSlotMv[sSlotOf[bestI]]);
            a.cost[blk] = make_int2(bestSad, (int)bestCost);
            if (a.best) a.best[blk] = inter ? make_int2(-1, ic) : make_int2(bestSad, (int)bestCost);
            sField[(byz + 1) * FW + bxz + 1] = finalMv;
            if (z + 1 < NPU) build(z + 1);                                                                   // the next block's list: no barrier in between
        }
        __syncthreads();
    }
}

} // namespace x265hip

namespace x265hip {

// the three entries: colMv / colDelta NULL = the list without a temporal candidate; v: the AMVP entry's own operands (checked there), else NULL
static int merge_decide_run(const char* who, const x265hip_merge_decide_params* p, const int32_t* colMv, const int16_t* colDelta, const int curDelta, void* stream,
                            const MergeAmvpArgs* v = nullptr)
{
    // argument checks first: they need no device
    if (merge_operands_refused(who, p, !p || !p->fenc || !p->fref || !p->mv || !p->inter_cost || !p->merge || !p->merge_idx || !p->mv_out || !p->mv_pred ||
                               !p->cost)) return X265HIP_EINVAL;
    // the walk reads a block's searched vector from mv and its neighbours' final motion from mv_out: one array for both would change what a
    // second run sees
    if (p->mv_out == p->mv || p->mv_pred == p->mv || p->mv_out == p->mv_pred)
    { set_error("%s: mv_out and mv_pred must not alias mv or each other", who); return X265HIP_EINVAL; }
    if (v)
    {
        const void* outs[] = { v->mvpIdx, v->mvd, v->inter, v->amvp, p->merge, p->merge_idx, p->mv_out, p->mv_pred, p->cost, p->best };
        for (int i = 0; i < 4; i++)
            for (int j = i + 1; j < 10; j++)
                if (outs[i] && outs[i] == outs[j]) { set_error("%s: mvp_idx, mvd, amvp and inter must not alias each other or another output", who); return X265HIP_EINVAL; }
    }
    int rc = ensure_device();
    if (rc) return rc;

    const int bpp = p->depth == 8 ? 1 : 2;
    MergeArgs a = {};
    a.fenc = (const uint8_t*)p->fenc; a.fencStrideB = (long)p->fenc_stride * bpp;
    a.fref = (const uint8_t*)p->fref; a.frefStrideB = (long)p->fref_stride * bpp;
    a.mv = (const int2*)p->mv; a.interCost = p->inter_cost; a.interCostStride = (long)p->inter_cost_stride;
    a.ctusW = p->width / 64; a.ctusH = p->height / 64; a.depth = p->depth; a.qp = p->qp; a.lambda8 = p->lambda8; a.maxMerge = p->max_merge;
    a.merge = p->merge; a.mergeIdx = p->merge_idx; a.mvOut = (int2*)p->mv_out; a.mvPred = (int2*)p->mv_pred;
    a.cost = (int2*)p->cost; a.best = (int2*)p->best; a.qpMap = p->qp_map; a.lambdaByQp = p->lambda8_by_qp;
    a.colMv = colMv; a.colDelta = colDelta; a.curDelta = curDelta;
    hipStream_t s = (hipStream_t)stream;
    merge_launch_waves(a.ctusW, a.ctusH, p->depth, p->level, colMv != nullptr, [&](auto px, auto size, auto col, const int n, const int w, const int cyLo)
    {
        if (v) hipLaunchKernelGGL((merge_decide_amvp_kernel<decltype(px), decltype(size)::value, decltype(col)::value>), dim3(n), dim3(256), 0, s, a, *v, w, cyLo);
        else hipLaunchKernelGGL((merge_decide_kernel<decltype(px), decltype(size)::value, decltype(col)::value>), dim3(n), dim3(256), 0, s, a, w, cyLo);
    });
    X265HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace x265hip

extern "C" int x265hip_merge_decide(const x265hip_merge_decide_params* p, void* stream)
{
    return x265hip::merge_decide_run("merge_decide", p, nullptr, nullptr, 0, stream);
}

extern "C" int x265hip_merge_decide_col(const x265hip_merge_decide_col_params* p, void* stream)
{
    using namespace x265hip;
    if (!p) { set_error("merge_decide_col: NULL operand"); return X265HIP_EINVAL; }
    if (col_operands_refused("merge_decide_col", p->col_mv, p->col_delta) || tmvp_delta_refused("merge_decide_col", "cur_delta", p->cur_delta)) return X265HIP_EINVAL;
    return merge_decide_run("merge_decide_col", &p->base, p->col_mv, p->col_delta, p->cur_delta, stream);
}

// x265hip_merge_decide_col with the inter candidate priced against its AMVP predictor (CUData::getPMV, Search::selectMVP,
// Search::checkBestMVP): the walk's inter_cost operand is the candidate's sa8d, the rate is added here once the predictor is known
extern "C" int x265hip_merge_decide_amvp(const x265hip_merge_decide_amvp_params* p, void* stream)
{
    using namespace x265hip;
    const char* who = "merge_decide_amvp";
    if (!p || !p->inter_sa8d || !p->bit_sizes || !p->mvp_idx || !p->mvd || !p->inter) { set_error("%s: NULL operand", who); return X265HIP_EINVAL; }
    if (col_operands_refused(who, p->base.col_mv, p->base.col_delta) || tmvp_delta_refused(who, "cur_delta", p->base.cur_delta)) return X265HIP_EINVAL;
    if (p->inter_sa8d_stride < 1) { set_error("%s: inter_sa8d_stride %ld below 1", who, (long)p->inter_sa8d_stride); return X265HIP_EINVAL; }
    // base_bits <= 4096 (+ at most 2 * 35 bits of a difference) and lambda8 <= 2^24 keep the rate term below 2^29
    if (p->base_bits < 0 || p->base_bits > 4096) { set_error("%s: base_bits %d out of [0, 4096]", who, p->base_bits); return X265HIP_EINVAL; }
    if (bit_sizes_len_refused(who, p->bit_sizes_len)) return X265HIP_EINVAL;
    x265hip_merge_decide_params base = p->base.base;            // the walk decides against the sa8d; base.inter_cost is not read
    base.inter_cost = p->inter_sa8d; base.inter_cost_stride = p->inter_sa8d_stride;
    MergeAmvpArgs v = {};
    v.bitSizes = p->bit_sizes; v.bitSizesLen = p->bit_sizes_len; v.baseBits = p->base_bits;
    v.mvpIdx = p->mvp_idx; v.mvd = (int2*)p->mvd; v.amvp = (int2*)p->amvp; v.inter = (int2*)p->inter;
    return merge_decide_run(who, &base, p->base.col_mv, p->base.col_delta, p->base.cur_delta, stream, &v);
}
