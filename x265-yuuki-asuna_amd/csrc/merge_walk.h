// merge_walk.h - the candidate walk the two merge stages share, on gfx950 (included at the end of tu_kernels.hip behind col_field.h, in front
// of merge_decide.h and b_merge_decide.h).
//
// One function of the reference, CUData::getInterMergeCandidates (common/cudata.cpp:1458-1712), serves a P slice and a B slice, without and
// with the temporal candidate of col_field.h.  What does not depend on the slice type is written here once, over the motion type M: a packed
// int (qx | qy << 16) for P with == as hasEqualMotion, BMotion with b_equal_motion for B.
//   field   the CTU's motion at block (bx, by) sits in LDS at [(by + 1) * FW + bx + 1], FW = BPC + 2: row 0 and column 0 are the border - the
//           left CTU's last column, the above CTU's last row and the two corners, the final motion earlier waves left in the outputs
//   list    A1 (left), B1 (above), B0 (above right), A0 (below left), B2 (above left, only while count < 4); pruned pairs B1-A1, B0-B1,
//           A0-A1, B2-A1, B2-B1 and no other (a B0 equal to A1 stays); `count < num` in front of every step is the reference's return at
//           count == maxNumMergeCand.  A neighbour is available inside the picture and before the block in coding order.
//   clipMv  cudata.cpp:1915-1928 (from Predict::motionCompensation, predict.cpp:92): x into [-((64 + 8 + x0 - 1) << 2), (width + 8 - x0 - 1)
//           << 2], y alike - for the prediction only; the CU keeps the unclipped vector, which later neighbours inherit.  A clipped vector
//           reaches at most 71 + 3 samples before the picture and N + 10 behind it: with the planes' margins (96 / 80) the N + 7 rows and
//           columns of a patch stay inside the padded plane at every level, so the kernels need no further guard.
//   price   bits = getTUBits(i, max_merge) = i + (i < max_merge - 1) (search.h:246-249), cost = dist + ((bits * lambda8 + 128) >> 8); the
//           best with strict <: the lowest index wins a tie (analysis.cpp:2833)
// Every piece is force-inlined, in the form in which the kernels' code stayed what it was with the pieces written out in each
// (profiles/merge_walk_code_identity.txt).  Host side: the operand checks and the launch loop of both stages' entries.
#pragma once

namespace x265hip {

__device__ __forceinline__ int merge_pack(const int qx, const int qy) { return (qx & 0xffff) | (int)((unsigned)qy << 16); }

// The border of the motion field: thread tid < FW + BPC owns one border slot.  store(slot, load(nctu, nz)) where the slot's block lies inside
// the picture - nctu / nz its CTU and z index -, store(slot, M{}) where it does not.
template <int N, class M, class Load, class Store>
__device__ __forceinline__ void merge_field_border(const int tid, const int cxb, const int cyb, const int ctusW, Load&& load, Store&& store)
{
    constexpr int BPC = 64 / N, FW = BPC + 2;
    if (tid < FW + BPC)
    {
        const int rx = tid < FW ? tid - 1 : -1, ry = tid < FW ? -1 : tid - FW;                  // relative to the CTU's first block
        const int gbx = cxb * BPC + rx, gby = cyb * BPC + ry;
        M m = {};
        if (gbx >= 0 && gby >= 0 && gbx < ctusW * BPC)
        {
            const int ncx = gbx / BPC, ncy = gby / BPC;
            m = load((size_t)(ncy * ctusW + ncx), ip_zidx(gbx - ncx * BPC, gby - ncy * BPC));
        }
        store((ry + 1) * FW + rx + 1, m);
    }
}

// getPULeft / getPUAbove / getPUAboveRight / getPUBelowLeft / getPUAboveLeft on this grid: block (nbx, nby) of the picture is inside it and
// coded before block z of CTU (cxb, cyb).  The lambda refers to the caller's variables: handed back with copies of them it costs
// instructions and scalar spills (profiles/merge_walk_code_identity.txt).
template <int N>
__device__ __forceinline__ auto merge_available(const int& cxb, const int& cyb, const int& ctu, const int& ctusW, const int& blocksW, const int& blocksH,
                                                const int& z)
{
    return [&](const int nbx, const int nby)
    {
        constexpr int BPC = 64 / N;
        if (nbx < 0 || nby < 0 || nbx >= blocksW || nby >= blocksH) return false;
        const int ncx = nbx / BPC, ncy = nby / BPC;
        if (ncx != cxb || ncy != cyb) return ncy * ctusW + ncx < ctu;
        return ip_zidx(nbx - ncx * BPC, nby - ncy * BPC) < z;
    };
}

// The spatial candidates of block (gbx, gby): motion(dx, dy) reads the field, put(m) appends and counts in `count`, equal(p, q) is
// hasEqualMotion (cudata.cpp:1439-1455)
template <class M, class Available, class Motion, class Equal, class Put>
__device__ __forceinline__ void merge_spatial_candidates(const int gbx, const int gby, const int num, const int& count, Available&& available,
                                                         Motion&& motion, Equal&& equal, Put&& put)
{
    const bool avA1 = available(gbx - 1, gby), avB1 = available(gbx, gby - 1), avB0 = available(gbx + 1, gby - 1);
    const bool avA0 = available(gbx - 1, gby + 1), avB2 = available(gbx - 1, gby - 1);
    const M none = {};
    const M mA1 = avA1 ? motion(-1, 0) : none, mB1 = avB1 ? motion(0, -1) : none, mB0 = avB0 ? motion(1, -1) : none;
    const M mA0 = avA0 ? motion(-1, 1) : none, mB2 = avB2 ? motion(-1, -1) : none;
    if (avA1) put(mA1);                                                                                          // cudata.cpp:1495-1510
    if (count < num && avB1 && (!avA1 || !equal(mA1, mB1))) put(mB1);                                            // :1517-1532
    if (count < num && avB0 && (!avB1 || !equal(mB1, mB0))) put(mB0);                                            // :1537-1551
    if (count < num && avA0 && (!avA1 || !equal(mA1, mA0))) put(mA0);                                            // :1556-1570
    if (count < num && count < 4 && avB2 && (!avA1 || !equal(mA1, mB2)) && (!avB1 || !equal(mB1, mB2))) put(mB2);   // :1573-1593
}

// clipMv of the block whose first sample is (x0, y0): the clip of one packed vector.  (merge_decide_kernel writes the same statements out:
// through this function two of its instances came out one instruction longer.)
__device__ __forceinline__ auto merge_clip(const int x0, const int y0, const int width, const int height)
{
    const int xmin = -((64 + 8 + x0 - 1) << 2), xmax = (width + 8 - x0 - 1) << 2;
    const int ymin = -((64 + 8 + y0 - 1) << 2), ymax = (height + 8 - y0 - 1) << 2;
    return [=](const int c) { return merge_pack(min(xmax, max(xmin, (int)(int16_t)(c & 0xffff))), min(ymax, max(ymin, (int)(int16_t)(c >> 16)))); };
}

// the best of num candidates, candidate i priced from slot slotOf[i]'s sa8d
struct MergeBest { int i, sad; long long cost; };
__device__ __forceinline__ MergeBest merge_price(const int num, const int lambda8, const int* slotSad, const int* slotOf)
{
    int bestI = 0, bestSad = 0;
    long long bestCost = 0;
    for (int i = 0; i < num; i++)
    {
        const int sad = slotSad[slotOf[i]];
        const int bits = i + (i < num - 1 ? 1 : 0);                                                  // getTUBits, search.h:246-249
        const long long cost = (long long)sad + rd_sad_rate(bits, lambda8);
        if (i == 0 || cost < bestCost) { bestI = i; bestSad = sad; bestCost = cost; }                // analysis.cpp:2833
    }
    return { bestI, bestSad, bestCost };
}

// what a decision reads of block z besides its motion, fetched off the serial chain: the inter cost to decide against and the block's lambda
template <int N, class Args>
__device__ __forceinline__ void merge_prefetch_block(const Args& a, const int ctu, const int cxb, const int cyb, const int z, int* inter, int* lambda)
{
    constexpr int NPU = (64 / N) * (64 / N);
    inter[z] = a.interCost[((size_t)ctu * NPU + z) * a.interCostStride];
    lambda[z] = block_lambda8(a.lambda8, a.lambdaByQp, a.qpMap, a.qp, a.depth, a.ctusW, (cxb * 64 + ip_zpos(z).x * N) >> 3, (cyb * 64 + ip_zpos(z).y * N) >> 3);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

// what the four merge entries refuse alike, in front of their own alias checks (at most 4 bits and lambda8 <= 2^24 keep the rate term below
// 2^19 and the cost inside int32)
template <class P>
static bool merge_operands_refused(const char* who, const P* p, const bool nullOperand)
{
    if (decision_record_refused(who, p, nullOperand)) return true;
    if (p->max_merge < 1 || p->max_merge > 5) { set_error("%s: max_merge %d out of 1..5", who, p->max_merge); return true; }
    return inter_cost_stride_refused(who, p->inter_cost_stride);
}

static bool col_operands_refused(const char* who, const void* colMv, const void* colDelta)
{
    if (!colMv != !colDelta) { set_error("%s: col_mv and col_delta go together", who); return true; }
    return false;
}

// One launch per wave of the coding order: launch(px, size, col, n, wave, cyLo) starts the kernel instance <decltype(px), size, col> on n CTUs;
// col: the instance with the temporal candidate
template <class Launch>
static void merge_launch_waves(const int ctusW, const int ctusH, const int depth, const int level, const bool col, Launch&& launch)
{
    for_each_wave(ctusW, ctusH, [&](const int w, const int cyLo, const int n)
    {
        for_depth_level(depth, level, [&](auto px, auto size)
        {
            if (col) launch(px, size, std::true_type(), n, w, cyLo);
            else launch(px, size, std::false_type(), n, w, cyLo);
        });
    });
}

} // namespace x265hip
