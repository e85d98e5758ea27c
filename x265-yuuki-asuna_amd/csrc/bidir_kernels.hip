// bidir_kernels.hip - the bidirectional decision of a B picture's blocks, on gfx950: which list(s) every NxN block is predicted from.
//
// Reference semantics: the bidirectional part of Search::predInterSearch (source/encoder/search.cpp:2473-2640) - the luma-only branch
// of the averaged prediction's cost (:2498-2510), the zero-vector candidate (bTryZero, :2515-2577, luma branch :2544-2551, strict '<'
// at :2566) and the selection between list 0, list 1 and both (:2581-2640, without the merge arm) - with Predict::predInterLumaPixel
// (source/common/predict.cpp:245-265: luma_hpp / luma_vpp / luma_hvpp / copy, i.e. ROUNDED AND CLIPPED pixels, not the 14-bit
// intermediates addAvg combines), pixelavg_pp ((a + b + 1) >> 1, source/common/pixel.cpp) and pu[].satd (pixel.cpp:210-297; tiled in
// 4x4s here - every 4x4's coefficient sum is even, so the tiling does not change the total).
//
// The pipeline searches each list around ONE predictor, (0,0) - that is what cost_q is indexed with everywhere - so the reference's
// predictor range check of the zero candidate (:2520-2528) always passes, and checkBestMVP (:2563-2564) has nothing to choose between:
// the zero candidate's vector cost is 4 * cost_q[qoff] (two components per list, both lists).
//
// Mapping: one workgroup of 256 threads per CTU, thread = one 4x4 tile of one block, a block's 4 / 16 / 64 tiles on consecutive lanes
// (the geometry of the sub-pel stage), the tile's source samples in registers.  Each thread forms its tile of both lists' predictions
// (tile_predict: the exact interpolation; with phase planes four dword loads per list instead), takes the SATD of the averaged
// prediction and of the zero candidate, and the two partial costs are summed over the block's lanes with DPP moves - a block never
// straddles a wavefront, so the sums need no LDS and no barrier.  One lane per block decides and writes.  No atomics.
#include "common.h"
#include "tile_interp.h"

namespace x265hip {

struct BidirArgs
{
    const uint8_t* fenc; long fencStrideB;
    const uint8_t* fref[2]; long frefStrideB;
    int ctusW, depth;
    const int2* mv[2];                   // {cost, qx | qy << 16} per PU, [ctu][85]
    const uint16_t* costQ; int qoff;
    int dirCost[3];
    int refId[2];
    const uint8_t* planes[2]; long planeBytes;       // sample (0,0) of phase 1 of each list's reference; NULL = interpolate
    uint8_t* dir;
    int8_t* ref[2];
    int2* mvOut[2];
    int* costOut;                        // [ctu][blocks][4]
};

// Several references per list (x265hip_bidir_decide_refs): every block is measured against the two pictures IT chose - list index
// refIdx[l][blk] (x265hip_ref_select's ref_idx) into the launch's tables of reference planes, phase planes, reference bits and picture
// ids, per list.  At level 2 a wavefront holds one block: its list index is uniform and the tables are read where they arrive, in the
// kernel arguments, with a scalar index.  At levels 0 and 1 a wavefront holds 16 or 4 blocks, the index varies from lane to lane, and a
// table in the kernel arguments indexed by a vector register would be copied to scratch memory: there every wavefront stages a quarter
// of the tables in LDS once per workgroup with scalar indices (its lane 0 writes) and a lane reads its block's entries - the one use of
// LDS and the one barrier of this file.
struct BdRefTables
{
    const uint8_t* fref[2][X265HIP_MAX_REFS];          // entries behind nrefs repeat the last one
    const uint8_t* planes[2][X265HIP_MAX_REFS];
    int refCost[2][X265HIP_MAX_REFS];
    int refId[2][X265HIP_MAX_REFS];
};
struct BidirRefsArgs
{
    BidirArgs b;                                        // b.fref / b.planes / b.refId are not read
    BdRefTables t;
    const int8_t* refIdx[2];                            // [ctu][blocks]
    int nrefs[2];
};
__device__ __forceinline__ const BidirArgs& bd_base_args(const BidirArgs& a) { return a; }
__device__ __forceinline__ const BidirArgs& bd_base_args(const BidirRefsArgs& ra) { return ra.b; }

template <int LEVEL> struct BdGeom
{
    static constexpr int N = 8 << LEVEL, NPU = 64 >> (2 * LEVEL);
    static constexpr int TSHIFT = 2 * LEVEL + 2, NTILES = 1 << TSHIFT, TPR = N >> 2;     // 4x4 tiles per block; NPU * NTILES = 256
    static constexpr int LBASE = LEVEL == 0 ? 0 : (LEVEL == 1 ? 64 : 80);
};

// The decision of one block from the summed SATDs of the bidirectional candidate (sBi) and of the zero candidate (sZ): one lane per block.
// tab != NULL (several references per list): i0 / i1 = the block's list indices - the reference bits of both lists stay in the bidirectional
// candidate and in the zero candidate (search.cpp:2473-2480, 2554-2558), and ref[] gets the picture ids of the block's two references.
template <bool REFS = false>
__device__ __forceinline__ void bd_decide(const BidirArgs& a, size_t blk, size_t rec, int2 r0, int2 r1, int sBi, int sZ,
                                          const BdRefTables* tab = nullptr, const int i0 = 0, const int i1 = 0)
{
    auto mvc = [&](const int w) { return (int)a.costQ[a.qoff + (int16_t)(w & 0xffff)] + (int)a.costQ[a.qoff + (w >> 16)]; };
    const int c0 = r0.x + a.dirCost[0], c1 = r1.x + a.dirCost[1];
    int rb = 0;
    if constexpr (REFS) rb = tab->refCost[0][i0] + tab->refCost[1][i1];
    const int cRef = REFS ? sBi + mvc(r0.y) + mvc(r1.y) + a.dirCost[2] + rb : sBi + mvc(r0.y) + mvc(r1.y) + a.dirCost[2];
    int cbi = cRef, cz = -1, m0 = r0.y, m1 = r1.y;
    if (m0 != 0 || m1 != 0)                                      // bTryZero
    {
        cz = sZ + 4 * (int)a.costQ[a.qoff] + a.dirCost[2];
        if constexpr (REFS) cz += rb;
        if (cz < cbi) { cbi = cz; m0 = 0; m1 = 0; }
    }
    const int dir = (cbi < c0 && cbi < c1) ? 3 : (c0 <= c1 ? 1 : 2);
    a.dir[blk] = (uint8_t)dir;
    if constexpr (REFS)
    {
        if (a.ref[0]) a.ref[0][blk] = (int8_t)((dir & 1) ? tab->refId[0][i0] : -1);
        if (a.ref[1]) a.ref[1][blk] = (int8_t)((dir & 2) ? tab->refId[1][i1] : -1);
    }
    else
    {
        if (a.ref[0]) a.ref[0][blk] = (int8_t)((dir & 1) ? a.refId[0] : -1);
        if (a.ref[1]) a.ref[1][blk] = (int8_t)((dir & 2) ? a.refId[1] : -1);
    }
    a.mvOut[0][rec] = dir == 3 ? make_int2(cbi, m0) : make_int2(c0, dir == 1 ? m0 : 0);
    a.mvOut[1][rec] = dir == 3 ? make_int2(cbi, m1) : make_int2(c1, dir == 2 ? m1 : 0);
    if (a.costOut) { int* co = a.costOut + blk * 4; co[0] = c0; co[1] = c1; co[2] = cRef; co[3] = cz; }
}

// Args = BidirArgs: both lists hold one picture (x265hip_bidir_decide).  Args = BidirRefsArgs (REFS): every block against the two
// pictures it chose (x265hip_bidir_decide_refs).  REFS is a parameter of the kernel: each instance is compiled from one body with the
// other flavour's statements discarded, and the single-reference instances keep their code instruction for instruction.
template <typename Px, int LEVEL, bool PL, class Args = BidirArgs>
__global__ void __launch_bounds__(256) bidir_decide_kernel(Args ra)
{
    constexpr bool REFS = std::is_same<Args, BidirRefsArgs>::value;
    const BidirArgs& a = bd_base_args(ra);
    typedef BdGeom<LEVEL> G;
    constexpr int BPP = sizeof(Px), N = G::N;
    const int ctu = xcd_swizzle(blockIdx.x, gridDim.x);
    const int cx = (ctu % a.ctusW) * 64, cy = (ctu / a.ctusW) * 64;
    const int tid = threadIdx.x;
    const int pu = tid >> G::TSHIFT, tile = tid & (G::NTILES - 1);
    const int bxz = (pu & 1) | ((pu >> 1) & 2) | ((pu >> 2) & 4), byz = ((pu >> 1) & 1) | ((pu >> 2) & 2) | ((pu >> 3) & 4);
    const int ty = tile / G::TPR, tx = tile % G::TPR;
    const int px = cx + bxz * N + tx * 4, py = cy + byz * N + ty * 4;

    int src[4][4];
    tile_predict<BPP>(a.fenc + (long)py * a.fencStrideB + (long)px * BPP, a.fencStrideB, 0, 0, a.depth, src);

    const size_t rec = (size_t)ctu * 85 + G::LBASE + pu;
    const int2 r0 = a.mv[0][rec], r1 = a.mv[1][rec];
    const long tileOff = (long)py * a.frefStrideB + (long)px * BPP;
    // REFS: the block's two list indices, clamped into the lists like the TU stages clamp theirs (every lane of the block reads the same
    // bytes).  Their loads are issued with those of the source tile and the records, in front of the barrier below.
    int idx[2] = { 0, 0 };
    const BdRefTables* tab = nullptr;
    if constexpr (REFS)
    {
        const size_t blk = (size_t)ctu * G::NPU + pu;
        idx[0] = clip3(0, ra.nrefs[0] - 1, (int)ra.refIdx[0][blk]);
        idx[1] = clip3(0, ra.nrefs[1] - 1, (int)ra.refIdx[1][blk]);
        if constexpr (G::NTILES == 64)
        {
            tab = &ra.t;
            idx[0] = __builtin_amdgcn_readfirstlane(idx[0]);
            idx[1] = __builtin_amdgcn_readfirstlane(idx[1]);
        }
        else
        {
            // wavefront w stages entries [4 (w & 1), + 4) of list w >> 1; nothing reads the tables before the barrier
            __shared__ BdRefTables sTab;
            const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int l = w >> 1, k0 = (w & 1) * (X265HIP_MAX_REFS / 2);
            if ((tid & 63) == 0)
            {
#pragma unroll
                for (int k = 0; k < X265HIP_MAX_REFS / 2; k++)
                {
                    sTab.fref[l][k0 + k] = ra.t.fref[l][k0 + k];
                    if (PL) sTab.planes[l][k0 + k] = ra.t.planes[l][k0 + k];
                    sTab.refCost[l][k0 + k] = ra.t.refCost[l][k0 + k];
                    sTab.refId[l][k0 + k] = ra.t.refId[l][k0 + k];
                }
            }
            __syncthreads();
            tab = &sTab;
        }
    }

    // P0 + P1 at the refined vectors and at (0,0): one pass per list, the interpolation code exists once
    int sumP[4][4] = {}, sumZ[4][4] = {};
#pragma unroll 1
    for (int l = 0; l < 2; l++)
    {
        const int w = l ? r1.y : r0.y;
        const int qx = (int16_t)(w & 0xffff), qy = w >> 16;
        const int xf = qx & 3, yf = qy & 3, ph = yf * 4 + xf;
        const uint8_t* z;
        const uint8_t* org;
        if constexpr (REFS)
        {
            const int i = l ? idx[1] : idx[0];
            z = tab->fref[l][i] + tileOff;
            org = ((PL && ph) ? tab->planes[l][i] + (long)(ph - 1) * a.planeBytes + tileOff : z)
                  + (long)(qy >> 2) * a.frefStrideB + (long)(qx >> 2) * BPP;
        }
        else
        {
            z = a.fref[l] + tileOff;
            org = ((PL && ph) ? a.planes[l] + (long)(ph - 1) * a.planeBytes + tileOff : z)
                  + (long)(qy >> 2) * a.frefStrideB + (long)(qx >> 2) * BPP;
        }
        int d[4][4];
        tile_predict<BPP>(org, a.frefStrideB, PL ? 0 : xf, PL ? 0 : yf, a.depth, d);
#pragma unroll
        for (int y = 0; y < 4; y++)
#pragma unroll
            for (int x = 0; x < 4; x++) sumP[y][x] += d[y][x];
        tile_predict<BPP>(z, a.frefStrideB, 0, 0, a.depth, d);
#pragma unroll
        for (int y = 0; y < 4; y++)
#pragma unroll
            for (int x = 0; x < 4; x++) sumZ[y][x] += d[y][x];
    }
#pragma unroll
    for (int y = 0; y < 4; y++)
#pragma unroll
        for (int x = 0; x < 4; x++)
        {
            sumP[y][x] = src[y][x] - ((sumP[y][x] + 1) >> 1);
            sumZ[y][x] = src[y][x] - ((sumZ[y][x] + 1) >> 1);
        }
    int sBi = tile_satd4(sumP), sZ = tile_satd4(sumZ);
    // sum over the block's NTILES consecutive lanes (every lane takes part)
    sBi = quad_sum(sBi); sZ = quad_sum(sZ);
    if (G::NTILES >= 16) { sBi = row_sum_of_quads(sBi); sZ = row_sum_of_quads(sZ); }
    if (G::NTILES >= 64) { sBi = wave_sum_of_rows(sBi); sZ = wave_sum_of_rows(sZ); }

    if constexpr (REFS) { if (tile == 0) bd_decide<true>(a, (size_t)ctu * G::NPU + pu, rec, r0, r1, sBi, sZ, tab, idx[0], idx[1]); }
    else if (tile == 0) bd_decide(a, (size_t)ctu * G::NPU + pu, rec, r0, r1, sBi, sZ);
}

// The chroma flavour (x265hip_bidir_decide_chroma): the records come from the chroma refinement, and the bidirectional candidate is
// measured on the motion-compensated prediction of all three planes - Predict::motionCompensation's bi arm without weights:
// predInterLumaShort / predInterChromaShort of both lists (14-bit intermediates) combined by addAvg (search.cpp:2487-2497, 2533-2543) -
// with satd(Y) + satd_c(Cb) + satd_c(Cr).  Same mapping; a block's NTILES / 4 chroma tiles per plane go to its lanes [0, NTILES / 4)
// (Cb) and [NTILES / 4, NTILES / 2) (Cr) after the luma tile, and the partial SATDs are added in front of the same DPP sums.
struct BidirChromaArgs
{
    const uint8_t* fencCb; const uint8_t* fencCr; long fencStrideCB;
    const uint8_t* fref0Cb; const uint8_t* fref0Cr;
    const uint8_t* fref1Cb; const uint8_t* fref1Cr; long frefStrideCB;
};

// SATD of one 4x4 tile against addAvg of both lists' intermediates, at the records' vectors (sBi) and at zero vectors (sZ).  z0 / z1 =
// byte address of the tile's sample (0,0) in each list's plane; CHROMA: eighth-sample vectors and the 4-tap filters.
template <int BPP, bool CHROMA>
__device__ __forceinline__ void bd_tile_costs(const uint8_t* fe, long fencStrideB, const uint8_t* z0, const uint8_t* z1, long frefStrideB,
                                              int w0, int w1, int depth, int& sBi, int& sZ)
{
    constexpr int SH = CHROMA ? 3 : 2, MASK = CHROMA ? 7 : 3;
    int src[4][4];
    tile_predict<BPP>(fe, fencStrideB, 0, 0, depth, src);
    int sumP[4][4] = {}, sumZ[4][4] = {};
#pragma unroll 1
    for (int l = 0; l < 2; l++)
    {
        const int w = l ? w1 : w0;
        const int qx = (int16_t)(w & 0xffff), qy = w >> 16;
        const uint8_t* z = l ? z1 : z0;
        const uint8_t* org = z + (long)(qy >> SH) * frefStrideB + (long)(qx >> SH) * BPP;
        int d[4][4], e[4][4];
        if (CHROMA) tile_predict_chroma<BPP, true>(org, frefStrideB, qx & MASK, qy & MASK, depth, d);
        else tile_predict<BPP, true>(org, frefStrideB, qx & MASK, qy & MASK, depth, d);
        tile_predict<BPP, true>(z, frefStrideB, 0, 0, depth, e);
#pragma unroll
        for (int y = 0; y < 4; y++)
#pragma unroll
            for (int x = 0; x < 4; x++)
            {
                sumP[y][x] = l ? src[y][x] - tile_add_avg(sumP[y][x], d[y][x], depth) : d[y][x];
                sumZ[y][x] = l ? src[y][x] - tile_add_avg(sumZ[y][x], e[y][x], depth) : e[y][x];
            }
    }
    sBi += tile_satd4(sumP); sZ += tile_satd4(sumZ);
}

template <typename Px, int LEVEL>
__global__ void __launch_bounds__(256) bidir_decide_chroma_kernel(BidirArgs a, BidirChromaArgs c)
{
    typedef BdGeom<LEVEL> G;
    constexpr int BPP = sizeof(Px), N = G::N, CTILES = G::NTILES / 4;
    const int ctu = xcd_swizzle(blockIdx.x, gridDim.x);
    const int cx = (ctu % a.ctusW) * 64, cy = (ctu / a.ctusW) * 64;
    const int tid = threadIdx.x;
    const int pu = tid >> G::TSHIFT, tile = tid & (G::NTILES - 1);
    const int bxz = (pu & 1) | ((pu >> 1) & 2) | ((pu >> 2) & 4), byz = ((pu >> 1) & 1) | ((pu >> 2) & 2) | ((pu >> 3) & 4);
    const int ty = tile / G::TPR, tx = tile % G::TPR;
    const int px = cx + bxz * N + tx * 4, py = cy + byz * N + ty * 4;

    const size_t rec = (size_t)ctu * 85 + G::LBASE + pu;
    const int2 r0 = a.mv[0][rec], r1 = a.mv[1][rec];
    const long tileOff = (long)py * a.frefStrideB + (long)px * BPP;

    int sBi = 0, sZ = 0;
    bd_tile_costs<BPP, false>(a.fenc + (long)py * a.fencStrideB + (long)px * BPP, a.fencStrideB, a.fref[0] + tileOff, a.fref[1] + tileOff, a.frefStrideB,
                              r0.y, r1.y, a.depth, sBi, sZ);
    if (tile < 2 * CTILES)
    {
        const int cpl = tile >= CTILES, ct = tile - cpl * CTILES;
        const int ccx = cx / 2 + bxz * (N / 2) + (ct % (G::TPR / 2)) * 4, ccy = cy / 2 + byz * (N / 2) + (ct / (G::TPR / 2)) * 4;
        const long cOff = (long)ccy * c.frefStrideCB + (long)ccx * BPP;
        bd_tile_costs<BPP, true>((cpl ? c.fencCr : c.fencCb) + (long)ccy * c.fencStrideCB + (long)ccx * BPP, c.fencStrideCB,
                                 (cpl ? c.fref0Cr : c.fref0Cb) + cOff, (cpl ? c.fref1Cr : c.fref1Cb) + cOff, c.frefStrideCB, r0.y, r1.y, a.depth, sBi, sZ);
    }
    sBi = quad_sum(sBi); sZ = quad_sum(sZ);
    if (G::NTILES >= 16) { sBi = row_sum_of_quads(sBi); sZ = row_sum_of_quads(sZ); }
    if (G::NTILES >= 64) { sBi = wave_sum_of_rows(sBi); sZ = wave_sum_of_rows(sZ); }

    if (tile == 0) bd_decide(a, (size_t)ctu * G::NPU + pu, rec, r0, r1, sBi, sZ);
}

template <typename Px>
static void bidir_chroma_launch(int level, int nctu, hipStream_t s, const BidirArgs& a, const BidirChromaArgs& c)
{
    switch (level)
    {
    case 0: hipLaunchKernelGGL((bidir_decide_chroma_kernel<Px, 0>), dim3(nctu), dim3(256), 0, s, a, c); break;
    case 1: hipLaunchKernelGGL((bidir_decide_chroma_kernel<Px, 1>), dim3(nctu), dim3(256), 0, s, a, c); break;
    default: hipLaunchKernelGGL((bidir_decide_chroma_kernel<Px, 2>), dim3(nctu), dim3(256), 0, s, a, c); break;
    }
}

template <typename Px, bool PL, class Args>
static void bidir_launch(int level, int nctu, hipStream_t s, const Args& a)
{
    switch (level)
    {
    case 0: hipLaunchKernelGGL((bidir_decide_kernel<Px, 0, PL, Args>), dim3(nctu), dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((bidir_decide_kernel<Px, 1, PL, Args>), dim3(nctu), dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((bidir_decide_kernel<Px, 2, PL, Args>), dim3(nctu), dim3(256), 0, s, a); break;
    }
}
// the luma decision of either record: phase planes or interpolation, one or two bytes per sample
template <class Args>
static void bidir_launch_luma(const bool planes, const int bpp, int level, int nctu, hipStream_t s, const Args& a)
{
    if (planes) { if (bpp == 1) bidir_launch<uint8_t, true>(level, nctu, s, a); else bidir_launch<uint16_t, true>(level, nctu, s, a); }
    else { if (bpp == 1) bidir_launch<uint8_t, false>(level, nctu, s, a); else bidir_launch<uint16_t, false>(level, nctu, s, a); }
}

// The decision reads both lists' records of a block after other blocks' outputs may have been written: the outputs must be buffers of their
// own.  True where mv0_out / mv1_out ([nctu * 85][2] int32 each) overlap mv0 / mv1 or each other.
static bool bidir_records_alias(const int nctu, const void* mv0, const void* mv1, const void* mv0Out, const void* mv1Out)
{
    const uintptr_t len = (uintptr_t)nctu * 85 * 8;
    const uintptr_t in[2] = { (uintptr_t)mv0, (uintptr_t)mv1 }, out[2] = { (uintptr_t)mv0Out, (uintptr_t)mv1Out };
    bool alias = out[0] < out[1] + len && out[1] < out[0] + len;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) alias = alias || (out[i] < in[j] + len && in[j] < out[i] + len);
    return alias;
}

} // namespace x265hip

using namespace x265hip;

extern "C" int x265hip_bidir_decide(const x265hip_bidir_params* p, void* stream)
{
    return x265hip_bidir_decide_chroma(p, nullptr, stream);
}

extern "C" int x265hip_bidir_decide_chroma(const x265hip_bidir_params* p, const x265hip_bidir_chroma* c, void* stream)
{
    // argument checks first: they need no device
    if (!p || !p->fenc || !p->fref0 || !p->fref1 || !p->mv0 || !p->mv1 || !p->cost_q || !p->dir || !p->mv0_out || !p->mv1_out)
    { set_error("bidir_decide: NULL operand"); return X265HIP_EINVAL; }
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("bidir_decide: depth %d", p->depth); return X265HIP_EINVAL; }
    if (p->level < 0 || p->level > 2) { set_error("bidir_decide: level %d out of [0,2]", p->level); return X265HIP_EINVAL; }
    if ((p->width & 63) || (p->height & 63) || p->width <= 0 || p->height <= 0) { set_error("bidir_decide: width/height must be multiples of 64"); return X265HIP_EINVAL; }
    const int nctu = (p->width / 64) * (p->height / 64);
    if (bidir_records_alias(nctu, p->mv0, p->mv1, p->mv0_out, p->mv1_out))
    { set_error("bidir_decide: mv0_out / mv1_out must not alias mv0 / mv1 or each other"); return X265HIP_EINVAL; }
    const bool planes = p->phase_planes0 || p->phase_planes1;
    if (planes && (!p->phase_planes0 || !p->phase_planes1 || p->phase_plane_samples <= 0))
    { set_error("bidir_decide: phase planes of both lists and phase_plane_samples are needed together"); return X265HIP_EINVAL; }
    if (c)
    {
        if (!c->fenc_cb || !c->fenc_cr || !c->fref0_cb || !c->fref0_cr || !c->fref1_cb || !c->fref1_cr)
        { set_error("bidir_decide_chroma: NULL chroma plane"); return X265HIP_EINVAL; }
        if (c->fenc_stride_c <= 0 || c->fref_stride_c <= 0) { set_error("bidir_decide_chroma: chroma strides must be positive"); return X265HIP_EINVAL; }
        if (planes) { set_error("bidir_decide_chroma: the luma phase planes hold rounded pixels and cannot serve the chroma flavour"); return X265HIP_EINVAL; }
    }
    int rc = ensure_device();
    if (rc) return rc;

    const int bpp = p->depth == 8 ? 1 : 2;
    BidirArgs a;
    a.fenc = (const uint8_t*)p->fenc; a.fencStrideB = (long)p->fenc_stride * bpp;
    a.fref[0] = (const uint8_t*)p->fref0; a.fref[1] = (const uint8_t*)p->fref1; a.frefStrideB = (long)p->fref_stride * bpp;
    a.ctusW = p->width / 64; a.depth = p->depth;
    a.mv[0] = (const int2*)p->mv0; a.mv[1] = (const int2*)p->mv1;
    a.costQ = p->cost_q; a.qoff = p->qoff;
    for (int i = 0; i < 3; i++) a.dirCost[i] = p->dir_cost[i];
    a.refId[0] = p->ref_id0; a.refId[1] = p->ref_id1;
    a.planes[0] = (const uint8_t*)p->phase_planes0; a.planes[1] = (const uint8_t*)p->phase_planes1;
    a.planeBytes = (long)p->phase_plane_samples * bpp;
    a.dir = p->dir; a.ref[0] = p->ref0; a.ref[1] = p->ref1;
    a.mvOut[0] = (int2*)p->mv0_out; a.mvOut[1] = (int2*)p->mv1_out;
    a.costOut = p->cost_out;
    hipStream_t s = (hipStream_t)stream;
    if (c)
    {
        BidirChromaArgs ca;
        ca.fencCb = (const uint8_t*)c->fenc_cb; ca.fencCr = (const uint8_t*)c->fenc_cr; ca.fencStrideCB = (long)c->fenc_stride_c * bpp;
        ca.fref0Cb = (const uint8_t*)c->fref0_cb; ca.fref0Cr = (const uint8_t*)c->fref0_cr;
        ca.fref1Cb = (const uint8_t*)c->fref1_cb; ca.fref1Cr = (const uint8_t*)c->fref1_cr; ca.frefStrideCB = (long)c->fref_stride_c * bpp;
        if (bpp == 1) bidir_chroma_launch<uint8_t>(p->level, nctu, s, a, ca); else bidir_chroma_launch<uint16_t>(p->level, nctu, s, a, ca);
    }
    else bidir_launch_luma(planes, bpp, p->level, nctu, s, a);
    X265HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int x265hip_bidir_decide_refs(const x265hip_bidir_refs_params* p, void* stream)
{
    // argument checks first: they need no device
    if (!p || !p->fenc || !p->mv0 || !p->mv1 || !p->ref_idx0 || !p->ref_idx1 || !p->cost_q || !p->dir || !p->mv0_out || !p->mv1_out)
    { set_error("bidir_decide_refs: NULL operand"); return X265HIP_EINVAL; }
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("bidir_decide_refs: depth %d", p->depth); return X265HIP_EINVAL; }
    if (p->level < 0 || p->level > 2) { set_error("bidir_decide_refs: level %d out of [0,2]", p->level); return X265HIP_EINVAL; }
    if ((p->width & 63) || (p->height & 63) || p->width <= 0 || p->height <= 0) { set_error("bidir_decide_refs: width/height must be multiples of 64"); return X265HIP_EINVAL; }
    const int nrefs[2] = { p->nrefs0, p->nrefs1 };
    const void* const* fref[2] = { p->fref0, p->fref1 };
    const void* const* pplanes[2] = { p->phase_planes0, p->phase_planes1 };
    int withPlanes = 0;
    for (int l = 0; l < 2; l++)
    {
        if (nrefs[l] < 1 || nrefs[l] > X265HIP_MAX_REFS) { set_error("bidir_decide_refs: nrefs%d %d out of [1,%d]", l, nrefs[l], X265HIP_MAX_REFS); return X265HIP_EINVAL; }
        for (int k = 0; k < nrefs[l]; k++)
        {
            if (!fref[l][k]) { set_error("bidir_decide_refs: NULL plane of reference %d of list %d", k, l); return X265HIP_EINVAL; }
            withPlanes += pplanes[l][k] != nullptr;
        }
    }
    const int nctu = (p->width / 64) * (p->height / 64);
    if (bidir_records_alias(nctu, p->mv0, p->mv1, p->mv0_out, p->mv1_out))
    { set_error("bidir_decide_refs: mv0_out / mv1_out must not alias mv0 / mv1 or each other"); return X265HIP_EINVAL; }
    const bool planes = withPlanes != 0;
    if (planes && (withPlanes != nrefs[0] + nrefs[1] || p->phase_plane_samples <= 0))
    { set_error("bidir_decide_refs: phase planes of every listed reference and phase_plane_samples are needed together"); return X265HIP_EINVAL; }
    int rc = ensure_device();
    if (rc) return rc;

    const int bpp = p->depth == 8 ? 1 : 2;
    BidirRefsArgs ra = {};
    BidirArgs& a = ra.b;
    a.fenc = (const uint8_t*)p->fenc; a.fencStrideB = (long)p->fenc_stride * bpp;
    a.frefStrideB = (long)p->fref_stride * bpp;
    a.ctusW = p->width / 64; a.depth = p->depth;
    a.mv[0] = (const int2*)p->mv0; a.mv[1] = (const int2*)p->mv1;
    a.costQ = p->cost_q; a.qoff = p->qoff;
    for (int i = 0; i < 3; i++) a.dirCost[i] = p->dir_cost[i];
    a.planeBytes = (long)p->phase_plane_samples * bpp;
    a.dir = p->dir; a.ref[0] = p->ref0; a.ref[1] = p->ref1;
    a.mvOut[0] = (int2*)p->mv0_out; a.mvOut[1] = (int2*)p->mv1_out;
    a.costOut = p->cost_out;
    const int32_t* refCost[2] = { p->ref_cost0, p->ref_cost1 };
    const int* refIds[2] = { p->ref_ids0, p->ref_ids1 };
    for (int l = 0; l < 2; l++)
    {
        // entries behind nrefs repeat the last reference: the kernel clamps the index, and no entry of the tables is left dangling
        for (int k = 0; k < X265HIP_MAX_REFS; k++)
        {
            const int r = k < nrefs[l] ? k : nrefs[l] - 1;
            ra.t.fref[l][k] = (const uint8_t*)fref[l][r];
            ra.t.planes[l][k] = planes ? (const uint8_t*)pplanes[l][r] : nullptr;
            ra.t.refCost[l][k] = refCost[l][r];
            ra.t.refId[l][k] = refIds[l][r];
        }
        ra.nrefs[l] = nrefs[l];
    }
    ra.refIdx[0] = p->ref_idx0; ra.refIdx[1] = p->ref_idx1;
    bidir_launch_luma(planes, bpp, p->level, nctu, (hipStream_t)stream, ra);
    X265HIP_TRY(hipGetLastError());
    return 0;
}
