// intra_picture.h - one I picture on the block grid of the TU stages, on gfx950 (included at the end of tu_kernels.hip: it codes its blocks
// with that file's tu_chain / TuOpsFor, which are local to it).
//
// Every N x N block (N = 8 << level) is a 2Nx2N intra CU with one TU.  Per block, in coding order (CTUs in raster order, blocks in
// z-order inside a CTU):
//   neighbours   Predict::initIntraNeighbors + fillReferenceSamples (source/common/predict.cpp:664-876, I-slice arm): a neighbouring block
//                is available iff it lies inside the picture and precedes the block in coding order.  All blocks have one size and the
//                picture is made of whole CTUs, so availability is ONE flag per arm - below-left, left, corner, above, above-right - and the
//                substitution walk has a closed form per sample: an unavailable arm takes the last sample of the nearest available arm
//                before it on the path bottom-left -> corner -> top-right, a leading unavailable run the first sample of the first
//                available arm, and 1 << (depth - 1) when nothing is available.  Unavailable samples are never read.
//   filtering    Predict::initAdiPattern, ALL_IDX arm (:600-650): the bilinear form for 32x32 under strong_intra_smoothing when both
//                threshold tests pass, else intraFilter's [1 2 1] (intrapred.cpp:32-51)
//   decision     Search::checkIntraInInter without bEnableFastIntra (source/encoder/search.cpp:1344-1446): sa8d of all 35 predictions,
//                cost = sad + ((bits * lambda8 + 128) >> 8), strict '<' in the order DC, planar, 2..34; bits from the three most probable
//                modes of CUData::getIntraDirLumaPredictor (cudata.cpp:910-953)
//   coding       the contract of x265hip_intra_recon_batch for the winner, luma and (4:2:0, DM_CHROMA) both chroma blocks
//
// Schedule: CTU (cx, cy) reads reconstructed samples of CTUs (cx - 1, cy), (cx - 1, cy - 1), (cx, cy - 1) and (cx + 1, cy - 1), so it may
// run in wave cx + 2 cy.  The entry issues ONE LAUNCH PER WAVE on the caller's stream: launch boundaries give ordering and visibility,
// there is no wait of one workgroup on another.  Inside a launch one workgroup of 256 threads walks the blocks of its CTU; the CTU's own
// reconstruction lives in LDS (tu_chain reconstructs into it), only neighbours of earlier CTUs are read from the recon planes.
//
// The 35-mode scan: a work item is (scan position, 8x8 tile, row); eight consecutive lanes hold the eight rows of one tile's difference,
// predicted sample by sample with intra_sample().  The 8x8 Hadamard runs in registers (rows in the lane, columns across the eight
// lanes), the four tiles of a 16x16 unit sit on 32 consecutive lanes and are rounded once (sa8d_16x16, pixel.cpp:341-352).  Unit sums go
// to LDS - one writer per slot - and 35 lanes of wavefront 0 form the costs and take the minimum of cost << 6 | scan position by
// shuffles.  No atomics.
//
// x265hip_intra_in_inter is the same kernel body for the blocks of a P picture (Args = IntraInInterArgs): the tiles start as the inter
// reconstruction, and a block is coded only where its intra cost is strictly below the inter candidate's (x265hip_inter_sa8d_cost).
#pragma once

namespace x265hip {

struct IntraPicArgs
{
    const uint8_t* fenc[3]; long fencStrideB[3];          // Y, Cb, Cr: sample (0,0)
    uint8_t* recon[3]; long reconStrideB[3];
    int ctusW, ctusH, depth, qp[3], flags, strong, chroma;
    int lambda8, modeBits[3];
    uint8_t* mode;
    int16_t* levels[3]; uint32_t* numSig[3]; unsigned long long* dist[3];
    int2* cost;                                           // optional [ctu][blocks] {winning sad, winning cost}
    const int8_t* qpMap;                                  // optional int8 [3][ctusH * 8][ctusW * 8]: the quantiser QPs of Y, Cb, Cr per 8x8 cell of the luma grid
    const uint32_t* lambdaByQp;                           // optional, indexed by the block's luma quantiser QP
};

// x265hip_intra_in_inter: the same record plus the inter candidate's cost per block and the flags the choice leaves
struct IntraInInterArgs
{
    IntraPicArgs a;
    const int32_t* interCost; long interCostStride;       // inter_cost[blk * stride]: x265hip_inter_sa8d_cost's cost word
    uint8_t* intra;                                       // [ctu][blocks]: 1 = the block is intra
};
__device__ __forceinline__ const IntraPicArgs& ip_args(const IntraPicArgs& a) { return a; }
__device__ __forceinline__ const IntraPicArgs& ip_args(const IntraInInterArgs& r) { return r.a; }

// The 4M + 1 reference samples of an M x M block at (bx0, by0) of its CTU's tile (TW x TW samples of type Px in LDS, the CTU's own
// reconstruction) into nb[]: [0] corner, [1..2M] above + above-right, [2M+1..4M] left + below-left.  av = availability of the arms
// below-left, left, corner, above, above-right; plane = sample (0,0) of the CTU in the recon plane (earlier CTUs' samples).
template <typename Px, int M, int TW>
__device__ __forceinline__ void ip_fill_neighbours(int16_t* nb, const Px* tile, const Px* plane, const long stride, const int bx0, const int by0,
                                                   const bool (&av)[5], const int dcValue)
{
    const int segStart[5] = { 0, M, 2 * M, 2 * M + 1, 3 * M + 1 }, segEnd[5] = { M - 1, 2 * M - 1, 2 * M, 3 * M, 4 * M };
    for (int i = threadIdx.x; i <= 4 * M; i += blockDim.x)
    {
        const int seg = i < M ? 0 : (i < 2 * M ? 1 : (i == 2 * M ? 2 : (i <= 3 * M ? 3 : 4)));
        int src = -1;
        if (av[seg]) src = i;
        else
        {
#pragma unroll
            for (int s = 0; s < 5; s++) if (s < seg && av[s]) src = segEnd[s];                       // the nearest available arm before
            if (src < 0)
            {
#pragma unroll
                for (int s = 4; s >= 0; s--) if (s > seg && av[s]) src = segStart[s];               // a leading run: the first available sample
            }
        }
        int v = dcValue;
        if (src >= 0)
        {
            const int x = src < 2 * M ? bx0 - 1 : (src == 2 * M ? bx0 - 1 : bx0 + src - 2 * M - 1);
            const int y = src < 2 * M ? by0 + 2 * M - 1 - src : by0 - 1;
            v = (x >= 0 && y >= 0 && x < TW && y < TW) ? (int)tile[y * TW + x] : (int)plane[(long)y * stride + x];
        }
        nb[i < 2 * M ? 4 * M - i : (i == 2 * M ? 0 : i - 2 * M)] = (int16_t)v;
    }
}

// Args = IntraPicArgs: an I picture.  Args = IntraInInterArgs (INP): the intra candidate of a P picture's blocks - the CTU's tiles start as
// the inter reconstruction the inter TU stages left in the recon planes, and a block is coded only where its intra cost is strictly below
// the inter candidate's (Analysis::compressInterCU_rd0_4, analysis.cpp:1664); a block that stays inter reads as DC to its neighbours' most
// probable modes (getIntraDirLumaPredictor tests isIntra).  INP is a parameter of the kernel, as REFS is of inter_recon_kernel: the I
// instances are compiled from the same body with the other flavour's statements discarded.
template <typename Px, int N, class Args = IntraPicArgs>
__global__ void __launch_bounds__(256) intra_picture_kernel(Args ra, const int wave, const int cyLo)
{
    constexpr bool INP = std::is_same<Args, IntraInInterArgs>::value;
    const IntraPicArgs& a = ip_args(ra);
    constexpr int NN = N * N, LOG2N = N == 8 ? 3 : (N == 16 ? 4 : 5), NC = N / 2, BPC = 64 / N, NPU = BPC * BPC, BPP = sizeof(Px);
    constexpr int UNITS = N == 32 ? 4 : 1, TPU = N == 8 ? 1 : 4, ITEMS = 35 * UNITS * TPU * 8;
    __shared__ __attribute__((aligned(16))) Px tileY[64 * 64];
    __shared__ __attribute__((aligned(16))) Px tileC[2][32 * 32];
    __shared__ int16_t nbU[4 * N + 4], nbF[4 * N + 4];
    __shared__ __attribute__((aligned(16))) int16_t pred[NN], fe[NN], A[NN], B[NN];
    __shared__ unsigned long long red[4];
    __shared__ int sNumSig, sDc, sBest[3], sUnit[35 * UNITS];
    __shared__ uint8_t sMode[64];

    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63;
    const int cyb = cyLo + (int)blockIdx.x, cxb = wave - 2 * cyb;
    const int ctu = cyb * a.ctusW + cxb;
    const int maxVal = (1 << a.depth) - 1, dcValue = 1 << (a.depth - 1);
    const int blocksW = a.ctusW * BPC, blocksH = a.ctusH * BPC;
    TuOpsFor<N, false> ops;
    ops.init(lane);
    TuOpsFor<NC, false> opsC;
    opsC.init(lane);
    const Px* planeY = reinterpret_cast<const Px*>(a.recon[0] + (long)cyb * 64 * a.reconStrideB[0]) + cxb * 64;
    const long strideY = a.reconStrideB[0] / BPP;
    if constexpr (INP)
    {
        // the CTU's tiles = its inter reconstruction: a block that stays inter keeps it, and later blocks predict from it
        for (int i = tid; i < 64 * 64; i += nth) tileY[i] = planeY[(long)(i >> 6) * strideY + (i & 63)];
        if (a.chroma)
            for (int c = 0; c < 2; c++)
            {
                const Px* planeC = reinterpret_cast<const Px*>(a.recon[1 + c] + (long)cyb * 32 * a.reconStrideB[1 + c]) + cxb * 32;
                const long strideC = a.reconStrideB[1 + c] / BPP;
                for (int i = tid; i < 32 * 32; i += nth) tileC[c][i] = planeC[(long)(i >> 5) * strideC + (i & 31)];
            }
        __syncthreads();
    }

    for (int z = 0; z < NPU; z++)
    {
        const int bxz = ip_zpos(z).x, byz = ip_zpos(z).y;
        const int gbx = cxb * BPC + bxz, gby = cyb * BPC + byz;
        // a neighbouring block is available iff it is inside the picture and precedes this one in coding order
        auto available = [&](const int nbx, const int nby)
        {
            if (nbx < 0 || nby < 0 || nbx >= blocksW || nby >= blocksH) return false;
            const int ncx = nbx / BPC, ncy = nby / BPC;
            if (ncx != cxb || ncy != cyb) return ncy * a.ctusW + ncx < ctu;
            return ip_zidx(nbx - ncx * BPC, nby - ncy * BPC) < z;
        };
        const bool av[5] = { available(gbx - 1, gby + 1), available(gbx - 1, gby), available(gbx - 1, gby - 1), available(gbx, gby - 1),
                             available(gbx + 1, gby - 1) };
        // the block's own three QPs and lambda (uniform: scalar loads, see tu_map_qp); without the pointers the record's values
        int qpB[3] = { a.qp[0], a.qp[1], a.qp[2] };
        if (a.qpMap)
        {
            const int cell = (gby * (N >> 3)) * (a.ctusW * 8) + gbx * (N >> 3), plane = (a.ctusH * 8) * (a.ctusW * 8);
#pragma unroll
            for (int c = 0; c < 3; c++) qpB[c] = tu_map_qp(a.qpMap + (size_t)c * plane, cell, a.depth);
        }
        int lambda8 = a.lambda8;
        if (a.lambdaByQp)
        {
            typedef const uint32_t __attribute__((address_space(4))) * ConstWords;
            const uint32_t l = ((ConstWords)reinterpret_cast<uintptr_t>(a.lambdaByQp))[__builtin_amdgcn_readfirstlane(qpB[0])];
            lambda8 = clamp_lambda8(l);
        }
        // ---- luma: reference samples, filtered copy, source block -----------------------------------------------------------------
        ip_fill_neighbours<Px, N, 64>(nbU, tileY, planeY, strideY, bxz * N, byz * N, av, dcValue);
        {
            const Px* f = reinterpret_cast<const Px*>(a.fenc[0] + (long)(gby * N) * a.fencStrideB[0]) + gbx * N;
            const long fst = a.fencStrideB[0] / BPP;
            for (int i = tid; i < NN; i += nth) { const int y = i >> LOG2N, x = i & (N - 1); fe[i] = (int16_t)f[y * fst + x]; }
        }
        if (tid == 0) sNumSig = 0;
        __syncthreads();
        {
            const int topLeft = nbU[0], topLast = nbU[2 * N], leftLast = nbU[4 * N];
            bool strong = false;
            if (N == 32 && a.strong)
            {
                const int threshold = 1 << (a.depth - 5);
                strong = abs(topLeft + topLast - 2 * (int)nbU[32]) < threshold && abs(topLeft + leftLast - 2 * (int)nbU[2 * N + 32]) < threshold;
            }
            for (int i = tid; i <= 4 * N; i += nth)
            {
                int v;
                if (i == 2 * N || i == 4 * N) v = nbU[i];
                else if (strong)
                {
                    const int k = i > 2 * N ? i - 2 * N : i;
                    v = i == 0 ? topLeft : (((topLeft << 6) + N + ((i > 2 * N ? leftLast : topLast) - topLeft) * k) >> 6);
                }
                else if (i == 0) v = (2 * topLeft + (int)nbU[1] + (int)nbU[2 * N + 1] + 2) >> 2;
                else v = (2 * (int)nbU[i] + (i == 2 * N + 1 ? topLeft : (int)nbU[i - 1]) + (int)nbU[i + 1] + 2) >> 2;
                nbF[i] = (int16_t)v;
            }
            // dcVal (intrapred.cpp:95-110) of the unfiltered neighbours
            if (tid < 64)
            {
                int part = 0;
                for (int i = tid; i < 2 * N; i += 64) part += i < N ? nbU[1 + i] : nbU[2 * N + 1 + (i - N)];
                part = group_sum<64>(part);
                if (tid == 0) sDc = (part + N) / (2 * N);
            }
        }
        __syncthreads();
        const int dc = sDc;
        constexpr int bFilter = N <= 16;
        // ---- the scan: sa8d of the 35 predictions -------------------------------------------------------------------------------------
        for (int t0 = 0; t0 < ITEMS; t0 += 256)
        {
            const int t = t0 + tid;
            const bool live = t < ITEMS;
            const int tt = live ? t : 0;
            const int row = tt & 7, pair = tt >> 3, q = pair % TPU, mu = pair / TPU, unit = mu % UNITS, s = mu / UNITS;
            const int mode = s == 0 ? 1 : (s == 1 ? 0 : s);
            const int tx = (unit & 1) * 2 + (q & 1), ty = (unit >> 1) * 2 + (q >> 1);
            const int y = ty * 8 + row, x0 = tx * 8;
            const int16_t* nbm = (mode != 1 && (kIsFilterFlags[mode] & N)) ? nbF : nbU;
            int d[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                d[i] = live ? (int)fe[y * N + x0 + i] - intra_sample(nbm, N, LOG2N, mode, bFilter, dc, maxVal, x0 + i, y) : 0;
            int raw = ip_hadamard8x8(d, lane);
            if (TPU == 4) { raw += __shfl_xor(raw, 8, 64); raw += __shfl_xor(raw, 16, 64); }
            if (live && (tt & (8 * TPU - 1)) == 0) sUnit[mu] = (raw + 2) >> 2;
        }
        __syncthreads();
        // ---- most probable modes, costs, the minimum ------------------------------------------------------------------------------------
        if (tid < 64)
        {
            int left = 1, above = 1;                                        // DC_IDX where the neighbour does not count
            if (gbx > 0) left = bxz > 0 ? (int)sMode[ip_zidx(bxz - 1, byz)] : (int)a.mode[(size_t)(ctu - 1) * NPU + ip_zidx(BPC - 1, byz)];
            if (byz > 0) above = sMode[ip_zidx(bxz, byz - 1)];              // the above block counts only inside the CTU
            int p0, p1, p2;
            if (left == above)
            {
                if (left >= 2) { p0 = left; p1 = ((left - 2 + 31) & 31) + 2; p2 = ((left - 2 + 1) & 31) + 2; }
                else { p0 = 0; p1 = 1; p2 = 26; }
            }
            else { p0 = left; p1 = above; p2 = (left && above) ? 0 : (left + above < 2 ? 26 : 1); }
            unsigned long long key = ~0ull;
            int sad = 0;
            long long cost = 0;
            const int mode = tid == 0 ? 1 : (tid == 1 ? 0 : tid);
            if (tid < 35)
            {
#pragma unroll
                for (int u = 0; u < UNITS; u++) sad += sUnit[tid * UNITS + u];
                const int bits = mode == p0 ? a.modeBits[0] : ((mode == p1 || mode == p2) ? a.modeBits[1] : a.modeBits[2]);
                cost = (long long)sad + rd_sad_rate(bits, lambda8);
                key = ((unsigned long long)cost << 6) | (unsigned)tid;
            }
            unsigned long long best = key;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) { const unsigned long long o = __shfl_xor(best, m, 64); best = o < best ? o : best; }
            if (tid < 35 && key == best) { sBest[0] = mode; sBest[1] = sad; sBest[2] = (int)cost; }
        }
        __syncthreads();
        if constexpr (INP)
        {
            // intra wins iff its cost is strictly lower; a block that stays inter keeps every output of the inter TU stages
            const size_t blkP = (size_t)ctu * NPU + z;
            if (!(sBest[2] < ra.interCost[blkP * ra.interCostStride]))
            {
                if (tid == 0)
                {
                    a.mode[blkP] = 1;
                    sMode[z] = 1;
                    ra.intra[blkP] = 0;
                    if (a.cost) a.cost[blkP] = make_int2(sBest[1], sBest[2]);
                }
                __syncthreads();
                continue;
            }
        }
        const int mode = sBest[0];
        {
            const int16_t* nbm = (mode != 1 && (kIsFilterFlags[mode] & N)) ? nbF : nbU;
            for (int i = tid; i < NN; i += nth)
                pred[i] = (int16_t)intra_sample(nbm, N, LOG2N, mode, bFilter, dc, maxVal, i & (N - 1), i >> LOG2N);
        }
        __syncthreads();
        const size_t blk = (size_t)ctu * NPU + z;
        const int scanLuma = N == 8 ? (mode >= 22 && mode <= 30 ? TU_SCAN_HOR : (mode >= 6 && mode <= 14 ? TU_SCAN_VER : TU_SCAN_DIAG)) : TU_SCAN_DIAG;
        tu_chain<Px, N, false, false>(ops, pred, fe, A, B, red, sNumSig, a.depth, qpB[0], a.flags, a.levels[0] + blk * NN, &a.numSig[0][blk], &a.dist[0][blk],
                                      tileY + (byz * N) * 64 + bxz * N, 64, scanLuma);
        __syncthreads();
        {
            Px* r = reinterpret_cast<Px*>(a.recon[0] + (long)(gby * N) * a.reconStrideB[0]) + gbx * N;
            for (int i = tid; i < NN; i += nth) { const int y = i >> LOG2N, x = i & (N - 1); r[y * strideY + x] = tileY[(byz * N + y) * 64 + bxz * N + x]; }
            if (tid == 0)
            {
                a.mode[blk] = (uint8_t)mode;
                sMode[z] = (uint8_t)mode;
                if (a.cost) a.cost[blk] = make_int2(sBest[1], sBest[2]);
                if constexpr (INP) ra.intra[blk] = 1;
            }
        }
        // ---- chroma (4:2:0): the luma mode, unfiltered neighbours of the plane's own reconstruction, no edge smoothing ---------------
        if (a.chroma)
        {
            constexpr int NNC = NC * NC, LOG2NC = LOG2N - 1;
            const int scanC = NC == 4 ? (mode >= 22 && mode <= 30 ? TU_SCAN_HOR : (mode >= 6 && mode <= 14 ? TU_SCAN_VER : TU_SCAN_DIAG)) : TU_SCAN_DIAG;
            for (int c = 0; c < 2; c++)
            {
                const long strideC = a.reconStrideB[1 + c] / BPP;
                const Px* planeC = reinterpret_cast<const Px*>(a.recon[1 + c] + (long)cyb * 32 * a.reconStrideB[1 + c]) + cxb * 32;
                __syncthreads();                                          // pred / fe / nbU of the previous chain are free
                ip_fill_neighbours<Px, NC, 32>(nbU, tileC[c], planeC, strideC, bxz * NC, byz * NC, av, dcValue);
                {
                    const Px* f = reinterpret_cast<const Px*>(a.fenc[1 + c] + (long)(gby * NC) * a.fencStrideB[1 + c]) + gbx * NC;
                    const long fst = a.fencStrideB[1 + c] / BPP;
                    for (int i = tid; i < NNC; i += nth) { const int y = i >> LOG2NC, x = i & (NC - 1); fe[i] = (int16_t)f[y * fst + x]; }
                }
                if (tid == 0) sNumSig = 0;
                __syncthreads();
                if (tid < 64)
                {
                    int part = 0;
                    for (int i = tid; i < 2 * NC; i += 64) part += i < NC ? nbU[1 + i] : nbU[2 * NC + 1 + (i - NC)];
                    part = group_sum<64>(part);
                    if (tid == 0) sDc = (part + NC) / (2 * NC);
                }
                __syncthreads();
                const int dcC = sDc;
                for (int i = tid; i < NNC; i += nth)
                    pred[i] = (int16_t)intra_sample(nbU, NC, LOG2NC, mode, 0, dcC, maxVal, i & (NC - 1), i >> LOG2NC);
                __syncthreads();
                tu_chain<Px, NC, false, false>(opsC, pred, fe, A, B, red, sNumSig, a.depth, c ? qpB[2] : qpB[1], a.flags, a.levels[1 + c] + blk * NNC,
                                               &a.numSig[1 + c][blk], &a.dist[1 + c][blk], tileC[c] + (byz * NC) * 32 + bxz * NC, 32, scanC);
                __syncthreads();
                Px* r = reinterpret_cast<Px*>(a.recon[1 + c] + (long)(gby * NC) * a.reconStrideB[1 + c]) + gbx * NC;
                for (int i = tid; i < NNC; i += nth) { const int y = i >> LOG2NC, x = i & (NC - 1); r[y * strideC + x] = tileC[c][(byz * NC + y) * 32 + bxz * NC + x]; }
            }
        }
        __syncthreads();
    }
}

} // namespace x265hip

/* waves of the I-picture schedule: CTU (cx, cy) runs in wave cx + 2 cy */
extern "C" int x265hip_intra_picture_waves(int width, int height)
{
    if ((width & 63) || (height & 63) || width <= 0 || height <= 0) { x265hip::set_error("intra_picture_waves: width/height must be multiples of 64"); return X265HIP_EINVAL; }
    return x265hip::decision_wave_count(width / 64, height / 64);
}

namespace x265hip {

// The argument checks and the wave-by-wave launches of x265hip_intra_picture_qp and x265hip_intra_in_inter (inP: the P flavour, with its three operands).
static int intra_picture_launch(const char* who, const x265hip_intra_picture_params* p, const int8_t* qp_map, const uint32_t* lambda8_by_qp,
                                const int32_t* inter_cost, intptr_t inter_cost_stride, uint8_t* intra, const bool inP, void* stream)
{
    // argument checks first: they need no device
    if (decision_record_refused(who, p, !p || !p->fenc || !p->recon || !p->mode || !p->levels || !p->num_sig || !p->dist || (inP && (!inter_cost || !intra))))
        return X265HIP_EINVAL;
    const int qpMax = 51 + 6 * (p->depth - 8);
    const bool chroma = p->fenc_cb || p->fenc_cr || p->recon_cb || p->recon_cr;
    if (chroma)
    {
        if (!p->fenc_cb || !p->fenc_cr || !p->recon_cb || !p->recon_cr || !p->levels_cb || !p->levels_cr || !p->num_sig_cb || !p->num_sig_cr || !p->dist_cb || !p->dist_cr)
        { set_error("%s: the chroma planes and outputs of Cb and Cr are needed together", who); return X265HIP_EINVAL; }
        if (p->qp_cb < 0 || p->qp_cb > qpMax || p->qp_cr < 0 || p->qp_cr > qpMax) { set_error("%s: chroma qp %d / %d out of range", who, p->qp_cb, p->qp_cr); return X265HIP_EINVAL; }
    }
    if (inP)
    {
        if (inter_cost_stride_refused(who, inter_cost_stride)) return X265HIP_EINVAL;
        if (p->flags & TU_FLAG_INTRA_SLICE) { set_error("%s: X265HIP_TU_INTRA_SLICE in the flags of a P slice", who); return X265HIP_EINVAL; }
    }
    if (p->flags & ~(TU_FLAG_INTRA_SLICE | TU_FLAG_SIGN_HIDE)) { set_error("%s: unknown flag bits 0x%x", who, p->flags); return X265HIP_EINVAL; }
    if (chroma && (p->fenc_stride_c < p->width / 2 || p->recon_stride_c < p->width / 2)) { set_error("%s: chroma stride below half the width", who); return X265HIP_EINVAL; }
    // mode_bits <= 4096: with the shared bound of lambda8 the winning cost fits the int32 of `cost`
    for (int i = 0; i < 3; i++)
        if (p->mode_bits[i] < 0 || p->mode_bits[i] > 4096) { set_error("%s: mode_bits[%d] = %d out of [0, 4096]", who, i, p->mode_bits[i]); return X265HIP_EINVAL; }
    if (p->fenc == p->recon || (chroma && (p->fenc_cb == p->recon_cb || p->fenc_cr == p->recon_cr || p->recon_cb == p->recon_cr)))
    { set_error("%s: the recon planes must not alias the source planes or each other", who); return X265HIP_EINVAL; }
    if (p->tables) { set_error("%s: tables are not supported by this stage (pass NULL)", who); return X265HIP_EINVAL; }
    int rc = ensure_device();
    if (rc) return rc;

    const int bpp = p->depth == 8 ? 1 : 2;
    IntraPicArgs a = {};
    a.fenc[0] = (const uint8_t*)p->fenc; a.fencStrideB[0] = (long)p->fenc_stride * bpp;
    a.recon[0] = (uint8_t*)p->recon; a.reconStrideB[0] = (long)p->recon_stride * bpp;
    a.levels[0] = p->levels; a.numSig[0] = p->num_sig; a.dist[0] = (unsigned long long*)p->dist;
    a.qp[0] = p->qp;
    if (chroma)
    {
        a.fenc[1] = (const uint8_t*)p->fenc_cb; a.fenc[2] = (const uint8_t*)p->fenc_cr; a.fencStrideB[1] = a.fencStrideB[2] = (long)p->fenc_stride_c * bpp;
        a.recon[1] = (uint8_t*)p->recon_cb; a.recon[2] = (uint8_t*)p->recon_cr; a.reconStrideB[1] = a.reconStrideB[2] = (long)p->recon_stride_c * bpp;
        a.levels[1] = p->levels_cb; a.numSig[1] = p->num_sig_cb; a.dist[1] = (unsigned long long*)p->dist_cb;
        a.levels[2] = p->levels_cr; a.numSig[2] = p->num_sig_cr; a.dist[2] = (unsigned long long*)p->dist_cr;
        a.qp[1] = p->qp_cb; a.qp[2] = p->qp_cr;
    }
    a.ctusW = p->width / 64; a.ctusH = p->height / 64; a.depth = p->depth;
    a.flags = p->flags; a.strong = p->strong_intra_smoothing != 0; a.chroma = chroma;
    a.lambda8 = p->lambda8;
    for (int i = 0; i < 3; i++) a.modeBits[i] = p->mode_bits[i];
    a.mode = p->mode; a.cost = (int2*)p->cost;
    a.qpMap = qp_map; a.lambdaByQp = lambda8_by_qp;
    IntraInInterArgs ia = { a, inter_cost, (long)inter_cost_stride, intra };
    hipStream_t s = (hipStream_t)stream;
    for_each_wave(a.ctusW, a.ctusH, [&](const int w, const int cyLo, const int n)
    {
        for_depth_level(p->depth, p->level, [&](auto px, auto size)
        {
            using Px = decltype(px);
            constexpr int N = decltype(size)::value;
            if (inP) hipLaunchKernelGGL((intra_picture_kernel<Px, N, IntraInInterArgs>), dim3(n), dim3(256), 0, s, ia, w, cyLo);
            else hipLaunchKernelGGL((intra_picture_kernel<Px, N, IntraPicArgs>), dim3(n), dim3(256), 0, s, a, w, cyLo);
        });
    });
    X265HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace x265hip

extern "C" int x265hip_intra_picture_qp(const x265hip_intra_picture_params* p, const int8_t* qp_map, const uint32_t* lambda8_by_qp, void* stream)
{
    return x265hip::intra_picture_launch("intra_picture", p, qp_map, lambda8_by_qp, nullptr, 0, nullptr, false, stream);
}

extern "C" int x265hip_intra_in_inter(const x265hip_intra_picture_params* p, const int32_t* inter_cost, intptr_t inter_cost_stride, uint8_t* intra,
                                      const int8_t* qp_map, const uint32_t* lambda8_by_qp, void* stream)
{
    return x265hip::intra_picture_launch("intra_in_inter", p, qp_map, lambda8_by_qp, inter_cost, inter_cost_stride, intra, true, stream);
}

extern "C" int x265hip_intra_picture(const x265hip_intra_picture_params* p, void* stream) { return x265hip_intra_picture_qp(p, nullptr, nullptr, stream); }
