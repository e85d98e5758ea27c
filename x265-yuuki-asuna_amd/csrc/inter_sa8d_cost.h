// inter_sa8d_cost.h - the inter candidate's sa8d cost per block of a P picture, on gfx950 (included at the end of tu_kernels.hip behind
// intra_picture.h: it predicts with that file's luma taps and transforms with sa8d_tile_sums of decision_common.h).
//
// Analysis::checkInter_rd0_4 at RD level <= 2 (source/encoder/analysis.cpp:3023-3071; m_bChromaSa8d is off, so luma only), per N x N block
// (N = 8 << level) of the TU stages' grid:
//   dist = cu[].sa8d(fenc, predY)           predY = Predict::predInterLumaPixel of the block's quarter-sample vector (predict.cpp:245-265)
//   bits = base_bits + bitcost(mv)          bitcost.h:48-52 against the predictor (0, 0): (uint32_t)(s_bitsizes[x] + s_bitsizes[y] + 0.5f)
//   cost = dist + ((bits * lambda8 + 128) >> 8)                                                       (calcRdSADCost, rdcost.h:148-153)
// sa8d: 8x8 = (sum |H8 d| + 2) >> 2; a 16x16 unit sums its four 8x8 transforms and rounds once (sa8d_16x16, pixel.cpp:341-352); a 32x32
// block is the sum of its four units.
//
// The body from the patches to the Hadamard sums is sa8d_slots(), which merge_decide_kernel (merge_decide.h) calls too.
// Mapping: one workgroup of 256 threads per 32x32 quarter of a CTU (16 / 4 / 1 blocks).  The blocks' reference patches go to LDS, the
// prediction is formed like inter_recon_kernel's (horizontal pass into `immed` only where both phases are set), the difference to the
// source lands in LDS, and 128 lanes run the sixteen 8x8 Hadamard transforms - rows in the lane, columns across eight lanes, the four
// tiles of a 16x16 unit on 32 consecutive lanes.  Blocks are independent: one launch per picture, no atomics.
#pragma once

namespace x265hip {

struct InterCostArgs
{
    const uint8_t* fenc; long fencStrideB;
    const uint8_t* fref; long frefStrideB;
    const int2* mv;                     // [ctu*85] {cost, qx | qy << 16}
    const float* bitSizes; int bitSizesLen;
    int ctusW, ctusH, depth, qp, baseBits, lambda8;
    int2* cost;                         // [ctu][blocks] {sa8d, cost}
    const int8_t* qpMap;                // optional: the luma plane of tu_qp, int8 [ctusH * 8][ctusW * 8]
    const uint32_t* lambdaByQp;         // optional, indexed by the block's luma quantiser QP
};

// The LDS of the patch -> prediction -> difference -> Hadamard body below: NB = (32 / N)^2 slots of one N x N block each.
template <int N>
struct Sa8dLds
{
    static constexpr int BPR = 32 / N, NB = BPR * BPR, PW = N + 7, PP = PW + 1;
    int16_t patch[NB * PW * PP];
    int16_t immed[NB * PW * N];
    int16_t diff[32 * 32];
    int mv[NB], sum[16];
};

// sa8d of the luma prediction of the first nAct slots (nAct <= NB): slot b predicts from fref at pos(b) (the block's first luma sample, int2)
// displaced by s.mv[b] (qx | qy << 16) and is compared with fenc at pos(b).  s.mv must be visible to the workgroup on entry; s.sum is on
// return (read it with sa8d_slot_sum<N>(s.sum, b)).  All 256 threads call it.  inter_sa8d_cost_kernel and merge_decide_kernel (merge_decide.h) share it,
// so the two price a vector alike.
template <typename Px, int N, class Pos>
__device__ __forceinline__ void sa8d_slots(Sa8dLds<N>& s, const int nAct, const Pos pos, const Px* fref, const long rst, const Px* fenc, const long fst,
                                           const int depth)
{
    constexpr int LOG2N = N == 8 ? 3 : (N == 16 ? 4 : 5), BPR = 32 / N;
    constexpr int APRON = 3, PW = N + 7, PP = PW + 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const int maxVal = (1 << depth) - 1, headRoom = 14 - depth;
    // ---- the blocks' reference patches: N + 7 rows and columns around the full-sample position ----------------------------------------
    for (int i = tid; i < nAct * PW * PW; i += 256)
    {
        const int b = i / (PW * PW), r = i - b * (PW * PW), y = r / PW, x = r - y * PW;
        const int qx = (int16_t)(s.mv[b] & 0xffff), qy = (int16_t)(s.mv[b] >> 16);
        const int2 o = pos(b);
        const int px = o.x + (qx >> 2) - APRON + x, py = o.y + (qy >> 2) - APRON + y;
        s.patch[b * (PW * PP) + y * PP + x] = (int16_t)fref[(long)py * rst + px];
    }
    __syncthreads();
    // ---- predInterLumaPixel: where both phases are set, the horizontal pass at 14-bit precision first ---------------------------------
    for (int i = tid; i < nAct * PW * N; i += 256)
    {
        const int b = i / (PW * N), r = i - b * (PW * N), y = r >> LOG2N, x = r & (N - 1);
        const int xf = s.mv[b] & 3, yf = (s.mv[b] >> 16) & 3;
        if (xf && yf)
        {
            const int shiftPS = 6 - headRoom, offPS = -(8192 << shiftPS);
            int acc = 0;
#pragma unroll
            for (int t = 0; t < 8; t++) acc += (int)s.patch[b * (PW * PP) + y * PP + x + t] * (int)kTuTaps[xf][t];
            s.immed[i] = (int16_t)((acc + offPS) >> shiftPS);
        }
    }
    __syncthreads();
    for (int i = tid; i < 32 * 32; i += 256)
    {
        const int ry = i >> 5, rx = i & 31, b = (ry >> LOG2N) * BPR + (rx >> LOG2N), y = ry & (N - 1), x = rx & (N - 1);
        if (b >= nAct) continue;
        const int xf = s.mv[b] & 3, yf = (s.mv[b] >> 16) & 3;
        const int16_t* pt = s.patch + b * (PW * PP);
        int v;
        if (xf && yf)
        {
            const int shiftSP = 6 + headRoom, offSP = (1 << (shiftSP - 1)) + (8192 << 6);
            int acc = 0;
#pragma unroll
            for (int t = 0; t < 8; t++) acc += (int)s.immed[b * (PW * N) + (y + t) * N + x] * (int)kTuTaps[yf][t];
            v = tu_clip16((acc + offSP) >> shiftSP, maxVal);
        }
        else if (!(xf | yf)) v = pt[(y + APRON) * PP + x + APRON];
        else
        {
            int acc = 0;
#pragma unroll
            for (int t = 0; t < 8; t++) acc += (int)(xf ? pt[(y + APRON) * PP + x + t] : pt[(y + t) * PP + x + APRON]) * (int)kTuTaps[xf ? xf : yf][t];
            v = tu_clip16((acc + 32) >> 6, maxVal);
        }
        const int2 o = pos(b);
        s.diff[i] = (int16_t)((int)fenc[(long)(o.y + y) * fst + o.x + x] - v);
    }
    __syncthreads();
    // ---- sixteen 8x8 Hadamard transforms on wavefronts 0 and 1 -------------------------------------------------------------------------
    // (the tiles of a slot at or beyond nAct transform whatever the difference array holds; nothing reads their sums)
    if (tid < 128) sa8d_tile_sums<N>(s.diff, s.sum, tid, lane);
    __syncthreads();
}

template <typename Px, int N>
__global__ void __launch_bounds__(256) inter_sa8d_cost_kernel(InterCostArgs a)
{
    constexpr int BPR = 32 / N, NB = BPR * BPR, BPC = 64 / N, NPU = BPC * BPC, BPP = sizeof(Px);
    __shared__ Sa8dLds<N> s;

    const int tid = threadIdx.x;
    const int ctu = (int)blockIdx.x >> 2, quarter = (int)blockIdx.x & 3;
    const int cx = ctu % a.ctusW, cy = ctu / a.ctusW;
    const int rx0 = cx * 64 + (quarter & 1) * 32, ry0 = cy * 64 + (quarter >> 1) * 32;         // the quarter's first luma sample
    const int lbase = level_record_base<N>();
    // block b of the quarter (raster order inside it) -> its z index inside the CTU
    auto zof = [&](const int b) { return ip_zidx((quarter & 1) * BPR + (b & (BPR - 1)), (quarter >> 1) * BPR + (b / BPR)); };
    if (tid < NB) s.mv[tid] = a.mv[(size_t)ctu * 85 + lbase + zof(tid)].y;
    __syncthreads();
    sa8d_slots<Px, N>(s, NB, [&](const int b) { return make_int2(rx0 + (b & (BPR - 1)) * N, ry0 + (b / BPR) * N); },
                      reinterpret_cast<const Px*>(a.fref), a.frefStrideB / BPP, reinterpret_cast<const Px*>(a.fenc), a.fencStrideB / BPP, a.depth);
    if (tid < NB)
    {
        const int b = tid;
        const int sad = sa8d_slot_sum<N>(s.sum, b);
        const int bits = a.baseBits + mv_bitcost(a.bitSizes, a.bitSizesLen, s.mv[b]);
        const int lambda8 = block_lambda8(a.lambda8, a.lambdaByQp, a.qpMap, a.qp, a.depth, a.ctusW, (rx0 + (b & (BPR - 1)) * N) >> 3, (ry0 + (b / BPR) * N) >> 3);
        const long long cost = (long long)sad + rd_sad_rate(bits, lambda8);
        a.cost[(size_t)ctu * NPU + zof(b)] = make_int2(sad, (int)cost);
    }
}

} // namespace x265hip

extern "C" int x265hip_inter_sa8d_cost(const x265hip_inter_sa8d_cost_params* p, void* stream)
{
    using namespace x265hip;
    // argument checks first: they need no device
    if (decision_record_refused("inter_sa8d_cost", p, !p || !p->fenc || !p->fref || !p->mv || !p->bit_sizes || !p->cost)) return X265HIP_EINVAL;
    // base_bits <= 4096 (+ at most 2 * 33 bits of a vector) and lambda8 <= 2^24 keep the rate term below 2^29 and the cost inside int32
    if (p->base_bits < 0 || p->base_bits > 4096) { set_error("inter_sa8d_cost: base_bits %d out of [0, 4096]", p->base_bits); return X265HIP_EINVAL; }
    if (bit_sizes_len_refused("inter_sa8d_cost", p->bit_sizes_len)) return X265HIP_EINVAL;
    int rc = ensure_device();
    if (rc) return rc;

    const int bpp = p->depth == 8 ? 1 : 2;
    InterCostArgs a = {};
    a.fenc = (const uint8_t*)p->fenc; a.fencStrideB = (long)p->fenc_stride * bpp;
    a.fref = (const uint8_t*)p->fref; a.frefStrideB = (long)p->fref_stride * bpp;
    a.mv = (const int2*)p->mv; a.bitSizes = p->bit_sizes; a.bitSizesLen = p->bit_sizes_len;
    a.ctusW = p->width / 64; a.ctusH = p->height / 64; a.depth = p->depth; a.qp = p->qp; a.baseBits = p->base_bits; a.lambda8 = p->lambda8;
    a.cost = (int2*)p->cost; a.qpMap = p->qp_map; a.lambdaByQp = p->lambda8_by_qp;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a.ctusW * a.ctusH * 4);
    for_depth_level(p->depth, p->level, [&](auto px, auto size)
    { hipLaunchKernelGGL((inter_sa8d_cost_kernel<decltype(px), decltype(size)::value>), grid, dim3(256), 0, s, a); });
    X265HIP_TRY(hipGetLastError());
    return 0;
}
