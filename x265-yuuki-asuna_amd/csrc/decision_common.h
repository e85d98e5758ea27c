// decision_common.h - what the sa8d decision stages share, on gfx950 (included at the end of tu_kernels.hip in front of intra_picture.h,
// inter_sa8d_cost.h, b_sa8d_decide.h, merge_decide.h and b_merge_decide.h; it uses that file's clip3 and group_sum).
//
// Device side: the block grid (z-order, the 85-slot record table), the block's lambda, the rate term and the vector bit cost of the sa8d
// costs, and the 8x8 Hadamard stage of a 32x32 difference plane.  Host side: the argument checks all five entries make alike, the wave
// schedule of the three walks that follow the coding order, and the depth x level dispatch of every launch.
//
// Two things stay where they are because sharing them changed the kernels' code for the worse (more instructions, more scalar spills):
// the "inside the picture and coded before this block" test of intra_picture_kernel, and the quarter geometry (zof / rx0 / ry0) of
// inter_sa8d_cost_kernel and b_sa8d_decide_kernel.  The two merge kernels share that test, with the rest of their candidate walk, through
// merge_walk.h: there it kept their code as a lambda that refers to the kernel's own variables (profiles/merge_walk_code_identity.txt).
#pragma once

namespace x265hip {

// z-order index of block (bx, by) of a CTU
__device__ __forceinline__ int ip_zidx(int bx, int by)
{
    return (bx & 1) | ((by & 1) << 1) | ((bx & 2) << 1) | ((by & 2) << 2) | ((bx & 4) << 2) | ((by & 4) << 3);
}

// the inverse: block (x, y) of z index z
__device__ __forceinline__ int2 ip_zpos(int z)
{
    return make_int2((z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4), ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4));
}

// the first record of the N x N level in a CTU's 85-slot table: 64 8x8 records, 16 16x16, 4 32x32, one 64x64
template <int N> __device__ __forceinline__ constexpr int level_record_base() { return N == 8 ? 0 : (N == 16 ? 64 : 80); }

// an entry of lambda8_by_qp counts at most 2^24, the bound of the record's lambda8
__device__ __forceinline__ int clamp_lambda8(const uint32_t l) { return (int)(l < (1u << 24) ? l : (1u << 24)); }

// The lambda of the block whose first luma sample lies in 8x8 cell (gx8, gy8): the record's without a table; with one, the entry of the
// record's QP or, with a map (the luma plane of tu_qp, int8 [ctusH * 8][ctusW * 8]), of the cell's QP clipped to the depth's range
__device__ __forceinline__ int block_lambda8(const int lambda8, const uint32_t* lambdaByQp, const int8_t* qpMap, int qp, const int depth, const int ctusW,
                                             const int gx8, const int gy8)
{
    if (!lambdaByQp) return lambda8;
    if (qpMap) qp = clip3(0, 51 + 6 * (depth - 8), (int)qpMap[(size_t)gy8 * (ctusW * 8) + gx8]);
    return clamp_lambda8(lambdaByQp[qp]);
}

// BitCost::bitcost (bitcost.h:48-52) of the vector qx | qy << 16 against the predictor (0, 0): (uint32_t)(s_bitsizes[x] + s_bitsizes[y] +
// 0.5f); a component beyond the table prices as the table's last entry
__device__ __forceinline__ int mv_bitcost(const float* bitSizes, const int len, const int w)
{
    const int qx = (int16_t)(w & 0xffff), qy = (int16_t)(w >> 16);
    const int ix = min(abs(qx), len - 1), iy = min(abs(qy), len - 1);
    return (int)(uint32_t)(bitSizes[ix] + bitSizes[iy] + 0.5f);
}

// the rate term of calcRdSADCost / getCost (rdcost.h:148-153): cost = sad + rd_sad_rate(bits, lambda8)
__device__ __forceinline__ long long rd_sad_rate(const int bits, const int lambda8) { return ((long long)bits * lambda8 + 128) >> 8; }

// sum of the absolute 8x8 Hadamard coefficients of a difference block whose row r sits in lane (lane & ~7) + r; valid in all eight lanes
__device__ __forceinline__ int ip_hadamard8x8(int (&v)[8], const int lane)
{
#pragma unroll
    for (int step = 1; step < 8; step <<= 1)
#pragma unroll
        for (int i = 0; i < 8; i += step << 1)
#pragma unroll
            for (int j = i; j < i + step; j++) { const int p = v[j], q = v[j + step]; v[j] = p + q; v[j + step] = p - q; }
#pragma unroll
    for (int s = 1; s < 8; s <<= 1)
    {
        const bool hi = (lane & s) != 0;
#pragma unroll
        for (int k = 0; k < 8; k++) { const int o = __shfl_xor(v[k], s, 64); v[k] = hi ? o - v[k] : v[k] + o; }
    }
    int acc = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) acc += abs(v[k]);
    return group_sum<8>(acc);
}

// The sixteen 8x8 Hadamard transforms of a 32x32 difference plane on 128 threads (two whole wavefronts; t = 0..127, lane = the thread's
// lane): unit u = 16x16 (ux, uy), tile q inside it, row r - rows in the lane, columns across eight lanes, the four tiles of a unit on 32
// consecutive lanes.  sa8d: 8x8 = (sum |H8 d| + 2) >> 2; a 16x16 unit sums its four transforms and rounds once (sa8d_16x16,
// pixel.cpp:341-352).  sum16 gets the sixteen 8x8 sums in raster order (N = 8) or the four unit sums; one writer per slot.
template <int N>
__device__ __forceinline__ void sa8d_tile_sums(const int16_t* diff32x32, int* sum16, const int t, const int lane)
{
    const int row = t & 7, q = (t >> 3) & 3, u = t >> 5;
    const int tx = (u & 1) * 2 + (q & 1), ty = (u >> 1) * 2 + (q >> 1);
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = diff32x32[(ty * 8 + row) * 32 + tx * 8 + i];
    int raw = ip_hadamard8x8(d, lane);
    if (N == 8) { if (row == 0) sum16[ty * 4 + tx] = (raw + 2) >> 2; }                        // the block at (tx, ty) of the quarter
    else
    {
        raw += __shfl_xor(raw, 8, 64); raw += __shfl_xor(raw, 16, 64);
        if ((t & 31) == 0) sum16[u] = (raw + 2) >> 2;
    }
}

// slot b's sa8d from those sums: an 8x8 or 16x16 slot is one rounded sum, the 32x32 slot the sum of its four units
template <int N>
__device__ __forceinline__ int sa8d_slot_sum(const int* sum, const int b)
{
    return N == 32 ? sum[0] + sum[1] + sum[2] + sum[3] : sum[b];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

// What the five entries refuse alike, before they ask for a device: true, with the error text set, when the record is refused.  P is one
// of the five parameter records, which name these fields alike; nullOperand = the record or one of the entry's operands is NULL, reported
// before anything else.  lambda8 <= 2^24 and at most 4096 + 4096 + 4096 + 4 * 33 bits (the entries' own checks) keep every rate term
// below 2^30; the largest sa8d of a 32x32 block of 12-bit samples is below 2^27: every cost fits its int32.
template <class P>
static bool decision_record_refused(const char* who, const P* p, const bool nullOperand)
{
    if (nullOperand) { set_error("%s: NULL operand", who); return true; }
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("%s: depth %d", who, p->depth); return true; }
    if (p->level < 0 || p->level > 2) { set_error("%s: level %d (0..2 = 8x8, 16x16, 32x32)", who, p->level); return true; }
    if ((p->width & 63) || (p->height & 63) || p->width <= 0 || p->height <= 0) { set_error("%s: width/height must be multiples of 64", who); return true; }
    // the second luma plane is the reconstruction of the intra record and the reference of the others
    constexpr bool intra = std::is_same<P, x265hip_intra_picture_params>::value;
    intptr_t other;
    if constexpr (intra) other = p->recon_stride; else other = p->fref_stride;
    if (p->fenc_stride < p->width || other < p->width) { set_error(intra ? "%s: luma stride below the width" : "%s: stride below the width", who); return true; }
    if (p->qp < 0 || p->qp > 51 + 6 * (p->depth - 8)) { set_error("%s: qp %d out of range", who, p->qp); return true; }
    if (p->lambda8 < 0 || p->lambda8 > (1 << 24)) { set_error("%s: lambda8 %d out of [0, 2^24]", who, p->lambda8); return true; }
    return false;
}
static bool bit_sizes_len_refused(const char* who, const int len)
{
    if (len < 1) { set_error("%s: bit_sizes_len %d below 1", who, len); return true; }
    return false;
}
static bool inter_cost_stride_refused(const char* who, const intptr_t stride)
{
    if (stride < 1) { set_error("%s: inter_cost_stride %ld below 1", who, (long)stride); return true; }
    return false;
}

// The wave schedule of the walks that follow the coding order: CTU (cx, cy) depends on (cx - 1, cy), (cx - 1, cy - 1), (cx, cy - 1) and
// (cx + 1, cy - 1), so it may run in wave cx + 2 cy.  f(wave, cyLo, n) for every wave that has CTUs: n of them, cy = cyLo .. cyLo + n - 1,
// cx = wave - 2 cy (a picture one CTU wide has no CTU in its odd waves).
static int decision_wave_count(const int ctusW, const int ctusH) { return ctusW + 2 * (ctusH - 1); }
template <class F>
static void for_each_wave(const int ctusW, const int ctusH, F&& f)
{
    for (int w = 0; w < decision_wave_count(ctusW, ctusH); w++)
    {
        const int over = w - (ctusW - 1);
        const int cyLo = over > 0 ? (over + 1) / 2 : 0, cyHi = w / 2 < ctusH - 1 ? w / 2 : ctusH - 1;
        if (cyHi >= cyLo) f(w, cyLo, cyHi - cyLo + 1);
    }
}

// f(Px(), std::integral_constant<int, N>()) with the sample type of `depth` and N = 8 << level: the kernel instance of a checked record
template <class F>
static void for_depth_level(const int depth, const int level, F&& f)
{
    auto of = [&](auto px)
    {
        if (level == 0) f(px, std::integral_constant<int, 8>());
        else if (level == 1) f(px, std::integral_constant<int, 16>());
        else f(px, std::integral_constant<int, 32>());
    };
    if (depth == 8) of(uint8_t()); else of(uint16_t());
}

} // namespace x265hip
