// col_field.h - the collocated motion field of a coded picture and the temporal merge candidate read from it, on gfx950 (included at the
// end of tu_kernels.hip behind decision_common.h and in front of merge_decide.h / b_merge_decide.h, whose _col instances use tmvp_*).
//
// x265hip_col_field_build compresses a coded picture's motion to what CUData::getColMVP (common/cudata.cpp:1968-2000) can see of it:
// partUnitIdx & TMVP_UNIT_MASK (0xF0) names the first 4x4 unit of a 16x16 luma unit, so one entry per 16x16 unit, 16 per CTU in raster
// order.  Unit (ux, uy) takes the motion of the block of the picture's grid that covers sample (16 ux, 16 uy): at level 0 the upper-left
// 8x8 of the four, at level 1 the block itself, at level 2 the 32x32 block around it.  col_delta = colPOC - colRefPOC of the block's
// reference index (poc_delta[ref_idx], entry 0 without ref_idx), 0 where the block is intra: getColMVP returns false there.
// Only list 0 of the collocated picture is modelled: the collocated picture of every step here is a P or I anchor, because B pictures
// are not referenced.  One thread per unit, one launch, capturable.
//
// The temporal candidate of a block whose first sample is (x0, y0) (cudata.cpp:1594-1650): the bottom-right position (x0 + N, y0 + N),
// tried only inside the picture (:1601-1602) and not below the CTU; in this CTU where (x0 % 64) + N < 64, otherwise in CTU + 1 at unit
// column 0 (:1609-1622; a block in the CTU's last row or lower right corner has no try).  Where the try is absent or false the centre
// (x0 + N / 2, y0 + N / 2) of this CTU (:1630-1634, deriveCenterIdx).  The vector is scaled by scaleMvByPOCDist (:2030-2045) with scaleMv
// (:104-110).
#pragma once

namespace x265hip {

struct ColFieldArgs
{
    const int2* mv;                     // [ctu*85] {cost, qx | qy << 16}: the picture's final motion
    const uint8_t* intra;               // optional [ctu][blocks]
    const int8_t* refIdx;               // optional [ctu][blocks]
    int pocDelta[8];
    int nunits;                         // ctus * 16
    int32_t* colMv; int16_t* colDelta;  // [ctu][16]
};

template <int N>
__global__ void __launch_bounds__(256) col_field_kernel(ColFieldArgs a)
{
    constexpr int BPC = 64 / N, NPU = BPC * BPC;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= a.nunits) return;
    const int ctu = i >> 4, ux = i & 3, uy = (i >> 2) & 3;
    const int z = ip_zidx((ux * 16) / N, (uy * 16) / N);               // the block that covers sample (16 ux, 16 uy)
    const size_t blk = (size_t)ctu * NPU + z;
    const bool isIntra = a.intra && a.intra[blk];
    const int r = a.refIdx ? (int)a.refIdx[blk] : 0;
    const bool has = !isIntra && r >= 0 && r < 8;                       // a negative index: no list-0 motion
    a.colMv[i] = has ? a.mv[(size_t)ctu * 85 + level_record_base<N>() + z].y : 0;
    a.colDelta[i] = (int16_t)(has ? a.pocDelta[r] : 0);
}

// scaleMvByPOCDist (cudata.cpp:2030-2045) of the packed vector v: curDelta = curPOC - curRefPOC, colDelta = colPOC - colRefPOC (not 0)
__device__ __forceinline__ int tmvp_scale_mv(const int v, const int curDelta, const int colDelta)
{
    if (curDelta == colDelta) return v;
    const int tdb = clip3(-128, 127, curDelta), tdd = clip3(-128, 127, colDelta);
    const int x = (0x4000 + abs(tdd / 2)) / tdd;
    const int scale = clip3(-4096, 4095, (tdb * x + 32) >> 6);
    const int px = scale * (int)(int16_t)(v & 0xffff), py = scale * (int)(int16_t)(v >> 16);
    const int qx = clip3(-32768, 32767, (px + 127 + (px < 0 ? 1 : 0)) >> 8);                   // scaleMv, :104-110
    const int qy = clip3(-32768, 32767, (py + 127 + (py < 0 ? 1 : 0)) >> 8);
    return (qx & 0xffff) | (int)((unsigned)qy << 16);
}

// The collocated entry the temporal candidate of the N x N block at (lx, ly) of CTU (cxb, cyb) takes: the bottom-right try, then the
// centre.  Returns false where neither has motion; otherwise the UNSCALED vector and its distance.
template <int N>
__device__ __forceinline__ bool tmvp_collocated(const int32_t* colMv, const int16_t* colDelta, const int ctu, const int cxb, const int cyb, const int ctusW,
                                                const int ctusH, const int lx, const int ly, int& mv, int& delta)
{
    const int x0 = cxb * 64 + lx, y0 = cyb * 64 + ly;
    if (x0 + N < ctusW * 64 && y0 + N < ctusH * 64 && ly + N < 64)                              // :1601-1602, bNotLastRow
    {
        const bool here = lx + N < 64;                                                          // bNotLastCol; otherwise CTU + 1, column 0
        const size_t u = (size_t)(here ? ctu : ctu + 1) * 16 + ((ly + N) >> 4) * 4 + (here ? (lx + N) >> 4 : 0);
        delta = colDelta[u];
        if (delta) { mv = colMv[u]; return true; }
    }
    const size_t u = (size_t)ctu * 16 + ((ly + N / 2) >> 4) * 4 + ((lx + N / 2) >> 4);          // deriveCenterIdx
    delta = colDelta[u];
    mv = colMv[u];
    return delta != 0;
}

static bool tmvp_delta_refused(const char* who, const char* name, const int d)
{
    if (d == 0 || d < -32768 || d > 32767) { set_error("%s: %s %d is 0 or outside -32768..32767", who, name, d); return true; }
    return false;
}

} // namespace x265hip

extern "C" int x265hip_col_field_build(const x265hip_col_field_params* p, void* stream)
{
    using namespace x265hip;
    if (!p || !p->mv || !p->col_mv || !p->col_delta) { set_error("col_field_build: NULL operand"); return X265HIP_EINVAL; }
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("col_field_build: depth %d", p->depth); return X265HIP_EINVAL; }
    if (p->level < 0 || p->level > 2) { set_error("col_field_build: level %d (0..2 = 8x8, 16x16, 32x32)", p->level); return X265HIP_EINVAL; }
    if ((p->width & 63) || (p->height & 63) || p->width <= 0 || p->height <= 0)
    { set_error("col_field_build: width/height must be multiples of 64"); return X265HIP_EINVAL; }
    for (int r = 0; r < (p->ref_idx ? 8 : 1); r++)                     // every index that can be read
        if (tmvp_delta_refused("col_field_build", "poc_delta", p->poc_delta[r])) return X265HIP_EINVAL;
    int rc = ensure_device();
    if (rc) return rc;

    ColFieldArgs a = {};
    a.mv = (const int2*)p->mv; a.intra = p->intra; a.refIdx = p->ref_idx;
    for (int r = 0; r < 8; r++) a.pocDelta[r] = p->ref_idx || r == 0 ? p->poc_delta[r] : 0;
    a.nunits = (p->width / 64) * (p->height / 64) * 16;
    a.colMv = p->col_mv; a.colDelta = p->col_delta;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((a.nunits + 255) / 256);
    if (p->level == 0) hipLaunchKernelGGL(col_field_kernel<8>, grid, dim3(256), 0, s, a);
    else if (p->level == 1) hipLaunchKernelGGL(col_field_kernel<16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(col_field_kernel<32>, grid, dim3(256), 0, s, a);
    X265HIP_TRY(hipGetLastError());
    return 0;
}
