// cu_qp_maps.hip - the step between the lookahead's QP offsets and the coding stages: one QP per block of the TU stages' grid.
// Host logic (no device work): the non-hevcAq arm of Analysis::calculateQpforCuSize (encoder/analysis.cpp:3679-3713) and
// Quant::setQPforQuant / setChromaQP (common/quant.cpp:221-244) for 4:2:0 pictures.
#include "common.h"

using namespace x265hip;

// g_chromaScale (constants.cpp:346-350; the standard's table 8-10 for ChromaArrayType 1), from 30 up
static const int8_t kChromaScaleFrom30[28] = { 29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51 };

extern "C" int x265hip_cu_qp_maps(const x265hip_cu_qp_params* p)
{
    if (!p || (!p->cu_qp && !p->tu_qp)) { set_error("cu_qp_maps: NULL operand"); return X265HIP_EINVAL; }
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("cu_qp_maps: depth %d", p->depth); return X265HIP_EINVAL; }
    if ((p->width & 63) || (p->height & 63) || p->width <= 0 || p->height <= 0) { set_error("cu_qp_maps: width/height must be multiples of 64"); return X265HIP_EINVAL; }
    if (p->level < 0 || p->level > 2) { set_error("cu_qp_maps: level %d (0..2 = 8x8, 16x16, 32x32)", p->level); return X265HIP_EINVAL; }
    if (p->qg_size != 16 && p->qg_size != 8) { set_error("cu_qp_maps: qg_size %d", p->qg_size); return X265HIP_EINVAL; }
    if (p->qp_min < 0 || p->qp_max > 51 || p->qp_min > p->qp_max) { set_error("cu_qp_maps: qp_min %d / qp_max %d (0..51)", p->qp_min, p->qp_max); return X265HIP_EINVAL; }
    if (p->cb_qp_offset < -24 || p->cb_qp_offset > 24 || p->cr_qp_offset < -24 || p->cr_qp_offset > 24)
    { set_error("cu_qp_maps: chroma QP offsets %d / %d (PPS + slice: -24..24)", p->cb_qp_offset, p->cr_qp_offset); return X265HIP_EINVAL; }
    const int bdOffset = 6 * (p->depth - 8);                      // QP_BD_OFFSET
    const int loopIncr = p->qg_size == 8 ? 8 : 16;
    const int maxCols = (p->width + loopIncr - 1) / loopIncr;
    const int blockSize = 8 << p->level, cells = blockSize >> 3, w8 = p->width >> 3;
    const size_t plane = (size_t)(p->height >> 3) * w8;
    auto chroma = [&](const int qpin)
    {
        int qp = qpin < -bdOffset ? -bdOffset : (qpin > 57 ? 57 : qpin);
        if (qp >= 30) qp = kChromaScaleFrom30[qp - 30];
        return qp + bdOffset;
    };
    for (int by = 0; by < p->height; by += blockSize)
        for (int bx = 0; bx < p->width; bx += blockSize)
        {
            double qp = p->base_qp;
            if (p->qp_offsets)
            {
                double dQpOffset = 0;
                int cnt = 0;
                for (int yy = by; yy < by + blockSize && yy < p->height; yy += loopIncr)
                    for (int xx = bx; xx < bx + blockSize && xx < p->width; xx += loopIncr)
                    {
                        dQpOffset += p->qp_offsets[(size_t)(yy / loopIncr) * maxCols + xx / loopIncr];
                        cnt++;
                    }
                dQpOffset /= cnt;
                qp += dQpOffset;
            }
            // (int)(qp + 0.5) of the reference; a value no int can hold (offsets the lookahead never produces) is clipped before the conversion
            const double r = qp + 0.5;
            const int cu = r > (double)p->qp_min ? (r >= (double)p->qp_max + 1 ? p->qp_max : (int)r) : p->qp_min;
            const int v[4] = { cu, cu + bdOffset, chroma(cu + p->cb_qp_offset), chroma(cu + p->cr_qp_offset) };
            for (int cy = 0; cy < cells; cy++)
                for (int cx = 0; cx < cells; cx++)
                {
                    const size_t i = (size_t)((by >> 3) + cy) * w8 + (bx >> 3) + cx;
                    if (p->cu_qp) p->cu_qp[i] = (int8_t)v[0];
                    if (p->tu_qp) for (int c = 0; c < 3; c++) p->tu_qp[c * plane + i] = (int8_t)v[1 + c];
                }
        }
    return 0;
}
