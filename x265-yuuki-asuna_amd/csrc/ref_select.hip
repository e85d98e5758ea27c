// ref_select.hip - the reference picture of every block of a P picture with several references, on gfx950.
//
// Reference semantics: the uni-directional loop of Search::predInterSearch (source/encoder/search.cpp:2386-2471) for a P slice's 2Nx2N:
// every reference of list 0 is searched, its cost gets the bits of its index (m_listSelBits[0] + MVP_IDX_BITS + getTUBits(ref, numRefIdx),
// :2403-2404, source/encoder/search.h:246-249) and the first smallest total wins (strict '<', :2457).  The per-reference searches are the
// x265hip_me_fullsearch + x265hip_subpel_refine passes the caller ran; what is left is a comparison of nrefs records per block.
//
// Mapping: one lane per block of the level's grid, blocks in [ctu][z] order over consecutive lanes - a lane reads nrefs 8-byte records and
// writes one record, one or two bytes and (optionally) nrefs costs.  No LDS, no atomics, no cross-lane traffic.
#include "common.h"

namespace x265hip {

struct RefSelectArgs
{
    const int2* mv[X265HIP_MAX_REFS];
    int refCost[X265HIP_MAX_REFS];
    int refId[X265HIP_MAX_REFS];
    int nrefs, level, nblocks;
    int8_t* refIdx; int8_t* refIdOut;
    int2* mvOut;
    int* costOut;
};

__global__ void __launch_bounds__(256) ref_select_kernel(RefSelectArgs a)
{
    const int blk = blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= a.nblocks) return;
    const int shift = 6 - 2 * a.level;                                 // log2 of the blocks per CTU
    const int ctu = blk >> shift, z = blk - (ctu << shift);
    const int lbase = a.level == 0 ? 0 : (a.level == 1 ? 64 : 80);
    const size_t rec = (size_t)ctu * 85 + lbase + z;
    int2 bestRec = make_int2(0, 0);
    int best = 0, bestId = 0;
    // the table of record pointers, costs and ids sits in the kernel arguments and r is uniform: scalar loads, every lane the same entry
#pragma unroll
    for (int r = 0; r < X265HIP_MAX_REFS; r++)
    {
        if (r >= a.nrefs) break;
        const int2 q = a.mv[r][rec];
        const int c = q.x + a.refCost[r];
        if (a.costOut) a.costOut[(size_t)blk * a.nrefs + r] = c;
        if (r == 0 || c < bestRec.x) { bestRec = make_int2(c, q.y); best = r; bestId = a.refId[r]; }
    }
    a.refIdx[blk] = (int8_t)best;
    if (a.refIdOut) a.refIdOut[blk] = (int8_t)bestId;
    a.mvOut[rec] = bestRec;
}

} // namespace x265hip

using namespace x265hip;

extern "C" int x265hip_ref_select(const x265hip_ref_select_params* p, void* stream)
{
    // argument checks first: they need no device
    if (!p || !p->ref_idx || !p->mv_out) { set_error("ref_select: NULL operand"); return X265HIP_EINVAL; }
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("ref_select: depth %d", p->depth); return X265HIP_EINVAL; }
    if (p->level < 0 || p->level > 2) { set_error("ref_select: level %d out of [0,2]", p->level); return X265HIP_EINVAL; }
    if ((p->width & 63) || (p->height & 63) || p->width <= 0 || p->height <= 0) { set_error("ref_select: width/height must be multiples of 64"); return X265HIP_EINVAL; }
    if (p->nrefs < 1 || p->nrefs > X265HIP_MAX_REFS) { set_error("ref_select: nrefs %d out of [1,%d]", p->nrefs, X265HIP_MAX_REFS); return X265HIP_EINVAL; }
    for (int r = 0; r < p->nrefs; r++)
        if (!p->mv[r]) { set_error("ref_select: NULL records of reference %d", r); return X265HIP_EINVAL; }
    const int nctu = (p->width / 64) * (p->height / 64);
    {
        // a block's records are read after other blocks' outputs may have been written: the output is a buffer of its own
        const uintptr_t len = (uintptr_t)nctu * 85 * 8, out = (uintptr_t)p->mv_out;
        for (int r = 0; r < p->nrefs; r++)
        {
            const uintptr_t in = (uintptr_t)p->mv[r];
            if (out < in + len && in < out + len) { set_error("ref_select: mv_out must not alias or overlap mv[%d]", r); return X265HIP_EINVAL; }
        }
    }
    int rc = ensure_device();
    if (rc) return rc;

    RefSelectArgs a = {};
    for (int r = 0; r < p->nrefs; r++) { a.mv[r] = (const int2*)p->mv[r]; a.refCost[r] = p->ref_cost[r]; a.refId[r] = p->ref_ids[r]; }
    a.nrefs = p->nrefs; a.level = p->level; a.nblocks = nctu * (64 >> (2 * p->level));
    a.refIdx = p->ref_idx; a.refIdOut = p->ref_id; a.mvOut = (int2*)p->mv_out; a.costOut = p->cost_out;
    hipLaunchKernelGGL(ref_select_kernel, dim3((a.nblocks + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    X265HIP_TRY(hipGetLastError());
    return 0;
}
