// row_pictures.hip - see csrc/row_pictures.h
#include "row_pictures.h"

#include <cstdio>
#include <cstring>

namespace x265hip {

namespace {

// primitives.weight_pp (common/pixel.cpp:518-543) over whole buffer lines, margins included: the plane MotionReference::applyWeight
// builds row by row (encoder/reference.cpp:119-178: weight_pp on the picture, then the borders replicated) is the reconstructed
// plane weighted sample by sample - a replicated border sample weights to the replicated weighted sample.
template <typename Px>
__global__ void __launch_bounds__(256) weight_lines_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t ndw, int w0, int round, int shift, int offset,
                                                           int correction, int maxVal)
{
    constexpr int PER = 4 / (int)sizeof(Px), BITS = 8 * (int)sizeof(Px);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ndw; i += (size_t)gridDim.x * blockDim.x)
    {
        const uint32_t v = src[i];
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < PER; k++)
        {
            const int px = (int)((v >> (k * BITS)) & ((1u << BITS) - 1));
            const int val = (int)(int16_t)(px << correction);                       // "simulating pixel to short conversion" (pixel.cpp:535)
            o |= (uint32_t)clip3(0, maxVal, ((w0 * val + round) >> shift) + offset) << (k * BITS);
        }
        dst[i] = o;
    }
}

// centre of every CTU's window = the displacement of its 64x64 block's minimum SAD in the +-big search, clamped to +-maxX / [-maxY, maxYDown] (downwards the
// candidates must stay inside the reference rows that exist when the row is computed)
__global__ void centre_kernel(const unsigned long long* __restrict__ best, int16_t* __restrict__ centres, int nctu, int big, int maxX, int maxY, int maxYDown)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nctu) return;
    const uint32_t idx = (uint32_t)best[(size_t)i * 85 + 84];
    const int ncb = 2 * big + 1;
    const int mx = (int)(idx % ncb) - big, my = (int)(idx / ncb) - big;
    centres[2 * i] = (int16_t)clip3(-maxX, maxX, mx);
    centres[2 * i + 1] = (int16_t)clip3(-maxY, maxYDown, my);
}

} // namespace

int weight_lines_launch(int depth, const void* src, void* dst, size_t ndw, const x265hip_weight& w, hipStream_t stream)
{
    const int correction = 14 - depth, maxVal = (1 << depth) - 1;
    size_t blocks = (ndw + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (depth == 8)
        hipLaunchKernelGGL(weight_lines_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, ndw, w.w0, w.round, w.shift, w.offset,
                           correction, maxVal);
    else
        hipLaunchKernelGGL(weight_lines_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, ndw, w.w0, w.round, w.shift, w.offset,
                           correction, maxVal);
    X265HIP_TRY(hipGetLastError());
    return 0;
}

int centres_launch(const unsigned long long* best, int16_t* centres, int nctu, int big, int maxX, int maxY, int maxYDown, hipStream_t stream)
{
    hipLaunchKernelGGL(centre_kernel, dim3((nctu + 63) / 64), dim3(64), 0, stream, best, centres, nctu, big, maxX, maxY, maxYDown);
    X265HIP_TRY(hipGetLastError());
    return 0;
}

PlaneGeometry plane_geometry(int depth, intptr_t stride, intptr_t stride_c, int rows, int rows_c, int margin_y, int margin_y_c)
{
    PlaneGeometry g;
    g.depth = depth;
    g.bpp = depth == 8 ? 1 : 2;
    g.ctuRows = (rows - 2 * margin_y) / 64;
    g.nplanes = rows_c > 0 ? 3 : 1;
    g.stride[0] = stride; g.stride[1] = stride_c;
    g.pitch[0] = (size_t)stride * g.bpp; g.pitch[1] = (size_t)stride_c * g.bpp;
    g.rows[0] = rows; g.rows[1] = rows_c;
    g.planeBytes[0] = g.pitch[0] * rows; g.planeBytes[1] = g.pitch[1] * rows_c;
    g.margin[0] = margin_y; g.margin[1] = margin_y_c;
    g.ctuLines[0] = 64; g.ctuLines[1] = 32;
    g.nph[0] = 15; g.nph[1] = 63;
    return g;
}

// ---------------------------------------------------------------- worker
bool worker_wait(RowWorker& w, std::unique_lock<std::mutex>& lk)
{
    w.cv.wait(lk, [&w] { return w.stop || w.dirty; });
    if (w.stop) return false;
    w.dirty = false;
    return true;
}

void worker_round_end(RowWorker& w, hipStream_t stream, int rc, const Pins& pins, double t0)
{
    if (rc)
    {
        snprintf(w.error, sizeof(w.error), "%s", x265hip_last_error());
        (void)hipStreamSynchronize(stream);                     // nothing queued may still read a picture whose pin goes below
    }
    {
        // a pinned entry stays its picture's until here: a view or pair that closed with its last rows no longer holds it, and a host thread
        // staging a NEW picture into the same pinned memory would race the upload still reading it
        std::lock_guard<std::mutex> lk(w.mu);
        for (int* busy : pins) --*busy;
    }
    w.usBusy += (uint64_t)(now_us() - t0);
}

void worker_stop(RowWorker& w, hipStream_t stream)
{
    {
        std::lock_guard<std::mutex> lk(w.mu);
        w.stop = true;
    }
    w.cv.notify_all();
    if (w.thread.joinable()) w.thread.join();
    (void)hipStreamSynchronize(stream);
}

// ---------------------------------------------------------------- picture pool
int device_alloc_zeroed(uint8_t** p, size_t bytes)
{
    X265HIP_TRY(hipMalloc((void**)p, bytes));
    X265HIP_TRY(hipMemset(*p, 0, bytes));
    return 0;
}

int wait_for_fills()
{
    // hipMemset returns before a DEVICE memset has run (it is queued on the null stream), and the worker's stream is non-blocking: an
    // upload of the first rows could be overtaken by the zero fill queued before it (seen as planes that intermittently did not equal
    // the whole-picture planes when other work sat in front of the memsets, round 4) - wait for the fills once, before the worker starts
    X265HIP_TRY(hipDeviceSynchronize());
    return 0;
}

int pool_alloc(PicturePool& pool, const PlaneGeometry& g, int pictures)
{
    pool.pics = std::vector<Pic>(pictures);
    for (auto& pc : pool.pics)
    {
        pc.staged.assign(g.ctuRows, 0);
        for (int i = 0; i < g.nplanes; i++)
        {
            const int k = i ? 1 : 0;
            X265HIP_TRY(hipHostMalloc((void**)&pc.stage[i], g.planeBytes[k], hipHostMallocDefault));
            int rc = device_alloc_zeroed(&pc.dSrc[i], g.planeBytes[k] + 256);
            if (rc) return rc;
        }
    }
    return 0;
}

void pool_free(PicturePool& pool)
{
    for (auto& pc : pool.pics)
        for (int i = 0; i < 3; i++)
        {
            if (pc.stage[i]) (void)hipHostFree(pc.stage[i]);
            if (pc.dSrc[i]) (void)hipFree(pc.dSrc[i]);
        }
}

void stage_rows(RowWorker& w, const PlaneGeometry& g, Pic& pc, uint64_t key, const void* const bufs[3], int r0, int n)
{
    for (int pl = 0; pl < g.nplanes; pl++)
    {
        const int k = pl ? 1 : 0;
        int y0, y1;
        g.lines(k, r0, n, y0, y1);
        memcpy(pc.stage[pl] + (size_t)y0 * g.pitch[k], (const uint8_t*)bufs[pl] + (size_t)y0 * g.pitch[k], (size_t)(y1 - y0) * g.pitch[k]);
    }
    {
        std::lock_guard<std::mutex> lk(w.mu);
        pc.busy--;
        if (pc.used && pc.key == key)
            for (int r = r0; r < r0 + n; r++) pc.staged[r] = 1;
        w.dirty = true;
    }
    w.cv.notify_one();
}

void take_staged_prefixes(PicturePool& pool, int ctuRows, std::vector<RowUpload>& ups, Pins& pins)
{
    for (int i = 0; i < (int)pool.pics.size(); i++)
    {
        Pic& pc = pool.pics[i];
        if (!pc.used) continue;
        int r1 = pc.nextRow;
        while (r1 < ctuRows && pc.staged[r1]) r1++;             // views grow top to bottom: only a contiguous prefix is useful
        if (r1 > pc.nextRow) { ups.push_back({ i, pc.nextRow, r1 }); pc.nextRow = r1; pin(pins, pc.busy); }
    }
}

int upload(const PlaneGeometry& g, const Pic& pc, int r0, int r1, hipStream_t stream, std::atomic<uint64_t>& bytesUp)
{
    for (int pl = 0; pl < g.nplanes; pl++)
    {
        const int k = pl ? 1 : 0;
        int y0, y1;
        g.lines(k, r0, r1 - r0, y0, y1);
        const size_t off = (size_t)y0 * g.pitch[k], bytes = (size_t)(y1 - y0) * g.pitch[k];
        X265HIP_TRY(hipMemcpyAsync(pc.dSrc[pl] + off, pc.stage[pl] + off, bytes, hipMemcpyHostToDevice, stream));
        bytesUp += bytes;
    }
    return 0;
}

// ---------------------------------------------------------------- view
int view_alloc(View& v, const PlaneGeometry& g, size_t outSlack)
{
    for (int i = 0; i < g.nplanes; i++)
    {
        const int k = i ? 1 : 0;
        int rc = device_alloc_zeroed(&v.dW[i], g.planeBytes[k] + 256);
        if (rc) return rc;
        X265HIP_TRY(hipMalloc((void**)&v.dOut[i], g.planeBytes[k] * g.nph[k] + outSlack));
    }
    return 0;
}

void view_free(View& v)
{
    for (int i = 0; i < 3; i++)
    {
        if (v.dW[i]) (void)hipFree(v.dW[i]);
        if (v.dOut[i]) (void)hipFree(v.dOut[i]);
    }
}

void view_reset(View& v, int pic, uint32_t picEpoch, const x265hip_weight* w, unsigned mask)
{
    v.pic = pic; v.picEpoch = picEpoch;
    v.mask = mask;
    for (int c = 0; c < 3; c++) v.w[c] = (mask & (1u << c)) ? w[c] : x265hip_weight{ 0, 0, 0, 0 };
    v.rowsSeen = 0; v.done[0] = v.done[1] = 0;
    v.active = true;
}

bool take_view_job(const PicturePool& pool, int ctuRows, View& v, int index, ViewJob& job)
{
    if (!v.active) return false;
    const Pic& pc = pool.pics[v.pic];
    if (!pc.used || pc.epoch != v.picEpoch) { v.active = false; return false; }      // the picture went away: what is finished stays valid
    if (pc.nextRow <= v.rowsSeen) return false;
    job = { index, v.pic, v.rowsSeen, pc.nextRow, { v.done[0], v.done[1] }, v.mask, { v.w[0], v.w[1], v.w[2] } };
    v.rowsSeen = pc.nextRow;
    if (v.rowsSeen == ctuRows) v.active = false;
    return true;
}

int grow_view(const PlaneGeometry& g, const Pic& pc, const View& v, const ViewJob& job, hipStream_t stream, LineRange out[2], std::atomic<uint64_t>& linesWeighted)
{
    out[0] = out[1] = { 0, 0 };
    for (int pl = 0; pl < g.nplanes; pl++)
    {
        const int k = pl ? 1 : 0;
        const uint8_t* src = pc.dSrc[pl];
        if (job.mask & (1u << pl))
        {
            int y0, y1;
            g.lines(k, job.r0, job.r1 - job.r0, y0, y1);
            const size_t off = (size_t)y0 * g.pitch[k];
            int rc = weight_lines_launch(g.depth, src + off, v.dW[pl] + off, (size_t)(y1 - y0) * g.pitch[k] / 4, job.w[pl], stream);
            if (rc) return rc;
            linesWeighted += (uint64_t)(y1 - y0);
            src = v.dW[pl];
        }
        // every source line below the job's last row is on the device (or queued before this on the stream)
        int b0, b1;
        if (!producible_lines(g, k, job.r0, job.r1, job.done[k], b0, b1)) continue;
        const size_t lineOff = (size_t)(b0 - 4) * g.pitch[k];
        int rc = phase_planes_launch(g.depth, k, src + lineOff, v.dOut[pl] + lineOff, g.stride[k], b1 - b0 + 12, g.planeBytes[k], stream);
        if (rc) return rc;
        out[k] = { b0, b1 };
    }
    return 0;
}

} // namespace x265hip
