// row_pictures.h - the reconstructed picture that arrives CTU row by CTU row and the view that grows behind it: plane geometry, picture
// pool, view growth and the worker's round end of csrc/phase_stream.hip and csrc/cost_stream.hip (code in csrc/row_pictures.hip).
// csrc/me_stream.hip keeps a picture table of its own - rows in any order (ROW_NONE / STAGED / ON_DEVICE per row, not a prefix), derived
// (weighted) pictures in the same table, two streams, event-deferred un-pinning: only the leaves at the top of this file apply to it.
#pragma once

#include "common.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace x265hip {

// ---------------------------------------------------------------- leaves (all three row-granular services)
// primitives.weight_pp over `ndw` dwords of whole buffer lines; w = the arguments of weight_pp, round / shift including the 14 - depth correction
int weight_lines_launch(int depth, const void* src, void* dst, size_t ndw, const x265hip_weight& w, hipStream_t stream);
// such a shift is one weight_pp can have been called with
inline bool weight_shift_ok(int depth, int shift) { return shift >= 14 - depth && shift <= 31; }
// centres[ctu] = the displacement of the CTU's 64x64 minimum in best[] (a +-big search), clamped to +-maxX / [-maxY, maxYDown]
int centres_launch(const unsigned long long* best, int16_t* centres, int nctu, int big, int maxX, int maxY, int maxYDown, hipStream_t stream);

// ---------------------------------------------------------------- plane geometry
struct PlaneGeometry
{
    int depth, bpp, ctuRows, nplanes;       // nplanes: 1 (luma only) or 3 (4:2:0)
    intptr_t stride[2];                     // per plane KIND k: 0 luma, 1 chroma (plane pl is of kind pl ? 1 : 0)
    size_t pitch[2], planeBytes[2];
    int rows[2], margin[2], ctuLines[2], nph[2];

    // buffer lines [y0, y1) of plane kind k that CTU rows [r0, r0 + n) occupy; margins travel with the first / last row
    void lines(int k, int r0, int n, int& y0, int& y1) const
    {
        y0 = r0 == 0 ? 0 : margin[k] + r0 * ctuLines[k];
        y1 = r0 + n == ctuRows ? rows[k] : margin[k] + (r0 + n) * ctuLines[k];
    }
};
// rows = ctu rows * 64 + 2 * margin_y; rows_c = 0: luma only, otherwise ctu rows * 32 + 2 * margin_y_c (the caller has validated that)
PlaneGeometry plane_geometry(int depth, intptr_t stride, intptr_t stride_c, int rows, int rows_c, int margin_y, int margin_y_c);

// phase lines [b0, b1) of plane kind k that become producible when CTU rows [r0, r1) join `done` finished lines: a line needs 3 source
// lines above and up to 8 below it, so the last 8 lines of a row wait for the next row; false = fewer than 4, nothing is launched
inline bool producible_lines(const PlaneGeometry& g, int k, int r0, int r1, int done, int& b0, int& b1)
{
    int y0, y1;
    g.lines(k, r0, r1 - r0, y0, y1);
    b0 = done < 4 ? 4 : done; b1 = y1 - 8;
    return b1 - b0 >= 4;
}

// ---------------------------------------------------------------- the worker both services run
struct RowWorker
{
    std::mutex mu;                          // guards every picture / view / slot field that is not an atomic
    std::condition_variable cv;
    bool stop = false, dirty = false;
    std::thread thread;
    std::atomic<uint64_t> usBusy{0};
    char error[256] = "";                   // x265hip_last_error() of the last failed round
};
typedef std::vector<int*> Pins;             // the busy counters a round holds
inline void pin(Pins& pins, int& busy) { busy++; pins.push_back(&busy); }      // under the lock

// worker, lock held: sleeps until there is work (true, dirty cleared) or the service stops (false)
bool worker_wait(RowWorker& w, std::unique_lock<std::mutex>& lk);
// the round that started at t0 has been synchronised (rc = 0) or has failed: its pins go
void worker_round_end(RowWorker& w, hipStream_t stream, int rc, const Pins& pins, double t0);
void worker_stop(RowWorker& w, hipStream_t stream);

// ---------------------------------------------------------------- picture pool
struct Pic
{
    uint64_t key = 0; bool used = false; uint32_t epoch = 0; uint64_t stamp = 0; int busy = 0;
    uint8_t* stage[3] = { nullptr, nullptr, nullptr };      // pinned planes, rows staged by the host threads
    uint8_t* dSrc[3] = { nullptr, nullptr, nullptr };
    std::vector<uint8_t> staged;                            // per CTU row
    int nextRow = 0;                                        // rows [0, nextRow) are uploaded (or queued on the stream)
};
struct PicturePool
{
    std::vector<Pic> pics;
    uint64_t clock = 0;
};
struct RowUpload { int pic, r0, r1; };

int  device_alloc_zeroed(uint8_t** p, size_t bytes);            // hipMalloc + a zero fill that wait_for_fills() completes
int  wait_for_fills();
int  pool_alloc(PicturePool& pool, const PlaneGeometry& g, int pictures);
void pool_free(PicturePool& pool);
// host thread, entry pinned by the caller: copies CTU rows [r0, r0 + n) of the three planes into staging, then (under the lock) lets go
// of the pin, marks the rows staged if the entry is still picture `key`, and wakes the worker
void stage_rows(RowWorker& w, const PlaneGeometry& g, Pic& pc, uint64_t key, const void* const bufs[3], int r0, int n);
// worker, lock held: every picture's contiguous staged prefix becomes an upload; the entry is pinned for the round
void take_staged_prefixes(PicturePool& pool, int ctuRows, std::vector<RowUpload>& ups, Pins& pins);
int  upload(const PlaneGeometry& g, const Pic& pc, int r0, int r1, hipStream_t stream, std::atomic<uint64_t>& bytesUp);

// lock held: index of the picture named `key`, created when it is new in the least recently used entry that is not pinned and that
// held(i) does not claim; -1 = every entry is held
template <typename Held>
int find_or_make(PicturePool& pool, uint64_t key, Held held)
{
    for (int i = 0; i < (int)pool.pics.size(); i++)
        if (pool.pics[i].used && pool.pics[i].key == key) { pool.pics[i].stamp = ++pool.clock; return i; }
    int victim = -1;
    for (int i = 0; i < (int)pool.pics.size(); i++)
    {
        const Pic& p = pool.pics[i];
        if (!p.used) { victim = i; break; }
        if (p.busy || held(i)) continue;
        if (victim < 0 || p.stamp < pool.pics[victim].stamp) victim = i;
    }
    if (victim < 0) return -1;
    Pic& p = pool.pics[victim];
    p.used = true; p.key = key; p.epoch++; p.stamp = ++pool.clock; p.busy = 0;
    std::fill(p.staged.begin(), p.staged.end(), (uint8_t)0);
    p.nextRow = 0;
    return victim;
}

// ---------------------------------------------------------------- view: every fractional phase of one picture, optionally weighted first
struct View
{
    int pic = -1; uint32_t picEpoch = 0; bool active = false;      // active: still growing behind its picture
    unsigned mask = 0; x265hip_weight w[3] = {};
    uint8_t* dW[3] = { nullptr, nullptr, nullptr };         // the picture's planes weighted (only the planes of the mask)
    uint8_t* dOut[3] = { nullptr, nullptr, nullptr };       // every phase plane of the view on the device
    int rowsSeen = 0;                                       // rows [0, rowsSeen) of the picture are worked into this view
    int done[2] = { 0, 0 };                                 // buffer lines finished per plane kind
};
struct ViewJob { int view, pic, r0, r1; int done[2]; unsigned mask; x265hip_weight w[3]; };      // the view's state is snapshot under the lock
struct LineRange { int b0, b1; };

int  view_alloc(View& v, const PlaneGeometry& g, size_t outSlack);
void view_free(View& v);
// lock held: v becomes the view of picture `pic` with the planes of `mask` weighted by w (mask = 0: as reconstructed)
void view_reset(View& v, int pic, uint32_t picEpoch, const x265hip_weight* w, unsigned mask);
// worker, lock held: the job for the rows the picture has gained since the view last looked (false: none); the caller pins what the job reads
bool take_view_job(const PicturePool& pool, int ctuRows, View& v, int index, ViewJob& job);
// weights the job's new lines where the mask says so and launches the phase planes on what became producible: out[k] = those lines of
// plane kind k (b1 <= b0: none), every phase plane of them is in v.dOut once the stream has run
int  grow_view(const PlaneGeometry& g, const Pic& pc, const View& v, const ViewJob& job, hipStream_t stream, LineRange out[2], std::atomic<uint64_t>& linesWeighted);

} // namespace x265hip
