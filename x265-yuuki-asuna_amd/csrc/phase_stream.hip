// phase_stream.hip - the ROW-GRANULAR consumer of x265hip_phase_planes, for hosts that encode several pictures at once.
//
// x265hip_phase_cache (csrc/phase_cache.hip) takes a finished reference picture.  Under the reference's frame threads a picture is
// searched while it is still being reconstructed, CTU row by CTU row (Frame::m_reconRowFlag, encoder/framefilter.cpp:664; consumers wait
// row by row, encoder/frameencoder.cpp:852-868).  Two kinds of object (round 4):
//
//   PICTURE  a reconstructed picture named by a key: the producer hands every CTU row over where it raises the flag
//            (x265hip_phase_stream_picture_rows: copied into pinned staging inside the call); the worker uploads the rows.
//   VIEW     a slot = every fractional phase of ONE picture, optionally WEIGHTED first: x265's default --weightp lets a slice search the
//            plane MotionReference::applyWeight materialises (primitives.weight_pp of every finished row, encoder/reference.cpp:119-178,
//            encoder/frameencoder.cpp:865-866), and interpolating a weighted plane is not weighting an interpolated one - so a weighted
//            reference is a view of its own, keyed by (picture, weight triple).  A consumer opens the view the first time a search refers
//            to it (x265hip_phase_stream_view_open); the worker weights the picture's rows on the device as they arrive (margins included:
//            a replicated border sample weights to the replicated weighted sample), interpolates every fractional phase of the lines that
//            became computable (a line needs 3 source lines above and up to 8 below it, so the last 8 lines of a row wait for the next row)
//            and copies those lines of all 15 luma / 2 x 63 chroma planes into the view's pinned host memory.
//
// progress[0] (luma) and progress[1] (chroma) of a view = generation << 32 | lines finished, counted from the top of the buffer: a block
// whose last line is below that is the host's to interpolate itself - same samples either way (MotionEstimate::subpelCompare,
// motion.cpp:1571-1664; Predict::predInterLumaPixel / predInterChromaPixel, predict.cpp:261-351).  Readers check progress before AND after
// reading (view_open clears it before a slot's planes can be rewritten).
// x265hip_phase_stream_open / _rows (round 3: one anonymous picture per slot, opened by the producer) are kept on top of the two.
#include "row_pictures.h"

#include <cstring>
#include <new>

using namespace x265hip;

struct x265hip_phase_stream
{
    x265hip_phase_stream_params prm;
    PlaneGeometry geo;
    int device;
    hipStream_t stream = nullptr;
    struct Slot : View
    {
        uint8_t* out[3] = { nullptr, nullptr, nullptr };        // dOut in pinned host memory
        std::atomic<uint64_t> progress[2];
        int generation = 0;
    };
    PicturePool pool;
    std::vector<Slot> slots;
    uint64_t anon = 0;
    RowWorker w;
    std::atomic<uint64_t> opened{0}, completed{0}, bands{0}, failed{0}, bytesDown{0}, bytesUp{0}, weightedViews{0}, linesWeighted{0};
};

namespace {

typedef x265hip_phase_stream PS;

struct SlotJob : ViewJob { int gen; };      // view = the slot, gen = its generation when the job was cut

int run_round(PS* s, const std::vector<RowUpload>& ups, const std::vector<SlotJob>& jobs)
{
    const PlaneGeometry& g = s->geo;
    X265HIP_TRY(hipSetDevice(s->device));
    apply_wait_policy(s->device);
    int rc;
    for (const RowUpload& u : ups)
        if ((rc = upload(g, s->pool.pics[u.pic], u.r0, u.r1, s->stream, s->bytesUp))) return rc;
    std::vector<int> newDone(jobs.size() * 2);
    for (size_t j = 0; j < jobs.size(); j++)
    {
        const SlotJob& job = jobs[j];
        PS::Slot& sl = s->slots[job.view];
        LineRange made[2];
        if ((rc = grow_view(g, s->pool.pics[job.pic], sl, job, s->stream, made, s->linesWeighted))) return rc;
        newDone[2 * j] = job.done[0]; newDone[2 * j + 1] = job.done[1];
        for (int pl = 0; pl < g.nplanes; pl++)
        {
            const int k = pl ? 1 : 0;
            if (made[k].b1 <= made[k].b0) continue;
            const size_t o = (size_t)made[k].b0 * g.pitch[k], w = (size_t)(made[k].b1 - made[k].b0) * g.pitch[k];
            X265HIP_TRY(hipMemcpy2DAsync(sl.out[pl] + o, g.planeBytes[k], sl.dOut[pl] + o, g.planeBytes[k], w, g.nph[k], hipMemcpyDeviceToHost, s->stream));
            s->bytesDown += w * g.nph[k];
            newDone[2 * j + k] = made[k].b1;
        }
    }
    X265HIP_TRY(hipStreamSynchronize(s->stream));
    {
        std::lock_guard<std::mutex> lk(s->w.mu);             // against view_open(): a reopened slot keeps its cleared progress
        for (size_t j = 0; j < jobs.size(); j++)
        {
            const SlotJob& job = jobs[j];
            PS::Slot& sl = s->slots[job.view];
            if (sl.generation != job.gen) continue;
            for (int k = 0; k < 2; k++)
            {
                sl.done[k] = newDone[2 * j + k];
                sl.progress[k].store((uint64_t)(uint32_t)job.gen << 32 | (uint32_t)sl.done[k], std::memory_order_release);
            }
            if (job.r1 == g.ctuRows) s->completed++;
        }
    }
    s->bands += jobs.size();
    return 0;
}

void ps_worker(PS* s)
{
    for (;;)
    {
        std::vector<RowUpload> ups;
        std::vector<SlotJob> jobs;
        Pins pins;
        {
            std::unique_lock<std::mutex> lk(s->w.mu);
            if (!worker_wait(s->w, lk)) return;
            take_staged_prefixes(s->pool, s->geo.ctuRows, ups, pins);
            for (int i = 0; i < (int)s->slots.size(); i++)
            {
                SlotJob job;
                if (!take_view_job(s->pool, s->geo.ctuRows, s->slots[i], i, job)) continue;
                job.gen = s->slots[i].generation;
                jobs.push_back(job);
                pin(pins, s->pool.pics[job.pic].busy);
            }
        }
        if (ups.empty() && jobs.empty()) continue;
        const double t0 = now_us();
        const int rc = run_round(s, ups, jobs);
        if (rc) s->failed++;
        worker_round_end(s->w, s->stream, rc, pins, t0);
    }
}

void ps_free(PS* s)
{
    pool_free(s->pool);
    for (auto& sl : s->slots)
    {
        view_free(sl);
        for (int i = 0; i < 3; i++)
            if (sl.out[i]) (void)hipHostFree(sl.out[i]);
    }
    if (s->stream) (void)hipStreamDestroy(s->stream);
}

// lock held: the entry of picture `key`; an entry an active view is still being fed from is not recycled
int ps_picture(PS* s, uint64_t key)
{
    return find_or_make(s->pool, key, [s](int i) {
        bool held = false;
        for (const auto& sl : s->slots) held |= sl.active && sl.pic == i && sl.picEpoch == s->pool.pics[i].epoch;
        return held;
    });
}

int ps_view_open_locked(PS* s, int slot, int pic, const x265hip_weight* w, unsigned mask)
{
    PS::Slot& sl = s->slots[slot];
    if (++sl.generation <= 0) sl.generation = 1;
    sl.progress[0].store(0, std::memory_order_release); sl.progress[1].store(0, std::memory_order_release);      // before anything is rewritten
    view_reset(sl, pic, s->pool.pics[pic].epoch, w, w ? mask : 0);
    s->opened++;
    if (sl.mask) s->weightedViews++;
    s->w.dirty = true;
    return sl.generation;
}

} // namespace

extern "C" {

int x265hip_phase_stream_create(x265hip_phase_stream** out, const x265hip_phase_stream_params* p)
{
    if (!out || !p) { set_error("phase_stream_create: NULL argument"); return X265HIP_EINVAL; }
    *out = nullptr;
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("phase_stream_create: depth %d", p->depth); return X265HIP_EINVAL; }
    if (p->stride <= 0 || (p->stride & 3) || p->ctu_rows < 1 || p->margin_y < 8 || (p->margin_y & 3))
    { set_error("phase_stream_create: luma pitch %ld / %d CTU rows / margin %d", (long)p->stride, p->ctu_rows, p->margin_y); return X265HIP_EINVAL; }
    if (p->rows_c < 0 || (p->rows_c > 0 && (p->stride_c <= 0 || (p->stride_c & 3) || p->margin_y_c < 8 || (p->margin_y_c & 3) ||
                                            p->rows_c != p->ctu_rows * 32 + 2 * p->margin_y_c)))
    { set_error("phase_stream_create: chroma geometry (4:2:0: rows_c = ctu_rows * 32 + 2 * margin_y_c)"); return X265HIP_EINVAL; }
    if (p->rows != p->ctu_rows * 64 + 2 * p->margin_y) { set_error("phase_stream_create: rows %d != ctu_rows * 64 + 2 * margin_y", p->rows); return X265HIP_EINVAL; }
    if (p->slots < 1 || p->slots > 64 || p->pictures < 0 || p->pictures > 256) { set_error("phase_stream_create: slots %d out of [1,64] / pictures %d out of [0,256]", p->slots, p->pictures); return X265HIP_EINVAL; }
    int rc = ensure_device();
    if (rc) return rc;
    if (p->device_plus_1 < 0 || p->device_plus_1 > x265hip_device_count()) { set_error("phase_stream_create: device %d of %d", p->device_plus_1 - 1, x265hip_device_count()); return X265HIP_ENODEV; }
    if (p->device_plus_1 > 0 && (rc = x265hip_init(p->device_plus_1 - 1))) return rc;       // pinned to a GPU: current for the creating thread from here on
    PS* s = new (std::nothrow) PS;
    if (!s) { set_error("phase_stream_create: out of memory"); return X265HIP_EINVAL; }
    s->prm = *p;
    s->geo = plane_geometry(p->depth, p->stride, p->stride_c, p->rows, p->rows_c, p->margin_y, p->margin_y_c);
    const PlaneGeometry& g = s->geo;
    if (hipGetDevice(&s->device) != hipSuccess) s->device = 0;
    auto fail = [s] { ps_free(s); delete s; return X265HIP_ENODEV; };
#define PS_TRY(expr) do { if (check_hip((expr), #expr)) return fail(); } while (0)
    PS_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if (pool_alloc(s->pool, g, p->pictures ? p->pictures : p->slots)) return fail();
    s->slots = std::vector<PS::Slot>(p->slots);
    for (auto& sl : s->slots)
    {
        sl.progress[0].store(0); sl.progress[1].store(0);
        if (view_alloc(sl, g, 0)) return fail();
        for (int i = 0; i < g.nplanes; i++)
            PS_TRY(hipHostMalloc((void**)&sl.out[i], g.planeBytes[i ? 1 : 0] * g.nph[i ? 1 : 0], hipHostMallocDefault));
    }
#undef PS_TRY
    if (wait_for_fills()) return fail();
    s->w.thread = std::thread(ps_worker, s);
    *out = s;
    return 0;
}

void x265hip_phase_stream_destroy(x265hip_phase_stream* s)
{
    if (!s) return;
    worker_stop(s->w, s->stream);
    ps_free(s);
    delete s;
}

/* CTU rows [ctu_row0, ctu_row0 + ctu_rows) of the picture named `key` are final in the three buffers (whole allocated planes; cb / cr
 * may be NULL when rows_c = 0); copied before the call returns.  X265HIP_EBUSY: every picture entry still feeds a view. */
int x265hip_phase_stream_picture_rows(x265hip_phase_stream* s, uint64_t key, const void* luma_buf, const void* cb_buf, const void* cr_buf, int ctu_row0, int ctu_rows)
{
    if (!s || !luma_buf || (s->prm.rows_c > 0 && (!cb_buf || !cr_buf)) || ctu_row0 < 0 || ctu_rows < 1 || ctu_row0 + ctu_rows > s->geo.ctuRows)
    { set_error("phase_stream_picture_rows: bad argument"); return X265HIP_EINVAL; }
    int idx;
    {
        std::lock_guard<std::mutex> lk(s->w.mu);
        idx = ps_picture(s, key);
        if (idx < 0) { set_error("phase_stream_picture_rows: every picture entry still feeds a view (pictures = %d)", (int)s->pool.pics.size()); return X265HIP_EBUSY; }
        s->pool.pics[idx].busy++;
    }
    const void* bufs[3] = { luma_buf, cb_buf, cr_buf };
    stage_rows(s->w, s->geo, s->pool.pics[idx], key, bufs, ctu_row0, ctu_rows);
    return 0;
}

/* `slot` becomes the view of picture `key` - w = NULL: as reconstructed; otherwise plane c (0 luma, 1 Cb, 2 Cr) is weighted with w[c]
 * (the arguments of primitives.weight_pp, round / shift including the 14 - depth correction) when bit c of planes_weighted is set.
 * The picture's rows may arrive before or after.  Returns the slot's new GENERATION (> 0); progress is cleared before anything is
 * rewritten. */
int x265hip_phase_stream_view_open(x265hip_phase_stream* s, int slot, uint64_t key, const x265hip_weight* w, unsigned planes_weighted)
{
    if (!s || slot < 0 || slot >= (int)s->slots.size()) { set_error("phase_stream_view_open: bad slot"); return X265HIP_EINVAL; }
    if (w)
        for (int c = 0; c < s->geo.nplanes; c++)
            if ((planes_weighted & (1u << c)) && !weight_shift_ok(s->prm.depth, w[c].shift))
            { set_error("phase_stream_view_open: plane %d shift %d (it includes the 14 - depth correction of weight_pp)", c, w[c].shift); return X265HIP_EINVAL; }
    int gen;
    {
        std::lock_guard<std::mutex> lk(s->w.mu);
        const bool was = s->slots[slot].active;
        s->slots[slot].active = false;                        // the slot's previous view no longer holds its picture
        const int pic = ps_picture(s, key);
        if (pic < 0) { s->slots[slot].active = was; set_error("phase_stream_view_open: no picture entry free (pictures = %d)", (int)s->pool.pics.size()); return X265HIP_EBUSY; }
        gen = ps_view_open_locked(s, slot, pic, w, planes_weighted & ((1u << s->geo.nplanes) - 1));
    }
    s->w.cv.notify_one();
    return gen;
}

/* round-3 entry: a new reconstructed picture takes `slot` (an anonymous picture of its own, unweighted view) */
int x265hip_phase_stream_open(x265hip_phase_stream* s, int slot)
{
    if (!s || slot < 0 || slot >= (int)s->slots.size()) { set_error("phase_stream_open: bad slot"); return X265HIP_EINVAL; }
    uint64_t key;
    {
        std::lock_guard<std::mutex> lk(s->w.mu);
        key = (1ull << 63) | ((uint64_t)slot << 40) | (++s->anon & 0xffffffffffull);
    }
    return x265hip_phase_stream_view_open(s, slot, key, nullptr, 0);
}

int x265hip_phase_stream_rows(x265hip_phase_stream* s, int slot, int gen, const void* luma_buf, const void* cb_buf, const void* cr_buf, int ctu_row0, int ctu_rows)
{
    if (!s || slot < 0 || slot >= (int)s->slots.size()) { set_error("phase_stream_rows: bad argument"); return X265HIP_EINVAL; }
    uint64_t key;
    {
        std::lock_guard<std::mutex> lk(s->w.mu);
        PS::Slot& sl = s->slots[slot];
        if (sl.generation != gen || sl.pic < 0 || !s->pool.pics[sl.pic].used || s->pool.pics[sl.pic].epoch != sl.picEpoch)
        { set_error("phase_stream_rows: slot %d was reopened (generation %d, not %d)", slot, sl.generation, gen); return X265HIP_EBUSY; }
        key = s->pool.pics[sl.pic].key;
    }
    return x265hip_phase_stream_picture_rows(s, key, luma_buf, cb_buf, cr_buf, ctu_row0, ctu_rows);
}

const void* x265hip_phase_stream_planes(x265hip_phase_stream* s, int slot, int plane)
{
    return (s && slot >= 0 && slot < (int)s->slots.size() && plane >= 0 && plane < 3) ? s->slots[slot].out[plane] : nullptr;
}

const volatile uint64_t* x265hip_phase_stream_progress(x265hip_phase_stream* s, int slot)
{
    return (s && slot >= 0 && slot < (int)s->slots.size()) ? reinterpret_cast<const volatile uint64_t*>(s->slots[slot].progress) : nullptr;
}

int x265hip_phase_stream_stats(x265hip_phase_stream* s, x265hip_phase_stream_stats_t* st)
{
    if (!s || !st) { set_error("phase_stream_stats: NULL"); return X265HIP_EINVAL; }
    st->opened = s->opened; st->completed = s->completed; st->bands = s->bands; st->failed = s->failed; st->us_busy = s->w.usBusy;
    st->bytes_downloaded = s->bytesDown; st->bytes_uploaded = s->bytesUp;
    st->bytes_per_picture = s->geo.planeBytes[0] * 15 + 2 * s->geo.planeBytes[1] * 63;
    st->weighted_views = s->weightedViews; st->lines_weighted = s->linesWeighted;
    if (s->failed) set_error("phase_stream worker: %s", s->w.error);
    return 0;
}

} // extern "C"
