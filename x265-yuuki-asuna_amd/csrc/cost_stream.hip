// cost_stream.hip - the ROW-GRANULAR service of the sub-sample cost tables (include/x265hip.h, "SUB-SAMPLE COST TABLES"): what a host
// that runs the reference's frame threads plugs behind MotionEstimate::subpelCompare.
//
//   PICTURE  source or reconstructed picture (three planes, PicYuv layout) named by a key; a source picture arrives in one piece, a
//            reconstructed one CTU row by CTU row where the reference raises Frame::m_reconRowFlag (encoder/framefilter.cpp:664).
//   VIEW     (reconstructed picture, weights): the planes a search on that reference reads - MotionReference::applyWeight's weight_pp
//            planes when the slice weights the reference (encoder/reference.cpp:119-178) - and all their fractional phases
//            (x265hip_phase_planes), growing line by line behind the rows.  DEVICE memory only; pairs on the same view share it.
//   PAIR     slot = (source picture, view): per CTU row, as soon as the source row and the view's lines the row's candidates can reach
//            (reference rows <= r + 2: what the host's own frame encoder waits for, encoder/frameencoder.cpp:161-164,852-868) are there:
//            centre search (+-centre_range minima, SAD alone) -> SAD rasters of +-window around each CTU's centre -> candidates of every
//            PU shape -> SATD tables around them (csrc/cost_kernels.hip) -> records to pinned host memory, ready[row] = generation.
// One worker thread, one HIP stream: uploads, weighting, interpolation and the table chain of a round are stream-ordered; the round ends
// with one synchronisation, then the flags of its bands are raised.  Readers never wait and never lock (ready[row] before AND after the
// read); whatever is not served is the host primitive's to compute - the same integers.
#include "row_pictures.h"

#include <cstring>
#include <new>

using namespace x265hip;

struct x265hip_cost_stream
{
    x265hip_cost_stream_params prm;
    PlaneGeometry geo;
    int device, ctusW, bandRows, npu, recBytes, maxCx, maxCy, maxCyDown;
    size_t ctuBytes, rowBytes;
    hipStream_t stream = nullptr;
    struct View : x265hip::View
    {
        bool used = false; uint64_t stamp = 0; int busy = 0;          // busy: launches of the running round read it
    };
    struct Slot
    {
        uint8_t* tables = nullptr;                              // pinned host memory
        std::atomic<int>* ready = nullptr;
        int generation = 0;
        int fenc = -1, view = -1; uint32_t fencEpoch = 0; uint64_t viewStamp = 0;
        int nextRow = 0; bool active = false;
        int bandLimit = 1;                                      // rows of the pair's next band: 1, 2, 4 ... band_rows - the first rows of EVERY open pair land before anybody's last ones
        uint16_t* hMvCost = nullptr; uint16_t* dMvCost = nullptr; bool hasCost = false;      // the pair's vector-cost table (pinned staging, device copy); !hasCost: rank by SAD alone
    };
    PicturePool pool;
    std::vector<View> views;
    std::vector<Slot> slots;
    // one band's scratch
    uint8_t* dSurf = nullptr; unsigned long long* dBest = nullptr; uint16_t* dZeroCost = nullptr; int16_t* dCentres = nullptr; int16_t* dCand = nullptr; uint8_t* dTables = nullptr;
    RowWorker w;
    std::atomic<uint64_t> pairsOpened{0}, pairsCompleted{0}, bands{0}, rowsServed{0}, rowsUploaded{0}, failed{0}, stalePairs{0}, viewsOpened{0}, viewsShared{0}, linesWeighted{0};
    std::atomic<uint64_t> bytesDown{0}, bytesUp{0};
};

namespace {

typedef x265hip_cost_stream CS;

struct Band { int slot, gen, r0, r1, fenc, view; bool hasCost; };

int run_round(CS* s, const std::vector<RowUpload>& ups, const std::vector<ViewJob>& jobs, const std::vector<Band>& bands)
{
    const PlaneGeometry& g = s->geo;
    X265HIP_TRY(hipSetDevice(s->device));
    apply_wait_policy(s->device);
    int rc;
    for (const RowUpload& u : ups)
    {
        if ((rc = upload(g, s->pool.pics[u.pic], u.r0, u.r1, s->stream, s->bytesUp))) return rc;
        s->rowsUploaded += u.r1 - u.r0;
    }
    for (const ViewJob& job : jobs)
    {
        LineRange made[2];              // the worker has advanced the view's done[] by the same rule
        if ((rc = grow_view(g, s->pool.pics[job.pic], s->views[job.view], job, s->stream, made, s->linesWeighted))) return rc;
    }
    const size_t org = ((size_t)s->prm.margin_y * s->prm.stride + s->prm.margin_x) * g.bpp;
    for (const Band& b : bands)
    {
        CS::Slot& sl = s->slots[b.slot];
        const CS::View& v = s->views[b.view];
        const int n = b.r1 - b.r0 + 1, nctuBand = n * s->ctusW;
        const size_t bandOff = (size_t)b.r0 * 64 * g.pitch[0];
        const uint8_t* refL = (v.mask & 1) ? v.dW[0] : s->pool.pics[v.pic].dSrc[0];
        x265hip_me_params p;
        memset(&p, 0, sizeof(p));
        p.depth = s->prm.depth; p.width = s->prm.width; p.height = n * 64;
        p.fenc = s->pool.pics[b.fenc].dSrc[0] + org + bandOff; p.fenc_stride = s->prm.stride;
        p.fref = refL + org + bandOff; p.fref_stride = s->prm.stride;
        if (s->prm.centre_range)
        {
            if ((rc = x265hip_me_best_reset((uint64_t*)s->dBest, (size_t)nctuBand * 85, s->stream))) return rc;
            p.range = s->prm.centre_range; p.best = (uint64_t*)s->dBest; p.cost_x = p.cost_y = s->dZeroCost;
            if ((rc = x265hip_me_fullsearch(&p, s->stream))) return rc;
            if ((rc = centres_launch((const unsigned long long*)s->dBest, s->dCentres, nctuBand, s->prm.centre_range, s->maxCx, s->maxCy, s->maxCyDown, s->stream))) return rc;
            p.best = nullptr; p.cost_x = p.cost_y = nullptr;
        }
        else
            X265HIP_TRY(hipMemsetAsync(s->dCentres, 0, (size_t)nctuBand * 4, s->stream));
        p.centres = s->dCentres;
        p.range = s->prm.window; p.surf_format = X265HIP_SURF_I32; p.surf = (int32_t*)s->dSurf;
        if ((rc = x265hip_me_fullsearch(&p, s->stream))) return rc;
        const uint16_t* mvCost = nullptr;
        if (b.hasCost)
        {
            // a slot reopened under this copy belongs to a stale generation: its band is discarded below
            X265HIP_TRY(hipMemcpyAsync(sl.dMvCost, sl.hMvCost, (2 * (size_t)s->prm.window + 1) * sizeof(uint16_t), hipMemcpyHostToDevice, s->stream));
            mvCost = sl.dMvCost;
        }
        x265hip_cost_candidates_params c = { nctuBand, s->prm.window, (const int32_t*)s->dSurf, s->dCentres, s->prm.shapes, s->prm.candidates, s->dCand, mvCost };
        if ((rc = x265hip_cost_candidates(&c, s->stream))) return rc;
        x265hip_cost_tables_params t;
        memset(&t, 0, sizeof(t));
        t.depth = s->prm.depth; t.width = s->prm.width; t.stride = s->prm.stride; t.margin_x = s->prm.margin_x; t.margin_y = s->prm.margin_y;
        t.stride_c = s->prm.stride_c; t.margin_y_c = s->prm.margin_y_c; t.ctu_row0 = b.r0; t.ctu_rows = n;
        for (int pl = 0; pl < g.nplanes; pl++)
        {
            t.fenc[pl] = s->pool.pics[b.fenc].dSrc[pl];
            t.ref[pl] = (v.mask & (1u << pl)) ? v.dW[pl] : s->pool.pics[v.pic].dSrc[pl];
            t.phases[pl] = v.dOut[pl];
        }
        t.plane_bytes = g.planeBytes[0]; t.plane_bytes_c = g.planeBytes[1];
        t.shapes = s->prm.shapes; t.candidates = s->prm.candidates; t.subme = s->prm.subme; t.chroma = s->prm.chroma; t.sad_costs = s->prm.sad_costs;
        t.cand = s->dCand; t.tables = s->dTables;
        if ((rc = x265hip_cost_tables(&t, s->stream))) return rc;
        X265HIP_TRY(hipMemcpyAsync(sl.tables + (size_t)b.r0 * s->rowBytes, s->dTables, (size_t)n * s->rowBytes, hipMemcpyDeviceToHost, s->stream));
        s->bytesDown += (size_t)n * s->rowBytes;
    }
    X265HIP_TRY(hipStreamSynchronize(s->stream));
    if (!bands.empty())
    {
        std::lock_guard<std::mutex> lk(s->w.mu);                    // against pair_open: a reopened slot keeps its cleared flags
        for (const Band& b : bands)
        {
            CS::Slot& sl = s->slots[b.slot];
            if (sl.generation == b.gen)
            {
                for (int r = b.r0; r <= b.r1; r++) sl.ready[r].store(b.gen, std::memory_order_release);
                if (b.r1 == g.ctuRows - 1) s->pairsCompleted++;
            }
            s->bands++; s->rowsServed += b.r1 - b.r0 + 1;
        }
    }
    return 0;
}

void cs_worker(CS* s)
{
    const int ctuRows = s->geo.ctuRows;
    for (;;)
    {
        std::vector<RowUpload> ups;
        std::vector<ViewJob> jobs;
        std::vector<Band> bands;
        Pins pins;
        {
            std::unique_lock<std::mutex> lk(s->w.mu);
            if (!worker_wait(s->w, lk)) return;
            take_staged_prefixes(s->pool, ctuRows, ups, pins);
            for (int i = 0; i < (int)s->views.size(); i++)
            {
                CS::View& v = s->views[i];
                ViewJob job;
                if (!v.used || !take_view_job(s->pool, ctuRows, v, i, job)) continue;
                jobs.push_back(job);
                pin(pins, s->pool.pics[job.pic].busy); pin(pins, v.busy);
                // the lines this job will have produced (the launches are stream-ordered before any band of this round)
                for (int k = 0; k < (s->geo.nplanes > 1 ? 2 : 1); k++)
                {
                    int b0, b1;
                    if (producible_lines(s->geo, k, job.r0, job.r1, v.done[k], b0, b1)) v.done[k] = b1;
                }
            }
            for (int i = 0; i < (int)s->slots.size(); i++)
            {
                CS::Slot& sl = s->slots[i];
                if (!sl.active) continue;
                const Pic& pf = s->pool.pics[sl.fenc];
                const CS::View& v = s->views[sl.view];
                if (!pf.used || pf.epoch != sl.fencEpoch || !v.used || v.stamp != sl.viewStamp ||
                    (v.rowsSeen < ctuRows && (!s->pool.pics[v.pic].used || s->pool.pics[v.pic].epoch != v.picEpoch)))
                { sl.active = false; s->stalePairs++; continue; }
                int r1 = sl.nextRow - 1;
                while (r1 + 1 < ctuRows && r1 + 1 - sl.nextRow < sl.bandLimit)
                {
                    const int r = r1 + 1;
                    const int need = r + 2 > ctuRows ? ctuRows : r + 2;          // the candidates of row r reach <= 44 luma lines below it (maxCyDown + window + 2)
                    if (pf.nextRow <= r || v.rowsSeen < need) break;
                    r1 = r;
                }
                if (r1 < sl.nextRow) continue;
                bands.push_back({ i, sl.generation, sl.nextRow, r1, sl.fenc, sl.view, sl.hasCost });
                pin(pins, s->pool.pics[sl.fenc].busy); pin(pins, s->pool.pics[v.pic].busy); pin(pins, s->views[sl.view].busy);
                sl.nextRow = r1 + 1;
                sl.bandLimit = sl.bandLimit * 2 > s->bandRows ? s->bandRows : sl.bandLimit * 2;
                if (sl.nextRow == ctuRows) sl.active = false;
                else s->w.dirty = true;
            }
        }
        if (ups.empty() && jobs.empty() && bands.empty()) continue;
        const double t0 = now_us();
        const int rc = run_round(s, ups, jobs, bands);
        if (rc) s->failed += bands.size() + 1;
        worker_round_end(s->w, s->stream, rc, pins, t0);
    }
}

void cs_free(CS* s)
{
    pool_free(s->pool);
    for (auto& v : s->views) view_free(v);
    for (auto& sl : s->slots) { if (sl.tables) (void)hipHostFree(sl.tables); if (sl.hMvCost) (void)hipHostFree(sl.hMvCost); if (sl.dMvCost) (void)hipFree(sl.dMvCost); delete[] sl.ready; }
    if (s->dSurf) (void)hipFree(s->dSurf);
    if (s->dBest) (void)hipFree(s->dBest);
    if (s->dZeroCost) (void)hipFree(s->dZeroCost);
    if (s->dCentres) (void)hipFree(s->dCentres);
    if (s->dCand) (void)hipFree(s->dCand);
    if (s->dTables) (void)hipFree(s->dTables);
    if (s->stream) (void)hipStreamDestroy(s->stream);
}

bool cs_pic_held(const CS* s, int i)
{
    const Pic& p = s->pool.pics[i];
    for (const auto& v : s->views)
        if (v.used && v.pic == i && v.picEpoch == p.epoch)
        {
            if (v.active) return true;
            // a finished view still reads its picture's planes where it is not weighted (phase 0 = the picture itself)
            for (const auto& sl : s->slots) if (sl.active && sl.view == (int)(&v - &s->views[0]) && sl.viewStamp == v.stamp) return true;
        }
    for (const auto& sl : s->slots) if (sl.active && sl.fenc == i && sl.fencEpoch == p.epoch) return true;
    return false;
}

// lock held: the entry of picture `key` (find_or_make); cs_pic_held() entries are not recycled
int cs_picture(CS* s, uint64_t key)
{
    const int i = find_or_make(s->pool, key, [s](int i) { return cs_pic_held(s, i); });
    // views of a recycled entry (they carry its previous epoch) are void: their unweighted planes are the picture's own
    if (i >= 0)
        for (auto& v : s->views) if (v.used && v.pic == i && v.picEpoch != s->pool.pics[i].epoch) { v.used = false; v.active = false; }
    return i;
}

bool same_w(const x265hip_weight& a, const x265hip_weight& b) { return a.w0 == b.w0 && a.round == b.round && a.shift == b.shift && a.offset == b.offset; }

// the view of (pic, weights): an existing one (shared) or a new one in the least recently used entry no active pair reads; -1 = all held
int cs_find_or_make_view(CS* s, int pic, const x265hip_weight* w, unsigned mask)
{
    const Pic& pc = s->pool.pics[pic];
    for (int i = 0; i < (int)s->views.size(); i++)
    {
        CS::View& v = s->views[i];
        if (!v.used || v.pic != pic || v.picEpoch != pc.epoch || v.mask != mask) continue;
        bool same = true;
        for (int c = 0; c < 3 && same; c++) if (mask & (1u << c)) same = same_w(v.w[c], w[c]);
        if (same) { s->viewsShared++; return i; }
    }
    int victim = -1;
    for (int i = 0; i < (int)s->views.size(); i++)
    {
        CS::View& v = s->views[i];
        if (!v.used) { victim = i; break; }
        bool held = v.busy > 0 || v.active;
        for (const auto& sl : s->slots) held |= sl.active && sl.view == i && sl.viewStamp == v.stamp;
        if (!held && (victim < 0 || v.stamp < s->views[victim].stamp)) victim = i;
    }
    if (victim < 0) return -1;
    CS::View& v = s->views[victim];
    v.used = true; v.stamp = ++s->pool.clock; v.busy = 0;
    view_reset(v, pic, pc.epoch, w, mask);
    s->viewsOpened++;
    return victim;
}

} // namespace

extern "C" {

int x265hip_cost_stream_create(x265hip_cost_stream** out, const x265hip_cost_stream_params* p)
{
    if (!out || !p) { set_error("cost_stream_create: NULL argument"); return X265HIP_EINVAL; }
    *out = nullptr;
    if (p->depth != 8 && p->depth != 10 && p->depth != 12) { set_error("cost_stream_create: depth %d", p->depth); return X265HIP_EINVAL; }
    if (p->width < 64 || (p->width & 63) || p->height < 64 || (p->height & 63) || p->stride < p->width + 2 * p->margin_x || (p->stride & 3) || (p->margin_x & 3) ||
        p->margin_y < 16 || (p->margin_y & 3))
    { set_error("cost_stream_create: luma geometry %dx%d pitch %ld margins %d / %d", p->width, p->height, (long)p->stride, p->margin_x, p->margin_y); return X265HIP_EINVAL; }
    const bool hasC = p->stride_c > 0;
    if (hasC && (p->stride_c < p->width / 2 + 2 * p->margin_x || (p->stride_c & 3) || p->margin_y_c < 8 || (p->margin_y_c & 3) || p->margin_y_c * 2 > p->margin_y))
    { set_error("cost_stream_create: chroma geometry pitch %ld margin %d", (long)p->stride_c, p->margin_y_c); return X265HIP_EINVAL; }
    if (p->chroma && !hasC) { set_error("cost_stream_create: chroma costs need the chroma planes"); return X265HIP_EINVAL; }
    if (p->window < 0 || p->window > 32 || p->centre_range < 0 || p->centre_range + 12 > p->margin_x || p->centre_range + 12 > p->margin_y || p->candidates < 1 || p->candidates > 2 || p->shapes < 0 || p->shapes > 2 ||
        x265hip_cost_record_bytes(p->subme, 0) == 0)
    { set_error("cost_stream_create: window %d / centre range %d / %d candidates / shape set %d / subme %d", p->window, p->centre_range, p->candidates, p->shapes, p->subme); return X265HIP_EINVAL; }
    if (p->slots < 1 || p->slots > 256 || p->pictures < 2 || p->pictures > 256 || p->views < 1 || p->views > 64)
    { set_error("cost_stream_create: %d slots / %d pictures / %d views", p->slots, p->pictures, p->views); return X265HIP_EINVAL; }
    // the candidates of a CTU lie within centre +- window; the fractional positions reach 2 samples further, the phase planes' lines [4, rows - 8) are valid
    // (chroma: the vector halves): |candidate| <= margin_y - 20 vertically, margin_x - 12 horizontally.  DOWNWARDS a row's candidates must stay inside the
    // reference rows <= r + 1 (the row is computed one reference row before the host may start it): the view's lines end 8 above the last row's end, so a luma
    // block may reach 64 - 8 - 2 = 54 lines, a chroma block 32 - 8 - 2 = 22 = luma 42: candidate <= 42 (luma only: 54)
    const int maxCx = p->margin_x - p->window - 12, maxCy = (hasC && p->margin_y_c * 2 < p->margin_y ? p->margin_y_c * 2 : p->margin_y) - p->window - 20;
    const int maxCyDownRaw = (hasC ? 42 : 54) - p->window;
    if (maxCx < 0 || maxCy < 0 || maxCyDownRaw < 0) { set_error("cost_stream_create: margins %d / %d too small for a window of +-%d", p->margin_x, p->margin_y, p->window); return X265HIP_EINVAL; }
    int rc = ensure_device();
    if (rc) return rc;
    if (p->device_plus_1 < 0 || p->device_plus_1 > x265hip_device_count()) { set_error("cost_stream_create: device %d of %d", p->device_plus_1 - 1, x265hip_device_count()); return X265HIP_ENODEV; }
    if (p->device_plus_1 > 0 && (rc = x265hip_init(p->device_plus_1 - 1))) return rc;
    CS* s = new (std::nothrow) CS;
    if (!s) { set_error("cost_stream_create: out of memory"); return X265HIP_EINVAL; }
    s->prm = *p;
    s->geo = plane_geometry(p->depth, p->stride, p->stride_c, p->height + 2 * p->margin_y, hasC ? p->height / 2 + 2 * p->margin_y_c : 0, p->margin_y, p->margin_y_c);
    const PlaneGeometry& g = s->geo;
    const int ctuRows = g.ctuRows;
    s->ctusW = p->width / 64;
    s->bandRows = p->band_rows > 0 ? p->band_rows : 8;
    if (s->bandRows > ctuRows) s->bandRows = ctuRows;
    s->npu = x265hip_cost_pu_count(p->shapes);
    s->recBytes = x265hip_cost_record_bytes(p->subme, p->sad_costs);
    s->ctuBytes = x265hip_cost_ctu_bytes(p->subme, p->shapes, p->candidates, p->sad_costs);
    s->rowBytes = s->ctuBytes * s->ctusW;
    s->maxCx = maxCx; s->maxCy = maxCy;
    if (p->centre_range && (s->maxCx > p->centre_range)) s->maxCx = p->centre_range;
    if (p->centre_range && (s->maxCy > p->centre_range)) s->maxCy = p->centre_range;
    s->maxCyDown = maxCyDownRaw < s->maxCy ? maxCyDownRaw : s->maxCy;
    if (hipGetDevice(&s->device) != hipSuccess) s->device = 0;
    auto fail = [s] { cs_free(s); delete s; return X265HIP_ENODEV; };
#define CS_TRY(expr) do { if (check_hip((expr), #expr)) return fail(); } while (0)
    CS_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if (pool_alloc(s->pool, g, p->pictures)) return fail();
    s->views = std::vector<CS::View>(p->views);
    for (auto& v : s->views)
        if (view_alloc(v, g, 256)) return fail();
    s->slots = std::vector<CS::Slot>(p->slots);
    for (auto& sl : s->slots)
    {
        CS_TRY(hipHostMalloc((void**)&sl.tables, s->rowBytes * ctuRows, hipHostMallocDefault));
        CS_TRY(hipHostMalloc((void**)&sl.hMvCost, (2 * (size_t)p->window + 1) * sizeof(uint16_t), hipHostMallocDefault));
        CS_TRY(hipMalloc((void**)&sl.dMvCost, (2 * (size_t)p->window + 1) * sizeof(uint16_t)));
        sl.ready = new (std::nothrow) std::atomic<int>[ctuRows];
        if (!sl.ready) { set_error("cost_stream_create: out of memory"); cs_free(s); delete s; return X265HIP_EINVAL; }
        for (int r = 0; r < ctuRows; r++) sl.ready[r].store(0);
    }
    const size_t nctuBand = (size_t)s->bandRows * s->ctusW;
    CS_TRY(hipMalloc((void**)&s->dSurf, nctuBand * x265hip_surf_ctu_bytes(X265HIP_SURF_I32, p->window) + 256));
    CS_TRY(hipMalloc((void**)&s->dBest, nctuBand * 85 * sizeof(unsigned long long)));
    CS_TRY(hipMalloc((void**)&s->dZeroCost, (2 * (size_t)(p->centre_range ? p->centre_range : 1) + 1) * sizeof(uint16_t)));
    CS_TRY(hipMemset(s->dZeroCost, 0, (2 * (size_t)(p->centre_range ? p->centre_range : 1) + 1) * sizeof(uint16_t)));
    CS_TRY(hipMalloc((void**)&s->dCentres, nctuBand * 4));
    CS_TRY(hipMalloc((void**)&s->dCand, nctuBand * s->npu * p->candidates * 4));
    CS_TRY(hipMalloc((void**)&s->dTables, nctuBand * s->ctuBytes));
#undef CS_TRY
    if (wait_for_fills()) return fail();
    s->w.thread = std::thread(cs_worker, s);
    *out = s;
    return 0;
}

void x265hip_cost_stream_destroy(x265hip_cost_stream* s)
{
    if (!s) return;
    worker_stop(s->w, s->stream);
    cs_free(s);
    delete s;
}

int x265hip_cost_stream_picture_rows(x265hip_cost_stream* s, uint64_t key, const void* luma_buf, const void* cb_buf, const void* cr_buf, int ctu_row0, int ctu_rows)
{
    if (!s || !luma_buf || (s->geo.nplanes > 1 && (!cb_buf || !cr_buf)) || ctu_row0 < 0 || ctu_rows < 1 || ctu_row0 + ctu_rows > s->geo.ctuRows)
    { set_error("cost_stream_picture_rows: bad argument"); return X265HIP_EINVAL; }
    int idx;
    {
        std::lock_guard<std::mutex> lk(s->w.mu);
        idx = cs_picture(s, key);
        if (idx < 0) { set_error("cost_stream_picture_rows: every picture entry is still read (pictures = %d)", (int)s->pool.pics.size()); return X265HIP_EBUSY; }
        s->pool.pics[idx].busy++;
    }
    const void* bufs[3] = { luma_buf, cb_buf, cr_buf };
    stage_rows(s->w, s->geo, s->pool.pics[idx], key, bufs, ctu_row0, ctu_rows);
    return 0;
}

int x265hip_cost_stream_pair_open(x265hip_cost_stream* s, int slot, uint64_t fenc_key, uint64_t ref_key, const x265hip_weight* w, unsigned planes_weighted, const uint16_t* mv_cost)
{
    if (!s || slot < 0 || slot >= (int)s->slots.size()) { set_error("cost_stream_pair_open: bad slot"); return X265HIP_EINVAL; }
    unsigned mask = w ? planes_weighted & ((1u << s->geo.nplanes) - 1) : 0;
    for (int c = 0; c < s->geo.nplanes; c++)
        if ((mask & (1u << c)) && !weight_shift_ok(s->prm.depth, w[c].shift))
        { set_error("cost_stream_pair_open: plane %d shift %d (it includes the 14 - depth correction of weight_pp)", c, w[c].shift); return X265HIP_EINVAL; }
    int gen;
    {
        std::lock_guard<std::mutex> lk(s->w.mu);
        CS::Slot& sl = s->slots[slot];
        const bool was = sl.active;
        sl.active = false;                                    // the slot's previous pair no longer holds anything
        const int fenc = cs_picture(s, fenc_key);
        if (fenc >= 0) s->pool.pics[fenc].busy++;                  // not the victim of the next line
        const int ref = fenc < 0 ? -1 : cs_picture(s, ref_key);
        if (fenc >= 0) s->pool.pics[fenc].busy--;
        const int view = ref < 0 ? -1 : cs_find_or_make_view(s, ref, w, mask);
        if (view < 0)
        {
            sl.active = was;
            set_error("cost_stream_pair_open: no %s entry free (pictures = %d, views = %d)", ref < 0 ? "picture" : "view", (int)s->pool.pics.size(), (int)s->views.size());
            return X265HIP_EBUSY;
        }
        if (++sl.generation <= 0) sl.generation = 1;
        for (int r = 0; r < s->geo.ctuRows; r++) sl.ready[r].store(0, std::memory_order_release);      // before anything is rewritten
        sl.fenc = fenc; sl.fencEpoch = s->pool.pics[fenc].epoch; sl.view = view; sl.viewStamp = s->views[view].stamp;
        sl.nextRow = 0; sl.active = true; sl.bandLimit = 1;
        sl.hasCost = mv_cost != nullptr;
        if (mv_cost) memcpy(sl.hMvCost, mv_cost, (2 * (size_t)s->prm.window + 1) * sizeof(uint16_t));
        gen = sl.generation;
        s->pairsOpened++;
        s->w.dirty = true;
    }
    s->w.cv.notify_one();
    return gen;
}

const void* x265hip_cost_stream_tables(x265hip_cost_stream* s, int slot) { return (s && slot >= 0 && slot < (int)s->slots.size()) ? s->slots[slot].tables : nullptr; }

const volatile int* x265hip_cost_stream_ready(x265hip_cost_stream* s, int slot)
{
    return (s && slot >= 0 && slot < (int)s->slots.size()) ? reinterpret_cast<const volatile int*>(s->slots[slot].ready) : nullptr;
}

int x265hip_cost_stream_stats(x265hip_cost_stream* s, x265hip_cost_stream_stats_t* st)
{
    if (!s || !st) { set_error("cost_stream_stats: NULL"); return X265HIP_EINVAL; }
    st->pairs_opened = s->pairsOpened; st->pairs_completed = s->pairsCompleted; st->bands = s->bands; st->rows_served = s->rowsServed; st->rows_uploaded = s->rowsUploaded;
    st->failed = s->failed; st->stale_pairs = s->stalePairs; st->views_opened = s->viewsOpened; st->views_shared = s->viewsShared; st->lines_weighted = s->linesWeighted;
    st->us_busy = s->w.usBusy; st->bytes_downloaded = s->bytesDown; st->bytes_uploaded = s->bytesUp; st->table_bytes = s->rowBytes * s->geo.ctuRows;
    if (s->failed) set_error("cost_stream worker: %s", s->w.error);
    return 0;
}

} // extern "C"
