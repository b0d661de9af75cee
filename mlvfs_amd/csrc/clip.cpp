// clip.cpp -- per-clip state and its part of the device-resident C API (PART 2 of
// include/mlvfs_amd.h): pixel-map dependency analysis, stripe-coefficient
// computation around the histogram kernels.  The fused pass over a clip's frames: fused_pass.cpp.
#include "fused_pass.h"
#include <memory>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

namespace mlv {

// ------------------------------------------------------------------ stripes solve
int stripes_solve(const int32_t *hist, const int32_t num[8], int frame_size, int32_t coeffs[8])
{
    for (int j = 0; j < 8; j++) {                                   // stripes.c:218-234
        if (num[j] < frame_size / 128) continue;
        int t = 0;
        for (int k = 0; k < 65536; k++) {
            t += hist[j * 65536 + k];
            if (t >= num[j] / 2) {
                coeffs[j] = (int32_t)(pow(2.0, (double)(k - 32768) / 32768) * 65536);
                break;
            }
        }
    }
    coeffs[0] = coeffs[1] = 65536;
    int needed = 0;
    for (int j = 0; j < 8; j++) {
        const double c = (double)coeffs[j] / 65536;
        if (c < 0.998 || c > 1.002) needed = 1;
    }
    return needed;
}

// ------------------------------------------------------------------ pixel map
static int entry_kind(int x, int y, int w, int h, int rules, int dual_iso)
{
    if (x > 2 && x < w - 3 && y > 2 && y < h - 3) return dual_iso ? 2 : 1;      // cs.c:320-329 / 468-478
    if (rules == 0) return 0;
    const long long i = x + (long long)y * w;
    if (!(i > 0 && i < (long long)w * h)) return 0;                              // cs.c:479
    const bool h_edge = (x >= w - 3 && x < w) || (x >= 0 && x <= 3);
    const bool v_edge = (y >= h - 3 && y < h) || (y >= 0 && y <= 3);
    if (h_edge && !v_edge && !dual_iso) return 3;
    if (v_edge && !h_edge) return 2;
    if (x >= 0 && x <= 3) return 4;
    if (x >= w - 3 && x < w) return 5;
    return 0;
}

static void taps_of_kind(int kind, bool (&used)[12])
{
    for (int t = 0; t < 12; t++) used[t] = false;
    if (kind == 1) for (int t = 0; t < 12; t++) used[t] = true;
    if (kind == 2) for (int t = 0; t < 6; t++) used[t] = true;
    if (kind == 3) for (int t = 6; t < 12; t++) used[t] = true;
    if (kind == 4) used[4] = true;
    if (kind == 5) used[1] = true;
}

static int tap_offset_host(int t, int w)
{
    const int d = (t % 6) < 3 ? (t % 6) - 3 : (t % 6) - 2;
    return t < 6 ? d : d * w;
}

int Clip::set_pixel_map(const int32_t *xy_in, size_t count, int rules_in, int dual_iso_in)
{
    std::lock_guard<std::mutex> lk(mu);
    xy.assign(xy_in, xy_in + 2 * count);
    rules = rules_in;
    dual_iso = dual_iso_in;
    n_entries = 0;
    n_levels = 0;
    n_level0 = 0;
    n_rec[0] = n_rec[1] = 0;
    if (count == 0) return MLVFS_AMD_OK;

    const int w = g.w, h = g.h;
    const int crop_x = (pan_x + 7) & ~7, crop_y = pan_y & ~1;                   // cs.c:224-225
    std::vector<PixEntry> ent(count);
    std::vector<int> level(count, 0);
    // position -> latest earlier entry: a plain array over the frame (a focus-pixel map has 150 000 entries with twelve taps each;
    // as a hash map this loop and the one over the cells below were 10 of the 28 ms of a map's first use)
    // (a bad-pixel map of a few hundred entries keeps the hash map: clearing an array of the frame's size would cost more than it saves)
    const long long npos = (long long)w * h;
    const bool dense = count >= 8192 && npos <= (1ll << 28);
    std::vector<int> last_dense(dense ? (size_t)npos : 0, -1);
    std::unordered_map<long long, int> last_sparse;
    if (!dense) last_sparse.reserve(count * 2);
    auto last_at = [&](long long at) -> int {
        if (at < 0 || at >= npos) return -1;
        if (dense) return last_dense[(size_t)at];
        auto it = last_sparse.find(at);
        return it == last_sparse.end() ? -1 : it->second;
    };
    int max_level = 0;
    for (size_t m = 0; m < count; m++) {
        const int x = xy[2 * m] - crop_x, y = xy[2 * m + 1] - crop_y;
        PixEntry &e = ent[m];
        e.kind = entry_kind(x, y, w, h, rules, dual_iso);
        e.pos = (e.kind != 0) ? x + y * w : -1;
        e.emit = 0;
        for (int t = 0; t < 12; t++) e.dep[t] = -1;
        if (e.kind == 0) continue;
        bool used[12];
        taps_of_kind(e.kind, used);
        int lv = 0;
        for (int t = 0; t < 12; t++) {
            if (!used[t]) continue;
            const long long at = (long long)e.pos + tap_offset_host(t, w);
            const int d = last_at(at);
            if (d >= 0) {
                e.dep[t] = d;
                lv = std::max(lv, level[d] + 1);
            }
        }
        level[m] = lv;
        max_level = std::max(max_level, lv);
        if (dense) last_dense[(size_t)e.pos] = (int)m; else last_sparse[e.pos] = (int)m;
    }
    for (size_t m = 0; m < count; m++)
        if (ent[m].kind != 0 && last_at(ent[m].pos) == (int)m) ent[m].emit = 1;          // the last writer of a position wins

    // stable order by level; remap dependency indices
    std::vector<int> order(count), where(count);
    for (size_t m = 0; m < count; m++) order[m] = (int)m;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return level[a] < level[b]; });
    for (size_t k = 0; k < count; k++) where[order[k]] = (int)k;
    std::vector<PixEntry> sorted(count);
    std::vector<int> off(max_level + 2, 0);
    for (size_t k = 0; k < count; k++) {
        sorted[k] = ent[order[k]];
        for (int t = 0; t < 12; t++)
            if (sorted[k].dep[t] >= 0) sorted[k].dep[t] = where[sorted[k].dep[t]];
        off[level[order[k]] + 1]++;
    }
    for (int l = 0; l <= max_level; l++) off[l + 1] += off[l];

    // per-tile lists for the fused kernel, one set per tile geometry: the cells that hold repaired pixels (the entries that
    // are the last writers of their positions), each listed in every tile whose plane rectangle (tile + 2-cell halo) contains it
    std::vector<CellRec> cell_list;
    {
        const int cw = (w >> 1) + 1;
        std::vector<int> cell_dense(dense ? (size_t)cw * ((h >> 1) + 1) : 0, -1);
        std::unordered_map<int, int> cell_sparse;
        if (!dense) cell_sparse.reserve(count * 2);
        for (size_t k = 0; k < count; k++) {
            const PixEntry &e = sorted[k];
            if (e.kind == 0 || !e.emit) continue;
            const int x = e.pos % w, y = e.pos / w;
            const int key = (x >> 1) | ((y >> 1) << 16);
            int slot;
            if (dense) {
                int &sd = cell_dense[(size_t)(y >> 1) * cw + (x >> 1)];
                if (sd < 0) { sd = (int)cell_list.size(); cell_list.push_back(CellRec{ key, { -1, -1, -1, -1 } }); }
                slot = sd;
            } else {
                auto it = cell_sparse.find(key);
                if (it == cell_sparse.end()) { it = cell_sparse.emplace(key, (int)cell_list.size()).first; cell_list.push_back(CellRec{ key, { -1, -1, -1, -1 } }); }
                slot = it->second;
            }
            cell_list[slot].e[(x & 1) + 2 * (y & 1)] = (int)k;
        }
    }
    std::vector<int> tile_off[FRAME_GEOS];
    std::vector<CellRec> tile_rec[FRAME_GEOS];
    for (int geo = 0; geo < FRAME_GEOS; geo++) {
        const int tch = frame_tile_rows(geo);
        const int tx_n = frame_tiles_x(w), ty_n = frame_tiles_y(h, geo);
        std::vector<std::vector<int>> per_tile((size_t)tx_n * ty_n);
        for (size_t k = 0; k < cell_list.size(); k++) {
            const int cx = cell_list[k].cell & 0xFFFF, cy = cell_list[k].cell >> 16;
            // (only the tiles around the cell are looked at: a focus-pixel map has tens of thousands of entries)
            for (int ty = std::max(0, (cy - FRAME_HC) / tch - 1); ty < std::min(ty_n, (cy + FRAME_HC) / tch + 1); ty++) {
                if (cy < ty * tch - FRAME_HC || cy >= (ty + 1) * tch + FRAME_HC) continue;
                for (int tx = std::max(0, (cx - FRAME_HC) / FRAME_TCW - 1); tx < std::min(tx_n, (cx + FRAME_HC) / FRAME_TCW + 1); tx++) {
                    if (cx < tx * FRAME_TCW - FRAME_HC || cx >= (tx + 1) * FRAME_TCW + FRAME_HC) continue;
                    per_tile[(size_t)ty * tx_n + tx].push_back((int)k);
                }
            }
        }
        tile_off[geo].assign(per_tile.size() + 1, 0);
        for (size_t i = 0; i < per_tile.size(); i++) {
            tile_off[geo][i + 1] = tile_off[geo][i] + (int)per_tile[i].size();
            for (int k : per_tile[i]) tile_rec[geo].push_back(cell_list[k]);
        }
        n_rec[geo] = (int)tile_rec[geo].size();
        if (tile_rec[geo].empty()) tile_rec[geo].push_back(CellRec{ 0, { -1, -1, -1, -1 } });
    }

    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    for (int geo = 0; geo < FRAME_GEOS; geo++) {
        if (const int rc = d_tile_off[geo].reserve(sizeof(int) * tile_off[geo].size())) return rc;
        if (const int rc = d_tile_rec[geo].reserve(sizeof(CellRec) * tile_rec[geo].size())) return rc;
        MLV_HIP(hipMemcpy(d_tile_off[geo], tile_off[geo].data(), sizeof(int) * tile_off[geo].size(), hipMemcpyHostToDevice));
        MLV_HIP(hipMemcpy(d_tile_rec[geo], tile_rec[geo].data(), sizeof(CellRec) * tile_rec[geo].size(), hipMemcpyHostToDevice));
    }
    // behind the entries: {pos, kind | emit << 8} per entry -- all the dependency-free level needs of one (k_pixfix_flat reads 8
    // bytes per entry instead of 60: a focus-pixel map has 150 000 of them)
    std::vector<int2> compact(count);
    for (size_t k = 0; k < count; k++) compact[k] = make_int2(sorted[k].pos, sorted[k].kind | (sorted[k].emit << 8));
    if (const int rc = d_entries.reserve((sizeof(PixEntry) + sizeof(int2)) * count)) return rc;
    if (const int rc = d_level_off.reserve(sizeof(int) * off.size())) return rc;
    MLV_HIP(hipMemcpy(d_entries, sorted.data(), sizeof(PixEntry) * count, hipMemcpyHostToDevice));
    MLV_HIP(hipMemcpy((uint8_t *)d_entries + sizeof(PixEntry) * count, compact.data(), sizeof(int2) * count, hipMemcpyHostToDevice));
    MLV_HIP(hipMemcpy(d_level_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice));
    n_entries = (int)count;
    n_levels = max_level + 1;
    n_level0 = off[1];
    return MLVFS_AMD_OK;
}

// ------------------------------------------------------------------ detection
int Clip::detect_bad_pixels(const void *d_frame, int aggressive, int dual_iso_in, hipStream_t stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    const int w = g.w, h = g.h;
    const int wpr = (w + 63) / 64;
    const int crop_x = (pan_x + 7) & ~7, crop_y = pan_y & ~1;
    int cap = 1 << 16;
    std::vector<int32_t> host_list;
    for (;;) {
        const size_t mask_b = (size_t)h * wpr * 8, cnt_b = ((size_t)h * 4 + 15) / 16 * 16, list_b = (size_t)cap * 8;
        int rc = d_scratch.reserve(mask_b + cnt_b + list_b);
        if (rc) return rc;
        uint8_t *base = (uint8_t *)d_scratch;
        int *d_cnt = (int *)(base + mask_b);
        void *d_list = base + mask_b + cnt_b;
        rc = launch_badpix_detect(d_frame, w, h, g.black, aggressive, crop_x, crop_y, base, wpr, d_cnt, d_list, cap,
                                  c->dev->luts, stream);
        if (rc) return rc;
        std::vector<int> cnt(h);
        MLV_HIP(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * h, hipMemcpyDeviceToHost, stream));
        MLV_HIP(hipStreamSynchronize(stream));
        long long total = 0;
        for (int v : cnt) total += v;
        if (total > cap) { cap = (int)total; continue; }
        host_list.resize(2 * (size_t)total);
        if (total) {
            MLV_HIP(hipMemcpyAsync(host_list.data(), d_list, (size_t)total * 8, hipMemcpyDeviceToHost, stream));
            MLV_HIP(hipStreamSynchronize(stream));
        }
        break;
    }
    return set_pixel_map(host_list.data(), host_list.size() / 2, 0, dual_iso_in);
}

int Clip::fix_pixels(void *d_frames, size_t stride, int nframes, hipStream_t stream)
{
    if (n_entries == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    int rc = d_patches.reserve(patch_buffer_bytes(nframes));
    if (rc) return rc;
    return launch_pixfix(false, d_frames, stride, g.w, g.black, d_entries, d_level_off, n_levels, n_level0, n_entries, d_patches,
                         d_frames, stride, nframes, c->dev->luts, stream);
}

int Clip::fix_pixels_shared(void *d_frame, size_t stride, int black, ThreadCtx *c) const
{
    if (n_entries == 0) return MLVFS_AMD_OK;
    int rc = c->ensure_patch((size_t)n_entries * sizeof(int2));
    if (rc) return rc;
    return launch_pixfix(false, d_frame, stride, g.w, black, d_entries, d_level_off, n_levels, n_level0, n_entries, c->d_patch,
                         d_frame, stride, 1, c->dev->luts, c->stream);
}

// ------------------------------------------------------------------ stripes
struct RecheckHost { int hist, a, b, r1, r2; };

int Clip::stripes_compute(const void *d_frame, int frame_size, int rand_mode, hipStream_t stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    StripesWork wk;
    int rc = wk.init(this, g, 0, g.h);
    if (rc) return rc;
    long long accepted = 0;
    rc = wk.count(d_frame, &accepted, stream);
    if (rc) return rc;

    // the dither stream: two values per accepted call, in raster order
    const size_t n_rnd = (size_t)(2 * accepted) + 2;
    DevBuf d_rand;
    if ((rc = d_rand.reserve(n_rnd * 2 + 16))) return rc;
    RandState app, app_after;
    // one clip at a time takes values from the application's generator: a second thread that read the state before the first has
    // put it back would draw the SAME values (with rand() itself the calls of two threads interleave, they never repeat)
    static std::mutex app_stream_mu;
    std::unique_lock<std::mutex> app_stream_lk(app_stream_mu, std::defer_lock);
    if (rand_mode == 0) app_stream_lk.lock();
    bool bulk = false;
    if (rand_mode == 0 && LibcRandGuard::take_app_state(app.x)) {
        // The process-global libc stream (drop-in path).  Calling rand() once per value -- 9.4 M calls for a 3584x1320 frame, each
        // behind glibc's lock -- took 300 ms of this function's 305 (the reference's whole stripes_compute_correction: 360 ms).  The
        // application's generator is parked while the library runs (LibcRandGuard), its buffer is glibc's documented TYPE_3 state:
        // the values come from the device generator started at THAT state, and the state as it is after them goes back into the
        // buffer -- the application's next rand() is the same as after the reference's calls (tests/test_gpu_parity.py:
        // test_stripes_dropin checks exactly that).  Whatever goes wrong on the way -- the device generator, the state changing
        // hands before it is written back -- leaves the application's stream where it was: the values are then drawn call by call
        // below, as the reference draws them (the reference cannot fail here).
        int rb = rand_stream_device_from(app, (uint16_t *)d_rand, (size_t)(2 * accepted), stream, &app_after);
        if (rb == MLVFS_AMD_OK && hipMemsetAsync((uint16_t *)d_rand + 2 * accepted, 0, 4, stream) != hipSuccess) rb = MLVFS_AMD_ERR_HIP;
        if (rb == MLVFS_AMD_OK && hipStreamSynchronize(stream) != hipSuccess) rb = MLVFS_AMD_ERR_HIP;
        bulk = rb == MLVFS_AMD_OK && LibcRandGuard::put_app_state(app_after.x);
        if (!bulk) (void)hipGetLastError();
    }
    if (rand_mode == 0 && !bulk) {
        // another generator type (the application called initstate() with a size of its own), or the bulk path gave up: drawn on the
        // host, call by call (not zero-initialised: the generator touches the pages first)
        std::unique_ptr<uint16_t[]> rnd(new uint16_t[n_rnd]);
        rnd[n_rnd - 1] = rnd[n_rnd - 2] = 0;
        LibcRandGuard::draw_mod1024(rnd.get(), 2 * accepted);
        hipError_t e = hipMemcpy(d_rand, rnd.get(), n_rnd * 2, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("rand upload failed"); return MLVFS_AMD_ERR_HIP; }
    } else if (rand_mode == 0) {
        // (the bulk path's values are in place)
    } else {
        // a fresh process's stream (seed 1), generated where it is consumed
        rc = rand_stream_device((uint16_t *)d_rand, (size_t)(2 * accepted), 0, 1, stream);
        if (rc == MLVFS_AMD_OK && hipMemsetAsync((uint16_t *)d_rand + 2 * accepted, 0, 4, stream) != hipSuccess) rc = MLVFS_AMD_ERR_HIP;
        if (rc) return rc;
    }

    if (app_stream_lk.owns_lock()) app_stream_lk.unlock();
    std::vector<int32_t> hist(8 * 65536);
    int32_t num[8];
    rc = wk.hist_to_host(d_frame, d_rand, 2 * accepted, hist.data(), num, stream);
    d_rand.release();
    if (rc) return rc;

    std::lock_guard<std::mutex> lk(mu);
    needed = stripes_solve(hist.data(), num, frame_size, coef);
    return MLVFS_AMD_OK;
}

// scratch layout for one shard of rows
int StripesWork::init(Clip *owner_, const Geom &g_, int row0_, int row1_)
{
    owner = owner_; g = g_; row0 = row0_; row1 = row1_;
    gpr = stripes_groups_per_row(g.w);
    n_groups = gpr * (row1 - row0);
    nblk = (n_groups + 255) / 256;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    o_counts = 0;
    o_bsum = o_counts + up((size_t)std::max(n_groups, 1));
    o_boff = o_bsum + up(sizeof(int) * (size_t)std::max(nblk, 1));
    o_total = o_boff + up(sizeof(long long) * (size_t)std::max(nblk, 1));
    o_hist = o_total + 256;
    o_num = o_hist + (size_t)8 * 65536 * 4;
    o_nre = o_num + 256;
    o_re = o_nre + 256;
    o_copies = (o_re + sizeof(RecheckHost) * RECHECK_CAP + 255) / 256 * 256;
    bytes = o_copies + stripes_hist_copies_bytes();
    int rc = owner->d_scratch.reserve(bytes);
    if (rc) return rc;
    base = (uint8_t *)owner->d_scratch;
    return MLVFS_AMD_OK;
}

int StripesWork::count(const void *d_frame, long long *accepted, hipStream_t stream)
{
    int rc = launch_stripes_count(d_frame, g.w, row0, row1, g.black, g.white, base + o_counts, (int *)(base + o_bsum),
                                  (long long *)(base + o_boff), (long long *)(base + o_total), stream);
    if (rc) return rc;
    MLV_HIP(hipMemcpyAsync(accepted, base + o_total, sizeof(long long), hipMemcpyDeviceToHost, stream));
    MLV_HIP(hipStreamSynchronize(stream));
    return MLVFS_AMD_OK;
}

int StripesWork::hist_dev(const void *d_frame, const void *d_rand, long long n_rand, int *d_hist, int *d_num,
                          hipStream_t stream)
{
    MLV_HIP(hipMemsetAsync(base + o_nre, 0, 4, stream));
    return launch_stripes_hist(d_frame, g.w, row0, row1, g.black, g.white, base + o_counts, (long long *)(base + o_boff),
                               d_rand, n_rand, d_hist, d_num, base + o_re, RECHECK_CAP, (int *)(base + o_nre), base + o_copies, stream);
}

// bins the samples the device refused to bin (too close to a bin edge for its log2)
int StripesWork::recheck_into(int32_t *hist_host_or_null, int *d_hist, hipStream_t stream)
{
    int n_re = 0;
    MLV_HIP(hipMemcpyAsync(&n_re, base + o_nre, 4, hipMemcpyDeviceToHost, stream));
    MLV_HIP(hipStreamSynchronize(stream));
    if (n_re > RECHECK_CAP) { set_error("stripes: %d samples need host re-binning (cap %d)", n_re, RECHECK_CAP); return MLVFS_AMD_ERR_ARG; }
    if (n_re == 0) return MLVFS_AMD_OK;
    std::vector<RecheckHost> re(n_re);
    MLV_HIP(hipMemcpy(re.data(), base + o_re, sizeof(RecheckHost) * n_re, hipMemcpyDeviceToHost));
    std::vector<int> idx(n_re);
    for (int i = 0; i < n_re; i++) {
        const double af = re[i].a + re[i].r1 / 1024.0 - 0.5, bf = re[i].b + re[i].r2 / 1024.0 - 0.5;
        const double ev = log2(af / bf);
        int bin = (int)(65536 / 2 + ev * 65536 / 2);
        bin = bin < 0 ? 0 : (bin > 65535 ? 65535 : bin);
        idx[i] = re[i].hist * 65536 + bin;
    }
    if (hist_host_or_null) {
        for (int i : idx) hist_host_or_null[i]++;
    } else {
        // device histogram (multi-GPU path): the bins go back in one copy (into the recheck buffer, which has been read) and
        // one small kernel adds them -- a few hundred samples; one pair of 4-byte copies per sample cost 5 ms per clip
        MLV_HIP(hipMemcpyAsync(base + o_re, idx.data(), sizeof(int) * n_re, hipMemcpyHostToDevice, stream));
        int rc = launch_hist_bump(d_hist, (const int *)(base + o_re), n_re, stream);
        if (rc) return rc;
        MLV_HIP(hipStreamSynchronize(stream));                   // idx is a local
    }
    return MLVFS_AMD_OK;
}

int StripesWork::hist_to_host(const void *d_frame, const void *d_rand, long long n_rand, int32_t *hist, int32_t num[8],
                              hipStream_t stream)
{
    int *d_hist = (int *)(base + o_hist), *d_num = (int *)(base + o_num);
    MLV_HIP(hipMemsetAsync(d_hist, 0, (size_t)8 * 65536 * 4, stream));
    MLV_HIP(hipMemsetAsync(d_num, 0, 32, stream));
    int rc = hist_dev(d_frame, d_rand, n_rand, d_hist, d_num, stream);
    if (rc) return rc;
    MLV_HIP(hipMemcpyAsync(hist, d_hist, (size_t)8 * 65536 * 4, hipMemcpyDeviceToHost, stream));
    MLV_HIP(hipMemcpyAsync(num, d_num, 32, hipMemcpyDeviceToHost, stream));
    MLV_HIP(hipStreamSynchronize(stream));
    return recheck_into(hist, nullptr, stream);
}

}  // namespace mlv

// ==================================================================== C ABI
using namespace mlv;

extern "C" {

mlvfs_amd_clip_t *mlvfs_amd_clip_create(const mlvfs_amd_geom_t *geom)
{
    if (!geom || geom->width <= 0 || geom->height <= 0) { set_error("clip_create: bad geometry"); return nullptr; }
    ThreadCtx *c = thread_ctx();
    if (!c) return nullptr;
    Clip *clip = new Clip;
    clip->g = Geom{ geom->width, geom->height, geom->bpp, geom->black, geom->white };
    clip->pan_x = geom->pan_x;
    clip->pan_y = geom->pan_y;
    clip->device = c->dev->id;
    return reinterpret_cast<mlvfs_amd_clip_t *>(clip);
}

void mlvfs_amd_clip_destroy(mlvfs_amd_clip_t *clip) { delete reinterpret_cast<Clip *>(clip); }

int mlvfs_amd_clip_set_stripes(mlvfs_amd_clip_t *clip_, int needed, const int32_t coeffs[8])
{
    Clip *clip = reinterpret_cast<Clip *>(clip_);
    std::lock_guard<std::mutex> lk(clip->mu);
    clip->needed = needed;
    memcpy(clip->coef, coeffs, sizeof clip->coef);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_clip_get_stripes(const mlvfs_amd_clip_t *clip_, int *needed, int32_t coeffs[8])
{
    const Clip *clip = reinterpret_cast<const Clip *>(clip_);
    if (needed) *needed = clip->needed;
    if (coeffs) memcpy(coeffs, clip->coef, sizeof clip->coef);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_clip_set_pixel_map(mlvfs_amd_clip_t *clip, const int32_t *xy, size_t count, int kind, int dual_iso)
{
    return reinterpret_cast<Clip *>(clip)->set_pixel_map(xy, count, kind, dual_iso);
}

size_t mlvfs_amd_clip_get_pixel_map(const mlvfs_amd_clip_t *clip_, int32_t *xy, size_t cap)
{
    const Clip *clip = reinterpret_cast<const Clip *>(clip_);
    const size_t n = clip->xy.size() / 2;
    if (xy) memcpy(xy, clip->xy.data(), std::min(n, cap) * 8);
    return n;
}

static Geom to_geom(const mlvfs_amd_geom_t *g) { return Geom{ g->width, g->height, g->bpp, g->black, g->white }; }

int mlvfs_amd_unpack_dev(const mlvfs_amd_geom_t *geom, const void *d_packed, size_t packed_stride, void *d_out,
                         size_t out_stride, int nframes, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return launch_unpack(d_packed, packed_stride, d_out, out_stride, 0, (uint32_t)geom->width * geom->height, geom->bpp,
                         nframes, pick_stream(stream, c));
}

int mlvfs_amd_chroma_smooth_dev(const mlvfs_amd_geom_t *geom, const void *d_in, void *d_out, size_t stride, int method,
                                int nframes, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    if (method != 2 && method != 3 && method != 5) { set_error("Unsupported chroma smooth method"); return MLVFS_AMD_ERR_ARG; }
    if (black_too_large(geom->black)) { set_error("Black level too large for processing"); return MLVFS_AMD_ERR_ARG; }
    return launch_frame(c->dev, to_geom(geom), false, d_in, stride, d_out, stride, nframes, method, nullptr, false,
                        nullptr, pick_stream(stream, c));
}

int mlvfs_amd_detect_bad_pixels_dev(mlvfs_amd_clip_t *clip, const void *d_frame, int aggressive, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return reinterpret_cast<Clip *>(clip)->detect_bad_pixels(d_frame, aggressive, 0, pick_stream(stream, c));
}

int mlvfs_amd_fix_pixels_dev(mlvfs_amd_clip_t *clip, void *d_frames, size_t stride, int nframes, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return reinterpret_cast<Clip *>(clip)->fix_pixels(d_frames, stride, nframes, pick_stream(stream, c));
}

// The shard entry points share one scratch area per calling thread.
static thread_local Clip *t_shard_scratch = nullptr;
static thread_local StripesWork t_work;

int mlvfs_amd_stripes_count_dev(const mlvfs_amd_geom_t *geom, const void *d_frame, int row0, int row1, int64_t *accepted,
                                void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    if (row0 < 0 || row1 > geom->height || row0 > row1) { set_error("stripes shard rows out of range"); return MLVFS_AMD_ERR_ARG; }
    if (!t_shard_scratch) t_shard_scratch = new Clip;
    int rc = t_work.init(t_shard_scratch, to_geom(geom), row0, row1);
    if (rc) return rc;
    long long acc = 0;
    rc = t_work.count(d_frame, &acc, pick_stream(stream, c));
    *accepted = acc;
    return rc;
}

int mlvfs_amd_stripes_hist_dev(const mlvfs_amd_geom_t *geom, const void *d_frame, int row0, int row1, const void *d_rand,
                               int64_t n_rand, void *d_hist, void *d_num, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    if (!t_shard_scratch || t_work.row0 != row0 || t_work.row1 != row1 || t_work.g.w != geom->width) {
        set_error("stripes_hist_dev must follow stripes_count_dev for the same shard");
        return MLVFS_AMD_ERR_ARG;
    }
    hipStream_t s = pick_stream(stream, c);
    int rc = t_work.hist_dev(d_frame, d_rand, n_rand, (int *)d_hist, (int *)d_num, s);
    if (rc) return rc;
    return t_work.recheck_into(nullptr, (int *)d_hist, s);
}

int mlvfs_amd_stripes_solve(const int32_t *hist, const int32_t num[8], int frame_size, int32_t coeffs[8])
{
    return stripes_solve(hist, num, frame_size, coeffs);
}

int mlvfs_amd_stripes_compute_dev(mlvfs_amd_clip_t *clip, const void *d_frame, int frame_size, int rand_mode, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return reinterpret_cast<Clip *>(clip)->stripes_compute(d_frame, frame_size, rand_mode, pick_stream(stream, c));
}

int mlvfs_amd_stripes_apply_dev(const mlvfs_amd_clip_t *clip_, void *d_frames, size_t stride, int nframes, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    const Clip *clip = reinterpret_cast<const Clip *>(clip_);
    if (!clip->needed) return MLVFS_AMD_OK;                                     // stripes.c:252
    return launch_stripes_apply(d_frames, stride, (size_t)clip->g.w * clip->g.h, clip->g.w, clip->g.black, clip->g.white,
                                clip->coef, nframes, pick_stream(stream, c));
}

int mlvfs_amd_clip_set_t16_layout(mlvfs_amd_clip_t *clip_, int layout)
{
    Clip *clip = reinterpret_cast<Clip *>(clip_);
    if (!clip || layout < 0 || layout > 2) { set_error("clip_set_t16_layout: layout must be 0 (auto), 1 (plain) or 2 (spread)"); return MLVFS_AMD_ERR_ARG; }
    clip->t16_layout = layout;
    return MLVFS_AMD_OK;
}

int mlvfs_amd_clip_get_t16_layout(const mlvfs_amd_clip_t *clip_)
{
    const Clip *clip = reinterpret_cast<const Clip *>(clip_);
    return clip ? clip->t16_layout : 0;
}

}  // extern "C"
