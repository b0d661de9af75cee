// lj92enc.cpp -- host side of lj92_encode (lj92.h:65-68): the Huffman table of the reference's encoder and the call itself.
//
//   table      mlvfs/lj92.c:788-937 (createEncodeTable): code sizes by merging the two rarest of 18 entries in FLOAT frequencies
//              (17 SSSS classes + one reserved entry of frequency 1.0), the value list in order of size, canonical codes
//   header     mlvfs/lj92.c:939-984 (SOI, SOF3, DHT, SOS with predictor 6, EOI)
//   kernels    csrc/k_lj92enc.hip (histogram, bit packing, byte stuffing), every one with the frame as a grid dimension
//   batch      lje_encode_batch: n frames in device memory -> n complete streams in device memory with ONE host round trip (n x 20
//              counters down, n tables with their marker segments up) and one copy of lengths and states.  The mount's lossless
//              .dng files (mount.cpp), mlvfs_amd_lj92_encode_batch_dev and -- as a batch of one -- lj92_encode all go through it.
//              The bits a frame needs are known exactly once its table is (sum of count x (code length + class)): the bit buffer
//              is sized from that, not from 32 bits per pixel.
//
// What the reference's table builder does and a textbook one does not -- all of it kept, the streams are compared byte for byte:
//  * the reserved entry has the LARGEST frequency, so it takes a short code instead of the longest one;
//  * it is counted in BITS but has no value, so the value list is one entry short and its last entry is the zero the list was
//    cleared to: class 0 appears twice in the DHT, and because symbols are assigned walking the list upwards, SSSS = 0 is
//    written with the LAST (longest, all-ones) code;
//  * ties: the first candidate is the last of the rarest entries, the second the first of the remaining rarest.
// Where the reference runs off its arrays the call fails with LJ92_ERROR_CORRUPT instead: a difference that needs 17 bits
// (hist[17], huffsym[17]: 16-bit material only), all 17 classes in use (an 18th code is written behind huffenc[] / huffbits[]),
// a code longer than 16 bits (bits[17+]), a value beyond the delinearisation table, an empty image.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "clip.h"
#include "lj92enc.h"

namespace mlv {

namespace {

struct EncTable {
    int bits[17];              // codes per length (index 0 unused), the reserved entry included
    int values[17];            // DHT value list
    int nvalues;               // = sum of bits[]: one more than the classes in use
    uint8_t len[17];           // per SSSS class: length and code it is written with
    uint16_t code[17];
};

// returns nullptr or why the reference's own procedure leaves its arrays
const char *build_table(const uint32_t hist[17], int width_times_height, EncTable *t)
{
    enum { N = 18, NONE = -1 };
    float f[N];
    int size[N], chain[N];
    const float total = (float)width_times_height;
    int used = 0;
    for (int i = 0; i < 17; i++) { f[i] = (float)(int)hist[i] / total; used += hist[i] != 0; }
    f[17] = 1.0f;
    for (int i = 0; i < N; i++) { size[i] = 0; chain[i] = NONE; }
    if (used == 0) return "no pixels";
    if (used == 17) return "all 17 difference classes in use: the reference writes an 18th code behind its tables";
    for (;;) {
        int a = NONE, b = NONE;
        float fa = 3.0f, fb = 3.0f;
        for (int i = 0; i < N; i++) if (f[i] > 0.0f && f[i] <= fa) { fa = f[i]; a = i; }            // last of the rarest
        for (int i = 0; i < N; i++) if (i != a && f[i] > 0.0f && f[i] < fb) { fb = f[i]; b = i; }    // first of the rest
        if (b == NONE) break;
        f[a] += f[b];
        f[b] = 0.0f;
        // every member of both groups moves one level down; b's group is appended to a's
        int e = a;
        for (;; e = chain[e]) { size[e]++; if (chain[e] == NONE) break; }
        chain[e] = b;
        for (e = b; e != NONE; e = chain[e]) size[e]++;
    }
    memset(t, 0, sizeof *t);
    for (int i = 0; i < N; i++) {
        if (size[i] > 16) return "a Huffman code longer than 16 bits";
        if (size[i]) { t->bits[size[i]]++; t->nvalues++; }
    }
    int k = 0;
    for (int l = 1; l <= 16; l++)
        for (int j = 0; j < 17; j++) if (size[j] == l) t->values[k++] = j;
    // canonical codes in list order; list position -> class; the walk upwards lets the list's cleared last entry (class 0) win
    int lens[18], codes[18], n = 0;
    unsigned next = 0;
    for (int l = 1; l <= 16; l++) {
        for (int j = 0; j < t->bits[l]; j++) { lens[n] = l; codes[n] = (int)next++; n++; }
        next <<= 1;
    }
    int at[17] = { 0 };
    for (int i = 0; i < n && i < 17; i++) at[t->values[i]] = i;
    for (int s = 0; s < 17; s++) { t->len[s] = (uint8_t)lens[at[s]]; t->code[s] = (uint16_t)codes[at[s]]; }
    return nullptr;
}

int write_header(uint8_t *e, int width, int height, int bitdepth, const EncTable &t)
{
    int w = 0;
    auto put = [&](int v) { e[w++] = (uint8_t)v; };
    put(0xFF); put(0xD8);
    put(0xFF); put(0xC3); put(0); put(11); put(bitdepth); put(height >> 8); put(height); put(width >> 8); put(width); put(1); put(0); put(0x11); put(0);
    put(0xFF); put(0xC4); put(0); put(17 + 2 + t.nvalues); put(0);
    for (int l = 1; l <= 16; l++) put(t.bits[l]);
    for (int i = 0; i < t.nvalues; i++) put(t.values[i]);
    put(0xFF); put(0xDA); put(0); put(8); put(1); put(0); put(0); put(6); put(0); put(0);
    return w;
}

enum { LJ92_OK = 0, LJ92_CORRUPT = -1, LJ92_NO_MEMORY = -2 };      // lj92.h:29-35

struct FixedLayout {
    size_t src_at, hist_at, blockhist_at, off_at, ffoff_at, tabs_at, res_at, bytes;
    FixedLayout(uint32_t npix, int n)
    {
        const size_t nb = lje_blocks(npix);
        size_t a = 0;
        src_at = a; a += up256(sizeof(void *) * n);
        hist_at = a; a += up256(sizeof(uint32_t) * LJE_HIST * n);
        blockhist_at = a; a += up256(sizeof(uint32_t) * 17 * nb * n);
        off_at = a; a += up256(sizeof(uint32_t) * (nb + 1) * n);
        ffoff_at = a; a += up256(sizeof(uint32_t) * (nb + 1) * n);
        tabs_at = a; a += up256(sizeof(LjeFrame) * n);
        res_at = a; a += up256(sizeof(LjeOut) * n);
        bytes = a;
    }
};

}  // namespace

size_t lje_fixed_bytes(uint32_t npix, int nframes) { return FixedLayout(npix, nframes).bytes; }

int lje_encode_batch(const uint16_t *const *h_src, int n, int width, int height, int bitdepth, const uint16_t *d_delin, int delin_len,
                     void *d_fixed, LjeRoom &room, uint8_t **d_out_used, size_t *out_stride_used, LjeResult *res, hipStream_t s)
{
    const uint32_t npix = (uint32_t)((uint64_t)width * height);
    const FixedLayout L(npix, n);
    uint8_t *A = (uint8_t *)d_fixed;
    const uint16_t *const *d_src = (const uint16_t *const *)(A + L.src_at);
    uint32_t *d_hist = (uint32_t *)(A + L.hist_at);
    MLV_HIP(hipMemcpyAsync(A + L.src_at, h_src, sizeof(void *) * n, hipMemcpyHostToDevice, s));
    MLV_HIP(hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * LJE_HIST * n, s));
    int rc = lje_launch_hist(d_src, d_delin, delin_len, width, npix, bitdepth, n, d_hist, (uint32_t *)(A + L.blockhist_at), s);
    if (rc) return rc;
    // ---- the one round trip: the batch's histograms down, its tables, marker segments and bit offsets up
    std::vector<uint32_t> hist((size_t)LJE_HIST * n);
    MLV_HIP(hipMemcpyAsync(hist.data(), d_hist, sizeof(uint32_t) * hist.size(), hipMemcpyDeviceToHost, s));
    MLV_HIP(hipStreamSynchronize(s));
    std::vector<LjeFrame> tabs(n);
    size_t bits_dwords = 0, worst_stream = 0;
    int good = 0;
    for (int f = 0; f < n; f++) {
        const uint32_t *h = &hist[(size_t)LJE_HIST * f];
        LjeFrame &t = tabs[f];
        memset(&t, 0, sizeof t);
        LjeResult &r = res[f];
        r = LjeResult();
        for (int c = 0; c < 18; c++) if (h[c]) r.max_class = c;
        EncTable et;
        uint64_t total = 0;
        if (h[18]) r.status = LJE_DELIN;
        else if (h[17]) r.status = LJE_DIFF17;
        else if ((r.why = build_table(h, (int)npix, &et))) r.status = LJE_TABLE;
        else {
            for (int c = 0; c < 17; c++) total += (uint64_t)h[c] * (et.len[c] + c);
            if (total >= 0xFFF00000ull) { r.status = LJE_TABLE; r.why = "a stream of 2^32 bits or more"; }
        }
        t.status = (uint32_t)r.status;
        if (r.status != LJE_OK) continue;
        for (int c = 0; c < 17; c++) { t.len[c] = et.len[c]; t.code[c] = et.code[c]; }
        t.head_len = (uint8_t)write_header(t.head, width, height, bitdepth, et);
        t.bits_at = (uint32_t)bits_dwords;
        bits_dwords += ((size_t)(total >> 5) + 1 + 63) / 64 * 64;             // whole 256-byte lines per frame
        worst_stream = std::max(worst_stream, (size_t)t.head_len + 2 * (size_t)((total + 7) >> 3) + 2);
        good++;
    }
    if (bits_dwords >= 0xFFFFFFFFull) { set_error("lj92 encoder: a batch of more than 2^32 dwords of bits"); return MLVFS_AMD_ERR_ARG; }
    if (good) {
        void *d_bits = nullptr;
        rc = room.get(bits_dwords * 4, (worst_stream + 3) / 4 * 4, &d_bits, d_out_used, out_stride_used);
        if (rc) return rc;
        LjeFrame *d_tabs = (LjeFrame *)(A + L.tabs_at);
        LjeOut *d_res = (LjeOut *)(A + L.res_at);
        MLV_HIP(hipMemcpyAsync(d_tabs, tabs.data(), sizeof(LjeFrame) * n, hipMemcpyHostToDevice, s));
        rc = lje_launch_pack(d_src, d_delin, delin_len, width, npix, bitdepth, n, d_tabs, (const uint32_t *)(A + L.blockhist_at),
                             (uint32_t *)(A + L.off_at), (uint32_t *)(A + L.ffoff_at), (uint32_t *)d_bits, *d_out_used, *out_stride_used, d_res, s);
        if (rc) return rc;
        std::vector<LjeOut> out(n);
        MLV_HIP(hipMemcpyAsync(out.data(), d_res, sizeof(LjeOut) * n, hipMemcpyDeviceToHost, s));
        MLV_HIP(hipStreamSynchronize(s));
        for (int f = 0; f < n; f++) {
            if (res[f].status != LJE_OK) continue;
            res[f].status = (int)out[f].status;
            res[f].length = out[f].length;
        }
    }
    return MLVFS_AMD_OK;
}

}  // namespace mlv

using namespace mlv;

namespace {

// the thread's scratch: d_a holds the caller's part and the fixed scratch, d_b the bit streams and (drop-in) the stream
struct ThreadRoom : LjeRoom {
    ThreadCtx *c;
    bool own_out;
    ThreadRoom(ThreadCtx *c_, bool own_out_) : c(c_), own_out(own_out_) {}
    int get(size_t bits_bytes, size_t stream_bytes, void **d_bits, uint8_t **d_out, size_t *out_stride) override
    {
        const size_t bits = up256(bits_bytes);
        if (c->ensure(c->d_a.bytes, bits + (own_out ? stream_bytes : 0))) return MLVFS_AMD_ERR_NOMEM;
        *d_bits = c->d_b;
        if (own_out) { *d_out = (uint8_t *)c->d_b + bits; *out_stride = stream_bytes; }
        return MLVFS_AMD_OK;
    }
};

}  // namespace

extern "C" {

// test hook (host only; tests/test_lj92_encode.py, hostcheck): the table the encoder would write for a histogram.
// out = bits[1..16], nvalues, values[17], len[17], code[17] as ints (68 of them).  Returns 0, or -1 with the error string set.
int mlvfs_amd_lj92_encode_table(const uint32_t hist[17], int npix, int *out)
{
    EncTable t;
    const char *why = build_table(hist, npix, &t);
    if (why) { set_error("lj92_encode: %s", why); return -1; }
    int k = 0;
    for (int l = 1; l <= 16; l++) out[k++] = t.bits[l];
    out[k++] = t.nvalues;
    for (int i = 0; i < 17; i++) out[k++] = t.values[i];
    for (int i = 0; i < 17; i++) out[k++] = t.len[i];
    for (int i = 0; i < 17; i++) out[k++] = t.code[i];
    return 0;
}

// Test hook, host only: how the encoder's kernels cut a frame of npix pixels (lj92enc.h -- the constants the kernels and their
// launchers are built with): pixels per block, blocks, threads of a scan workgroup, blocks per scan thread.
int mlvfs_amd_test_lj92_encode_plan(long long npix, long long out[4])
{
    if (!out || npix < 1 || npix >= (1ll << 27)) { set_error("lj92_encode: encode plan wants 1 <= npix < 2^27"); return MLVFS_AMD_ERR_ARG; }
    const uint32_t nb = lje_blocks((uint64_t)npix);
    out[0] = LJE_BLOCK; out[1] = nb; out[2] = LJE_SCAN_THREADS; out[3] = lje_scan_per(nb);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_lj92_encode_batch_dev(const void *d_frames, size_t stride, int nframes, int width, int height, int bitdepth, void *d_out,
                                    size_t out_stride, uint32_t *lengths, int *status, int *max_class, void *stream)
{
    if (!d_frames || !d_out || !lengths || !status) { set_error("lj92_encode_batch: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("lj92_encode_batch: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || (uint64_t)width * height >= (1u << 27)) {
        set_error("lj92_encode_batch: %dx%d not supported", width, height);
        return MLVFS_AMD_ERR_ARG;
    }
    if (bitdepth < 1 || bitdepth > 16) { set_error("lj92_encode_batch: bit depth %d out of range", bitdepth); return MLVFS_AMD_ERR_ARG; }
    const size_t img = (size_t)width * height * 2;
    if (((uintptr_t)d_frames & 1) || (nframes > 1 && (stride < img || (stride & 1)))) { set_error("lj92_encode_batch: stride %zu too small or odd", stride); return MLVFS_AMD_ERR_ARG; }
    if (((uintptr_t)d_out & 3) || (out_stride & 3) || out_stride < 128) { set_error("lj92_encode_batch: out_stride %zu too small or no multiple of 4", out_stride); return MLVFS_AMD_ERR_ARG; }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    if (c->ensure(lje_fixed_bytes((uint32_t)(img / 2), nframes), 0)) return MLVFS_AMD_ERR_NOMEM;
    hipStream_t s = pick_stream(stream, c);
    std::vector<const uint16_t *> src(nframes);
    for (int f = 0; f < nframes; f++) src[f] = (const uint16_t *)((const uint8_t *)d_frames + (size_t)f * stride);
    std::vector<LjeResult> res(nframes);
    ThreadRoom room(c, false);
    uint8_t *out = (uint8_t *)d_out;
    const int rc = lje_encode_batch(src.data(), nframes, width, height, bitdepth, nullptr, 0, c->d_a, room, &out, &out_stride, res.data(), s);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    for (int f = 0; f < nframes; f++) {
        lengths[f] = res[f].length;
        status[f] = res[f].status;
        if (max_class) max_class[f] = res[f].max_class;
    }
    return MLVFS_AMD_OK;
}

int lj92_encode(uint16_t *image, int width, int height, int bitdepth, int readLength, int skipLength,
                uint16_t *delinearize, int delinearizeLength, uint8_t **encoded, int *encodedLength)               // lj92.h:65-68
{
    if (!image || !encoded || !encodedLength || width <= 0 || height <= 0 || bitdepth < 1 || bitdepth > 16) { set_error("lj92_encode: bad argument"); return LJ92_CORRUPT; }
    const uint64_t npix64 = (uint64_t)width * height;
    if (npix64 >= (1u << 27)) { set_error("lj92_encode: more than 2^27 pixels"); return LJ92_NO_MEMORY; }
    const uint32_t npix = (uint32_t)npix64;
    if (delinearize && delinearizeLength <= 0) { set_error("lj92_encode: empty delinearisation table"); return LJ92_CORRUPT; }
    LibcRandGuard rand_guard;                      // HIP code may run: keep the caller's rand() stream out of its reach
    ThreadCtx *c = thread_ctx();
    if (!c) return LJ92_NO_MEMORY;
    // ---- device layout: d_a = tile, table, the batch's fixed scratch; d_b = bit stream, stuffed bytes (sized once the table is known)
    size_t a = 0;
    const size_t img_at = a; a += up256((size_t)npix * 2);
    const size_t delin_at = a; a += up256(delinearize ? (size_t)delinearizeLength * 2 : 0);
    const size_t fixed_at = a; a += lje_fixed_bytes(npix, 1);
    if (c->ensure(a, 0)) return LJ92_NO_MEMORY;
    uint8_t *A = (uint8_t *)c->d_a;
    hipStream_t s = c->stream;
    auto hip_ok = [](hipError_t e, const char *what) { if (e != hipSuccess) { set_error("lj92_encode: %s: %s", what, hipGetErrorString(e)); return false; } return true; };
    // ---- the tile: readLength values, skipLength apart (lj92.c:766-769), contiguous on the device
    if (readLength <= 0 || skipLength == 0 || (uint32_t)readLength >= npix) {
        if (!hip_ok(hipMemcpyAsync(A + img_at, image, (size_t)npix * 2, hipMemcpyHostToDevice, s), "upload")) return LJ92_CORRUPT;
    } else if (skipLength > 0) {
        const uint32_t rows = npix / (uint32_t)readLength, rest = npix - rows * (uint32_t)readLength;
        const size_t pitch = ((size_t)readLength + skipLength) * 2;
        if (!hip_ok(hipMemcpy2DAsync(A + img_at, (size_t)readLength * 2, image, pitch, (size_t)readLength * 2, rows, hipMemcpyHostToDevice, s), "upload")) return LJ92_CORRUPT;
        if (rest && !hip_ok(hipMemcpyAsync(A + img_at + (size_t)rows * readLength * 2, (const uint8_t *)image + rows * pitch, (size_t)rest * 2, hipMemcpyHostToDevice, s), "upload")) return LJ92_CORRUPT;
    } else {                                                           // overlapping or backwards runs: gathered here
        uint16_t *tile = (uint16_t *)malloc((size_t)npix * 2);
        if (!tile) return LJ92_NO_MEMORY;
        const uint16_t *p = image;
        for (uint32_t i = 0, scan = (uint32_t)readLength; i < npix; i++) { tile[i] = *p++; if (--scan == 0) { p += skipLength; scan = (uint32_t)readLength; } }
        const bool ok = hip_ok(hipMemcpyAsync(A + img_at, tile, (size_t)npix * 2, hipMemcpyHostToDevice, s), "upload") && hip_ok(hipStreamSynchronize(s), "upload");
        free(tile);
        if (!ok) return LJ92_CORRUPT;
    }
    if (delinearize && !hip_ok(hipMemcpyAsync(A + delin_at, delinearize, (size_t)delinearizeLength * 2, hipMemcpyHostToDevice, s), "upload")) return LJ92_CORRUPT;
    // ---- the batch path with one frame
    const uint16_t *src = (const uint16_t *)(A + img_at);
    ThreadRoom room(c, true);
    uint8_t *d_out = nullptr;
    size_t out_stride = 0;
    LjeResult r;
    if (lje_encode_batch(&src, 1, width, height, bitdepth, delinearize ? (const uint16_t *)(A + delin_at) : nullptr, delinearizeLength, A + fixed_at,
                         room, &d_out, &out_stride, &r, s)) {
        (void)hipStreamSynchronize(s);
        return LJ92_CORRUPT;
    }
    if (r.status == LJE_DELIN) { set_error("lj92_encode: a value beyond the delinearisation table"); return LJ92_CORRUPT; }
    if (r.status == LJE_DIFF17) { set_error("lj92_encode: a difference of 17 bits (the reference counts and looks it up behind its tables)"); return LJ92_CORRUPT; }
    if (r.status == LJE_TABLE) { set_error("lj92_encode: %s", r.why); return LJ92_CORRUPT; }
    if (r.status != LJE_OK) { set_error("lj92_encode: the stream does not fit its buffer"); return LJ92_CORRUPT; }
    if (r.length > 0x7FFFFFFFu) { set_error("lj92_encode: stream longer than an int can say"); return LJ92_NO_MEMORY; }
    uint8_t *e = (uint8_t *)malloc(r.length);                          // the caller frees it (lj92.c:1136-1139)
    if (!e) return LJ92_NO_MEMORY;
    if (!hip_ok(hipMemcpyAsync(e, d_out, r.length, hipMemcpyDeviceToHost, s), "download") || !hip_ok(hipStreamSynchronize(s), "download")) { free(e); return LJ92_CORRUPT; }
    *encoded = e;
    *encodedLength = (int)r.length;
    return LJ92_OK;
}

}  // extern "C"
