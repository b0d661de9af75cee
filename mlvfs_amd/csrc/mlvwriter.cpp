// mlvwriter.cpp -- a clip rewritten as an MLV with lossless-JPEG (LJ92) or plain packed payloads: what `mlv_dump -c` / `mlv_dump -d`
// do a frame at a time on a host core, in batches on the GPU.
//
// The container: every source chunk becomes one output chunk that holds the source chunk's blocks in the source's FILE order (the
// reference's index sort, mlvfs/index.c:78-98, is stable: its index over the output is then its index over the source, offsets
// aside).  Blocks are copied byte for byte except
//   MLVI   videoClass gets MLV_VIDEO_CLASS_FLAG_LJ92 (0x100) set or cleared and the LZMA flag (0x80) cleared (mlv.h:30-31);
//   VIDF   the header is copied, frameSpace = 0, blockSize = header + payload;
//            LJ92 payload   [u32 = w * h * 2][stream], the stream lj92_encode writes for the quadrant-tiled frame as ONE component of
//                           W x H at bits_per_pixel precision (what get_image_data, main.c:617-681, decodes and untiles);
//            plain payload  ceil(w * h * bpp / 16) little-endian words (what dng_get_image_data, dng.c:813-843, unpacks);
//   NULL, XREF   dropped (padding has no purpose once payload sizes change; a stale index would be wrong).  No .IDX is written.
// The walk over the chunks is the reader's own (reader_walk_blocks, mlvreader.cpp): it ends where the index ends.
//
// The frames, in batches of one geometry taken in a chunk's file order:
//   LJ92 output            reader_load_list (upload + k_unpack, LZMA decoded by the reader threads, or the GPU's LJ92 decoder)
//                          -> k_mlv_tile -> lje_encode_batch -> lengths and streams to page-locked staging -> file
//   plain from LJ92        GPU decode -> k_mlv_pack -> file
//   plain from plain/LZMA  host only: the packed bytes read_frames yields are written as they are (no HIP device needed)
// With a dark frame (mlvfs_amd_mlv_transcode_dark) reader_load_list subtracts it from every frame (stage 0: k_cal.hip), and a plain or
// LZMA source with plain output goes upload -> unpack + subtract -> k_mlv_pack, the route of an LJ92 source.
// At another bit depth (mlvfs_amd_mlv_transcode_bits, `mlv_dump -b`) every frame whose depth is not out_bpp is shifted
// after the dark frame, inside a pass its route makes anyway (k_mlvpack.hip), and every RAWI block of another depth is rewritten
// (mlvfs_amd_rawi_set_bits):
//   plain / LZMA -> plain   upload -> k_mlv_repack (unpack, subtract, shift, pack in one pass) -> file
//   plain / LZMA -> LJ92    upload -> k_mlv_unpack_shift -> k_mlv_tile (frames at out_bpp already: no shift) -> the encoder at out_bpp
//   LJ92 -> plain           GPU decode -> k_cal_apply if a dark frame is set -> k_mlv_pack with the shift inside -> file
//   LJ92 -> LJ92            GPU decode -> k_cal_apply if set -> k_mlv_tile with the shift inside -> the encoder at out_bpp
// launch_mlv_tile and launch_mlv_pack are told the depth of the frames in HBM and the depth to write, and shift where the two differ:
// frames already at out_bpp, and every frame when out_bpp is 0, run the instantiations without a shift.
// With a flat field (mlvfs_amd_mlv_transcode_cal) reader_load_list applies its gain after the dark frame (stage 0b:
// k_cal.hip) and delivers corrected 16-bit frames at the source's depth; k_mlv_tile or k_mlv_pack follow on every route, shifting
// where the depth changes, so a plain or LZMA source to plain output pays one pass more than k_mlv_repack.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "clip.h"
#include "lj92enc.h"

using namespace mlv;

namespace {

constexpr uint16_t CLASS_RAW = 0x01, CLASS_KIND = 0x0F, CLASS_DELTA = 0x40, CLASS_LZMA = 0x80, CLASS_LJ92 = 0x100;   // mlv.h:25-32
constexpr size_t VIDEO_CLASS_AT = 32;                                                           // offsetof(mlv_file_hdr_t, videoClass)
enum { SRC_PLAIN = PAYLOAD_PLAIN, SRC_LZMA = PAYLOAD_LZMA, SRC_LJ92 = PAYLOAD_LJ92 };

struct Block {
    uint8_t type[4];
    uint64_t off;
    uint32_t size;
    int frame;                 // VIDF: the video frame's number in the reader's index
};

struct Frame {
    int w, h, bpp, kind;
    int obpp;                  // bits per pixel of the payload written: bpp, or the call's out_bpp
    int black;                 // raw_info.black_level: what a flat field's gain is applied around
};

bool is(const uint8_t t[4], const char *tag) { return !memcmp(t, tag, 4); }

bool read_at(int fd, void *dst, size_t n, uint64_t off)
{
    uint8_t *p = (uint8_t *)dst;
    while (n) {
        const ssize_t r = pread(fd, p, n, (off_t)off);
        if (r <= 0) return false;
        p += r; off += (uint64_t)r; n -= (size_t)r;
    }
    return true;
}

bool write_all(int fd, const void *src, size_t n)
{
    const uint8_t *p = (const uint8_t *)src;
    while (n) {
        const ssize_t r = write(fd, p, n);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        p += r; n -= (size_t)r;
    }
    return true;
}

// this call's output files: whatever has been created goes away again unless the call succeeds
struct OutFiles {
    std::vector<std::string> made;
    int fd = -1;
    bool keep = false;
    bool create(const std::string &name)
    {
        close_current();
        fd = open(name.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
        if (fd < 0) { set_error("mlv transcode: cannot create %s: %s", name.c_str(), strerror(errno)); return false; }
        made.push_back(name);
        return true;
    }
    bool close_current()
    {
        const bool ok = fd < 0 || close(fd) == 0;
        fd = -1;
        return ok;
    }
    ~OutFiles()
    {
        (void)close_current();
        if (!keep) for (const std::string &n : made) (void)unlink(n.c_str());
    }
};

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// device memory and page-locked staging of one call
struct DevRoom : LjeRoom {
    DevBuf d_frames, d_aux, d_fixed, d_bits, d_streams;
    uint8_t *h_stage = nullptr;
    size_t stage_bytes = 0;
    int n = 0;                                                         // frames of the batch being encoded

    int frames(size_t bytes)
    {
        if (int rc = d_frames.reserve(bytes)) return rc;
        return d_aux.reserve(bytes);
    }
    int stage(size_t bytes)
    {
        if (stage_bytes >= bytes) return MLVFS_AMD_OK;
        mlvfs_amd_host_free(h_stage);
        stage_bytes = 0;
        h_stage = (uint8_t *)mlvfs_amd_host_alloc(bytes);
        if (!h_stage) return MLVFS_AMD_ERR_NOMEM;
        stage_bytes = bytes;
        return MLVFS_AMD_OK;
    }
    // the encoder's room: the batch's bit streams and one stream slot per frame
    int get(size_t bits, size_t stream_bytes, void **bits_out, uint8_t **d_out, size_t *out_stride) override
    {
        if (int rc = d_bits.reserve(up256(bits))) return rc;
        const size_t slot = up256(stream_bytes);
        if (int rc = d_streams.reserve(slot * (size_t)n)) return rc;
        *bits_out = d_bits;
        *d_out = (uint8_t *)d_streams;
        *out_stride = slot;
        return MLVFS_AMD_OK;
    }
    ~DevRoom() override { mlvfs_amd_host_free(h_stage); }
};

struct Job {
    const void *reader;
    const mlvfs_amd_dark_t *dark = nullptr;
    const mlvfs_amd_flat_t *flat = nullptr;
    int payload, batch, io_threads;
    int out_bpp = 0;                                                   // 0: every frame keeps its depth
    std::vector<Frame> frames;
    std::vector<std::vector<Block>> chunks;
    OutFiles out;
    std::unique_ptr<LibcRandGuard> rand_guard;                         // HIP code runs: the caller's rand() stream stays out of its reach
    std::unique_ptr<DevRoom> dev;                                      // made by the first batch that needs the GPU (and freed under the guard)
    ThreadCtx *ctx = nullptr;
    std::unique_ptr<uint8_t[]> host;                                   // host-only batches
    size_t host_bytes = 0;
    // the batch whose payloads are ready: frame -> where its payload lies and how long it is
    std::map<int, std::pair<const uint8_t *, size_t>> ready;
    long long frames_written = 0, bytes_in = 0, bytes_out = 0;
};

size_t plain_bytes(const Frame &f) { return (size_t)(((uint64_t)f.w * f.h * f.obpp + 15) / 16) * 2; }             // of the payload written

bool on_host(const Job &j, const Frame &f) { return j.payload == MLVFS_AMD_MLV_PLAIN && f.kind != SRC_LJ92 && !j.dark && !j.flat && f.obpp == f.bpp; }

bool same_batch(const Frame &a, const Frame &b) { return a.w == b.w && a.h == b.h && a.bpp == b.bpp && a.kind == b.kind; }

int device_of(Job &j)
{
    if (j.dev) return MLVFS_AMD_OK;
    j.rand_guard.reset(new LibcRandGuard);
    j.ctx = thread_ctx();
    if (!j.ctx) return MLVFS_AMD_ERR_HIP;
    preload_k_mlvpack();
    j.dev.reset(new DevRoom);
    return MLVFS_AMD_OK;
}

// plain and LZMA frames to plain payloads: the reader's packed bytes, one whole word more than the last pixel needs at most
int batch_host(Job &j, const std::vector<int> &list)
{
    const Frame &f = j.frames[list[0]];
    const size_t bytes = plain_bytes(f), stride = up(bytes + 2, 16);
    if (j.host_bytes < stride * list.size()) {
        j.host.reset();
        j.host_bytes = 0;
        j.host.reset(new uint8_t[stride * list.size()]);
        j.host_bytes = stride * list.size();
    }
    const int rc = reader_read_list(j.reader, list.data(), (int)list.size(), j.host.get(), stride, j.io_threads);
    if (rc) return rc;
    for (size_t k = 0; k < list.size(); k++) j.ready[list[k]] = { j.host.get() + k * stride, bytes };
    return MLVFS_AMD_OK;
}

int batch_device(Job &j, const std::vector<int> &list)
{
    if (int rc = device_of(j)) return rc;
    DevRoom &d = *j.dev;
    hipStream_t s = j.ctx->stream;
    const Frame &f = j.frames[list[0]];
    const int n = (int)list.size();
    const uint32_t npix = (uint32_t)f.w * (uint32_t)f.h;
    const size_t img = (size_t)npix * 2, dstride = up256(img);
    if (int rc = d.frames(dstride * n)) return rc;
    Calib cal;
    int rc = calib_on_device(j.dark, j.flat, j.ctx, f.w, f.h, f.bpp, f.black, &cal);
    if (rc) return rc;
    const bool conv = f.obpp != f.bpp, plain = j.payload == MLVFS_AMD_MLV_PLAIN;
    const size_t pstride = up(plain_bytes(f), 16);                     // (<= dstride: d_aux has the room)
    // at another depth a plain or LZMA source is shifted by the pass that reads it; to plain output that pass packs as well.  Not with
    // a flat field: the load corrects at the source's depth and the shift is left to the pass that follows, as for an LJ92 source
    const LoadBits bits{ f.obpp, plain };
    const bool in_load = conv && f.kind != SRC_LJ92 && !j.flat;
    const bool repacked = in_load && plain;
    rc = reader_load_list(j.reader, list.data(), n, f.w, f.h, f.bpp, repacked ? d.d_aux : d.d_frames, repacked ? pstride : dstride, j.io_threads, s,
                          true, &cal, in_load ? &bits : nullptr);
    if (rc) return rc;
    const int loaded = in_load ? f.obpp : f.bpp;                       // the depth of the frames in HBM: the pass that follows does the rest
    if (plain) {
        const size_t bytes = plain_bytes(f);
        if ((rc = d.stage(pstride * n))) return rc;
        if (!repacked && (rc = launch_mlv_pack(d.d_frames, dstride, d.d_aux, pstride, npix, loaded, f.obpp, n, s))) return rc;
        MLV_HIP(hipMemcpyAsync(d.h_stage, d.d_aux, pstride * n, hipMemcpyDeviceToHost, s));
        MLV_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < n; k++) j.ready[list[k]] = { d.h_stage + (size_t)k * pstride, bytes };
        return MLVFS_AMD_OK;
    }
    if ((rc = d.d_fixed.reserve(lje_fixed_bytes(npix, n)))) return rc;
    if ((rc = launch_mlv_tile(d.d_frames, dstride, d.d_aux, dstride, f.w, f.h, f.obpp - loaded, n, s))) return rc;
    std::vector<const uint16_t *> src(n);
    for (int k = 0; k < n; k++) src[k] = (const uint16_t *)((const uint8_t *)d.d_aux + (size_t)k * dstride);
    std::vector<LjeResult> res(n);
    uint8_t *d_streams = nullptr;
    size_t sstride = 0;
    d.n = n;
    if ((rc = lje_encode_batch(src.data(), n, f.w, f.h, f.obpp, nullptr, 0, d.d_fixed, d, &d_streams, &sstride, res.data(), s))) return rc;
    size_t longest = 0;
    for (int k = 0; k < n; k++) {
        const LjeResult &r = res[k];
        if (r.status != LJE_OK) {
            set_error("mlv transcode: frame %d cannot be encoded: %s", list[k],
                      r.status == LJE_DIFF17 ? "a difference of 17 bits" : r.status == LJE_TABLE && r.why ? r.why : "the stream does not fit its buffer");
            return MLVFS_AMD_ERR_ARG;
        }
        if (r.max_class >= 16) {                                       // the reference writes value bits the JPEG standard does not have
            set_error("mlv transcode: frame %d has a difference of class 16, which no standard lossless JPEG stream can hold", list[k]);
            return MLVFS_AMD_ERR_ARG;
        }
        longest = std::max<size_t>(longest, r.length);
    }
    const size_t hstride = up(4 + longest, 16);
    if ((rc = d.stage(hstride * n))) return rc;
    for (int k = 0; k < n; k++) {
        uint8_t *slot = d.h_stage + (size_t)k * hstride;
        const uint32_t decoded = npix * 2;                             // main.c:628-633: the size word in front of the JPEG
        memcpy(slot, &decoded, 4);
        MLV_HIP(hipMemcpyAsync(slot + 4, d_streams + (size_t)k * sstride, res[k].length, hipMemcpyDeviceToHost, s));
        j.ready[list[k]] = { slot, 4 + (size_t)res[k].length };
    }
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

// a block as it is; MLVI: with the video class of the output; RAWI of another depth than the call's out_bpp: at out_bpp
int copy_block(Job &j, int fd, const Block &b, std::vector<uint8_t> &buf)
{
    buf.resize(1 << 20);
    for (uint64_t done = 0; done < b.size;) {
        const size_t n = (size_t)std::min<uint64_t>(buf.size(), b.size - done);
        if (!read_at(fd, buf.data(), n, b.off + done)) { set_error("mlv transcode: short read in the %.4s block at 0x%llx", (const char *)b.type, (unsigned long long)b.off); return MLVFS_AMD_ERR_IO; }
        if (done == 0 && is(b.type, "MLVI") && n >= VIDEO_CLASS_AT + 2) {
            uint16_t vc;
            memcpy(&vc, buf.data() + VIDEO_CLASS_AT, 2);
            vc = (uint16_t)(vc & ~(CLASS_LZMA | CLASS_LJ92));
            if (j.payload == MLVFS_AMD_MLV_LJ92) vc |= CLASS_LJ92;
            memcpy(buf.data() + VIDEO_CLASS_AT, &vc, 2);
        }
        if (done == 0 && j.out_bpp && is(b.type, "RAWI") && n >= sizeof(mlv_rawi_hdr_t)) {
            mlv_rawi_hdr_t rawi;
            memcpy(&rawi, buf.data(), sizeof rawi);
            if (rawi.raw_info.bits_per_pixel != j.out_bpp) {
                if (mlvfs_amd_rawi_set_bits(&rawi, j.out_bpp) != MLVFS_AMD_OK) {
                    set_error("mlv transcode: the RAWI block at 0x%llx says %d bits per pixel", (unsigned long long)b.off, (int)rawi.raw_info.bits_per_pixel);
                    return MLVFS_AMD_ERR_ARG;
                }
                memcpy(buf.data(), &rawi, sizeof rawi);
            }
        }
        if (!write_all(j.out.fd, buf.data(), n)) { set_error("mlv transcode: write failed: %s", strerror(errno)); return MLVFS_AMD_ERR_IO; }
        done += n;
    }
    return MLVFS_AMD_OK;
}

int write_chunk(Job &j, int c, const std::string &name)
{
    if (!j.out.create(name)) return MLVFS_AMD_ERR_IO;
    const int fd = reader_chunk_fd(j.reader, c);
    const std::vector<Block> &blocks = j.chunks[c];
    std::vector<uint8_t> buf;
    for (size_t i = 0; i < blocks.size(); i++) {
        const Block &b = blocks[i];
        if (!is(b.type, "VIDF")) {
            if (int rc = copy_block(j, fd, b, buf)) return rc;
            continue;
        }
        if (!j.ready.count(b.frame)) {
            // the next batch: this frame and the video frames that follow it in the file, while they are of its kind
            j.ready.clear();
            const Frame &f = j.frames[b.frame];
            size_t cap = (size_t)j.batch;
            if (on_host(j, f)) cap = std::max<size_t>(1, std::min<size_t>(cap, ((size_t)1 << 30) / (plain_bytes(f) + 32)));
            std::vector<int> list;
            for (size_t k = i; k < blocks.size() && list.size() < cap; k++) {
                if (!is(blocks[k].type, "VIDF")) continue;
                if (!same_batch(j.frames[blocks[k].frame], f) || (j.flat && j.frames[blocks[k].frame].black != f.black)) break;
                list.push_back(blocks[k].frame);
            }
            const int rc = on_host(j, f) ? batch_host(j, list) : batch_device(j, list);
            if (rc) return rc;
        }
        const auto &p = j.ready[b.frame];
        mlv_vidf_hdr_t v;
        if (!read_at(fd, &v, sizeof v, b.off)) { set_error("mlv transcode: short read in the VIDF block at 0x%llx", (unsigned long long)b.off); return MLVFS_AMD_ERR_IO; }
        j.bytes_in += v.blockSize > sizeof v + (uint64_t)v.frameSpace ? (long long)(v.blockSize - sizeof v - v.frameSpace) : 0;
        v.frameSpace = 0;
        v.blockSize = (uint32_t)(sizeof v + p.second);
        if (!write_all(j.out.fd, &v, sizeof v) || !write_all(j.out.fd, p.first, p.second)) { set_error("mlv transcode: write failed: %s", strerror(errno)); return MLVFS_AMD_ERR_IO; }
        j.frames_written++;
        j.bytes_out += (long long)p.second;
    }
    if (!j.out.close_current()) { set_error("mlv transcode: closing %s failed: %s", name.c_str(), strerror(errno)); return MLVFS_AMD_ERR_IO; }
    return MLVFS_AMD_OK;
}

bool exists(const std::string &name) { struct stat st; return lstat(name.c_str(), &st) == 0; }

bool same_file(const std::string &a, const std::string &b)
{
    if (a == b) return true;
    struct stat sa, sb;
    return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

// chunk c of a clip named `first`: the .MLV itself, then .M00, .M01, ...
std::string chunk_name(const std::string &first, int c)
{
    if (c == 0) return first;
    char two[8];
    snprintf(two, sizeof two, "%02d", (c - 1) % 100);
    std::string n = first;
    n.replace(n.size() - 2, 2, two);
    return n;
}

// the blocks of every chunk in file order, from the reader's own walk (it ends where the index ends); NULL and XREF left out
bool list_blocks(Job &j, int nchunks, const std::map<std::pair<int, uint64_t>, int> &frame_at)
{
    j.chunks.assign(nchunks, {});
    bool ok = true;
    reader_walk_blocks(j.reader, [&](int c, uint64_t pos, const uint8_t *type, uint32_t size, const mlv_file_hdr_t *mlvi) {
        if (mlvi && size >= VIDEO_CLASS_AT + 2 && ((mlvi->videoClass & CLASS_KIND) != CLASS_RAW || (mlvi->videoClass & CLASS_DELTA))) {
            set_error("mlv transcode: video class 0x%x in chunk %d: only raw video without the DELTA flag is rewritten", mlvi->videoClass, c);
            return ok = false;
        }
        if (is(type, "NULL") || is(type, "XREF")) return true;
        Block b{};
        memcpy(b.type, type, 4);
        b.off = pos;
        b.size = size;
        b.frame = -1;
        if (is(type, "VIDF")) {
            const auto it = frame_at.find({ c, pos });
            if (it == frame_at.end()) { set_error("mlv transcode: the VIDF block at 0x%llx of chunk %d is not in the reader's index", (unsigned long long)pos, c); return ok = false; }
            if (size < sizeof(mlv_vidf_hdr_t)) { set_error("mlv transcode: the VIDF block at 0x%llx of chunk %d is shorter than its header", (unsigned long long)pos, c); return ok = false; }
            b.frame = it->second;
        }
        j.chunks[c].push_back(b);
        return true;
    });
    return ok;
}

int transcode(const void *reader, const char *out_path, int payload, int out_bpp, const mlvfs_amd_dark_t *dark, const mlvfs_amd_flat_t *flat,
              int batch_frames, int io_threads, long long stats[4])
{
    if (!reader || !out_path || !stats) { set_error("mlv transcode: null argument"); return MLVFS_AMD_ERR_ARG; }
    for (int i = 0; i < 4; i++) stats[i] = 0;
    if (payload != MLVFS_AMD_MLV_PLAIN && payload != MLVFS_AMD_MLV_LJ92) { set_error("mlv transcode: payload kind %d", payload); return MLVFS_AMD_ERR_ARG; }
    if (out_bpp != 0 && (out_bpp < 8 || out_bpp > 16)) { set_error("mlv transcode: %d bits per pixel: 8 to 16, or 0 to keep the clip's", out_bpp); return MLVFS_AMD_ERR_ARG; }
    const std::string out = out_path;
    if (out.size() < 5 || (out.compare(out.size() - 4, 4, ".MLV") && out.compare(out.size() - 4, 4, ".mlv"))) {
        set_error("mlv transcode: the output path must end in .MLV");
        return MLVFS_AMD_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(reader_stage_mutex(reader));         // one streaming call per reader at a time
    Job j;
    j.reader = reader;
    j.payload = payload;
    j.dark = dark;
    j.flat = flat;
    j.out_bpp = out_bpp;
    j.batch = batch_frames <= 0 ? 8 : batch_frames;
    j.io_threads = io_threads;
    const int nchunks = mlvfs_amd_mlv_chunk_count(reader), nframes = mlvfs_amd_mlv_frame_count(reader);
    if (nchunks > 100) { set_error("mlv transcode: %d chunks", nchunks); return MLVFS_AMD_ERR_ARG; }
    // ---- nothing is overwritten, least of all the source
    const std::string src = reader_path(reader);
    std::vector<std::string> names(nchunks);
    for (int c = 0; c < nchunks; c++) names[c] = chunk_name(out, c);
    std::string idx = out;
    idx.replace(idx.size() - 3, 3, "IDX");
    for (int c = 0; c < nchunks; c++)
        for (int k = 0; k < nchunks; k++)
            if (src.size() >= 3 && same_file(names[c], chunk_name(src, k))) { set_error("mlv transcode: %s is a file of the source clip", names[c].c_str()); return MLVFS_AMD_ERR_ARG; }
    for (const std::string &n : names)
        if (exists(n)) { set_error("mlv transcode: %s exists already", n.c_str()); return MLVFS_AMD_ERR_ARG; }
    if (exists(idx)) { set_error("mlv transcode: %s exists already (an index of another clip)", idx.c_str()); return MLVFS_AMD_ERR_ARG; }
    // ---- the frames: what each one is, and whether it can be rewritten at all
    std::map<std::pair<int, uint64_t>, int> frame_at;
    j.frames.resize(nframes);
    for (int k = 0; k < nframes; k++) {
        int c = 0;
        uint64_t off = 0;
        frame_headers fh;
        if (!reader_frame_place(reader, k, &c, &off) || !mlvfs_amd_mlv_frame_headers(reader, k, &fh)) { set_error("mlv transcode: frame %d has no usable headers", k); return MLVFS_AMD_ERR_ARG; }
        frame_at[{ c, off }] = k;
        const uint16_t vc = fh.file_hdr.videoClass;
        if ((vc & CLASS_KIND) != CLASS_RAW || (vc & CLASS_DELTA)) { set_error("mlv transcode: frame %d: video class 0x%x: only raw video without the DELTA flag is rewritten", k, vc); return MLVFS_AMD_ERR_ARG; }
        Frame &f = j.frames[k];
        f.w = fh.rawi_hdr.xRes;
        f.h = fh.rawi_hdr.yRes;
        f.bpp = fh.rawi_hdr.raw_info.bits_per_pixel;
        f.kind = payload_kind(vc);
        f.obpp = out_bpp ? out_bpp : f.bpp;
        f.black = fh.rawi_hdr.raw_info.black_level;
        if (f.w <= 0 || f.h <= 0 || f.bpp < 1 || f.bpp > 16 || (uint64_t)f.w * f.h >= (1u << 27)) { set_error("mlv transcode: frame %d: %dx%d at %d bits is not supported", k, f.w, f.h, f.bpp); return MLVFS_AMD_ERR_ARG; }
        if (payload == MLVFS_AMD_MLV_LJ92 && ((f.w | f.h) & 1)) {
            set_error("mlv transcode: frame %d: the quadrant tiling of an LJ92 payload takes even sizes, not %dx%d", k, f.w, f.h);
            return MLVFS_AMD_ERR_ARG;
        }
        if (dark && !darkframe_fits(dark, f.w, f.h, f.bpp)) {
            set_error("mlv transcode: frame %d: %dx%d at %d bits is not the dark frame's geometry", k, f.w, f.h, f.bpp);
            return MLVFS_AMD_ERR_ARG;
        }
        if (flat && !flatfield_fits(flat, f.w, f.h)) {
            set_error("mlv transcode: frame %d: %dx%d is not the flat field's geometry", k, f.w, f.h);
            return MLVFS_AMD_ERR_ARG;
        }
        size_t bytes;
        if (!reader_payload_bytes(reader, k, f.kind == SRC_LJ92, &bytes)) return MLVFS_AMD_ERR_ARG;
    }
    if (!list_blocks(j, nchunks, frame_at)) return MLVFS_AMD_ERR_ARG;
    // ---- the files
    int rc = MLVFS_AMD_OK;
    for (int c = 0; c < nchunks && rc == MLVFS_AMD_OK; c++) rc = write_chunk(j, c, names[c]);
    if (rc != MLVFS_AMD_OK) {
        if (j.ctx) (void)hipStreamSynchronize(j.ctx->stream);
        return rc;
    }
    j.out.keep = true;
    stats[0] = j.frames_written;
    stats[1] = j.bytes_in;
    stats[2] = j.bytes_out;
    stats[3] = (long long)j.out.made.size();
    return MLVFS_AMD_OK;
}

// what the entry points call: an exception (allocations sized from the file) becomes an error code
int guarded(const void *reader, const char *out_path, int payload, int out_bpp, const mlvfs_amd_dark_t *dark, const mlvfs_amd_flat_t *flat,
            int batch_frames, int io_threads, long long stats[4])
{
    try { return transcode(reader, out_path, payload, out_bpp, dark, flat, batch_frames, io_threads, stats); }
    catch (const std::exception &e) { set_error("mlv transcode: %s", e.what()); return MLVFS_AMD_ERR_NOMEM; }
}

}  // namespace

extern "C" {

int mlvfs_amd_mlv_transcode(const void *reader, const char *out_path, int payload, int batch_frames, int io_threads, long long stats[4])
{
    return guarded(reader, out_path, payload, 0, nullptr, nullptr, batch_frames, io_threads, stats);
}

int mlvfs_amd_mlv_transcode_dark(const void *reader, const char *out_path, int payload, const mlvfs_amd_dark_t *dark, int batch_frames,
                                 int io_threads, long long stats[4])
{
    return guarded(reader, out_path, payload, 0, dark, nullptr, batch_frames, io_threads, stats);
}

int mlvfs_amd_mlv_transcode_bits(const void *reader, const char *out_path, int payload, int out_bpp, const mlvfs_amd_dark_t *dark, int batch_frames,
                                 int io_threads, long long stats[4])
{
    return guarded(reader, out_path, payload, out_bpp, dark, nullptr, batch_frames, io_threads, stats);
}

int mlvfs_amd_mlv_transcode_cal(const void *reader, const char *out_path, int payload, int out_bpp, const mlvfs_amd_dark_t *dark,
                                const mlvfs_amd_flat_t *flat, int batch_frames, int io_threads, long long stats[4])
{
    return guarded(reader, out_path, payload, out_bpp, dark, flat, batch_frames, io_threads, stats);
}

int mlvfs_amd_rawi_set_bits(mlv_rawi_hdr_t *rawi, int out_bpp)
{
    if (!rawi) { set_error("rawi_set_bits: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (out_bpp < 8 || out_bpp > 16) { set_error("rawi_set_bits: %d bits per pixel: 8 to 16", out_bpp); return MLVFS_AMD_ERR_ARG; }
    struct raw_info ri;                                                // (the block is packed: its fields are copied out and back)
    memcpy(&ri, &rawi->raw_info, sizeof ri);
    if (ri.bits_per_pixel < 1 || ri.bits_per_pixel > 16) { set_error("rawi_set_bits: the block says %d bits per pixel", ri.bits_per_pixel); return MLVFS_AMD_ERR_ARG; }
    const int d = out_bpp - ri.bits_per_pixel;
    auto shifted = [d](int32_t v) { return d >= 0 ? (int32_t)((uint32_t)v << d) : v >> -d; };
    ri.black_level = shifted(ri.black_level);
    ri.white_level = shifted(ri.white_level);
    ri.bits_per_pixel = out_bpp;
    ri.pitch = (int32_t)((int64_t)ri.width * out_bpp / 8);
    ri.frame_size = (int32_t)((uint64_t)rawi->xRes * rawi->yRes * (uint64_t)out_bpp / 8);
    memcpy(&rawi->raw_info, &ri, sizeof ri);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_repack_dev(const mlvfs_amd_geom_t *geom, int out_bpp, const mlvfs_amd_dark_t *dark, const void *d_packed, size_t packed_stride,
                         void *d_out, size_t out_stride, int nframes, void *stream)
{
    if (!geom || !d_packed || !d_out) { set_error("repack: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("repack: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (geom->width <= 0 || geom->height <= 0 || (uint64_t)geom->width * geom->height >= (1u << 27)) { set_error("repack: %dx%d not supported", geom->width, geom->height); return MLVFS_AMD_ERR_ARG; }
    if (geom->bpp < 1 || geom->bpp > 16) { set_error("repack: unsupported bits_per_pixel %d", geom->bpp); return MLVFS_AMD_ERR_ARG; }
    if (out_bpp < 8 || out_bpp > 16) { set_error("repack: %d bits per pixel: 8 to 16", out_bpp); return MLVFS_AMD_ERR_ARG; }
    if (dark && !darkframe_fits(dark, geom->width, geom->height, geom->bpp)) {
        set_error("repack: %dx%d at %d bits is not the dark frame's geometry", geom->width, geom->height, geom->bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    const uint32_t npix = (uint32_t)geom->width * (uint32_t)geom->height;
    const size_t in = (size_t)(((uint64_t)npix * geom->bpp + 15) / 16) * 2, packed = (size_t)(((uint64_t)npix * out_bpp + 15) / 16) * 2;
    if (((uintptr_t)d_packed & 1) || ((uintptr_t)d_out & 1) || (nframes > 1 && (packed_stride < in || out_stride < packed || ((packed_stride | out_stride) & 1)))) {
        set_error("repack: strides %zu / %zu too small or odd", packed_stride, out_stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (d_packed == d_out) { set_error("repack: not in place"); return MLVFS_AMD_ERR_ARG; }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    Calib cal;
    if (int rc = calib_on_device(dark, nullptr, c, geom->width, geom->height, geom->bpp, geom->black, &cal)) return rc;
    return launch_mlv_repack(d_packed, packed_stride, d_out, out_stride, npix, geom->bpp, out_bpp, nframes, &cal, pick_stream(stream, c));
}

int mlvfs_amd_lj92_tile_dev(const void *d_frames, size_t stride, void *d_out, size_t out_stride, int width, int height, int nframes, void *stream)
{
    if (!d_frames || !d_out) { set_error("lj92_tile: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (d_frames == d_out) { set_error("lj92_tile: the tiling does not work in place"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("lj92_tile: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (width <= 0 || height <= 0 || (uint64_t)width * height >= (1u << 27)) { set_error("lj92_tile: %dx%d not supported", width, height); return MLVFS_AMD_ERR_ARG; }
    if ((width | height) & 1) { set_error("lj92_tile: the reference's quadrant map is no bijection for odd sizes (%dx%d)", width, height); return MLVFS_AMD_ERR_ARG; }
    const size_t img = (size_t)width * height * 2;
    if (((uintptr_t)d_frames & 1) || ((uintptr_t)d_out & 1) || (nframes > 1 && (stride < img || out_stride < img || ((stride | out_stride) & 1)))) {
        set_error("lj92_tile: strides %zu / %zu too small or odd", stride, out_stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return launch_mlv_tile(d_frames, stride, d_out, out_stride, width, height, 0, nframes, pick_stream(stream, c));
}

int mlvfs_amd_pack_dev(const mlvfs_amd_geom_t *geom, const void *d_frames, size_t stride, void *d_packed, size_t packed_stride, int nframes,
                       void *stream)
{
    if (!geom || !d_frames || !d_packed) { set_error("pack: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("pack: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (geom->width <= 0 || geom->height <= 0 || (uint64_t)geom->width * geom->height >= (1u << 27)) { set_error("pack: %dx%d not supported", geom->width, geom->height); return MLVFS_AMD_ERR_ARG; }
    if (geom->bpp < 1 || geom->bpp > 16) { set_error("pack: unsupported bits_per_pixel %d", geom->bpp); return MLVFS_AMD_ERR_ARG; }
    const uint32_t npix = (uint32_t)geom->width * (uint32_t)geom->height;
    const size_t img = (size_t)npix * 2, packed = (size_t)(((uint64_t)npix * geom->bpp + 15) / 16) * 2;
    if (((uintptr_t)d_frames & 1) || ((uintptr_t)d_packed & 1) || (nframes > 1 && (stride < img || packed_stride < packed || ((stride | packed_stride) & 1)))) {
        set_error("pack: strides %zu / %zu too small or odd", stride, packed_stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return launch_mlv_pack(d_frames, stride, d_packed, packed_stride, npix, geom->bpp, geom->bpp, nframes, pick_stream(stream, c));
}

}  // extern "C"
