// jpeg.cpp -- the host side of the renderings' baseline JPEG files (include/mlvfs_amd.h, "rendered frames as baseline JPEG files"):
// the quantisation tables of a quality, the four constant Huffman tables, the 629 bytes in front of the entropy-coded data, the layout
// of the encoder's scratch, every check of mlvfs_amd_jpeg_encode_dev, and the batch call the mount shares with it.  Kernels: k_jpeg.hip.
#include "clip.h"
#include "jpeg.h"

#include <cstring>
#include <mutex>

namespace mlv {

namespace {

// the example tables of the JPEG standard, Annex K.1 and K.2, natural order
const uint8_t kBase[2][64] = {
    { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
    { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 },
};

// scan position -> natural index
const uint8_t kZigzag[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

// the "typical" Huffman tables of Annex K.3 - K.6 as their DHT segments carry them: 16 counts, then the symbols by code length
// (DC luminance, AC luminance, DC chrominance, AC chrominance; 28, 178, 28, 178 bytes)
const char *const kHuffHex[4] = {
    "00010501010101010100000000000000" "000102030405060708090a0b",
    "0002010303020403050504040000017d"
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa",
    "00030101010101010101010000000000" "000102030405060708090a0b",
    "00020102040403040705040400010277"
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa",
};

struct HuffSpec {
    uint8_t bytes[4][16 + 162];
    int len[4];
    JpgHuff codes;
};

int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// the segments' bytes, and each symbol's code by the rule of Annex C
const HuffSpec &huff_spec()
{
    static HuffSpec spec;
    static std::once_flag once;
    std::call_once(once, [] {
        memset(&spec, 0, sizeof spec);
        for (int t = 0; t < 4; t++) {
            const char *h = kHuffHex[t];
            int n = 0;
            for (; h[2 * n]; n++) spec.bytes[t][n] = (uint8_t)(hexval(h[2 * n]) * 16 + hexval(h[2 * n + 1]));
            spec.len[t] = n;
            const int tab = t >> 1;
            uint32_t code = 0;
            int k = 16;
            for (int bits = 1; bits <= 16; bits++) {
                for (int c = 0; c < spec.bytes[t][bits - 1]; c++, k++, code++) {
                    const uint8_t sym = spec.bytes[t][k];
                    if (t & 1) { spec.codes.ac_len[tab][sym] = (uint8_t)bits; spec.codes.ac_code[tab][sym] = (uint16_t)code; }
                    else if (sym < 12) { spec.codes.dc_len[tab][sym] = (uint8_t)bits; spec.codes.dc_code[tab][sym] = (uint16_t)code; }
                }
                code <<= 1;
            }
        }
    });
    return spec;
}

void put16(uint8_t *&p, unsigned v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; }
void put(uint8_t *&p, const void *src, size_t n) { memcpy(p, src, n); p += n; }

bool jpg_size_ok(int pw, int ph) { return pw >= 1 && ph >= 1 && pw <= 65535 && ph <= 65535 && (uint64_t)pw * (uint64_t)ph < (1u << 25); }

void qtables(int quality, uint8_t out[128])
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) out[64 * t + k] = (uint8_t)std::min(std::max((kBase[t][k] * scale + 50) / 100, 1), 255);
}

}  // namespace

const JpgHuff &jpg_huff() { return huff_spec().codes; }

void jpg_quant(int quality, JpgQuant *out)
{
    qtables(quality, &out->q[0][0]);
    for (int k = 0; k < 128; k++) (&out->recip[0][0])[k] = (1u << 20) / (&out->q[0][0])[k] + 1u;
}

size_t jpg_rowcap_max(int pw, int ph, int sampling)
{
    const JpgMode &md = kJpgModes[sampling];
    const size_t mw = ((size_t)pw + md.mcw - 1) / md.mcw, mh = ((size_t)ph + md.mch - 1) / md.mch;
    return mh * ((mw * md.mcu_bytes() + 3) / 4 * 4);
}

JpgLayout jpg_layout(int pw, int ph, size_t rowcap_bytes, int sampling)
{
    const JpgMode &md = kJpgModes[sampling];
    JpgLayout l{};
    l.pw = (uint32_t)pw;
    l.ph = (uint32_t)ph;
    l.mw = ((uint32_t)pw + md.mcw - 1) / md.mcw;
    l.mh = ((uint32_t)ph + md.mch - 1) / md.mch;
    const size_t nm = (size_t)l.mw * l.mh;
    l.rowcap_dw = (uint32_t)((std::min(rowcap_bytes, jpg_rowcap_max(pw, ph, sampling)) + 3) / 4);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += up256(bytes); return here; };
    l.coef = take(nm * md.nb * 64 * sizeof(int16_t));
    l.dcv = take(nm * md.nb * sizeof(int16_t));
    l.bbits = take(nm * md.nb * sizeof(uint16_t));
    l.off = take(nm * sizeof(uint32_t));
    l.rowbits = take(l.mh * sizeof(uint32_t));
    l.rowat = take(l.mh * sizeof(uint32_t));
    l.rowff = take(l.mh * sizeof(uint32_t));
    l.rowdst = take(l.mh * sizeof(uint32_t));
    l.rowbuf = take((size_t)l.rowcap_dw * sizeof(uint32_t));
    l.frame_bytes = at;
    return l;
}

int jpg_encode_batch(const void *d_rgb, size_t stride, int pw, int ph, int quality, void *d_out, size_t out_stride, size_t room, void *d_scratch,
                     const JpgLayout &l, JpgOut *res, int nframes, hipStream_t s, int sampling)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    JpgQuant q;
    jpg_quant(quality, &q);
    const uint32_t room32 = (uint32_t)std::min<size_t>(room, 0xFFFFFFFFu);
    const int rc = jpg_launch((const uint8_t *)d_rgb, stride, l, q, jpg_huff(), (uint8_t *)d_out, out_stride, room32, (uint8_t *)d_scratch, nframes, s, sampling);
    if (rc) return rc;
    MLV_HIP(hipMemcpyAsync(res, d_scratch, sizeof(JpgOut) * (size_t)nframes, hipMemcpyDeviceToHost, s));
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

}  // namespace mlv

using namespace mlv;

extern "C" {

size_t mlvfs_amd_jpeg_header_size(void) { return JPG_HEADER_BYTES; }

int mlvfs_amd_jpeg_qtables(int quality, uint8_t out[128])
{
    if (!out) { set_error("jpeg_qtables: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (quality < 1 || quality > 100) { set_error("jpeg_qtables: a quality of %d (1 .. 100)", quality); return MLVFS_AMD_ERR_ARG; }
    qtables(quality, out);
    return MLVFS_AMD_OK;
}

size_t mlvfs_amd_jpeg_header(int pw, int ph, int quality, uint8_t *out, size_t cap)
{
    return mlvfs_amd_jpeg_header_sampled(pw, ph, quality, MLVFS_AMD_JPEG_420, out, cap);
}

size_t mlvfs_amd_jpeg_header_sampled(int pw, int ph, int quality, int sampling, uint8_t *out, size_t cap)
{
    if (!out) { set_error("jpeg_header: null argument"); return 0; }
    if (!jpg_sampling_ok(sampling)) { set_error("jpeg_header: a sampling of %d (0: 4:2:0, 1: 4:2:2, 2: 4:4:4)", sampling); return 0; }
    if (!jpg_size_ok(pw, ph)) { set_error("jpeg_header: %dx%d pixels not supported", pw, ph); return 0; }
    if (quality < 1 || quality > 100) { set_error("jpeg_header: a quality of %d (1 .. 100)", quality); return 0; }
    if (cap < (size_t)JPG_HEADER_BYTES) { set_error("jpeg_header: room for %zu bytes, the header takes %d", cap, JPG_HEADER_BYTES); return 0; }
    static const uint8_t soi_app0[] = { 0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00 };
    static const uint8_t factors[3] = { 0x22, 0x21, 0x11 };
    const uint8_t sof_tail[] = { 0x03, 0x01, factors[sampling], 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01 };
    static const uint8_t sos[] = { 0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00 };
    uint8_t head[JPG_HEADER_BYTES], q[128];
    uint8_t *p = head;
    put(p, soi_app0, sizeof soi_app0);
    qtables(quality, q);
    for (int t = 0; t < 2; t++) {
        put16(p, 0xFFDB);
        put16(p, 67);
        *p++ = (uint8_t)t;
        for (int k = 0; k < 64; k++) *p++ = q[64 * t + kZigzag[k]];
    }
    put16(p, 0xFFC0);
    put16(p, 17);
    *p++ = 8;
    put16(p, (unsigned)ph);
    put16(p, (unsigned)pw);
    put(p, sof_tail, sizeof sof_tail);
    const HuffSpec &hs = huff_spec();
    static const uint8_t ids[4] = { 0x00, 0x10, 0x01, 0x11 };
    for (int t = 0; t < 4; t++) {
        put16(p, 0xFFC4);
        put16(p, 3 + (unsigned)hs.len[t]);
        *p++ = ids[t];
        put(p, hs.bytes[t], (size_t)hs.len[t]);
    }
    put16(p, 0xFFDD);
    put16(p, 4);
    put16(p, ((unsigned)pw + kJpgModes[sampling].mcw - 1) / kJpgModes[sampling].mcw);
    put(p, sos, sizeof sos);
    if (p - head != JPG_HEADER_BYTES) { set_error("jpeg_header: %d bytes built, not %d", (int)(p - head), JPG_HEADER_BYTES); return 0; }
    memcpy(out, head, sizeof head);
    return JPG_HEADER_BYTES;
}

size_t mlvfs_amd_jpeg_scratch_bytes(int pw, int ph, int nframes) { return mlvfs_amd_jpeg_scratch_bytes_sampled(pw, ph, MLVFS_AMD_JPEG_420, nframes); }

size_t mlvfs_amd_jpeg_scratch_bytes_sampled(int pw, int ph, int sampling, int nframes)
{
    if (!jpg_sampling_ok(sampling)) { set_error("jpeg_scratch_bytes: a sampling of %d (0: 4:2:0, 1: 4:2:2, 2: 4:4:4)", sampling); return 0; }
    if (!jpg_size_ok(pw, ph) || nframes < 0) { set_error("jpeg_scratch_bytes: %d frames of %dx%d pixels not supported", nframes, pw, ph); return 0; }
    return jpg_scratch_bytes(jpg_layout(pw, ph, jpg_rowcap_max(pw, ph, sampling), sampling), nframes);
}

int mlvfs_amd_jpeg_mcus(int pw, int ph, int sampling, int *mw, int *mh)
{
    if (!mw || !mh) { set_error("jpeg_mcus: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (!jpg_sampling_ok(sampling)) { set_error("jpeg_mcus: a sampling of %d (0: 4:2:0, 1: 4:2:2, 2: 4:4:4)", sampling); return MLVFS_AMD_ERR_ARG; }
    if (!jpg_size_ok(pw, ph)) { set_error("jpeg_mcus: %dx%d pixels not supported", pw, ph); return MLVFS_AMD_ERR_ARG; }
    *mw = (pw + kJpgModes[sampling].mcw - 1) / kJpgModes[sampling].mcw;
    *mh = (ph + kJpgModes[sampling].mch - 1) / kJpgModes[sampling].mch;
    return MLVFS_AMD_OK;
}

int mlvfs_amd_jpeg_encode_dev(const void *d_rgb, size_t stride, int pw, int ph, int quality, void *d_out, size_t out_stride, size_t room,
                              void *d_scratch, size_t scratch_bytes, uint32_t *h_lengths, int *h_status, int nframes, void *stream)
{
    return mlvfs_amd_jpeg_encode_sampled_dev(d_rgb, stride, pw, ph, quality, MLVFS_AMD_JPEG_420, d_out, out_stride, room, d_scratch, scratch_bytes,
                                             h_lengths, h_status, nframes, stream);
}

int mlvfs_amd_jpeg_encode_sampled_dev(const void *d_rgb, size_t stride, int pw, int ph, int quality, int sampling, void *d_out, size_t out_stride,
                                      size_t room, void *d_scratch, size_t scratch_bytes, uint32_t *h_lengths, int *h_status, int nframes,
                                      void *stream)
{
    if (!d_rgb || !d_out || !d_scratch || !h_lengths || !h_status) { set_error("jpeg_encode: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (!jpg_sampling_ok(sampling)) { set_error("jpeg_encode: a sampling of %d (0: 4:2:0, 1: 4:2:2, 2: 4:4:4)", sampling); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0 || nframes > 65535) { set_error("jpeg_encode: %d frames (0 .. 65535)", nframes); return MLVFS_AMD_ERR_ARG; }
    if (!jpg_size_ok(pw, ph)) { set_error("jpeg_encode: %dx%d pixels not supported (1x1 up to 65535 a side, below 2^25 pixels)", pw, ph); return MLVFS_AMD_ERR_ARG; }
    if (quality < 1 || quality > 100) { set_error("jpeg_encode: a quality of %d (1 .. 100)", quality); return MLVFS_AMD_ERR_ARG; }
    const size_t img = (size_t)3 * pw * ph;
    if (nframes > 1 && (stride < img || out_stride < room)) {
        set_error("jpeg_encode: strides %zu / %zu smaller than a rendering (%zu) or the room (%zu)", stride, out_stride, img, room);
        return MLVFS_AMD_ERR_ARG;
    }
    if ((uintptr_t)d_scratch & 15) { set_error("jpeg_encode: the scratch is not 16-byte aligned"); return MLVFS_AMD_ERR_ARG; }
    const JpgLayout l = jpg_layout(pw, ph, jpg_rowcap_max(pw, ph, sampling), sampling);
    const size_t need = jpg_scratch_bytes(l, nframes);
    if (scratch_bytes < need) { set_error("jpeg_encode: %zu bytes of scratch, %d frames of %dx%d take %zu", scratch_bytes, nframes, pw, ph, need); return MLVFS_AMD_ERR_ARG; }
    if (nframes == 0) return MLVFS_AMD_OK;
    const uintptr_t a0 = (uintptr_t)d_rgb, a1 = a0 + (size_t)(nframes - 1) * stride + img;
    const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (size_t)(nframes - 1) * out_stride + room;
    const uintptr_t c0 = (uintptr_t)d_scratch, c1 = c0 + need;
    if ((a0 < b1 && b0 < a1) || (a0 < c1 && c0 < a1) || (b0 < c1 && c0 < b1)) {
        set_error("jpeg_encode: the renderings, the streams and the scratch overlap");
        return MLVFS_AMD_ERR_ARG;
    }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    std::vector<JpgOut> res((size_t)nframes);
    const int rc = jpg_encode_batch(d_rgb, stride, pw, ph, quality, d_out, out_stride, room, d_scratch, l, res.data(), nframes, pick_stream(stream, c), sampling);
    if (rc) return rc;
    for (int k = 0; k < nframes; k++) {
        h_status[k] = res[k].status ? 1 : 0;
        h_lengths[k] = res[k].length;
    }
    return MLVFS_AMD_OK;
}

}  // extern "C"
