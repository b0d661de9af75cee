// jpeg.h -- shared between csrc/jpeg.cpp (host: tables, header, checks, the batch call) and csrc/k_jpeg.hip (kernels); the mount
// (csrc/mount.cpp) encodes its renderings through jpg_encode_batch.  The definition: include/mlvfs_amd.h, "rendered frames as
// baseline JPEG files".
#pragma once
#include "common.h"

namespace mlv {

constexpr int JPG_HEADER_BYTES = 629;
constexpr int JPG_GROUP = 4;                            // MCUs (side by side) per workgroup of the transform kernel
constexpr int JPG_CHUNK = 16;                           // MCUs per workgroup of the emit kernel
constexpr int JPG_GROUP_422 = 4;                        // at 4:2:2 and 4:4:4 a workgroup of the transform kernel takes a
constexpr int JPG_GROUP_444 = 8;                        //   tile of 64 x 8 pixels: 4 MCUs of 4 blocks, or 8 MCUs of 3
constexpr int JPG_CHUNK_422 = 24;                       // ... and one of the emit kernel 96 blocks, as at 4:2:0: 24 MCUs of 4 blocks,
constexpr int JPG_CHUNK_444 = 32;                       //   or 32 MCUs of 3
constexpr int JPG_BLOCK_BITS = 20 + 63 * 26;            // a block at its longest: DC 9 + 11, 63 times AC 16 + 10
constexpr int JPG_MCU_BYTES = (6 * JPG_BLOCK_BITS + 7) / 8;

// a chroma sampling (MLVFS_AMD_JPEG_420, _422, _444 index kJpgModes): blocks per MCU, how many of them are luminance, the MCU's pixels,
// MCUs per workgroup of the transform and of the emit kernel
struct JpgMode {
    int nb, ny, mcw, mch, group, chunk;
    constexpr int mcu_bytes() const { return (nb * JPG_BLOCK_BITS + 7) / 8; }
};
constexpr JpgMode kJpgModes[3] = {
    { 6, 4, 16, 16, JPG_GROUP, JPG_CHUNK },
    { 4, 2, 16, 8, JPG_GROUP_422, JPG_CHUNK_422 },
    { 3, 1, 8, 8, JPG_GROUP_444, JPG_CHUNK_444 },
};
static_assert(kJpgModes[0].mcu_bytes() == JPG_MCU_BYTES, "4:2:0 is the sampling the constants above describe");
inline bool jpg_sampling_ok(int sampling) { return sampling >= 0 && sampling <= 2; }

// what the transform kernel needs of a quality: the tables in natural order and, per divisor, floor(2^20 / Q) + 1, which divides
// any dividend below 2^12 exactly ((n * r) >> 20: the error n / 2^20 stays below 1 / Q for Q <= 255)
struct JpgQuant {
    uint32_t recip[2][64];
    uint8_t q[2][64];
};

// the four Annex K tables as lengths and codes per symbol, [0] luminance, [1] chrominance
struct JpgHuff {
    uint16_t ac_code[2][256];
    uint16_t dc_code[2][12];
    uint8_t ac_len[2][256];
    uint8_t dc_len[2][12];
};

// where a frame's intermediate data lie in its part of the scratch (byte offsets, each a multiple of 256); nb: the sampling's blocks
// per MCU (6 at 4:2:0)
struct JpgLayout {
    uint32_t pw, ph, mw, mh;
    uint32_t rowcap_dw;        // dwords of the row buffer
    size_t coef;               // int16 [mh][mw][nb][64]: quantised coefficients in scan order
    size_t dcv;                // int16 [mh][mw][nb]: the blocks' DC values once more, side by side
    size_t bbits;              // uint16 [mh][mw][nb]: bits of a block's AC symbols
    size_t off;                // uint32 [mh][mw]: bit at which an MCU begins in its row
    size_t rowbits;            // uint32 [mh]: bits of a row before its padding
    size_t rowat;              // uint32 [mh]: first dword of a row in the row buffer
    size_t rowff;              // uint32 [mh]: 0xFF bytes of the padded row
    size_t rowdst;             // uint32 [mh]: first byte of the row in the stream
    size_t rowbuf;             // uint32 [rowcap_dw]: the rows, each padded to a byte and begun on a dword, before stuffing
    size_t frame_bytes;
};

struct JpgOut {
    uint32_t length;           // entropy-coded data + EOI
    uint32_t status;           // 1: longer than the room (or than the row buffer), nothing usable was written
};

// rowcap_bytes: room for the unstuffed rows; jpg_rowcap_max() always suffices
size_t jpg_rowcap_max(int pw, int ph, int sampling = 0);
JpgLayout jpg_layout(int pw, int ph, size_t rowcap_bytes, int sampling = 0);
// the batch's scratch: nframes results, then nframes frames
inline size_t jpg_scratch_bytes(const JpgLayout &l, int nframes) { return up256(sizeof(JpgOut) * (size_t)nframes) + l.frame_bytes * (size_t)nframes; }
void jpg_quant(int quality, JpgQuant *out);
const JpgHuff &jpg_huff();

// n renderings of pw x ph RGB bytes `stride` apart -> their entropy-coded data + EOI, out_stride apart; res[k] on return (synchronises s).
// l: jpg_layout() of the same sampling
int jpg_encode_batch(const void *d_rgb, size_t stride, int pw, int ph, int quality, void *d_out, size_t out_stride, size_t room, void *d_scratch,
                     const JpgLayout &l, JpgOut *res, int nframes, hipStream_t s, int sampling = 0);

// kernels (k_jpeg.hip)
int jpg_launch(const uint8_t *d_rgb, size_t stride, const JpgLayout &l, const JpgQuant &q, const JpgHuff &h, uint8_t *d_out, size_t out_stride,
               uint32_t room, uint8_t *d_scratch, int nframes, hipStream_t s, int sampling = 0);

}  // namespace mlv
