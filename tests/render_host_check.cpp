// render_host_check.cpp -- a stand-alone host program for tests/test_render_host.py: frame headers with the parameters the definition
// of mlvfs_amd/render.py expects, and TIFF headers, read from the file named on the command line, through mlvfs_amd_rgb_params and
// mlvfs_amd_rgb_header; then the table, the geometry and the refusals.  It is compiled and linked with -fsanitize=address,undefined
// against the sanitizer build of the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded
// runtime, no HIP device.
//
// The file: records of {uint32 kind; uint32 a; int32 b; ...}
//   kind 1: a = bytes of the frame_headers blob, b = gain_q8; the blob; 13 int32 expected
//   kind 2: a = pw, b = ph; the header's bytes expected (mlvfs_amd_rgb_header_size() of them)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "render_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

struct Head {
    uint32_t kind, a;
    int32_t b;
};

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: render_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const size_t hdr = mlvfs_amd_rgb_header_size();
    if (hdr == 0 || hdr % 16) return fail("the header's size is no multiple of 16", -1);
    int rec = 0;
    for (;; rec++) {
        Head hd;
        if (fread(&hd, sizeof hd, 1, f) != 1) break;
        if (hd.kind == 1) {
            if (hd.a != sizeof(struct frame_headers)) return fail("frame_headers of another size", rec);
            struct frame_headers fh, before;
            int32_t want[13];
            if (fread(&fh, sizeof fh, 1, f) != 1 || fread(want, sizeof want, 1, f) != 1) return fail("short file", rec);
            before = fh;
            // exactly 13 integers: a write one past them is the sanitizer's to see
            std::unique_ptr<int32_t[]> got(new int32_t[13]);
            if (mlvfs_amd_rgb_params(&fh, hd.b, got.get()) != MLVFS_AMD_OK) return fail("rgb_params refused", rec);
            if (memcmp(got.get(), want, sizeof want)) return fail("other parameters", rec);
            if (memcmp(&fh, &before, sizeof fh)) return fail("frame_headers changed", rec);
        } else if (hd.kind == 2) {
            std::unique_ptr<uint8_t[]> want(new uint8_t[hdr]), got(new uint8_t[hdr]);
            if (fread(want.get(), 1, hdr, f) != hdr) return fail("short file", rec);
            memset(got.get(), 0xA5, hdr);
            if (mlvfs_amd_rgb_header((int)hd.a, hd.b, got.get(), hdr) != hdr) return fail("another size returned", rec);
            if (memcmp(got.get(), want.get(), hdr)) return fail("another header", rec);
        } else return fail("a record of an unknown kind", rec);
    }
    fclose(f);
    // extreme headers: the levels and gains at the ends of their types, through the 128-bit arithmetic
    struct frame_headers fh;
    memset(&fh, 0, sizeof fh);
    fh.wbal_hdr.wb_mode = 6;
    const int32_t levels[][2] = { { INT32_MIN, INT32_MAX }, { INT32_MAX, INT32_MIN }, { 0, 0 }, { -1, 1 } };
    const uint32_t gains[][3] = { { 1, 1, 1 }, { 0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF }, { 0x7FFFFFFF, 1, 0x7FFFFFFF }, { 1, 0x7FFFFFFF, 1 }, { 0xFFFFFFFF, 1, 1 } };
    for (const auto &lv : levels)
        for (const auto &g : gains)
            for (int gain : { 1, 65535 }) {
                fh.rawi_hdr.raw_info.black_level = lv[0];
                fh.rawi_hdr.raw_info.white_level = lv[1];
                fh.wbal_hdr.wbgain_r = g[0];
                fh.wbal_hdr.wbgain_g = g[1];
                fh.wbal_hdr.wbgain_b = g[2];
                int32_t p[13];
                if (mlvfs_amd_rgb_params(&fh, gain, p) != MLVFS_AMD_OK || p[0] != lv[0]) return fail("rgb_params at an extreme", rec);
                for (int j = 1; j < 4; j++)
                    if (p[j] < 0) return fail("a negative A", rec);
            }
    int32_t p[13];
    for (int j = 0; j < 13; j++) p[j] = -7;
    if (mlvfs_amd_rgb_params(&fh, 0, p) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_params(&fh, 65536, p) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_rgb_params(nullptr, 256, p) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_params(&fh, 256, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of rgb_params did not happen", rec);
    for (int j = 0; j < 13; j++)
        if (p[j] != -7) return fail("a refusal of rgb_params wrote", rec);
    // the table: exactly 4096 bytes, monotone from 0 to 255
    std::unique_ptr<uint8_t[]> lut(new uint8_t[4096]);
    if (mlvfs_amd_rgb_lut(lut.get()) != MLVFS_AMD_OK || mlvfs_amd_rgb_lut(nullptr) != MLVFS_AMD_ERR_ARG) return fail("rgb_lut", rec);
    if (lut[0] != 0 || lut[4095] != 255) return fail("the table's ends", rec);
    for (int t = 1; t < 4096; t++)
        if (lut[t] < lut[t - 1]) return fail("the table is not monotone", rec);
    // the geometry and the refusals, which follow no pointer
    int pw = -7, ph = -7;
    if (mlvfs_amd_rgb_geom(3584, 1320, &pw, &ph) != MLVFS_AMD_OK || pw != 1792 || ph != 660) return fail("rgb_geom 3584x1320", rec);
    if (mlvfs_amd_rgb_geom(7, 5, &pw, &ph) != MLVFS_AMD_OK || pw != 3 || ph != 2) return fail("rgb_geom 7x5", rec);
    pw = ph = -7;
    if (mlvfs_amd_rgb_geom(1, 8, &pw, &ph) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_geom(1 << 14, 1 << 13, &pw, &ph) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_rgb_geom(8, 8, nullptr, &ph) != MLVFS_AMD_ERR_ARG || mlvfs_amd_rgb_geom(8, 8, &pw, nullptr) != MLVFS_AMD_ERR_ARG || pw != -7 || ph != -7)
        return fail("a refusal of rgb_geom did not happen", rec);
    uint8_t one = 0xA5;
    if (mlvfs_amd_rgb_header(4, 4, &one, 1) != 0 || mlvfs_amd_rgb_header(0, 4, &one, 1) != 0 || mlvfs_amd_rgb_header(4, 4, nullptr, hdr) != 0 || one != 0xA5)
        return fail("a refusal of rgb_header did not happen", rec);
    uint16_t px[16] = { 0 };
    uint8_t out[16] = { 0 };
    if (mlvfs_amd_render2_dev(px, 32, 4, 4, p, px, 12, 1, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_render2_dev(nullptr, 32, 4, 4, p, out, 12, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_render2_dev(px, 32, 1, 4, p, out, 12, 1, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_render2_dev(px, 32, 4, 4, nullptr, out, 12, 1, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of render2_dev did not happen", rec);
    printf("render_host_check: %d records\n", rec);
    return rec > 0 ? 0 : 1;
}
