// jpeg_host_check.cpp -- a stand-alone host program for tests/test_jpeg_host.py: headers and quantisation tables with the bytes the
// definition of mlvfs_amd/jpeg.py expects, read from the file named on the command line, through mlvfs_amd_jpeg_header and
// mlvfs_amd_jpeg_qtables; then the sizes and the refusals.  It is compiled and linked with -fsanitize=address,undefined against the
// sanitizer build of the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime,
// no HIP device.
//
// The file: records of {uint32 kind; int32 a, b, c; ...}
//   kind 1: a = pw, b = ph, c = quality; the header's bytes expected (mlvfs_amd_jpeg_header_size() of them)
//   kind 2: c = quality; the 128 table bytes expected
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "jpeg_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

struct Head {
    uint32_t kind;
    int32_t a, b, c;
};

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: jpeg_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const size_t hdr = mlvfs_amd_jpeg_header_size();
    if (hdr != 629) return fail("the header's size is not 629", -1);
    int rec = 0;
    for (;; rec++) {
        Head hd;
        if (fread(&hd, sizeof hd, 1, f) != 1) break;
        if (hd.kind == 1) {
            // exactly the header's size: a write one past it is the sanitizer's to see
            std::unique_ptr<uint8_t[]> want(new uint8_t[hdr]), got(new uint8_t[hdr]);
            if (fread(want.get(), 1, hdr, f) != hdr) return fail("short file", rec);
            memset(got.get(), 0xA5, hdr);
            if (mlvfs_amd_jpeg_header(hd.a, hd.b, hd.c, got.get(), hdr) != hdr) return fail("another size returned", rec);
            if (memcmp(got.get(), want.get(), hdr)) return fail("another header", rec);
        } else if (hd.kind == 2) {
            std::unique_ptr<uint8_t[]> want(new uint8_t[128]), got(new uint8_t[128]);
            if (fread(want.get(), 1, 128, f) != 128) return fail("short file", rec);
            if (mlvfs_amd_jpeg_qtables(hd.c, got.get()) != MLVFS_AMD_OK) return fail("qtables refused", rec);
            if (memcmp(got.get(), want.get(), 128)) return fail("other tables", rec);
        } else return fail("a record of an unknown kind", rec);
    }
    fclose(f);
    // the refusals, which follow no pointer and write nothing
    uint8_t one = 0xA5;
    if (mlvfs_amd_jpeg_header(4, 4, 90, &one, 1) != 0 || mlvfs_amd_jpeg_header(0, 4, 90, &one, 1) != 0 || mlvfs_amd_jpeg_header(4, 4, 0, &one, 1) != 0 ||
        mlvfs_amd_jpeg_header(4, 4, 101, &one, 1) != 0 || mlvfs_amd_jpeg_header(65536, 1, 90, &one, 1) != 0 || mlvfs_amd_jpeg_header(4, 4, 90, nullptr, hdr) != 0 ||
        one != 0xA5)
        return fail("a refusal of jpeg_header did not happen", rec);
    if (mlvfs_amd_jpeg_qtables(0, &one) != MLVFS_AMD_ERR_ARG || mlvfs_amd_jpeg_qtables(101, &one) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_jpeg_qtables(90, nullptr) != MLVFS_AMD_ERR_ARG || one != 0xA5)
        return fail("a refusal of jpeg_qtables did not happen", rec);
    if (mlvfs_amd_jpeg_scratch_bytes(0, 4, 1) != 0 || mlvfs_amd_jpeg_scratch_bytes(4, 4, -1) != 0 || mlvfs_amd_jpeg_scratch_bytes(8192, 4096, 1) != 0)
        return fail("a refusal of jpeg_scratch_bytes did not happen", rec);
    const size_t s1 = mlvfs_amd_jpeg_scratch_bytes(1792, 660, 1), s8 = mlvfs_amd_jpeg_scratch_bytes(1792, 660, 8);
    if (s1 < (size_t)112 * 42 * 768 || s8 <= 7 * s1 || s8 > 8 * s1) return fail("the scratch of 1792x660", rec);
    // the largest input: nothing overflows on the way to its layout
    if (mlvfs_amd_jpeg_scratch_bytes(65535, 511, 65535) == 0 || mlvfs_amd_jpeg_scratch_bytes(1, 65535, 2) == 0) return fail("the scratch of the largest input", rec);
    uint8_t px[16 * 16 * 3] = { 0 }, out[64] = { 0 };
    uint32_t len[2] = { 7, 7 };
    int st[2] = { 7, 7 };
    alignas(16) uint8_t scratch[64];
    if (mlvfs_amd_jpeg_encode_dev(nullptr, 768, 16, 16, 90, out, 64, 64, scratch, 1 << 30, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_jpeg_encode_dev(px, 768, 16, 16, 90, out, 64, 64, scratch, 64, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_jpeg_encode_dev(px, 768, 16, 16, 0, out, 64, 64, scratch, 1 << 30, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_jpeg_encode_dev(px, 768, 16, 16, 90, out, 64, 64, scratch, 1 << 30, nullptr, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        len[0] != 7 || st[0] != 7)
        return fail("a refusal of jpeg_encode_dev did not happen", rec);
    printf("jpeg_host_check: %d records\n", rec);
    return rec > 0 ? 0 : 1;
}
