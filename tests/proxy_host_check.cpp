// proxy_host_check.cpp -- a stand-alone host program for tests/test_proxy_host.py: frame headers and the proxy headers the rule of
// tests/proxy_cases.py expects, read from the file named on the command line, through mlvfs_amd_dng_header_proxy, and
// mlvfs_amd_proxy_geom with its refusals.  It is compiled and linked with -fsanitize=address,undefined against the sanitizer build of
// the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run directly: no Python, no preloaded runtime, no HIP device.
//
// The file: records of {uint32 blob bytes; double fps; int64 offset; uint64 max_size; uint32 stream_bytes, basename bytes, n;
// frame_headers blob; basename; the n = min(max_size, 65536) bytes expected; frame_headers as they are afterwards}.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "proxy_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

#pragma pack(push, 1)
struct Head {
    uint32_t blob;
    double fps;
    int64_t offset;
    uint64_t max_size;
    uint32_t stream, base, n;
};
#pragma pack(pop)

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: proxy_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0;
    for (;; rec++) {
        Head hd;
        if (fread(&hd, sizeof hd, 1, f) != 1) break;
        if (hd.blob != sizeof(struct frame_headers)) return fail("frame_headers of another size", rec);
        struct frame_headers fh, after;
        std::string base(hd.base, '\0');
        // exactly n bytes: a write one past the request is the sanitizer's to see
        std::unique_ptr<uint8_t[]> want(new uint8_t[hd.n]), got(new uint8_t[hd.n]);
        if (fread(&fh, sizeof fh, 1, f) != 1 || (hd.base && fread(&base[0], 1, hd.base, f) != hd.base) ||
            (hd.n && fread(want.get(), 1, hd.n, f) != hd.n) || fread(&after, sizeof after, 1, f) != 1)
            return fail("short file", rec);
        memset(got.get(), 0xA5, hd.n);
        const size_t n = mlvfs_amd_dng_header_proxy(&fh, got.get(), (off_t)hd.offset, (size_t)hd.max_size, hd.fps, base.c_str(), 2, hd.stream);
        if (n != hd.n) return fail("another size returned", rec);
        if (memcmp(got.get(), want.get(), hd.n)) return fail("another header", rec);
        if (memcmp(&fh, &after, sizeof fh)) return fail("frame_headers left in another state", rec);
    }
    fclose(f);
    // the geometry and the refusals, which follow no pointer
    int pw = -7, ph = -7;
    if (mlvfs_amd_proxy_geom(3584, 1320, 2, &pw, &ph) != MLVFS_AMD_OK || pw != 1792 || ph != 660) return fail("proxy_geom 3584x1320", rec);
    if (mlvfs_amd_proxy_geom(7, 5, 2, &pw, &ph) != MLVFS_AMD_OK || pw != 2 || ph != 2) return fail("proxy_geom 7x5", rec);
    pw = ph = -7;
    if (mlvfs_amd_proxy_geom(3, 8, 2, &pw, &ph) != MLVFS_AMD_ERR_ARG || mlvfs_amd_proxy_geom(8, 8, 4, &pw, &ph) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_proxy_geom(1 << 14, 1 << 13, 2, &pw, &ph) != MLVFS_AMD_ERR_ARG || mlvfs_amd_proxy_geom(8, 8, 2, nullptr, &ph) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_proxy_geom(8, 8, 2, &pw, nullptr) != MLVFS_AMD_ERR_ARG || pw != -7 || ph != -7)
        return fail("a refusal of proxy_geom did not happen", rec);
    struct frame_headers fh;
    memset(&fh, 0, sizeof fh);
    fh.rawi_hdr.xRes = 2;
    fh.rawi_hdr.yRes = 64;
    uint8_t one = 0xA5;
    if (mlvfs_amd_dng_header_proxy(&fh, &one, 0, 1, 0.0, "", 2, 0) != 0 || mlvfs_amd_dng_header_proxy(nullptr, &one, 0, 1, 0.0, "", 2, 0) != 0 ||
        mlvfs_amd_dng_header_proxy(&fh, nullptr, 0, 1, 0.0, "", 2, 0) != 0 || one != 0xA5)
        return fail("a refusal of dng_header_proxy did not happen", rec);
    fh.rawi_hdr.xRes = 64;
    if (mlvfs_amd_dng_header_proxy(&fh, &one, 0, 1, 0.0, "", 3, 0) != 0 || one != 0xA5) return fail("a factor of 3 was taken", rec);
    uint16_t px[16] = { 0 };
    if (mlvfs_amd_bin2_dev(px, 32, 4, 4, px, 32, 1, nullptr) != MLVFS_AMD_ERR_ARG || mlvfs_amd_bin2_dev(nullptr, 32, 4, 4, px, 8, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_bin2_dev(px, 32, 3, 4, px + 16, 8, 1, nullptr) != MLVFS_AMD_ERR_ARG)
        return fail("a refusal of bin2_dev did not happen", rec);
    printf("proxy_host_check: %d headers\n", rec);
    return rec > 0 ? 0 : 1;
}
