// flat_host_check.cpp -- a stand-alone host program for tests/test_flat_host.py: planes and the gain planes numpy expects, read from
// the file named on the command line, through mlvfs_amd_flat_create / _info / _gain / _destroy and their refusals.  It is compiled
// and linked with -fsanitize=address,undefined against the sanitizer build of the library's host code (`make -C mlvfs_amd/csrc
// hostcheck`) and run directly: no Python, no preloaded runtime, no HIP device.
//
// The file: records of {int32 w, h, bpp, black_f; uint32 means[4]; uint16 plane[w * h]; uint16 gain[w * h]}.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "flat_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: flat_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int rec = 0;
    for (;; rec++) {
        int32_t head[4];
        uint32_t means[4];
        if (fread(head, sizeof head, 1, f) != 1) break;
        if (fread(means, sizeof means, 1, f) != 1) return fail("short file", rec);
        const size_t npix = (size_t)head[0] * (size_t)head[1];
        // exactly npix entries each: a read or write one past the plane is the sanitizer's to see
        std::vector<uint16_t> plane(npix), want(npix), got(npix);
        if (fread(plane.data(), 2, npix, f) != npix || fread(want.data(), 2, npix, f) != npix) return fail("short file", rec);
        const mlvfs_amd_geom_t geom = { head[0], head[1], head[2], head[3], 0, 0, 0 };
        mlvfs_amd_flat_t *flat = mlvfs_amd_flat_create(&geom, plane.data());
        if (!flat) return fail("flat_create refused", rec);
        mlvfs_amd_geom_t back;
        int averaged = -1;
        uint32_t m[4];
        if (mlvfs_amd_flat_info(flat, &back, &averaged, m) != MLVFS_AMD_OK) return fail("flat_info", rec);
        if (back.width != head[0] || back.height != head[1] || back.bpp != head[2] || back.black != head[3] || averaged != 0) return fail("flat_info: other geometry", rec);
        if (memcmp(m, means, sizeof m)) return fail("other channel means", rec);
        if (npix > 0 && mlvfs_amd_flat_gain(flat, got.data(), npix - 1) != MLVFS_AMD_ERR_ARG) return fail("a cap one too small was taken", rec);
        if (mlvfs_amd_flat_gain(flat, got.data(), npix) != MLVFS_AMD_OK) return fail("flat_gain", rec);
        if (memcmp(got.data(), want.data(), npix * 2)) return fail("another gain plane", rec);
        mlvfs_amd_flat_destroy(flat);
    }
    fclose(f);
    // the refusals follow no pointer
    const uint16_t one = 5000;
    const mlvfs_amd_geom_t ok = { 1, 1, 14, 2048, 0, 0, 0 }, wide = { 1 << 14, 1 << 13, 14, 2048, 0, 0, 0 }, deep = { 1, 1, 17, 2048, 0, 0, 0 },
                           low = { 1, 1, 14, -1, 0, 0, 0 };
    if (mlvfs_amd_flat_create(nullptr, &one) || mlvfs_amd_flat_create(&ok, nullptr) || mlvfs_amd_flat_create(&wide, &one) ||
        mlvfs_amd_flat_create(&deep, &one) || mlvfs_amd_flat_create(&low, &one))
        return fail("a refusal did not happen", rec);
    mlvfs_amd_flat_destroy(nullptr);
    printf("flat_host_check: %d planes\n", rec);
    return rec > 0 ? 0 : 1;
}
