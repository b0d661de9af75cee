// jpeg_sampling_host_check.cpp -- a stand-alone host program for tests/test_jpeg_sampling_host.py: the host functions that take a chroma
// sampling (mlvfs_amd_jpeg_header_sampled, mlvfs_amd_jpeg_mcus, mlvfs_amd_jpeg_scratch_bytes_sampled) against the bytes and counts the
// definition of mlvfs_amd/jpeg.py expects, read from the file named on the command line; then the sizes and every refusal, those of
// mlvfs_amd_jpeg_encode_sampled_dev and mlvfs_amd_mount_set_jpeg_sampling included.  It is compiled and linked with
// -fsanitize=address,undefined against the sanitizer build of the library's host code (`make -C mlvfs_amd/csrc hostcheck`) and run
// directly: no Python, no preloaded runtime, no HIP device.
//
// The file: records of {uint32 kind; int32 a, b, c, d; ...}
//   kind 1: a = pw, b = ph, c = quality, d = sampling; the header's bytes expected (mlvfs_amd_jpeg_header_size() of them)
//   kind 2: a = pw, b = ph, d = sampling; then int32 mw, mh expected
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "mlvfs_amd.h"

static int fail(const char *what, int rec)
{
    fprintf(stderr, "jpeg_sampling_host_check: record %d: %s (%s)\n", rec, what, mlvfs_amd_last_error());
    return 1;
}

struct Head {
    uint32_t kind;
    int32_t a, b, c, d;
};

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: jpeg_sampling_host_check CASES.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const size_t hdr = mlvfs_amd_jpeg_header_size();
    if (hdr != 629) return fail("the header's size is not 629", -1);
    if (MLVFS_AMD_JPEG_420 != 0 || MLVFS_AMD_JPEG_422 != 1 || MLVFS_AMD_JPEG_444 != 2) return fail("the samplings' numbers", -1);
    int rec = 0;
    for (;; rec++) {
        Head hd;
        if (fread(&hd, sizeof hd, 1, f) != 1) break;
        if (hd.kind == 1) {
            // exactly the header's size: a write one past it is the sanitizer's to see
            std::unique_ptr<uint8_t[]> want(new uint8_t[hdr]), got(new uint8_t[hdr]);
            if (fread(want.get(), 1, hdr, f) != hdr) return fail("short file", rec);
            memset(got.get(), 0xA5, hdr);
            if (mlvfs_amd_jpeg_header_sampled(hd.a, hd.b, hd.c, hd.d, got.get(), hdr) != hdr) return fail("another size returned", rec);
            if (memcmp(got.get(), want.get(), hdr)) return fail("another header", rec);
            if (hd.d == MLVFS_AMD_JPEG_420) {
                memset(got.get(), 0xA5, hdr);
                if (mlvfs_amd_jpeg_header(hd.a, hd.b, hd.c, got.get(), hdr) != hdr || memcmp(got.get(), want.get(), hdr))
                    return fail("the call without a sampling is not 4:2:0", rec);
            }
        } else if (hd.kind == 2) {
            int32_t want[2];
            if (fread(want, sizeof want, 1, f) != 1) return fail("short file", rec);
            std::unique_ptr<int> mw(new int(-7)), mh(new int(-7));
            if (mlvfs_amd_jpeg_mcus(hd.a, hd.b, hd.d, mw.get(), mh.get()) != MLVFS_AMD_OK) return fail("jpeg_mcus refused", rec);
            if (*mw != want[0] || *mh != want[1]) return fail("another MCU grid", rec);
            // the scratch holds the coefficients at least, more with every frame, and no less than at a coarser sampling
            const size_t blocks = (size_t)*mw * *mh * (hd.d == 0 ? 6 : hd.d == 1 ? 4 : 3);
            const size_t s0 = mlvfs_amd_jpeg_scratch_bytes_sampled(hd.a, hd.b, hd.d, 0), s1 = mlvfs_amd_jpeg_scratch_bytes_sampled(hd.a, hd.b, hd.d, 1),
                         s2 = mlvfs_amd_jpeg_scratch_bytes_sampled(hd.a, hd.b, hd.d, 2), s3 = mlvfs_amd_jpeg_scratch_bytes_sampled(hd.a, hd.b, hd.d, 3);
            if (s0 != 0 || s1 < blocks * 128 || s2 <= s1 || s3 <= s2 || s3 - s2 != s2 - s1) return fail("the scratch does not grow with the frames", rec);
            if (hd.d == 0 && s2 != mlvfs_amd_jpeg_scratch_bytes(hd.a, hd.b, 2)) return fail("the scratch without a sampling is not 4:2:0's", rec);
        } else return fail("a record of an unknown kind", rec);
    }
    fclose(f);
    // the refusals, which follow no pointer and write nothing
    uint8_t one = 0xA5;
    for (int s = 0; s < 3; s++)
        if (mlvfs_amd_jpeg_header_sampled(4, 4, 90, s, &one, 1) != 0 || mlvfs_amd_jpeg_header_sampled(0, 4, 90, s, &one, 1) != 0 ||
            mlvfs_amd_jpeg_header_sampled(4, 4, 0, s, &one, 1) != 0 || mlvfs_amd_jpeg_header_sampled(4, 4, 101, s, &one, 1) != 0 ||
            mlvfs_amd_jpeg_header_sampled(65536, 1, 90, s, &one, 1) != 0 || mlvfs_amd_jpeg_header_sampled(4, 4, 90, s, nullptr, hdr) != 0 || one != 0xA5)
            return fail("a refusal of jpeg_header_sampled did not happen", rec);
    {
        std::unique_ptr<uint8_t[]> got(new uint8_t[hdr]);
        memset(got.get(), 0xA5, hdr);
        const int bad[] = { -1, 3, 4, 420, 422, 444, INT32_MIN, INT32_MAX };
        int mw = -7, mh = -7;
        for (int s : bad) {
            if (mlvfs_amd_jpeg_header_sampled(16, 16, 90, s, got.get(), hdr) != 0) return fail("jpeg_header_sampled took a sampling it does not have", rec);
            if (mlvfs_amd_jpeg_scratch_bytes_sampled(16, 16, s, 1) != 0) return fail("jpeg_scratch_bytes_sampled took a sampling it does not have", rec);
            if (mlvfs_amd_jpeg_mcus(16, 16, s, &mw, &mh) != MLVFS_AMD_ERR_ARG) return fail("jpeg_mcus took a sampling it does not have", rec);
        }
        for (size_t k = 0; k < hdr; k++) if (got[k] != 0xA5) return fail("a refused header was written", rec);
        if (mlvfs_amd_jpeg_mcus(0, 4, 2, &mw, &mh) != MLVFS_AMD_ERR_ARG || mlvfs_amd_jpeg_mcus(4, 65536, 2, &mw, &mh) != MLVFS_AMD_ERR_ARG ||
            mlvfs_amd_jpeg_mcus(8192, 4096, 2, &mw, &mh) != MLVFS_AMD_ERR_ARG || mlvfs_amd_jpeg_mcus(4, 4, 2, nullptr, &mh) != MLVFS_AMD_ERR_ARG ||
            mlvfs_amd_jpeg_mcus(4, 4, 2, &mw, nullptr) != MLVFS_AMD_ERR_ARG || mw != -7 || mh != -7)
            return fail("a refusal of jpeg_mcus did not happen", rec);
    }
    for (int s = 0; s < 3; s++) {
        if (mlvfs_amd_jpeg_scratch_bytes_sampled(0, 4, s, 1) != 0 || mlvfs_amd_jpeg_scratch_bytes_sampled(4, 4, s, -1) != 0 ||
            mlvfs_amd_jpeg_scratch_bytes_sampled(8192, 4096, s, 1) != 0)
            return fail("a refusal of jpeg_scratch_bytes_sampled did not happen", rec);
        // the largest input: nothing overflows on the way to its layout
        if (mlvfs_amd_jpeg_scratch_bytes_sampled(65535, 511, s, 65535) == 0 || mlvfs_amd_jpeg_scratch_bytes_sampled(1, 65535, s, 2) == 0 ||
            mlvfs_amd_jpeg_scratch_bytes_sampled(65535, 1, s, 2) == 0)
            return fail("the scratch of the largest input", rec);
    }
    // 4:4:4 has three bytes of coefficients per pixel where 4:2:0 has one and a half
    const size_t c420 = mlvfs_amd_jpeg_scratch_bytes_sampled(1792, 660, 0, 1), c422 = mlvfs_amd_jpeg_scratch_bytes_sampled(1792, 660, 1, 1),
                 c444 = mlvfs_amd_jpeg_scratch_bytes_sampled(1792, 660, 2, 1);
    if (!(c420 < c422 && c422 < c444) || c444 < (size_t)224 * 83 * 3 * 128 || 10 * c444 < 19 * c420 || c444 > 3 * c420) return fail("the scratch of 1792x660 per sampling", rec);
    uint8_t px[16 * 16 * 3] = { 0 }, out[64] = { 0 };
    uint32_t len[2] = { 7, 7 };
    int st[2] = { 7, 7 };
    alignas(16) uint8_t scratch[64];
    for (int s = 0; s < 3; s++)
        if (mlvfs_amd_jpeg_encode_sampled_dev(nullptr, 768, 16, 16, 90, s, out, 64, 64, scratch, 1 << 30, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
            mlvfs_amd_jpeg_encode_sampled_dev(px, 768, 16, 16, 90, s, out, 64, 64, scratch, 64, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
            mlvfs_amd_jpeg_encode_sampled_dev(px, 768, 16, 16, 0, s, out, 64, 64, scratch, 1 << 30, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
            mlvfs_amd_jpeg_encode_sampled_dev(px, 768, 16, 16, 90, s, out, 64, 64, scratch, 1 << 30, nullptr, st, 1, nullptr) != MLVFS_AMD_ERR_ARG)
            return fail("a refusal of jpeg_encode_sampled_dev did not happen", rec);
    if (mlvfs_amd_jpeg_encode_sampled_dev(px, 768, 16, 16, 90, 3, out, 64, 64, scratch, 1 << 30, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        mlvfs_amd_jpeg_encode_sampled_dev(px, 768, 16, 16, 90, -1, out, 64, 64, scratch, 1 << 30, len, st, 1, nullptr) != MLVFS_AMD_ERR_ARG ||
        len[0] != 7 || st[0] != 7)
        return fail("jpeg_encode_sampled_dev took a sampling it does not have", rec);
    if (mlvfs_amd_mount_set_jpeg_sampling(nullptr, 0) != MLVFS_AMD_ERR_ARG) return fail("mount_set_jpeg_sampling took a null handle", rec);
    printf("jpeg_sampling_host_check: %d records\n", rec);
    return rec > 0 ? 0 : 1;
}
