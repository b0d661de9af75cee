// look.cpp -- a look for the rendered frames, the host side (include/mlvfs_amd.h, "a look for the rendered frames"; k_tone_dev.h;
// DESIGN.md 3.16): a shaper of 4096 uint16 and a cube of n^3 RGB triples of uint16, packed into the image the look kernels read --
//     [0, 8192)            S[4096], uint16
//     [8192, 8192 + 8 n^3) the entries in the table's order (red fastest), each R, G, B, 0 as uint16: one 64-bit load per vertex
// -- and a handle that packs, uploads once and owns the device copy.  The handle belongs to no mount.
// mlvfs_amd_look_image_size and mlvfs_amd_look_pack are host code: no HIP device is needed.
// A deep look (include/mlvfs_amd.h, "rendered frames at 16 bits") is the same with a shaper of 65536 uint16 on the 16-bit
// index -- [0, 131072) S16, then the entries -- and n = 0 for no table at all; mlvfs_amd_look16_*.
#include "clip.h"
#include "render_route.h"

#include <cstring>
#include <vector>

using namespace mlv;

struct mlvfs_amd_look {
    int n = 0;
    int device = -1;                                    // where the image lies
    DevBuf image;
};

struct mlvfs_amd_look16 {
    int n = 0;                                          // 0: no table
    int device = -1;
    DevBuf image;
};

int mlv::look16_on_device(const mlvfs_amd_look16_t *look, ThreadCtx *c, LookArg *out)
{
    if (look->device != c->dev->id) {
        set_error("look16: the look was created on device %d, the call runs on device %d", look->device, c->dev->id);
        return MLVFS_AMD_ERR_ARG;
    }
    *out = LookArg{ (const uint8_t *)look->image.p, (uint32_t)look->n };
    return MLVFS_AMD_OK;
}

int mlv::look_on_device(const mlvfs_amd_look_t *look, ThreadCtx *c, LookArg *out)
{
    if (look->device != c->dev->id) {
        set_error("look: the look was created on device %d, the call runs on device %d", look->device, c->dev->id);
        return MLVFS_AMD_ERR_ARG;
    }
    *out = LookArg{ (const uint8_t *)look->image.p, (uint32_t)look->n };
    return MLVFS_AMD_OK;
}

extern "C" {

size_t mlvfs_amd_look_image_size(int n)
{
    if (n < 2 || n > 65) { set_error("look_image_size: a table of %d a side (2 .. 65)", n); return 0; }
    return LOOK_SHAPER_BYTES + (size_t)8 * n * n * n;
}

int mlvfs_amd_look_pack(const uint16_t shaper[4096], int n, const uint16_t *table, void *image, size_t cap)
{
    if (!shaper || !table || !image) { set_error("look_pack: null argument"); return MLVFS_AMD_ERR_ARG; }
    const size_t size = mlvfs_amd_look_image_size(n);
    if (!size) { set_error("look_pack: a table of %d a side (2 .. 65)", n); return MLVFS_AMD_ERR_ARG; }
    if (cap < size) { set_error("look_pack: room for %zu bytes, the image has %zu", cap, size); return MLVFS_AMD_ERR_ARG; }
    uint8_t *at = (uint8_t *)image;
    memcpy(at, shaper, LOOK_SHAPER_BYTES);
    at += LOOK_SHAPER_BYTES;
    const size_t entries = (size_t)n * n * n;
    for (size_t k = 0; k < entries; k++, at += 8) {
        const uint16_t e[4] = { table[3 * k], table[3 * k + 1], table[3 * k + 2], 0 };
        memcpy(at, e, 8);
    }
    return MLVFS_AMD_OK;
}

mlvfs_amd_look_t *mlvfs_amd_look_create(const uint16_t shaper[4096], int n, const uint16_t *table)
{
    if (!shaper || !table) { set_error("look_create: null argument"); return nullptr; }
    const size_t size = mlvfs_amd_look_image_size(n);
    if (!size) { set_error("look_create: a table of %d a side (2 .. 65)", n); return nullptr; }
    try {
        std::vector<uint8_t> host(size);
        if (mlvfs_amd_look_pack(shaper, n, table, host.data(), host.size())) return nullptr;
        ThreadCtx *c = thread_ctx();
        if (!c) return nullptr;
        std::unique_ptr<mlvfs_amd_look> look(new mlvfs_amd_look);
        look->n = n;
        look->device = c->dev->id;
        if (look->image.reserve(size)) return nullptr;                          // the error is set, nothing is held
        const hipError_t e = hipMemcpy(look->image.p, host.data(), size, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("look_create: uploading the image -> %s", hipGetErrorString(e)); return nullptr; }
        return look.release();
    } catch (const std::exception &e) { set_error("look_create: %s", e.what()); return nullptr; }
}

void mlvfs_amd_look_destroy(mlvfs_amd_look_t *look) { delete look; }

int mlvfs_amd_look_apply_dev(const mlvfs_amd_look_t *look, const uint16_t *d_t, size_t n, uint8_t *d_out, void *stream)
{
    if (!look || !d_t || !d_out) { set_error("look_apply: null argument"); return MLVFS_AMD_ERR_ARG; }
    if ((uintptr_t)d_t & 1) { set_error("look_apply: indices at an odd address"); return MLVFS_AMD_ERR_ARG; }
    if (n > ((size_t)1 << 40)) { set_error("look_apply: %zu triples", n); return MLVFS_AMD_ERR_ARG; }
    if (n == 0) return MLVFS_AMD_OK;
    const uintptr_t a0 = (uintptr_t)d_t, a1 = a0 + n * 6, b0 = (uintptr_t)d_out, b1 = b0 + n * 3;
    if (a0 < b1 && b0 < a1) { set_error("look_apply: the destination overlaps the indices"); return MLVFS_AMD_ERR_ARG; }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    LookArg lk;
    if (const int rc = look_on_device(look, c, &lk)) return rc;
    return launch_look_apply(lk, d_t, n, d_out, pick_stream(stream, c));
}

size_t mlvfs_amd_look16_image_size(int n)
{
    if (n != 0 && (n < 2 || n > 65)) { set_error("look16_image_size: a table of %d a side (0, or 2 .. 65)", n); return 0; }
    return LOOK16_SHAPER_BYTES + (size_t)8 * n * n * n;
}

int mlvfs_amd_look16_pack(const uint16_t shaper[65536], int n, const uint16_t *table, void *image, size_t cap)
{
    if (!shaper || !image || (n != 0 && !table)) { set_error("look16_pack: null argument"); return MLVFS_AMD_ERR_ARG; }
    const size_t size = mlvfs_amd_look16_image_size(n);
    if (!size) { set_error("look16_pack: a table of %d a side (0, or 2 .. 65)", n); return MLVFS_AMD_ERR_ARG; }
    if (cap < size) { set_error("look16_pack: room for %zu bytes, the image has %zu", cap, size); return MLVFS_AMD_ERR_ARG; }
    uint8_t *at = (uint8_t *)image;
    memcpy(at, shaper, LOOK16_SHAPER_BYTES);
    at += LOOK16_SHAPER_BYTES;
    const size_t entries = (size_t)n * n * n;
    for (size_t k = 0; k < entries; k++, at += 8) {
        const uint16_t e[4] = { table[3 * k], table[3 * k + 1], table[3 * k + 2], 0 };
        memcpy(at, e, 8);
    }
    return MLVFS_AMD_OK;
}

mlvfs_amd_look16_t *mlvfs_amd_look16_create(const uint16_t shaper[65536], int n, const uint16_t *table)
{
    if (!shaper || (n != 0 && !table)) { set_error("look16_create: null argument"); return nullptr; }
    const size_t size = mlvfs_amd_look16_image_size(n);
    if (!size) { set_error("look16_create: a table of %d a side (0, or 2 .. 65)", n); return nullptr; }
    try {
        std::vector<uint8_t> host(size);
        if (mlvfs_amd_look16_pack(shaper, n, table, host.data(), host.size())) return nullptr;
        ThreadCtx *c = thread_ctx();
        if (!c) return nullptr;
        std::unique_ptr<mlvfs_amd_look16> look(new mlvfs_amd_look16);
        look->n = n;
        look->device = c->dev->id;
        if (look->image.reserve(size)) return nullptr;                          // the error is set, nothing is held
        const hipError_t e = hipMemcpy(look->image.p, host.data(), size, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("look16_create: uploading the image -> %s", hipGetErrorString(e)); return nullptr; }
        return look.release();
    } catch (const std::exception &e) { set_error("look16_create: %s", e.what()); return nullptr; }
}

void mlvfs_amd_look16_destroy(mlvfs_amd_look16_t *look) { delete look; }

int mlvfs_amd_look16_apply_dev(const mlvfs_amd_look16_t *look, const uint16_t *d_t, size_t n, uint16_t *d_out, void *stream)
{
    if (!look || !d_t || !d_out) { set_error("look16_apply: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (((uintptr_t)d_t | (uintptr_t)d_out) & 1) { set_error("look16_apply: indices or samples at an odd address"); return MLVFS_AMD_ERR_ARG; }
    if (n > ((size_t)1 << 40)) { set_error("look16_apply: %zu triples", n); return MLVFS_AMD_ERR_ARG; }
    if (n == 0) return MLVFS_AMD_OK;
    const uintptr_t a0 = (uintptr_t)d_t, a1 = a0 + n * 6, b0 = (uintptr_t)d_out, b1 = b0 + n * 6;
    if (a0 < b1 && b0 < a1) { set_error("look16_apply: the destination overlaps the indices"); return MLVFS_AMD_ERR_ARG; }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    LookArg lk;
    if (const int rc = look16_on_device(look, c, &lk)) return rc;
    return launch_look16_apply(lk, d_t, n, d_out, pick_stream(stream, c));
}

}  // extern "C"
