// fused_pass.h -- the host side of the fused pass (k_pixfix + k_frame*), stated once: what one launch does to a run of frames of one
// geometry, the rules that switch its stages off, and the routine that runs it (fused_pass.cpp).
#pragma once

#include "clip.h"

namespace mlv {

// get_raw2ev() == NULL in the reference: above this black level there are no EV tables, and what needs them is skipped or refused
inline bool black_too_large(int black) { return black > 16384; }
// stripes.c:252, and the kernels' rows of whole 8-pixel groups
inline bool stripes_apply_to(bool asked, int needed, int w) { return asked && needed && w % 8 == 0; }

struct FusedPass {
    Geom g{};
    int src_bpp = 0;                  // 0: 16-bit frames; else the packed stream's bits per pixel
    int cs = 0;                       // chroma smoothing method (0: none)
    const Clip *map = nullptr;        // the clip whose pixel map is applied (read only), or none
    bool stripes = false;
    const int32_t *coef = nullptr;
    bool idle() const { return !map && !stripes && cs == 0; }
};

// the pass that frames of geometry g get for what the caller asks -- the three gating rules: no smoothing above the black level
// limit, a map (null: none asked for) only if it has entries, stripes only if the correction is needed and the width allows it
inline FusedPass fused_pass_of(const Geom &g, int src_bpp, int cs_method, const Clip *map, bool apply_stripes, int needed, const int32_t *coef)
{
    return FusedPass{ g, src_bpp, black_too_large(g.black) ? 0 : cs_method, map && map->n_entries > 0 ? map : nullptr,
                      stripes_apply_to(apply_stripes, needed, g.w), coef };
}
// ... of a clip that carries its own map and correction
inline FusedPass fused_pass_of(const Clip &clip, int src_bpp, int cs_method, bool fix_pixels, bool apply_stripes)
{
    return fused_pass_of(clip.g, src_bpp, cs_method, fix_pixels ? &clip : nullptr, apply_stripes, clip.needed, clip.coef);
}

// src -> dst on `stream`.  An idle pass unpacks (packed source) or copies (16-bit source); every other one repairs into `patches` where
// there is a map -- p.map->patch_buffer_bytes(nframes) bytes of the caller's --, then launches the fused kernel.  layout_of (callers
// that own their clip): its T16 layout is the launch's, decided between the two from the first frame when the pass smooths; else plain
int run_fused_pass(const Device *dev, const FusedPass &p, const void *src, size_t src_stride, void *dst, size_t dst_stride, int nframes,
                   void *patches, hipStream_t stream, Clip *layout_of = nullptr);

}  // namespace mlv
