"""ctypes binding of libmlvfs_amd.so (include/mlvfs_amd.h).

The library is the product: if it is missing this module raises -- there is no
Python/CPU fallback.  `build()` compiles it in-tree with hipcc for gfx950.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(HERE, "libmlvfs_amd.so")

OK = 0
ERR_HIP, ERR_ARG, ERR_LUT, ERR_NOMEM, ERR_IO = -1, -2, -3, -4, -5
MLV_PLAIN, MLV_LJ92 = 0, 1          # MLVFS_AMD_MLV_*: payload kinds mlvfs_amd_mlv_transcode writes


class Geom(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bpp", C.c_int32), ("black", C.c_int32),
                ("white", C.c_int32), ("pan_x", C.c_int32), ("pan_y", C.c_int32)]


class MountOpts(C.Structure):
    """mlvfs_amd_mount_opts_t (include/mlvfs_amd.h)"""
    _fields_ = [("chroma_smooth", C.c_int32), ("fix_bad_pixels", C.c_int32), ("fix_stripes", C.c_int32), ("dual_iso", C.c_int32),
                ("hdr_interpolation_method", C.c_int32), ("hdr_no_fullres", C.c_int32), ("hdr_no_alias_map", C.c_int32),
                ("deflicker", C.c_int32), ("fix_pattern_noise", C.c_int32), ("rand_mode", C.c_int32), ("fps", C.c_double)]


class TensorSpec(C.Structure):
    """mlvfs_amd_tensor_spec_t (include/mlvfs_amd.h; mlvfs_amd/tensor.py has the constants)"""
    _fields_ = [("kind", C.c_int32), ("size", C.c_int32), ("ow", C.c_int32), ("oh", C.c_int32), ("gain_q8", C.c_int32), ("dtype", C.c_int32),
                ("layout", C.c_int32), ("reserved", C.c_int32), ("look16", C.c_void_p), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


# every symbol include/mlvfs_amd.h declares (tests/test_cabi.py checks the export table against the header)
DROPIN_SYMBOLS = [
    "dng_get_image_data", "dng_get_header_data", "dng_get_header_size", "dng_get_image_size", "dng_get_size",
    "chroma_smooth", "fix_bad_pixels", "fix_focus_pixels", "free_focus_pixel_maps",
    "stripes_get_correction", "stripes_new_correction", "stripes_free_corrections",
    "stripes_compute_correction", "stripes_apply_correction",
    "hdr_convert_data", "cr2hdr20_convert_data", "fix_pattern_noise",
    "hist_create", "hist_add", "hist_median", "hist_destroy", "lj92_open", "lj92_decode", "lj92_close", "lj92_encode", "gif_get_data", "gif_get_size",
]
DEVICE_SYMBOLS = [
    "mlvfs_amd_device_count", "mlvfs_amd_device_pci_bus_id", "mlvfs_amd_thread_device", "mlvfs_amd_init", "mlvfs_amd_last_error", "mlvfs_amd_version",
    "mlvfs_amd_clip_create", "mlvfs_amd_clip_destroy", "mlvfs_amd_clip_set_stripes", "mlvfs_amd_clip_get_stripes",
    "mlvfs_amd_clip_set_pixel_map", "mlvfs_amd_clip_get_pixel_map", "mlvfs_amd_clip_set_t16_layout", "mlvfs_amd_clip_get_t16_layout",
    "mlvfs_amd_unpack_dev", "mlvfs_amd_chroma_smooth_dev", "mlvfs_amd_detect_bad_pixels_dev",
    "mlvfs_amd_fix_pixels_dev", "mlvfs_amd_stripes_count_dev", "mlvfs_amd_stripes_hist_dev",
    "mlvfs_amd_stripes_solve", "mlvfs_amd_stripes_compute_dev", "mlvfs_amd_stripes_apply_dev",
    "mlvfs_amd_rand_stream", "mlvfs_amd_rand_stream_dev", "mlvfs_amd_process_frames_dev", "mlvfs_amd_process_frames_host",
    "mlvfs_amd_host_alloc", "mlvfs_amd_host_free", "mlvfs_amd_host_owns", "mlvfs_amd_host_size", "mlvfs_amd_host_knows", "mlvfs_amd_host_trim", "mlvfs_amd_hdr_preview_dev",
    "mlvfs_amd_cr2hdr20_dev", "mlvfs_amd_cr2hdr20_batch_dev", "mlvfs_amd_dualiso_reset", "mlvfs_amd_dualiso_trim", "mlvfs_amd_dualiso_last_scalars", "mlvfs_amd_amaze_demosaic_dev", "mlvfs_amd_amaze_debug", "mlvfs_amd_amaze_rows_extent", "mlvfs_amd_amaze_rows_extra_mode",
    "mlvfs_amd_timer_begin", "mlvfs_amd_timer_end", "mlvfs_amd_selftest_host", "mlvfs_amd_selftest_tables", "mlvfs_amd_test_median_net", "mlvfs_amd_frame_begin", "mlvfs_amd_frame_end", "mlvfs_amd_frame_sync", "mlvfs_amd_dropin_stats", "mlvfs_amd_test_fail_next", "mlvfs_amd_dropin_transfers", "mlvfs_amd_dropin_profile",
    "mlvfs_amd_mlv_open", "mlvfs_amd_mlv_close", "mlvfs_amd_mlv_frame_count", "mlvfs_amd_mlv_chunk_count",
    "mlvfs_amd_mlv_xref", "mlvfs_amd_mlv_frame_headers", "mlvfs_amd_mlv_read_frames", "mlvfs_amd_mlv_process", "mlvfs_amd_mlv_process_dualiso",
    "mlvfs_amd_lj92_info", "mlvfs_amd_lj92_decode_dev", "mlvfs_amd_lj92_decode_untiled", "mlvfs_amd_lj92_encode_table", "mlvfs_amd_test_rand_layout", "mlvfs_amd_test_device_order", "mlvfs_amd_test_stream_plan", "mlvfs_amd_test_lj92_row_plan", "mlvfs_amd_test_lj92_encode_plan", "mlvfs_amd_test_frame_plan", "mlvfs_amd_test_last_frame_plan", "mlvfs_amd_test_stream_listed", "mlvfs_amd_test_dualiso_parts", "mlvfs_amd_lzma_uncompress",
    "mlvfs_amd_gif_size", "mlvfs_amd_gif_render", "mlvfs_amd_mlv_gif_data", "mlvfs_amd_process_unpacked_dev", "mlvfs_amd_deflicker_dev",
    "mlvfs_amd_fix_pattern_noise_dev", "mlvfs_amd_test_pn_scratch_cap", "mlvfs_amd_deflicker_batch_dev", "mlvfs_amd_hdr_preview_batch_dev",
    "mlvfs_amd_mount_open", "mlvfs_amd_mount_dng", "mlvfs_amd_mount_close",
    "mlvfs_amd_lj92_encode_batch_dev", "mlvfs_amd_dng_header_lossless", "mlvfs_amd_mount_dng_lossless",
    "mlvfs_amd_lj92_tile_dev", "mlvfs_amd_pack_dev", "mlvfs_amd_mlv_transcode",
    "mlvfs_amd_dark_create", "mlvfs_amd_dark_from_clip", "mlvfs_amd_dark_info", "mlvfs_amd_dark_plane", "mlvfs_amd_dark_destroy",
    "mlvfs_amd_dark_subtract_dev", "mlvfs_amd_mount_set_dark", "mlvfs_amd_mlv_transcode_dark",
    "mlvfs_amd_rawi_set_bits", "mlvfs_amd_repack_dev", "mlvfs_amd_mlv_transcode_bits",
    "mlvfs_amd_flat_create", "mlvfs_amd_flat_from_clip", "mlvfs_amd_flat_info", "mlvfs_amd_flat_gain", "mlvfs_amd_flat_destroy",
    "mlvfs_amd_flat_apply_dev", "mlvfs_amd_mount_set_flat", "mlvfs_amd_mlv_transcode_cal",
    "mlvfs_amd_proxy_geom", "mlvfs_amd_bin2_dev", "mlvfs_amd_dng_header_proxy", "mlvfs_amd_mount_set_proxy", "mlvfs_amd_mount_dng_size",
    "mlvfs_amd_rgb_geom", "mlvfs_amd_rgb_header_size", "mlvfs_amd_rgb_lut", "mlvfs_amd_rgb_params", "mlvfs_amd_rgb_header",
    "mlvfs_amd_render2_dev", "mlvfs_amd_mount_rgb", "mlvfs_amd_mount_rgb_size",
    "mlvfs_amd_jpeg_header_size", "mlvfs_amd_jpeg_header", "mlvfs_amd_jpeg_qtables", "mlvfs_amd_jpeg_scratch_bytes",
    "mlvfs_amd_jpeg_encode_dev", "mlvfs_amd_mount_jpeg",
    "mlvfs_amd_rgb_full_geom", "mlvfs_amd_render1_dev", "mlvfs_amd_mount_rgb_full", "mlvfs_amd_mount_jpeg_full", "mlvfs_amd_mount_rgb_full_size",
    "mlvfs_amd_rgb_fit", "mlvfs_amd_render_scaled_dev", "mlvfs_amd_mount_rgb_scaled", "mlvfs_amd_mount_jpeg_scaled",
    "mlvfs_amd_mount_rgb_scaled_size", "mlvfs_amd_test_scale_div", "mlvfs_amd_test_scale_plan",
    "mlvfs_amd_look_image_size", "mlvfs_amd_look_pack", "mlvfs_amd_look_create", "mlvfs_amd_look_destroy", "mlvfs_amd_look_apply_dev",
    "mlvfs_amd_render2_look_dev", "mlvfs_amd_render1_look_dev", "mlvfs_amd_render_scaled_look_dev", "mlvfs_amd_mount_set_look",
    "mlvfs_amd_look16_image_size", "mlvfs_amd_look16_pack", "mlvfs_amd_look16_create", "mlvfs_amd_look16_destroy", "mlvfs_amd_look16_apply_dev",
    "mlvfs_amd_rgb16_header", "mlvfs_amd_render2_deep_dev", "mlvfs_amd_render1_deep_dev", "mlvfs_amd_render_scaled_deep_dev",
    "mlvfs_amd_mount_rgb16", "mlvfs_amd_mount_rgb16_full", "mlvfs_amd_mount_rgb16_scaled",
    "mlvfs_amd_mount_rgb16_size", "mlvfs_amd_mount_rgb16_full_size", "mlvfs_amd_mount_rgb16_scaled_size",
    "mlvfs_amd_rgb_fit_full", "mlvfs_amd_render_resampled_dev", "mlvfs_amd_render_resampled_look_dev", "mlvfs_amd_render_resampled_deep_dev",
    "mlvfs_amd_mount_rgb_resampled", "mlvfs_amd_mount_jpeg_resampled", "mlvfs_amd_mount_rgb16_resampled",
    "mlvfs_amd_mount_rgb_resampled_size", "mlvfs_amd_mount_rgb16_resampled_size", "mlvfs_amd_test_resample_plan",
    "mlvfs_amd_rgb_amaze_geom", "mlvfs_amd_amaze_balance_dev", "mlvfs_amd_amaze_tone_dev", "mlvfs_amd_render1_amaze_dev",
    "mlvfs_amd_render1_amaze_look_dev", "mlvfs_amd_render1_amaze_deep_dev", "mlvfs_amd_mount_set_demosaic", "mlvfs_amd_test_amaze_render_plan",
    "mlvfs_amd_rgb_amaze_resample_geom", "mlvfs_amd_amaze_resample_dev", "mlvfs_amd_render_resampled_amaze_dev",
    "mlvfs_amd_render_resampled_amaze_look_dev", "mlvfs_amd_render_resampled_amaze_deep_dev", "mlvfs_amd_mount_set_resample_demosaic",
    "mlvfs_amd_test_amz_resample_plan",
    "mlvfs_amd_jpeg_header_sampled", "mlvfs_amd_jpeg_scratch_bytes_sampled", "mlvfs_amd_jpeg_mcus", "mlvfs_amd_jpeg_encode_sampled_dev",
    "mlvfs_amd_mount_set_jpeg_sampling",
    "mlvfs_amd_tensor_rgb_dev", "mlvfs_amd_tensor_bayer_params", "mlvfs_amd_tensor_bayer_dev", "mlvfs_amd_mount_tensor", "mlvfs_amd_mount_tensor_bytes",
]


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into mlvfs_amd/libmlvfs_amd.so."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc"), "-j8"]
    res = subprocess.run(cmd, capture_output=not verbose, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libmlvfs_amd.so failed:\n" + (res.stdout or "") + (res.stderr or ""))
    return SO_PATH


_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # MLVFS_AMD_LIB: another build of the same library -- the sanitizer build of the host-only code (`make -C mlvfs_amd/csrc
    # hostcheck`, tests/test_hostcheck.py); never set by the tests proper or by bench.py
    so_path = os.environ.get("MLVFS_AMD_LIB") or SO_PATH
    if not os.path.exists(so_path):
        raise FileNotFoundError(
            f"{so_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(mlvfs_amd has no CPU fallback)")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.  If our
    # library pulled in /opt/rocm's copy first, torch (imported later for device memory and
    # streams) would bring up a second runtime that sees no GPU.  Importing torch first makes
    # the dynamic linker resolve our DT_NEEDED libamdhip64.so.* to the copy already loaded.
    # (A C host such as MLVFS has no torch and simply uses the system runtime.)
    if not os.environ.get("MLVFS_AMD_LIB"):
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the drop-in symbols
            pass
    L = C.CDLL(so_path)
    vp, sz, i, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_int64
    gp = C.POINTER(Geom)
    fhp = C.POINTER(abi.FrameHeaders)
    scp = C.POINTER(abi.StripesCorrection)

    def sig(name, res, args):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args

    # drop-in symbols
    sig("dng_get_image_data", sz, [fhp, vp, vp, C.c_long, sz])
    sig("dng_get_header_data", sz, [fhp, vp, C.c_long, sz, C.c_double, C.c_char_p])
    sig("dng_get_header_size", sz, [])
    sig("dng_get_image_size", sz, [fhp])
    sig("dng_get_size", sz, [fhp])
    sig("chroma_smooth", None, [fhp, vp, i])
    sig("fix_bad_pixels", None, [fhp, vp, i, i])
    sig("fix_focus_pixels", None, [fhp, vp, i])
    sig("free_focus_pixel_maps", None, [])
    sig("stripes_get_correction", scp, [C.c_char_p])
    sig("stripes_new_correction", scp, [C.c_char_p])
    sig("stripes_free_corrections", None, [])
    sig("stripes_compute_correction", None, [fhp, scp, vp, C.c_long, sz])
    sig("stripes_apply_correction", None, [fhp, scp, vp, C.c_long, sz])
    sig("hdr_convert_data", i, [fhp, vp, C.c_long, sz])
    sig("cr2hdr20_convert_data", i, [fhp, vp, i, i, i, i, i])
    sig("fix_pattern_noise", None, [vp, i, i, i, i])
    sig("lj92_open", i, [C.POINTER(vp), vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)])
    sig("lj92_close", None, [vp])
    sig("gif_get_size", sz, [fhp])
    sig("gif_get_data", sz, [C.c_char_p, vp, C.c_long, sz])
    sig("lj92_decode", i, [vp, vp, i, i, vp, i])
    sig("hist_create", vp, [C.c_uint16])
    sig("hist_add", None, [vp, vp, C.c_uint32, C.c_uint16])
    sig("hist_median", C.c_uint16, [vp])
    sig("hist_destroy", None, [vp])
    # device API
    sig("mlvfs_amd_device_count", i, [])
    sig("mlvfs_amd_device_pci_bus_id", i, [i, C.c_char_p, i])
    sig("mlvfs_amd_thread_device", i, [])
    sig("mlvfs_amd_init", i, [i])
    sig("mlvfs_amd_last_error", C.c_char_p, [])
    sig("mlvfs_amd_version", C.c_char_p, [])
    sig("mlvfs_amd_clip_create", vp, [gp])
    sig("mlvfs_amd_clip_destroy", None, [vp])
    sig("mlvfs_amd_clip_set_stripes", i, [vp, i, vp])
    sig("mlvfs_amd_clip_get_stripes", i, [vp, C.POINTER(i), vp])
    sig("mlvfs_amd_clip_set_t16_layout", i, [vp, i])
    sig("mlvfs_amd_clip_get_t16_layout", i, [vp])
    sig("mlvfs_amd_clip_set_pixel_map", i, [vp, vp, sz, i, i])
    sig("mlvfs_amd_clip_get_pixel_map", sz, [vp, vp, sz])
    sig("mlvfs_amd_unpack_dev", i, [gp, vp, sz, vp, sz, i, vp])
    sig("mlvfs_amd_chroma_smooth_dev", i, [gp, vp, vp, sz, i, i, vp])
    sig("mlvfs_amd_detect_bad_pixels_dev", i, [vp, vp, i, vp])
    sig("mlvfs_amd_fix_pixels_dev", i, [vp, vp, sz, i, vp])
    sig("mlvfs_amd_stripes_count_dev", i, [gp, vp, i, i, C.POINTER(i64), vp])
    sig("mlvfs_amd_stripes_hist_dev", i, [gp, vp, i, i, vp, i64, vp, vp, vp])
    sig("mlvfs_amd_stripes_solve", i, [vp, vp, i, vp])
    sig("mlvfs_amd_stripes_compute_dev", i, [vp, vp, i, i, vp])
    sig("mlvfs_amd_stripes_apply_dev", i, [vp, vp, sz, i, vp])
    sig("mlvfs_amd_rand_stream", None, [vp, sz, C.c_uint64, C.c_uint])
    sig("mlvfs_amd_rand_stream_dev", i, [vp, sz, C.c_uint64, C.c_uint, vp])
    sig("mlvfs_amd_process_frames_dev", i, [vp, vp, sz, vp, sz, i, i, i, i, vp])
    sig("mlvfs_amd_process_frames_host", i, [vp, vp, sz, vp, sz, i, i, i, i, i])
    sig("mlvfs_amd_host_alloc", vp, [sz])
    sig("mlvfs_amd_host_free", None, [vp])
    sig("mlvfs_amd_host_owns", i, [vp, sz])
    sig("mlvfs_amd_host_size", sz, [vp])
    sig("mlvfs_amd_host_knows", i, [vp])
    sig("mlvfs_amd_host_trim", sz, [])
    sig("mlvfs_amd_hdr_preview_dev", i, [gp, vp, sz, vp])
    sig("mlvfs_amd_cr2hdr20_dev", i, [gp, vp, i, i, i, i, vp])
    sig("mlvfs_amd_cr2hdr20_batch_dev", i, [gp, vp, sz, i, i, i, i, i, vp, vp])
    sig("mlvfs_amd_dualiso_reset", None, [])
    sig("mlvfs_amd_dualiso_trim", None, [])
    sig("mlvfs_amd_dualiso_last_scalars", None, [vp])
    sig("mlvfs_amd_amaze_demosaic_dev", i, [vp, i, i, vp, vp, vp, vp])
    sig("mlvfs_amd_amaze_rows_extent", None, [i, i, C.POINTER(C.c_int), C.POINTER(C.c_int)])
    sig("mlvfs_amd_amaze_rows_extra_mode", i, [i, i, i, C.POINTER(C.c_int)])
    sig("mlvfs_amd_amaze_debug", i, [vp, i, i, vp, vp, vp, i, vp, sz, C.POINTER(C.c_int), C.POINTER(C.c_int)])
    sig("mlvfs_amd_timer_begin", i, [i])
    sig("mlvfs_amd_timer_end", i, [vp, i])
    sig("mlvfs_amd_selftest_host", i, [])
    sig("mlvfs_amd_selftest_tables", i, [vp, vp])
    sig("mlvfs_amd_test_median_net", i, [i, i, vp, vp])
    sig("mlvfs_amd_frame_begin", i, [])
    sig("mlvfs_amd_frame_end", i, [])
    sig("mlvfs_amd_frame_sync", i, [vp])
    sig("mlvfs_amd_dropin_stats", None, [vp])
    sig("mlvfs_amd_test_fail_next", None, [C.c_int])
    sig("mlvfs_amd_test_device_order", i, [vp, i, i, vp])
    sig("mlvfs_amd_test_stream_plan", i, [i, i, i, vp, vp, vp, vp])
    sig("mlvfs_amd_test_lj92_row_plan", i, [i, i, vp])
    sig("mlvfs_amd_test_lj92_encode_plan", i, [C.c_longlong, vp])
    sig("mlvfs_amd_test_frame_plan", i, [vp, vp])
    sig("mlvfs_amd_test_last_frame_plan", i, [vp])
    sig("mlvfs_amd_test_stream_listed", i, [vp, vp])
    sig("mlvfs_amd_test_dualiso_parts", i, [i, i, i, vp, i, vp])
    sig("mlvfs_amd_dropin_transfers", None, [vp])
    sig("mlvfs_amd_dropin_profile", None, [vp])
    sig("mlvfs_amd_process_unpacked_dev", i, [vp, vp, sz, vp, sz, i, i, i, i, vp])
    sig("mlvfs_amd_deflicker_dev", i, [gp, vp, sz, i, vp, vp])
    sig("mlvfs_amd_lzma_uncompress", i, [vp, sz, vp, sz, C.POINTER(sz)])
    sig("mlvfs_amd_gif_size", sz, [fhp])
    sig("mlvfs_amd_gif_render", i, [gp, vp, sz, i, i, vp])
    sig("mlvfs_amd_mlv_gif_data", sz, [vp, vp, C.c_long, sz])
    sig("mlvfs_amd_lj92_info", i, [vp, sz, vp])
    sig("mlvfs_amd_lj92_decode_dev", i, [vp, vp, i, i, i, vp, sz, vp])
    sig("mlvfs_amd_mlv_open", vp, [C.c_char_p, i])
    sig("mlvfs_amd_mlv_close", None, [vp])
    sig("mlvfs_amd_mlv_frame_count", i, [vp])
    sig("mlvfs_amd_mlv_chunk_count", i, [vp])
    sig("mlvfs_amd_mlv_xref", sz, [vp, vp, sz])
    sig("mlvfs_amd_mlv_frame_headers", i, [vp, i, fhp])
    sig("mlvfs_amd_mlv_read_frames", i, [vp, i, i, vp, sz, i])
    sig("mlvfs_amd_mlv_process", i, [vp, vp, i, i, vp, sz, i, i, i, i, i])
    sig("mlvfs_amd_mlv_process_dualiso", i, [vp, i, i, vp, sz, i, i, i, i, i, i, vp])
    sig("mlvfs_amd_fix_pattern_noise_dev", i, [gp, vp, sz, i, vp])
    sig("mlvfs_amd_test_pn_scratch_cap", sz, [sz])
    sig("mlvfs_amd_deflicker_batch_dev", i, [gp, vp, sz, i, sz, i, vp, vp])
    sig("mlvfs_amd_hdr_preview_batch_dev", i, [gp, vp, sz, i, sz, vp, vp])
    sig("mlvfs_amd_mount_open", vp, [vp, C.POINTER(MountOpts), C.c_char_p])
    sig("mlvfs_amd_mount_dng", i, [vp, i, i, vp, sz, i, i, vp])
    sig("mlvfs_amd_mount_close", None, [vp])
    sig("mlvfs_amd_lj92_encode_batch_dev", i, [vp, sz, i, i, i, i, vp, sz, vp, vp, vp, vp])
    sig("mlvfs_amd_dng_header_lossless", sz, [fhp, vp, C.c_long, sz, C.c_double, C.c_char_p, C.c_uint32])
    sig("mlvfs_amd_mount_dng_lossless", i, [vp, i, i, vp, sz, vp, vp, i, i, vp])
    sig("mlvfs_amd_lj92_tile_dev", i, [vp, sz, vp, sz, i, i, i, vp])
    sig("mlvfs_amd_pack_dev", i, [gp, vp, sz, vp, sz, i, vp])
    sig("mlvfs_amd_mlv_transcode", i, [vp, C.c_char_p, i, i, i, C.POINTER(C.c_longlong)])
    sig("mlvfs_amd_dark_create", vp, [gp, vp])
    sig("mlvfs_amd_dark_from_clip", vp, [vp, i, i, i, i])
    sig("mlvfs_amd_dark_info", i, [vp, gp, C.POINTER(i)])
    sig("mlvfs_amd_dark_plane", i, [vp, vp, sz])
    sig("mlvfs_amd_dark_destroy", None, [vp])
    sig("mlvfs_amd_dark_subtract_dev", i, [vp, gp, vp, sz, i, vp])
    sig("mlvfs_amd_mount_set_dark", i, [vp, vp])
    sig("mlvfs_amd_mlv_transcode_dark", i, [vp, C.c_char_p, i, vp, i, i, C.POINTER(C.c_longlong)])
    sig("mlvfs_amd_rawi_set_bits", i, [vp, i])
    sig("mlvfs_amd_repack_dev", i, [gp, i, vp, vp, sz, vp, sz, i, vp])
    sig("mlvfs_amd_mlv_transcode_bits", i, [vp, C.c_char_p, i, i, vp, i, i, C.POINTER(C.c_longlong)])
    sig("mlvfs_amd_flat_create", vp, [gp, vp])
    sig("mlvfs_amd_flat_from_clip", vp, [vp, i, i, vp, i, i])
    sig("mlvfs_amd_flat_info", i, [vp, gp, C.POINTER(i), vp])
    sig("mlvfs_amd_flat_gain", i, [vp, vp, sz])
    sig("mlvfs_amd_flat_destroy", None, [vp])
    sig("mlvfs_amd_flat_apply_dev", i, [vp, vp, gp, vp, sz, i, vp])
    sig("mlvfs_amd_mount_set_flat", i, [vp, vp])
    sig("mlvfs_amd_mlv_transcode_cal", i, [vp, C.c_char_p, i, i, vp, vp, i, i, C.POINTER(C.c_longlong)])
    sig("mlvfs_amd_proxy_geom", i, [i, i, i, C.POINTER(i), C.POINTER(i)])
    sig("mlvfs_amd_bin2_dev", i, [vp, sz, i, i, vp, sz, i, vp])
    sig("mlvfs_amd_dng_header_proxy", sz, [fhp, vp, C.c_long, sz, C.c_double, C.c_char_p, i, C.c_uint32])
    sig("mlvfs_amd_mount_set_proxy", i, [vp, i])
    sig("mlvfs_amd_mount_dng_size", sz, [vp, i])
    sig("mlvfs_amd_rgb_geom", i, [i, i, C.POINTER(i), C.POINTER(i)])
    sig("mlvfs_amd_rgb_header_size", sz, [])
    sig("mlvfs_amd_rgb_lut", i, [vp])
    sig("mlvfs_amd_rgb_params", i, [fhp, i, vp])
    sig("mlvfs_amd_rgb_header", sz, [i, i, vp, sz])
    sig("mlvfs_amd_render2_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp])
    sig("mlvfs_amd_mount_rgb", i, [vp, i, i, vp, sz, i, i, i, vp])
    sig("mlvfs_amd_mount_rgb_size", sz, [vp, i])
    sig("mlvfs_amd_jpeg_header_size", sz, [])
    sig("mlvfs_amd_jpeg_header", sz, [i, i, i, vp, sz])
    sig("mlvfs_amd_jpeg_qtables", i, [i, vp])
    sig("mlvfs_amd_jpeg_scratch_bytes", sz, [i, i, i])
    sig("mlvfs_amd_jpeg_encode_dev", i, [vp, sz, i, i, i, vp, sz, sz, vp, sz, vp, vp, i, vp])
    sig("mlvfs_amd_mount_jpeg", i, [vp, i, i, vp, sz, i, i, vp, vp, i, i, vp])
    sig("mlvfs_amd_jpeg_header_sampled", sz, [i, i, i, i, vp, sz])
    sig("mlvfs_amd_jpeg_scratch_bytes_sampled", sz, [i, i, i, i])
    sig("mlvfs_amd_jpeg_mcus", i, [i, i, i, vp, vp])
    sig("mlvfs_amd_jpeg_encode_sampled_dev", i, [vp, sz, i, i, i, i, vp, sz, sz, vp, sz, vp, vp, i, vp])
    sig("mlvfs_amd_mount_set_jpeg_sampling", i, [vp, i])
    sig("mlvfs_amd_rgb_full_geom", i, [i, i, C.POINTER(i), C.POINTER(i)])
    sig("mlvfs_amd_render1_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp])
    sig("mlvfs_amd_mount_rgb_full", i, [vp, i, i, vp, sz, i, i, i, vp])
    sig("mlvfs_amd_mount_jpeg_full", i, [vp, i, i, vp, sz, i, i, vp, vp, i, i, vp])
    sig("mlvfs_amd_mount_rgb_full_size", sz, [vp, i])
    sig("mlvfs_amd_rgb_fit", i, [i, i, i, i, C.POINTER(i), C.POINTER(i)])
    sig("mlvfs_amd_render_scaled_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp])
    sig("mlvfs_amd_mount_rgb_scaled", i, [vp, i, i, vp, sz, i, i, i, i, i, vp])
    sig("mlvfs_amd_mount_jpeg_scaled", i, [vp, i, i, vp, sz, i, i, i, i, vp, vp, i, i, vp])
    sig("mlvfs_amd_mount_rgb_scaled_size", sz, [vp, i, i, i])
    sig("mlvfs_amd_test_scale_div", i, [C.c_uint32, i, vp, vp])
    sig("mlvfs_amd_test_scale_plan", i, [i, i, i, i, i, vp])
    sig("mlvfs_amd_look_image_size", sz, [i])
    sig("mlvfs_amd_look_pack", i, [vp, i, vp, vp, sz])
    sig("mlvfs_amd_look_create", vp, [vp, i, vp])
    sig("mlvfs_amd_look_destroy", None, [vp])
    sig("mlvfs_amd_look_apply_dev", i, [vp, vp, sz, vp, vp])
    sig("mlvfs_amd_render2_look_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp, vp])
    sig("mlvfs_amd_render1_look_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp, vp])
    sig("mlvfs_amd_render_scaled_look_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp, vp])
    sig("mlvfs_amd_mount_set_look", i, [vp, vp])
    sig("mlvfs_amd_look16_image_size", sz, [i])
    sig("mlvfs_amd_look16_pack", i, [vp, i, vp, vp, sz])
    sig("mlvfs_amd_look16_create", vp, [vp, i, vp])
    sig("mlvfs_amd_look16_destroy", None, [vp])
    sig("mlvfs_amd_look16_apply_dev", i, [vp, vp, sz, vp, vp])
    sig("mlvfs_amd_rgb16_header", sz, [i, i, vp, sz])
    sig("mlvfs_amd_render2_deep_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp, vp])
    sig("mlvfs_amd_render1_deep_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp, vp])
    sig("mlvfs_amd_render_scaled_deep_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp, vp])
    sig("mlvfs_amd_mount_rgb16", i, [vp, i, i, vp, sz, i, vp, i, i, vp])
    sig("mlvfs_amd_mount_rgb16_full", i, [vp, i, i, vp, sz, i, vp, i, i, vp])
    sig("mlvfs_amd_mount_rgb16_scaled", i, [vp, i, i, vp, sz, i, i, i, vp, i, i, vp])
    sig("mlvfs_amd_mount_rgb16_size", sz, [vp, i])
    sig("mlvfs_amd_mount_rgb16_full_size", sz, [vp, i])
    sig("mlvfs_amd_mount_rgb16_scaled_size", sz, [vp, i, i, i])
    sig("mlvfs_amd_rgb_fit_full", i, [i, i, i, i, C.POINTER(i), C.POINTER(i)])
    sig("mlvfs_amd_render_resampled_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp])
    sig("mlvfs_amd_render_resampled_look_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp, vp])
    sig("mlvfs_amd_render_resampled_deep_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp, vp])
    sig("mlvfs_amd_mount_rgb_resampled", i, [vp, i, i, vp, sz, i, i, i, i, i, vp])
    sig("mlvfs_amd_mount_jpeg_resampled", i, [vp, i, i, vp, sz, i, i, i, i, vp, vp, i, i, vp])
    sig("mlvfs_amd_mount_rgb16_resampled", i, [vp, i, i, vp, sz, i, i, i, vp, i, i, vp])
    sig("mlvfs_amd_mount_rgb_resampled_size", sz, [vp, i, i, i])
    sig("mlvfs_amd_mount_rgb16_resampled_size", sz, [vp, i, i, i])
    sig("mlvfs_amd_test_resample_plan", i, [i, i, i, i, i, vp])
    sig("mlvfs_amd_rgb_amaze_geom", i, [i, i, C.POINTER(i), C.POINTER(i)])
    sig("mlvfs_amd_amaze_balance_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp])
    sig("mlvfs_amd_amaze_tone_dev", i, [vp, vp, vp, sz, i, i, vp, vp, sz, i, vp, vp, vp])
    sig("mlvfs_amd_render1_amaze_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp])
    sig("mlvfs_amd_render1_amaze_look_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp, vp])
    sig("mlvfs_amd_render1_amaze_deep_dev", i, [vp, sz, i, i, vp, vp, sz, i, vp, vp])
    sig("mlvfs_amd_mount_set_demosaic", i, [vp, i])
    sig("mlvfs_amd_test_amaze_render_plan", i, [i, i, i, sz, vp])
    sig("mlvfs_amd_rgb_amaze_resample_geom", i, [i, i, i, i])
    sig("mlvfs_amd_amaze_resample_dev", i, [vp, vp, vp, sz, i, i, vp, i, i, vp, sz, i, vp, vp, vp])
    sig("mlvfs_amd_render_resampled_amaze_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp])
    sig("mlvfs_amd_render_resampled_amaze_look_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp, vp])
    sig("mlvfs_amd_render_resampled_amaze_deep_dev", i, [vp, sz, i, i, vp, i, i, vp, sz, i, vp, vp])
    sig("mlvfs_amd_mount_set_resample_demosaic", i, [vp, i])
    sig("mlvfs_amd_test_amz_resample_plan", i, [i, i, i, i, i, vp])
    tsp = C.POINTER(TensorSpec)
    sig("mlvfs_amd_tensor_rgb_dev", i, [vp, sz, i, i, i, tsp, vp, sz, i, vp])
    sig("mlvfs_amd_tensor_bayer_params", i, [fhp, vp])
    sig("mlvfs_amd_tensor_bayer_dev", i, [vp, sz, i, i, vp, tsp, vp, sz, i, vp])
    sig("mlvfs_amd_mount_tensor", i, [vp, i, i, vp, sz, tsp, i, i, vp])
    sig("mlvfs_amd_mount_tensor_bytes", sz, [vp, i, tsp])
    _lib = L
    return L


class MlvfsAmdError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        raise MlvfsAmdError(f"{what} failed ({rc}): {load().mlvfs_amd_last_error().decode()}")


def ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)
