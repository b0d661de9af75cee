"""A clip served as MLVFS serves it, batch by batch (mlvfs_amd_mount_*, csrc/mount.cpp).

    with mlvfile.MlvReader(path) as r, Mount(r, MlvfsOptions(chroma_smooth=5, fix_pattern_noise=1), deflicker=3000,
                                              basename="/M07-1234.MLV") as m:
        files = m.dng(0, 16, batch=8)       # (16, dng_size) uint8: 65536 header bytes + pixels per frame

        small, flags = m.dng_lossless(16, 16)   # the same files with their pixels as one lossless-JPEG stream each

    Mount(r, opt, proxy=2) serves half-size Bayer proxies: the same frames after every stage, binned 2x2 within each CFA colour on the
    GPU (include/mlvfs_amd.h, "half-size Bayer proxies"), a quarter of the bytes per file.

    m.rgb(0, 16, gain=1.0) serves the same frames developed to 8-bit sRGB at half size, as TIFF files any viewer opens
    (include/mlvfs_amd.h, "rendered half-size sRGB frames"; mlvfs_amd/render.py is the definition in numpy).

    m.set_look(look.Look(S, n, T)) puts a shaper and a 3D table -- a .cube file -- in the place of the sRGB curve in every later rgb() and
    jpeg() call (include/mlvfs_amd.h, "a look for the rendered frames"; mlvfs_amd/look.py is the definition in numpy).

    m.rgb(0, 16, look16=look.Look16(S16, n, T)) serves them as 16-bit TIFF files toned from 16-bit linear light through a deep look that
    is passed per call (include/mlvfs_amd.h, "rendered frames at 16 bits").

    files, flags = m.jpeg(0, 16, gain=1.0, quality=90) serves the same renderings as baseline JPEG files encoded on the GPU, a tenth
    of the bytes (include/mlvfs_amd.h, "rendered frames as baseline JPEG files"; mlvfs_amd/jpeg.py is the definition in numpy).

    m.set_demosaic("amaze") makes the full-size calls demosaic with AMaZE instead of the linear filter (include/mlvfs_amd.h, "rendered
    full-size frames demosaiced by AMaZE"; mlvfs_amd/amaze_render.py is the definition).

    m.set_resample_demosaic("amaze") makes the resample=True calls demosaic with AMaZE (include/mlvfs_amd.h, "resampled rendered frames
    demosaiced by AMaZE"; mlvfs_amd/amaze_resample.py is the definition).

    t = m.tensor(0, 16, dtype=torch.float16, layout="NCHW") leaves the same renderings on the GPU as one (16, 3, h, w) torch tensor, and
    m.tensor(0, 16, kind="bayer") the frames themselves as four planes, black-subtracted and scaled by their own levels: nothing crosses
    the link (include/mlvfs_amd.h, "a clip's frames as device-resident tensors"; mlvfs_amd/tensor.py is the definition in numpy).

Successive calls on one Mount serve frames in call order, like one fresh MLVFS process serving .dng reads in that order.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, lib
from .pipeline import MlvfsOptions


def mount_opts(opt: MlvfsOptions, deflicker: int = 0, fps: float = 0.0, rand_mode: int = 1) -> lib.MountOpts:
    return lib.MountOpts(chroma_smooth=opt.chroma_smooth, fix_bad_pixels=opt.fix_bad_pixels, fix_stripes=opt.fix_stripes,
                         dual_iso=opt.dual_iso, hdr_interpolation_method=opt.hdr_interpolation_method,
                         hdr_no_fullres=opt.hdr_no_fullres, hdr_no_alias_map=opt.hdr_no_alias_map, deflicker=deflicker,
                         fix_pattern_noise=opt.fix_pattern_noise, rand_mode=rand_mode, fps=fps)


class Mount:
    """reader: an open mlvfile.MlvReader (or a raw mlvfs_amd_mlv_open handle); it must stay open while the Mount lives.
    dark: a mlvfs_amd.dark.Dark to subtract from every frame (stage 0), or None.
    flat: a mlvfs_amd.flat.Flat whose gain corrects every frame directly after that (stage 0b), or None.
    proxy: 1 full-size files, 2 half-size Bayer proxies (the last stage)."""

    def __init__(self, reader, opt: MlvfsOptions, deflicker: int = 0, fps: float = 0.0, basename: str = "", rand_mode: int = 1, dark=None,
                 flat=None, proxy: int = 1):
        self.L = lib.load()
        self._reader = reader
        handle = getattr(reader, "h", reader)
        self.opts = mount_opts(opt, deflicker, fps, rand_mode)
        self.h = self.L.mlvfs_amd_mount_open(handle, C.byref(self.opts), basename.encode())
        if not self.h:
            raise lib.MlvfsAmdError(self.L.mlvfs_amd_last_error().decode())
        self.frame_count = self.L.mlvfs_amd_mlv_frame_count(handle)
        self._dark = self._flat = self._look = None
        self.proxy = 1
        self.demosaic = "linear"
        self.resample_demosaic = "linear"
        self.jpeg_sampling = "4:2:0"
        try:
            if dark is not None:
                self.set_dark(dark)
            if flat is not None:
                self.set_flat(flat)
            if proxy != 1:
                self.set_proxy(proxy)
        except lib.MlvfsAmdError:
            self.close()
            raise

    def set_dark(self, dark) -> None:
        """dark: a mlvfs_amd.dark.Dark subtracted from every frame before any other stage (None clears); refused once a frame was
        served.  It must stay open while the Mount lives."""
        lib.check(self.L.mlvfs_amd_mount_set_dark(self.h, None if dark is None else dark.h), "mount_set_dark")
        self._dark = dark

    def set_flat(self, flat) -> None:
        """flat: a mlvfs_amd.flat.Flat of the clip's width and height applied to every frame after the dark frame and before any other
        stage (None clears); refused once a frame was served.  It must stay open while the Mount lives."""
        lib.check(self.L.mlvfs_amd_mount_set_flat(self.h, None if flat is None else flat.h), "mount_set_flat")
        self._flat = flat

    def set_look(self, look) -> None:
        """look: a mlvfs_amd.look.Look that every later rgb() and jpeg() call renders with, at all three sizes (None clears).  Allowed at
        any time between calls; dng(), dng_lossless(), the proxies and rgb(look16=...) never see it.  It must stay open while it is set."""
        lib.check(self.L.mlvfs_amd_mount_set_look(self.h, None if look is None else look.h), "mount_set_look")
        self._look = look

    DEMOSAICS = {"linear": 0, "amaze": 1}

    def set_demosaic(self, which: str) -> None:
        """which: "linear", the Malvar-He-Cutler filter (the default), or "amaze", the AMaZE demosaic (mlvfs_amd/amaze_render.py), in
        every later rgb(full=True), jpeg(full=True) and rgb(full=True, look16=...) call.  Allowed at any time between calls; no other
        call sees it, but with "amaze" set the resample=True calls are refused -- unless set_resample_demosaic("amaze") has given them
        AMaZE of their own -- and so are frames AMaZE does not take (a width that is no multiple of 4, a side below 36)."""
        if which not in self.DEMOSAICS:
            raise ValueError(f'demosaic {which!r} ("linear" or "amaze")')
        lib.check(self.L.mlvfs_amd_mount_set_demosaic(self.h, self.DEMOSAICS[which]), "mount_set_demosaic")
        self.demosaic = which

    def set_resample_demosaic(self, which: str) -> None:
        """which: "linear" (the default) or "amaze", the AMaZE demosaic (mlvfs_amd/amaze_resample.py), in every later
        rgb(resample=True), jpeg(resample=True) and rgb(resample=True, look16=...) call, whatever set_demosaic says.  Allowed at any
        time between calls; no other call sees it.  With "amaze" set, frames AMaZE does not take are refused."""
        if which not in self.DEMOSAICS:
            raise ValueError(f'resample demosaic {which!r} ("linear" or "amaze")')
        lib.check(self.L.mlvfs_amd_mount_set_resample_demosaic(self.h, self.DEMOSAICS[which]), "mount_set_resample_demosaic")
        self.resample_demosaic = which

    SAMPLINGS = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}

    def set_jpeg_sampling(self, which: str) -> None:
        """which: "4:2:0" (the default), "4:2:2" or "4:4:4", the chroma sampling of every later jpeg() call at every size and with either
        demosaic (mlvfs_amd/jpeg.py: sampling 420, 422, 444).  Allowed at any time between calls; no other call sees it."""
        if which not in self.SAMPLINGS:
            raise ValueError(f'JPEG sampling {which!r} ("4:2:0", "4:2:2" or "4:4:4")')
        lib.check(self.L.mlvfs_amd_mount_set_jpeg_sampling(self.h, self.SAMPLINGS[which]), "mount_set_jpeg_sampling")
        self.jpeg_sampling = which

    def set_proxy(self, factor: int) -> None:
        """factor 2: every frame is served binned to half size, 2 * (W // 4) x 2 * (H // 4), after all other stages; 1: off.  Refused
        once a frame was served."""
        lib.check(self.L.mlvfs_amd_mount_set_proxy(self.h, factor), "mount_set_proxy")
        self.proxy = factor

    def dng_size(self, index: int = 0) -> int:
        """bytes of file `index` as this handle serves it uncompressed (the proxy file's with a proxy set)"""
        size = int(self.L.mlvfs_amd_mount_dng_size(self.h, index))
        if not size:
            raise lib.MlvfsAmdError(self.L.mlvfs_amd_last_error().decode())
        return size

    @staticmethod
    def _results(results: np.ndarray | None, count: int) -> np.ndarray:
        """the int32 array a serving call writes its per-frame results to: the caller's, checked, or one of its own"""
        if results is None:
            return np.zeros(max(count, 1), np.int32)
        if not (isinstance(results, np.ndarray) and results.dtype == np.int32 and results.flags.c_contiguous and results.size >= count):
            raise ValueError(f"results must be a C-contiguous int32 array of at least {count} entries")
        return results

    def dng(self, first: int, count: int, batch: int = 8, io_threads: int = 0, results: np.ndarray | None = None) -> np.ndarray:
        """Frames first .. first + count - 1 as .dng files: a (count, dng_size) uint8 array."""
        out = np.zeros((count, self.dng_size(first) if count else 0), np.uint8)
        res = self._results(results, count)
        lib.check(self.L.mlvfs_amd_mount_dng(self.h, first, count, lib.ptr(out), out.shape[1], batch, io_threads, lib.ptr(res)),
                  "mount_dng")
        return out

    def dng_lossless(self, first: int, count: int, batch: int = 8, io_threads: int = 0, results: np.ndarray | None = None):
        """The same frames as losslessly compressed .dng files (TIFF Compression 7, one lossless-JPEG stream per file):
        -> (files, flags): files[k] the bytes of file k, flags[k] bit 0 set where the frame is served uncompressed (the file is then
        byte for byte dng()'s)."""
        stride = self.dng_size(first) if count else 0
        out = np.zeros((count, stride), np.uint8)
        sizes = np.zeros(max(count, 1), np.uintp)
        flags = np.zeros(max(count, 1), np.int32)
        res = self._results(results, count)
        lib.check(self.L.mlvfs_amd_mount_dng_lossless(self.h, first, count, lib.ptr(out), stride, lib.ptr(sizes), lib.ptr(flags), batch,
                                                      io_threads, lib.ptr(res)), "mount_dng_lossless")
        return [out[k, :int(sizes[k])].tobytes() for k in range(count)], [int(f) for f in flags[:count]]

    @staticmethod
    def _size_arg(size, full: bool, resample: bool = False):
        """(ow, oh) of a size= argument, or None"""
        if resample and (size is None or full):
            raise ValueError("resample=True takes a size= and no full=True")
        if size is None:
            return None
        if full:
            raise ValueError("size= and full=True exclude each other")
        ow, oh = size
        return int(ow), int(oh)

    # the C call of a rendering, by its size kind and its form ("rgb", "rgb16" or "jpeg"; "..._size": the size query).  The calls of the
    # two kinds with a size take ow, oh behind the gain (and the quality), the size queries behind the index
    RENDER_CALLS = {(kind, form): f"mount_{form}{kind}" for kind in ("", "_full", "_scaled", "_resampled") for form in ("rgb", "rgb16", "jpeg")}
    RENDER_CALLS.update({(kind, form + "_size"): f"mount_{form}{kind}_size" for kind in ("", "_full", "_scaled", "_resampled") for form in ("rgb", "rgb16")})

    def _render_call(self, form: str, full: bool, size, resample: bool):
        """-> (the C function, its name for an error message, the (ow, oh) it takes or ()); size: _size_arg's"""
        kind = "_resampled" if resample else "_scaled" if size is not None else "_full" if full else ""
        name = self.RENDER_CALLS[kind, form]
        return getattr(self.L, "mlvfs_amd_" + name), name, size or ()

    def rgb_size(self, index: int = 0, full: bool = False, size=None, bits: int = 8, resample: bool = False) -> int:
        """bytes of file `index` as rgb() serves it: the TIFF header + 3 * (W // 2) * (H // 2); full: + 3 * W * H; size=(ow, oh):
        + 3 * ow * oh, up to the half size, or with resample=True up to the frame's; bits=16: as rgb(look16=...) serves it, twice the
        pixel bytes"""
        if bits not in (8, 16):
            raise ValueError(f"{bits} bits per sample (8 or 16)")
        call, _, wh = self._render_call("rgb16_size" if bits == 16 else "rgb_size", full, self._size_arg(size, full, resample), resample)
        size = int(call(self.h, index, *wh))
        if not size:
            raise lib.MlvfsAmdError(self.L.mlvfs_amd_last_error().decode())
        return size

    def rgb(self, first: int, count: int, gain: float = 1.0, batch: int = 8, io_threads: int = 0, results: np.ndarray | None = None,
            full: bool = False, size=None, look16=None, resample: bool = False) -> np.ndarray:
        """Frames first .. first + count - 1 rendered to half-size 8-bit sRGB TIFF files: a (count, rgb_size) uint8 array.  gain: the
        exposure factor, in steps of 1 / 256 (gain_q8 = round(256 * gain), 1 .. 65535).  Not on a handle that serves proxies.
        full: at the frame's own size, demosaiced on the GPU (mlvfs_amd/demosaic.py): a (count, rgb_size(full=True)) array.
        size=(ow, oh): at any size up to half the frame's, area-averaged in linear light on the GPU (mlvfs_amd/scale.py): a
        (count, rgb_size(size=size)) array.  Not together with full=True.
        resample=True with size=(ow, oh): at any size up to the frame's own, area-averaged from the full-size rendering's demosaiced
        channels (mlvfs_amd/resample.py) -- another rendering than size= alone gives, also where both take the size.
        look16: a mlvfs_amd.look.Look16 -- the same renderings as 16-bit TIFF files toned from 16-bit linear light through that deep look
        (rgb_size(..., bits=16) bytes each).  It is passed per call; set_look() does not touch these files."""
        size = self._size_arg(size, full, resample)
        gain_q8 = int(round(256 * gain))
        if not 1 <= gain_q8 <= 65535:
            raise ValueError(f"gain {gain} outside 1 / 256 .. 65535 / 256")
        deep = look16 is not None
        out = np.zeros((count, self.rgb_size(first, full, size, 16 if deep else 8, resample) if count else 0), np.uint8)
        res = self._results(results, count)
        call, name, wh = self._render_call("rgb16" if deep else "rgb", full, size, resample)
        look = (look16.h,) if deep else ()
        lib.check(call(self.h, first, count, lib.ptr(out), out.shape[1], gain_q8, *wh, *look, batch, io_threads, lib.ptr(res)), name)
        return out

    def jpeg(self, first: int, count: int, gain: float = 1.0, quality: int = 90, batch: int = 8, io_threads: int = 0,
             results: np.ndarray | None = None, sampling: str | None = None, full: bool = False, size=None, resample: bool = False):
        """The renderings of rgb() as baseline JPEG files of `quality` (1 .. 100), encoded on the GPU:
        -> (files, flags): files[k] the bytes of file k, flags[k] bit 0 set where the JPEG file would be larger than the TIFF and the
        frame is served as rgb()'s TIFF, byte for byte.  full: the renderings of rgb(full=True); size=(ow, oh): those of rgb(size=size);
        with resample=True those of rgb(size=size, resample=True).  sampling: set_jpeg_sampling(sampling) first, which stays set."""
        if sampling is not None:
            self.set_jpeg_sampling(sampling)
        size = self._size_arg(size, full, resample)
        gain_q8 = int(round(256 * gain))
        if not 1 <= gain_q8 <= 65535:
            raise ValueError(f"gain {gain} outside 1 / 256 .. 65535 / 256")
        if not 1 <= quality <= 100:
            raise ValueError(f"quality {quality} outside 1 .. 100")
        stride = self.rgb_size(first, full, size, 8, resample) if count else 0
        out = np.zeros((count, stride), np.uint8)
        sizes = np.zeros(max(count, 1), np.uintp)
        flags = np.zeros(max(count, 1), np.int32)
        res = self._results(results, count)
        call, name, wh = self._render_call("jpeg", full, size, resample)
        lib.check(call(self.h, first, count, lib.ptr(out), stride, gain_q8, quality, *wh, lib.ptr(sizes), lib.ptr(flags), batch, io_threads,
                       lib.ptr(res)), name)
        return [out[k, :int(sizes[k])].tobytes() for k in range(count)], [int(f) for f in flags[:count]]

    def _tensor_spec(self, kind, dtype, layout, mean, std, gain, full, size, resample, look16):
        """-> (lib.TensorSpec, C) of a tensor call's arguments; dtype: a torch dtype or its name"""
        from . import tensor as T
        if kind not in ("rgb", "bayer"):
            raise ValueError(f'kind {kind!r} ("rgb" or "bayer")')
        name = str(dtype).replace("torch.", "")
        if name not in T.DTYPE_NAMES or layout not in T.LAYOUTS:
            raise ValueError(f"dtype {dtype} (float32, float16, bfloat16, uint8, uint16) or layout {layout!r} (NCHW, NHWC)")
        channels = 3 if kind == "rgb" else 4
        scale, bias = T.normalisation(mean, std, channels)
        spec = lib.TensorSpec(kind=T.RGB if kind == "rgb" else T.BAYER, dtype=T.DTYPE_NAMES[name], layout=T.LAYOUTS[layout])
        spec.scale[:], spec.bias[:] = scale.tolist(), bias.tolist()
        if kind == "rgb":
            wh = self._size_arg(size, full, resample)
            spec.size = T.RESAMPLED if resample else T.SCALED if wh is not None else T.FULL if full else T.HALF
            spec.ow, spec.oh = wh or (0, 0)
            spec.gain_q8 = int(round(256 * gain))
            if not 1 <= spec.gain_q8 <= 65535:
                raise ValueError(f"gain {gain} outside 1 / 256 .. 65535 / 256")
            spec.look16 = look16.h if look16 is not None else None
        return spec, channels

    def tensor_bytes(self, index: int, spec) -> int:
        """bytes of frame `index` as a tensor of that spec (a lib.TensorSpec)"""
        size = int(self.L.mlvfs_amd_mount_tensor_bytes(self.h, index, C.byref(spec)))
        if not size:
            raise lib.MlvfsAmdError(self.L.mlvfs_amd_last_error().decode())
        return size

    def tensor(self, first: int, count: int, kind: str = "rgb", dtype=None, layout: str = "NCHW", mean=None, std=None, gain: float = 1.0,
               full: bool = False, size=None, resample: bool = False, look16=None, out=None, batch: int = 8, io_threads: int = 0,
               results: np.ndarray | None = None):
        """Frames first .. first + count - 1 as one torch tensor on the handle's device, written there by the GPU: nothing crosses the
        link (include/mlvfs_amd.h, "a clip's frames as device-resident tensors"; mlvfs_amd/tensor.py is the definition in numpy).
        kind="rgb": the rendering rgb() would have served with the same gain, full, size, resample and look16 (and the handle's look),
        shape (count, 3, h, w) for layout "NCHW" or (count, h, w, 3) for "NHWC".  kind="bayer": the frame dng() would have served as four
        planes R, G1, G2, B of (H // 2, W // 2), px - black over white - black with that frame's own header levels, clamped at neither end.
        dtype: torch.float16 (the default), float32, bfloat16 -- sample / 255 (or / 65535 with look16), then (x - mean) / std per channel --
        or the integer samples themselves: torch.uint8 (8-bit rgb), torch.uint16 (rgb with look16, bayer: the raw pixels).
        out: a tensor of that shape and dtype on the device to write into; its frames must be contiguous and may lie any stride apart
        (out.stride(0)); anything else is refused.
        The call synchronises torch's current stream before it starts, so that a consumer still reading `out` is not overwritten, and
        the library's stream before it returns: the tensor is complete when the call returns.
        Not on a handle that serves proxies."""
        import torch
        from . import tensor as T
        dtype = torch.float16 if dtype is None else dtype
        spec, channels = self._tensor_spec(kind, dtype, layout, mean, std, gain, full, size, resample, look16)
        es = T.ELEM[spec.dtype]
        if count < 1:
            raise ValueError("a tensor call takes at least one frame")
        nbytes = self.tensor_bytes(first, spec)
        fh = abi.FrameHeaders()
        handle = getattr(self._reader, "h", self._reader)
        if not self.L.mlvfs_amd_mlv_frame_headers(handle, first, C.byref(fh)):
            raise lib.MlvfsAmdError(f"frame {first} has no usable headers")
        if kind == "bayer":
            h, w = fh.rawi_hdr.yRes // 2, fh.rawi_hdr.xRes // 2
        else:
            w = spec.ow if spec.size in (T.SCALED, T.RESAMPLED) else fh.rawi_hdr.xRes // (2 if spec.size == T.HALF else 1)
            h = nbytes // (es * 3 * w)
        assert channels * h * w * es == nbytes
        shape = (count,) + T.shape_of(channels, h, w, spec.layout)
        device = torch.device("cuda", max(self.L.mlvfs_amd_thread_device(), 0))
        tdtype = getattr(torch, str(dtype).replace("torch.", ""))
        if out is None:
            out = torch.empty(shape, dtype=tdtype, device=device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == tdtype and tuple(out.shape) == shape and out[0].is_contiguous()
                  and (count == 1 or out.stride(0) >= channels * h * w)):
            raise ValueError(f"out must be a {tdtype} tensor of shape {shape} on the GPU whose frames are contiguous")
        res = self._results(results, count)
        torch.cuda.current_stream(out.device).synchronize()
        stride = (out.stride(0) if count > 1 else channels * h * w) * es
        lib.check(self.L.mlvfs_amd_mount_tensor(self.h, first, count, C.c_void_p(out.data_ptr()), stride, C.byref(spec), batch, io_threads,
                                                lib.ptr(res)), "mount_tensor")
        return out

    def tensors(self, first: int, count: int, batch: int = 8, **spec):
        """tensor() batch by batch: a generator of tensors of up to `batch` frames each, in serve order; **spec: tensor()'s arguments"""
        for f0 in range(first, first + count, batch):
            yield self.tensor(f0, min(batch, first + count - f0), batch=batch, **spec)

    def close(self) -> None:
        if self.h:
            self.L.mlvfs_amd_mount_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
