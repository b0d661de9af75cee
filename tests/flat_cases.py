"""Cases and the numpy oracle of flat-field correction (csrc/cal.cpp, csrc/k_cal.hip), shared by
tests/test_flat_cases.py (CPU: the cases really test something), tests/test_flat_host.py and tests/test_gpu_flat.py.

    s[p]    = max(F[p] - black_f, 1)
    c       = (y & 1) * 2 + (x & 1)
    M_c     = (sum of s[p] over channel c + n_c // 2) // n_c
    gain[p] = min((M_c * 16384 + s[p] // 2) // s[p], 65535)
    out     = clamp(black + floor(((px - black) * gain[p] + 8192) / 16384), 0, 2^bpp - 1)

all in int64 here.  The reference has no flat-field code.  The tests tie the definition back to it so: a clip served or rewritten WITH
a flat field (with or without a dark frame) must equal what the reference's own process_frame text gives for a clip whose payloads
were corrected beforehand with apply() below."""
import numpy as np

import dark_cases as dc
from dark_cases import NAME, write_clip  # noqa: F401  (the clips' builder: dark_cases.write_clip, for sources and pre-corrected clips alike)

W, H = dc.W, dc.H
BLACK = dc.BLACK
ONE = 16384


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def channels(h, w):
    yy, xx = np.indices((h, w))
    return (yy & 1) * 2 + (xx & 1)


def signal(F, black_f):
    return np.maximum(np.asarray(F).astype(np.int64) - int(black_f), 1)


def channel_sums(F, black_f):
    s, c = signal(F, black_f), channels(*np.asarray(F).shape)
    return [int(s[c == k].sum()) for k in range(4)], [int((c == k).sum()) for k in range(4)]


def channel_means(F, black_f):
    sums, counts = channel_sums(F, black_f)
    return [(t + n // 2) // n if n else 0 for t, n in zip(sums, counts)]


def gains(F, black_f):
    """The Q14 gain plane of the flat plane F (height, width) with pedestal black_f."""
    s, c = signal(F, black_f), channels(*np.asarray(F).shape)
    m = np.array(channel_means(F, black_f), np.int64)[c]
    return np.minimum((m * ONE + s // 2) // s, 65535).astype(np.uint16)


def apply(px, gain, black, bpp):
    """a frame value above 2^bpp - 1 (no valid frame has one; a damaged LJ92 stream can decode to one) is taken as 2^bpp - 1"""
    px = np.minimum(np.asarray(px).astype(np.int64), (1 << bpp) - 1)
    v = int(black) + ((px - int(black)) * gain.astype(np.int64) + 8192) // ONE                                      # // is floor
    return np.clip(v, 0, (1 << bpp) - 1).astype(np.uint16)


def correct(frame, gain, black, bpp, dark=None, black_d=None):
    """stage 0, then stage 0b"""
    if dark is not None:
        frame = dc.subtract(frame, dark, black_d, bpp)
    return apply(frame, gain, black, bpp)


def truncated(px, gain, black, bpp):
    """what an implementation that truncates towards zero instead of flooring would give"""
    t = (np.asarray(px).astype(np.int64) - int(black)) * gain.astype(np.int64) + 8192
    v = int(black) + np.where(t < 0, -((-t) // ONE), t // ONE)
    return np.clip(v, 0, (1 << bpp) - 1).astype(np.uint16)


# ---- flat planes -------------------------------------------------------------------------------------------------------------
def _spread(F, idx, delta):
    """delta added to the sum of F over idx, as evenly as integers allow"""
    q, r = divmod(int(delta), len(idx))
    F.reshape(-1)[idx] += q
    F.reshape(-1)[idx[:r]] += 1


def flat_plane(w, h, bpp=14, black_f=None, seed=5, level=0.4, falloff=1.6, marks=False):
    """A plane as a camera's flat clip averages to: the pedestal plus an evenly lit target seen through vignetting (down to
    1 - falloff / 2 of the centre in the corners), a column pattern, a tint per Bayer channel and a little noise; entries AT black_f
    and BELOW it (s = 1), dust shadows deep enough for the 65535 cap and shallower ones below it.  marks: low entries (gain 2) under
    dark_cases.TOP_AT and ZERO_AT, where the clips' frames hold pixels near the top and near 0: the results clamp both ways.
    From 64 pixels on the plane is tuned (see tune())."""
    rng = np.random.default_rng(seed + 1000 * w + 10 * h + bpp)
    top = (1 << bpp) - 1
    black_f = dc.clip_black(bpp) if black_f is None else black_f
    yy, xx = np.indices((h, w))
    r2 = ((xx - (w - 1) / 2) / max(w, 2)) ** 2 + ((yy - (h - 1) / 2) / max(h, 2)) ** 2
    sig = level * (top - black_f) * (1 - falloff * r2) * (1 + 0.03 * (xx % 8 == 3)) * np.array([1.0, 0.8, 0.8, 0.6])[channels(h, w)]
    F = (black_f + sig + rng.integers(-6, 7, (h, w))).astype(np.int64)
    free = np.ones(w * h, bool)
    npix = w * h
    if npix >= 16:
        spec = rng.choice(npix, 12, replace=False)
        flat_sig = sig.reshape(-1)
        F.reshape(-1)[spec[0:3]] = black_f
        F.reshape(-1)[spec[3:6]] = black_f // 2
        F.reshape(-1)[spec[6:9]] = black_f + (flat_sig[spec[6:9]] / 8).astype(np.int64)
        F.reshape(-1)[spec[9:12]] = black_f + (flat_sig[spec[9:12]] * 0.3).astype(np.int64)
        free[spec] = False
    else:
        F.reshape(-1)[0] = black_f
        F.reshape(-1)[-1] = black_f // 2
        free[[0, npix - 1]] = False
    if marks:
        for (y, x) in dc.TOP_AT + dc.ZERO_AT:
            y, x = int(y * h / H), int(x * w / W)
            F[y, x] = black_f + int(sig[y, x] / 2)
            free[y * w + x] = False
    if npix >= 64:
        tune(F, black_f, top, free)
    assert F.min() >= 0 and F.max() <= top
    return F.astype(np.uint16)


def tune(F, black_f, top, free):
    """Put the roundings on their boundaries without changing what else the plane is.
    The mean: channel 0's sum becomes n/2 (mod n) -- for an even n exactly half way, M rounds up --, channel 1's one less (rounds down).
    The gain, with the channel sums kept as they are (what one pixel gains the free pixels of its channel lose): in every channel one
    pixel whose quotient M * 16384 / s is the largest fraction below one half, and, where the plane has the range for s = 32768 (an
    exact half needs s = 2^15 times an odd divisor of M), channel 0's M made odd and one pixel exactly half way."""
    h, w = F.shape
    c = channels(h, w).reshape(-1)
    flat = F.reshape(-1)
    for ch, off in ((0, 0), (1, -1)):
        idx = np.flatnonzero((c == ch) & free)
        n = int((c == ch).sum())
        total = int(signal(flat[c == ch], black_f).sum())
        _spread(F, idx, (n // 2 + off - total) % n)
    half = top - black_f >= 32768
    if half:
        idx = np.flatnonzero((c == 0) & free)
        if channel_means(F, black_f)[0] % 2 == 0:
            _spread(F, idx, int((c == 0).sum()))                          # the sum + n: M + 1, the same place mod n
    M = channel_means(F, black_f)
    for ch in range(4):
        idx = np.flatnonzero((c == ch) & free)
        if len(idx) < 8:
            continue
        wanted = []
        s = np.arange(max(M[ch] // 3, 3), min(2 * M[ch], top - black_f), dtype=np.int64)
        r = (M[ch] * ONE) % s
        below = s[(2 * r + 1 == s) | (2 * r + 2 == s)]
        if len(below):
            wanted.append(int(below[len(below) // 2]))
        if half and ch == 0:
            wanted.append(32768)
        for k, target in enumerate(wanted):
            p, rest = idx[k], idx[len(wanted):]
            delta = int(flat[p] - black_f) - target                        # what the others take over
            flat[p] = black_f + target
            _spread(F, rest, delta)
    assert channel_means(F, black_f) == M


def constant_plane(w, h, value=5000):
    return np.full((h, w), value, np.uint16)


def overflow_plane(w=640, h=480):
    """16 bits, black_f = 0, values near 60000: a channel's sum (76800 pixels) passes 2^32"""
    return flat_plane(w, h, 16, 0, level=0.94, falloff=0.05)


# the planes of the host test and of the GPU's gain kernels: (w, h, bpp, black_f)
HOST_GEOMETRIES = [(2, 2), (3, 3), (5, 4), (3, 16), (30, 10), (1, 8), (8, 1), (416, 264)]
GPU_GAIN_GEOMETRIES = [(3, 16), (30, 12), (64, 48)]


def rounding_classes(F, black_f):
    """-> dict of counts: what test_flat_cases asks the planes for"""
    s, c = signal(F, black_f), channels(*F.shape)
    sums, counts = channel_sums(F, black_f)
    M = np.array(channel_means(F, black_f), np.int64)[c]
    r = (M * ONE) % s
    g = gains(F, black_f)
    return dict(cap=int((g == 65535).sum()), at_black=int((F == black_f).sum()), below_black=int((F < black_f).sum()),
                gain_half=int((2 * r == s).sum()), gain_below_half=int(((2 * r + 1 == s) | (2 * r + 2 == s)).sum()),
                mean_half=sum(1 for t, n in zip(sums, counts) if n and 2 * (t % n) == n),
                mean_below_half=sum(1 for t, n in zip(sums, counts) if n > 2 and t % n == (n - 1) // 2 and 2 * (t % n) < n),
                sum_over_32_bits=sum(1 for t in sums if t >= 1 << 32))


# ---- mlvfs_amd_flat_apply_dev --------------------------------------------------------------------------------------------------
APPLY_GEOMETRIES = [(16, 2), (48, 6), (2, 2), (30, 10), (416, 264)]
APPLY_CASES = [(w, h, bpp, n, dark) for (w, h) in APPLY_GEOMETRIES for bpp in (10, 12, 14, 16) for n in (1, 3) for dark in (False, True)]


def apply_case(w, h, bpp, n, dark=False, flat_bpp=14, seed=0):
    """n frames of w x h at bpp bits over the whole range, a flat plane at flat_bpp bits (another depth than the frames' unless bpp
    is 14) and, with `dark`, a dark plane with pedestal black_d -> dict(frames, F, black_f, black, dark, black_d, want).
    The first pixels are near 0 and the last near the top, both under gains above 1 (the last pixel under the cap): the results clamp
    both ways, and at 16 bits the product under the cap passes 2^31.  From 16 pixels on, four pixels lie just below black."""
    rng = np.random.default_rng(4000 * w + 40 * h + bpp + n + seed)
    top, black = (1 << bpp) - 1, dc.clip_black(bpp)
    black_f = dc.clip_black(flat_bpp) - 11
    npix = w * h
    F = flat_plane(w, h, flat_bpp, black_f, seed=seed + bpp).astype(np.int64).reshape(-1)
    k = max(1, min(3, npix // 4))
    F[:k] = black_f + (F[:k] - black_f) // 2 + 1
    F[-k:] = black_f + (F[-k:] - black_f) // 2 + 1
    F[-1] = black_f                                                         # the cap
    F = F.astype(np.uint16).reshape(h, w)
    frames = [rng.integers(max(black - 8, 0), top + 1, npix).astype(np.uint16) for _ in range(n)]
    for f in frames:
        f[:k] = rng.integers(0, 4, k)
        f[-k:] = top - rng.integers(0, 3, k)
        if npix >= 16:
            f[k:k + 4] = black - np.array([1, 2, 3, 5])                     # a little below black: floor and truncation part ways
    frames = [f.reshape(h, w) for f in frames]
    plane_d = black_d = None
    if dark:
        black_d = black - 37
        plane_d = np.clip(black_d + rng.integers(-6, 7, npix), 0, top).astype(np.uint16)
        plane_d[min(1, npix - 1)] = top - 5
        plane_d[-2] = black_d // 4
        plane_d = plane_d.reshape(h, w)
    g = gains(F, black_f)
    return dict(frames=frames, F=F, black_f=black_f, black=black, dark=plane_d, black_d=black_d, gain=g,
                want=[correct(f, g, black, bpp, plane_d, black_d) for f in frames])


# ---- clips ---------------------------------------------------------------------------------------------------------------------
def clip_flat(w=W, h=H):
    """the 14-bit flat plane of the clip cases: milder vignetting than flat_plane's default (corners at 0.6), marks under TOP_AT / ZERO_AT"""
    return flat_plane(w, h, 14, BLACK, seed=11, falloff=0.8, marks=True)


def clip_case(kind="plain", n=5, w=W, h=H, dark=False):
    """dark_cases.clip_frames' material -> (frames, flat plane F (black_f = BLACK), dark plane or None, the frames corrected beforehand)"""
    frames, F = dc.clip_frames(kind, n, w, h), clip_flat(w, h)
    plane_d = dc.dark_plane(w, h) if dark else None
    g = gains(F, BLACK)
    return frames, F, plane_d, [correct(f, g, BLACK, 14, plane_d, BLACK) for f in frames]


DEPTH_CASES = dc.DEPTH_CASES        # (W, H, 12), (W, H, 10), (64, 48, 16), (30, 12, 14), (30, 12, 12)


def depth_case(w, h, bpp, dark=False, n=3):
    """dark_cases.depth_case's frames (and dark plane) at bpp bits under the 14-bit clip_flat: the flat's depth is not the frames'
    -> (frames, F, dark plane or None, black_d, the frames corrected beforehand)"""
    frames, plane_d, black_d, _ = dc.depth_case(w, h, bpp, n)
    F = clip_flat(w, h)
    g = gains(F, BLACK)
    if not dark:
        plane_d = None
    return frames, F, plane_d, black_d, [correct(f, g, dc.clip_black(bpp), bpp, plane_d, black_d) for f in frames]
