"""What the level and gain tests of the fused pass share (tests/test_level_cases.py on the CPU, tests/test_gpu_levels.py on the GPU): the
black / white level pairs, the stripe coefficient families, the reduced-depth and 16-bit cases, and footage at a case's black level.

The fused pass (unpack + pixel map + chroma smoothing + stripes: k_frame, k_frame_p, k_frame_p5, k_frame_s) has arithmetic relative to
the black level in its loader (2^23 + black, the `<= black`, `<= black + 64`, `<= black + 255` flags, the dark forms, the per-black
output table) and a stripes epilogue in three forms -- packed 16-bit, 32-bit (`__mul24`), 64-bit -- between which the launcher chooses
by an admission rule (csrc/k_frame.hip: launch_frame: every |coef - 65536| < 32768, and for the packed form 14/12/10-bit input, white >
black + 64, 0 <= black <= 16384).  The cases sit on both sides of every edge of that rule:

  levels     black 0, 1, 63 / 64 / 65 (where `a > 64` meets small absolute values), 1023, 2047, 4095, 8191, 16000, 16319 (no pixel more
             than 64 above black: stripes change nothing), 16384 (every 14-bit pixel below black, the rule's last black); white =
             black + 65 (the packed form's first white), black + 64 (its last refusal: the generic form, the streaming kernels
             decline), 15000, 16383 and 60000 (above every pixel).  Each case names the form it is there for ("packed" / "generic");
             the GPU test proves it from the plan the launch took, not from a restatement of the rule.
  families   a all unit; b realistic (+-0.5 %); c the packed form's last coefficients, 65536 +- 32767 (on phases 2..7, on all eight,
             and two sets in which every dword (0,1) (2,3) (4,5) (6,7) has exactly one unit column -- the epilogue's shortcut is for
             dwords of two); d one step beyond: one coefficient 65536 + 32768, one 65536 - 32768, one 0 (stripes.c:261: a zero
             coefficient leaves its column alone -- not even the clamp to white); e gains of 1.25 and 65536 + 32767 on every column with
             white 15000 (the clamp).  c-e at blacks 0, 2047, 8191.
  depths     12 bits at black 0 / 511 / 512 / 1000 with whites 3750 / 4095, 10 bits at 0 / 127 / 128 / 300 with 937 / 1023.
  16 bits    black 8192, white 60000 (a converted dual-ISO frame), and black 0 with pixels of 65535 and d = 32767: the largest
             product `__mul24` sees.
  cache      11 levels and a twelfth in use between them, for the per-device cache of 8 output tables.
  lone greens  frames in which chroma smoothing writes pixels within 64 of black although none was loaded there (LONE_GREEN).

Footage is the generators of mlvfs_amd.synth.  They take `black=` and add a fixed amplitude, so above black 2048 most of a frame
would sit at 16383: there the frame is drawn at black 2048 and what lies above black is scaled to the room the case leaves (scaled()),
here and not in synth, whose callers keep their frames.  At 16319 and 16384 saturation is the point: unscaled.  Every frame then gets
a few pixels at the values the kernels compare with (sprinkle()): below black, black, black + 1 / 63 / 64, + 65 / 66 / 254 / 255, +
256 / 257, wherever the depth has them -- the low ones in the frame's upper third, the middle ones in its middle third, so that tiles
and row steps of every flag combination exist."""
import numpy as np

from mlvfs_amd import synth

# ------------------------------------------------------------------ geometries
# (608, 250): two columns, the last of 14 items folded in four, five 30-row segments, vector layout 1; (264, 62): layout 2, one column
GEOMETRIES = ((608, 250), (264, 62))
REDUCED_GEOMETRIES = {12: ((256, 130), (264, 62)), 10: ((256, 130),)}     # 264 = 8 mod 16: rows of whole 8-pixel groups, 12-bit only
NFRAMES = 3

# ------------------------------------------------------------------ levels of 14-bit streams
BLACKS = (0, 1, 63, 64, 65, 1023, 2047, 4095, 8191, 16000, 16319, 16384)
SATURATED_BLACKS = (16319, 16384)
WHITE_KINDS = ("inner", "outer", "15000", "16383", "above")
ABOVE = 60000


def white_of(black, kind):
    return {"inner": black + 65, "outer": black + 64, "15000": 15000, "16383": 16383, "above": ABOVE}[kind]


# (black, white kind, the stripes form the case is there for).  Not a full cross: every black with two whites and more, every white
# kind with three blacks and more (tests/test_level_cases.py).  "outer" is the generic form by definition; of the absolute whites only
# pairs inside the rule are listed (16383 is black 16319's outer edge and listed as that).
LEVELS = [
    (0, "inner", "packed"), (0, "outer", "generic"), (0, "15000", "packed"),
    (1, "inner", "packed"), (1, "16383", "packed"),
    (63, "outer", "generic"), (63, "above", "packed"),
    (64, "inner", "packed"), (64, "outer", "generic"),
    (65, "inner", "packed"), (65, "15000", "packed"),
    (1023, "15000", "packed"), (1023, "16383", "packed"), (1023, "outer", "generic"),
    (2047, "inner", "packed"), (2047, "above", "packed"), (2047, "15000", "packed"),
    (4095, "outer", "generic"), (4095, "16383", "packed"),
    (8191, "inner", "packed"), (8191, "outer", "generic"), (8191, "15000", "packed"), (8191, "above", "packed"),
    (16000, "inner", "packed"), (16000, "16383", "packed"), (16000, "above", "packed"),
    (16319, "inner", "packed"), (16319, "outer", "generic"), (16319, "above", "packed"),
    (16384, "inner", "packed"), (16384, "outer", "generic"), (16384, "above", "packed"),
]


def level_id(case):
    return f"black{case[0]}-white{white_of(case[0], case[1])}"


def level_geometry(i):
    """Case i of LEVELS runs on one geometry: they alternate"""
    return GEOMETRIES[i % 2]


# ------------------------------------------------------------------ stripe coefficients (coef[8], phase = x & 7)
ONE = 65536
HI, LO = ONE + 32767, ONE - 32767                    # the packed (and the 32-bit) form's last coefficients
REALISTIC = (65536, 65536, 65354, 65738, 65241, 65868, 65450, 65640)
FAMILIES = {
    "a-unit": (ONE,) * 8,
    "b-realistic": REALISTIC,
    "c-edge-2to7": (ONE, ONE, HI, LO, LO, HI, HI, LO),
    "c-edge-all": (HI, LO, LO, HI, HI, LO, LO, HI),
    "c-one-unit": (ONE, HI, LO, ONE, ONE, LO, HI, ONE),
    "c-one-unit-mirror": (HI, ONE, ONE, LO, LO, ONE, ONE, HI),
    "d-plus-32768": REALISTIC[:5] + (ONE + 32768,) + REALISTIC[6:],
    "d-minus-32768": REALISTIC[:2] + (ONE - 32768,) + REALISTIC[3:],
    "d-zero": REALISTIC[:3] + (0,) + REALISTIC[4:],
    "e-gain-1.25": (ONE + ONE // 4,) * 8,
    "e-gain-edge": (HI,) * 8,
}
ONE_UNIT_FAMILIES = ("c-one-unit", "c-one-unit-mirror")
FAMILY_BLACKS = (0, 2047, 8191)
CLAMP_WHITE = 15000
# Family e is about the clamp: the generators' amplitude (about 8 000 above black) times 1.25 stays below 15000 at low blacks, so
# these clips are drawn with more of it -- in quarters: 8/4 at black 0, 7/4 at 2047 and, of the room scaled() leaves, at 8191
E_AMPLITUDE = {0: 8, 2047: 7, 8191: 7}


def family_form(name):
    """The stripes form a family is there for: d lies one step outside the packed form (and outside the 32-bit one)"""
    return "generic" if name.startswith("d-") else "packed"


# (family, black, white, form, amplitude in quarters): a, c, d, e at the three blacks (b runs in the level sweep)
FAMILY_CASES = [(name, black, CLAMP_WHITE if name.startswith("e-") else 16383, family_form(name),
                 E_AMPLITUDE[black] if name.startswith("e-") else 4)
                for name in FAMILIES if name != "b-realistic" for black in FAMILY_BLACKS]


def family_id(case):
    return f"{case[0]}-black{case[1]}"


def family_geometry(i):
    return GEOMETRIES[(i // len(FAMILY_BLACKS) + i) % 2]


# ------------------------------------------------------------------ 12- and 10-bit streams (the direct loader, vector layouts 3 / 4)
REDUCED = [(12, b, w) for b in (0, 511, 512, 1000) for w in (3750, 4095)] + [(10, b, w) for b in (0, 127, 128, 300) for w in (937, 1023)]

# ------------------------------------------------------------------ 16-bit input
UNPACKED_BLACK, UNPACKED_WHITE = 8192, 60000
# without chroma smoothing, stripes over the whole 16-bit range: (black, family).  b and c take the 32-bit form (16-bit input never the
# packed one), d the 64-bit one; black 0 with e-gain-edge multiplies 65535 by 32767
UNPACKED_STRIPES = [(UNPACKED_BLACK, "b-realistic"), (UNPACKED_BLACK, "c-edge-all"), (UNPACKED_BLACK, "c-one-unit"),
                    (UNPACKED_BLACK, "d-plus-32768"), (UNPACKED_BLACK, "d-minus-32768"), (UNPACKED_BLACK, "d-zero"),
                    (0, "e-gain-edge"), (0, "c-edge-all"), (0, "d-zero")]
UNPACKED_SMOOTH_FAMILIES = ("b-realistic", "c-edge-all", "d-minus-32768")

# ------------------------------------------------------------------ the output-table cache (csrc/k_frame.hip: e2r_table keeps 8 levels)
CACHE_LEVELS = (10, 200, 512, 1000, 1500, 2000, 3000, 5000, 7000, 9000, 12000)
CACHE_NEIGHBOUR = 2048           # a second clip in use between all of them
CACHE_GEOMETRY = (128, 64)


# ------------------------------------------------------------------ footage
KINDS = {0: ("normal", "low_light", "adversarial"), 2: ("normal", "low_light", "adversarial"), 3: ("normal", "low_light", "adversarial"),
         5: ("normal", "colour_cast", "low_light")}
DRAWN_AT = synth.BLACK           # where a scaled frame is drawn: none of the generators clips at 0 there
ROOM_AT = 16383 - DRAWN_AT


def generate(kind, w, h, k, black):
    gen = getattr(synth, kind + "_frame")
    if kind in ("low_light", "colour_cast"):
        return gen(w, h, seed=3 + k, black=black)
    return gen(w, h, frame=k, black=black)


def scaled(kind, w, h, k, black, quarters=4, top=16383):
    """Frame k of a kind at `black`: as the generator draws it where its amplitude fits (black <= 2048, amplitude as drawn) and at the
    saturated blacks; else drawn at 2048, what lies above black multiplied by quarters / 4 and by the share of the room above black
    that the case has left, what lies below kept"""
    if quarters == 4 and (black <= DRAWN_AT or black in SATURATED_BLACKS):
        return np.clip(generate(kind, w, h, k, black), 0, top).astype(np.uint16)
    lin = generate(kind, w, h, k, DRAWN_AT).astype(np.int64) - DRAWN_AT
    room = min(top - black, ROOM_AT)
    lin = np.where(lin > 0, lin * (room * quarters) // (ROOM_AT * 4), lin)
    return np.clip(lin + black, 0, top).astype(np.uint16)


SPRINKLE_LOW = (-3, -1, 0, 1, 63, 64)            # at most 64 above black: the upper third of the frame
SPRINKLE_MID = (65, 66, 254, 255, 256, 257)      # the middle third
SPRINKLE_EACH = 6


def sprinkle(f, black, top, seed):
    """A few pixels at the values on either side of the kernels' comparisons, where the depth has them; all column phases"""
    h, w = f.shape
    rng = np.random.default_rng(seed)
    for values, (y0, y1) in ((SPRINKLE_LOW, (4, max(h // 3, 6))), (SPRINKLE_MID, (h // 3, max(2 * h // 3, h // 3 + 2)))):
        for d in values:
            ys, xs = rng.integers(y0, y1, SPRINKLE_EACH), rng.integers(4, w - 4, SPRINKLE_EACH)
            if 0 <= black + d <= top:
                f[ys, xs] = black + d
    return f


def footage(kinds, w, h, black, quarters=4, bpp=14):
    """One frame per kind at a case's black level; reduced depths are the 14-bit frame at black << shift, shifted down"""
    shift = 14 - bpp
    out = []
    for k, kind in enumerate(kinds):
        f = (scaled(kind, w, h, k, black << shift, quarters) >> shift).astype(np.uint16)
        out.append(sprinkle(f, black, (1 << bpp) - 1, 1000 * black + 10 * bpp + k))
    return out


def footage16(kinds, w, h, black):
    """16-bit frames for chroma smoothing: a 14-bit frame as drawn at 2048, moved to `black`.  The reference's raw2ev is
    raw2ev_base[16384 + MAX_BLACK] entered at MAX_BLACK - black (main.c:158-176, MAX_BLACK = 16384: mlvfs.h:88), so a pixel p is inside
    its table for black - 16384 <= p <= black + 16383 and chroma_smooth.c:30-32, 50-57 read nothing else; at black 8192 the frames
    here span 6144 .. 22527 (and what sprinkle() adds lies around black)."""
    out = []
    for k, kind in enumerate(kinds):
        f = (generate(kind, w, h, k, DRAWN_AT).astype(np.int64) + (black - DRAWN_AT)).astype(np.uint16)
        assert black - 16384 <= int(f.min()) and int(f.max()) <= black + 16383
        out.append(sprinkle(f, black, 65535, 77 * black + k))
    return out


def full_range16(w, h, black, seed):
    """16-bit frames for stripes alone (stripes.c:250-266 reads no table): every value 0 .. 65535 can occur, 65535 and 0 on every
    column phase, and the values around black + 64"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    f[1, 8:16] = 65535
    f[2, 8:16] = 0
    f[3, 8:16] = min(black + 64, 65535)
    f[4, 8:16] = min(black + 65, 65535)
    return f


# ------------------------------------------------------------------ smoothed pixels that land within 64 of black
# k_frame_p, k_frame_p5 and k_frame_s pick a variant of the output stage from the pixels they LOAD: where none of them lies at most 64
# above black the stripes epilogue runs without its `a > 64` mask.  Chroma smoothing can still write a pixel below that line: a cell
# with dim greens among cells with bright greens, red and blue dim everywhere, gets EV = (its green) + median(red - green of the
# neighbours), a few levels above black -- which stripes.c:261 then leaves alone, and which an unmasked negative gain lowers by one.
# (green, red and blue) above black: no pixel at most 64 above black; none less than 256 above (the "bright" variants)
LONE_GREEN = ((2000, 70), (7000, 300))


def lone_green_frame(w, h, black, green, dim, seed):
    """Red and blue `dim` above black, green `green` above it, 4 % of the cells with both greens as dim as their red; 0 .. 8 of noise"""
    rng = np.random.default_rng(seed)
    f = black + dim + rng.integers(0, 9, (h, w))
    g = black + green + rng.integers(0, 9, (h // 2, w // 2))
    g = np.where(rng.random((h // 2, w // 2)) < 0.04, black + dim + 2, g)
    f[0::2, 1::2] = g
    f[1::2, 0::2] = g + 1
    return f.astype(np.uint16)


# ------------------------------------------------------------------ what a case must contain (tests/test_level_cases.py)
def populations(f, black):
    """Pixels of a frame below, at, 1..64, 65..255 and more than 255 above black"""
    lin = f.astype(np.int64) - black
    return {"below": int((lin < 0).sum()), "at": int((lin == 0).sum()), "1..64": int(((lin >= 1) & (lin <= 64)).sum()),
            "65..255": int(((lin >= 65) & (lin <= 255)).sum()), ">255": int((lin > 255).sum())}


def room_for(black, top=16383):
    """The populations the depth has values for at this black"""
    return {"below": black >= 1, "at": black <= top, "1..64": black + 1 <= top, "65..255": black + 65 <= top, ">255": black + 256 <= top}


def oracle_pass(oracle, frames, black, white, cs, pixels, coeffs):
    """The reference's order (main.c:942-997) with the clip's pixel map and coefficients given: repair, smooth, stripes"""
    out = []
    for f in frames:
        img = f if pixels is None else oracle.apply_bad_pixels(f, black, pixels)
        if cs:
            img = oracle.chroma_smooth(img, black, cs)
        if coeffs is not None:
            img = oracle.stripes_apply(img, black, white, 1, np.array(coeffs, np.int32))
        out.append(img)
    return out
