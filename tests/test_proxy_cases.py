"""The cases of tests/proxy_cases.py are not vacuous (no GPU, no library): the numpy restatement of the binning against a plain loop,
the content against what it is there to catch, the sizes against the paths they are there to reach, the header rule against values
worked out by hand."""
import struct

import numpy as np

import proxy_cases as pc


def loop_bin2(f):
    h, w = f.shape
    pw, ph = 2 * (w // 4), 2 * (h // 4)
    out = np.zeros((ph, pw), np.uint16)
    for Y in range(ph):
        for X in range(pw):
            y0, x0 = 4 * (Y >> 1) + (Y & 1), 4 * (X >> 1) + (X & 1)
            out[Y, X] = (int(f[y0, x0]) + int(f[y0, x0 + 2]) + int(f[y0 + 2, x0]) + int(f[y0 + 2, x0 + 2]) + 2) >> 2
    return out


def test_bin2_is_the_definition():
    for w, h in [s for s in pc.BIN_SIZES if s[0] * s[1] <= 48 * 12] + [(9, 11), (5, 4)]:
        for kind in pc.CONTENT:
            f = pc.content(kind, w, h, seed=3)
            got = pc.bin2(f)
            assert got.shape == (2 * (h // 4), 2 * (w // 4)) and got.dtype == np.uint16
            assert np.array_equal(got, loop_bin2(f)), (w, h, kind)
    assert pc.proxy_size(pc.BIG_W, pc.BIG_H) == (1792, 660) and pc.proxy_size(pc.DROP_W, pc.DROP_H) == (208, 132)


def test_dropped_columns_and_rows_are_never_read():
    f = pc.random_frame(7, 5)
    g = f.copy()
    g[4:, :] ^= 0xFFFF
    g[:, 4:] ^= 0xFFFF
    assert np.array_equal(pc.bin2(f), pc.bin2(g))
    dropped = {(w % 4, h % 4) for w, h in pc.BIN_SIZES + [(pc.DROP_W, pc.DROP_H)]}
    assert {2, 3} <= {a for a, _ in dropped} and {1, 2} <= {b for _, b in dropped}         # between them 1, 2 and 3
    assert (7 % 4, 5 % 4) == (3, 1) and (6 % 4, 6 % 4) == (2, 2) and pc.DROP_H % 4 == 2 and pc.DROP_W % 4 == 2


def test_sizes_reach_both_forms_and_the_wave_edges():
    fast = [(w, h) for w, h in pc.BIN_SIZES if w % 16 == 0]
    assert (16, 4) in fast and (32, 8) in fast and (20, 8) not in fast and (4, 4) not in fast
    assert 1024 // 16 == 64 and 1040 // 16 == 65                 # one wave of 16-pixel groups per row, and one lane more
    assert any(h // 4 > 1 for _, h in fast)                      # more than one block row
    assert 416 // 16 * (264 // 4) > 256                          # more than one workgroup
    assert pc.BIG_W % 16 == 0


def test_content_reaches_every_residue_and_sums_beyond_16_bits():
    for w, h in ((4, 4), (16, 4), (20, 8), (416, 264)):
        assert (pc.sums(pc.ones_frame(w, h)) == 4 * 65535).all() and (pc.bin2(pc.ones_frame(w, h)) == 65535).all()
    for w, h in ((16, 8), (48, 12), (416, 264), (pc.BIG_W, pc.BIG_H)):
        s = pc.sums(pc.random_frame(w, h))
        assert {int(v) for v in np.unique(s % 4)} == {0, 1, 2, 3} and s.max() > 65535, (w, h)
        s = pc.sums(pc.residue_frame(w, h))
        assert {int(v) for v in np.unique(s)} == {0, 1, 2, 3}, (w, h)
        assert {int(v) for v in np.unique(pc.bin2(pc.residue_frame(w, h)))} == {0, 1}       # (s + 2) >> 2: 0, 0, 1, 1
    # a packed 16-bit sum is wrong on these: the low 16 bits of the sum give another mean
    s = pc.sums(pc.random_frame(416, 264))
    assert (((s & 0xFFFF) + 2) >> 2 != (s + 2) >> 2).any()
    # truncation instead of rounding, and rounding up from 1, both show
    assert ((s >> 2) != ((s + 2) >> 2)).any() and (((s + 3) >> 2) != ((s + 2) >> 2)).any()


def test_parity_frame_bins_to_the_same_constants():
    for w, h in pc.BIN_SIZES:
        out = pc.bin2(pc.parity_frame(w, h))
        assert np.array_equal(out, pc.parity_frame(out.shape[1], out.shape[0])), (w, h)
    assert len(set(pc.PARITY_CONSTANTS)) == 4 and 65535 in pc.PARITY_CONSTANTS


def test_position_frame_shows_any_swap():
    for w, h in ((16, 8), (48, 12), (20, 8), (1040, 8)):
        f = pc.position_frame(w, h)
        want = pc.bin2(f)
        for a in range(0, 4 * (h // 4)):
            for b in range(a + 1, 4 * (h // 4)):
                g = f.copy()
                g[[a, b]] = g[[b, a]]
                # rows of one colour inside one block sum to the same: only such a swap may go unseen
                unseen = a // 4 == b // 4 and (a - b) % 2 == 0
                assert np.array_equal(pc.bin2(g), want) == unseen, (w, h, a, b)
        cols = range(0, min(4 * (w // 4), 24))
        for a in cols:
            for b in cols:
                if a < b:
                    g = f.copy()
                    g[:, [a, b]] = g[:, [b, a]]
                    unseen = a // 4 == b // 4 and (a - b) % 2 == 0
                    assert np.array_equal(pc.bin2(g), want) == unseen, (w, h, a, b)
        # output rows or columns swapped: seen
        assert not np.array_equal(want[::-1], want) and not np.array_equal(want[:, ::-1], want)
        for a in range(want.shape[0] - 1):
            assert not np.array_equal(want[a], want[a + 1])
        for a in range(want.shape[1] - 1):
            assert not np.array_equal(want[:, a], want[:, a + 1])


def test_batches_hold_distinct_frames():
    for n in (1, 3):
        b = pc.batch(48, 12, n)
        assert len(b) == n and all(not np.array_equal(b[i], b[j]) for i in range(n) for j in range(i))


def test_lo_and_hi():
    assert [pc.lo(v) for v in range(0, 10)] == [0, 2, 2, 2, 2, 4, 4, 4, 4, 6]
    assert [pc.hi(v, 100) for v in range(0, 10)] == [0, 0, 0, 0, 2, 2, 2, 2, 4, 4]
    assert pc.hi(1320, 660) == 660 and pc.hi(3950, 660) == 660 and pc.lo(146) == 74 and pc.lo(29) == 16


def _header(w, h, area, crop, fp=(5760000, 1461, 3840000, 972)):
    """a minimal header with the tags the rule reads: IFD0 = 256, 257, 259, 278, 279, 34665, 50719, 50720, 50829; EXIF = 41486, 41487"""
    buf = bytearray(65536)
    struct.pack_into("<HHI", buf, 0, 0x4949, 42, 8)
    ifd0 = [(256, 4, 1, w), (257, 4, 1, h), (259, 3, 1, 1), (278, 3, 1, h), (279, 4, 1, w * h * 2), (34665, 4, 1, 200),
            (50719, 3, 2, crop[0] | crop[1] << 16), (50720, 3, 2, ((area[2] - area[0]) & 0xFFFF) | ((area[3] - area[1]) & 0xFFFF) << 16),
            (50829, 4, 4, 400)]
    struct.pack_into("<H", buf, 8, len(ifd0))
    for i, e in enumerate(ifd0):
        struct.pack_into("<HHII", buf, 10 + 12 * i, *e)
    struct.pack_into("<H", buf, 200, 2)
    struct.pack_into("<HHII", buf, 202, 41486, 5, 1, 416)
    struct.pack_into("<HHII", buf, 214, 41487, 5, 1, 424)
    struct.pack_into("<4i", buf, 400, area[1], area[0], area[3], area[2])
    struct.pack_into("<4i", buf, 416, *fp)
    return buf


class _Fh:
    class rawi_hdr:
        xRes = yRes = 0


def _fields(w, h, area, crop, stream=0):
    fh = _Fh()
    fh.rawi_hdr = type("R", (), dict(xRes=w, yRes=h))
    buf = _header(w, h, area, crop)
    got = pc.proxy_header(buf, fh, stream)
    t = pc.header_tags(got)
    diff = {i for i in range(65536) if got[i] != buf[i]}
    allowed = set()
    for tag, (at, val) in pc.proxy_tags(pc.header_tags(buf), buf, fh, stream).items():
        allowed |= set(range(at, at + len(val)))
    assert diff <= allowed
    return t, got


def test_the_header_rule_by_hand():
    # 3584x1320 with the area (146, 29) .. (3583, 1319) and the crop origin (7, 3)
    t, got = _fields(3584, 1320, (146, 29, 3583, 1319), (7, 3))
    assert (t[256][2], t[257][2], t[278][2], t[279][2], t[259][2]) == (1792, 660, 660, 1792 * 660 * 2, 1)
    assert t[50719][2] == 4 | 2 << 16                                         # lo(7) = 2 * ceil(7 / 4), lo(3)
    assert struct.unpack_from("<4i", got, 400) == (16, 74, 658, 1790)          # lo(29), lo(146), hi(1319), hi(3583)
    assert t[50720][2] == (1790 - 74) | (658 - 16) << 16
    assert struct.unpack_from("<4i", got, 416) == (5760000, 2922, 3840000, 1944)
    # the whole frame: the whole proxy
    t, got = _fields(1920, 1080, (0, 0, 1920, 1080), (0, 0), stream=12345)
    assert (t[256][2], t[257][2], t[279][2], t[259][2]) == (960, 540, 12345, 7)
    assert struct.unpack_from("<4i", got, 400) == (0, 0, 540, 960) and t[50720][2] == 960 | 540 << 16
    fh = type("F", (), dict(rawi_hdr=type("R", (), dict(xRes=1920, yRes=1080))))
    full = _header(1920, 1080, (0, 0, 1920, 1080), (0, 0))
    assert pc.proxy_header_from_proxy(pc.proxy_header(full, fh), 12345) == got
    # dropped columns and rows bound the area: 1923 -> 960 columns, hi(1923) = 960
    t, got = _fields(1923, 1081, (5, 3, 1923, 1081), (2, 2))
    assert struct.unpack_from("<4i", got, 400) == (2, 4, 540, 960) and t[50719][2] == 2 | 2 << 16
    # an area that vanishes: sizes clamp at 0
    t, got = _fields(16, 16, (9, 9, 11, 11), (0, 0))
    assert struct.unpack_from("<4i", got, 400) == (6, 6, 4, 4) and t[50720][2] == 0


def test_header_cases_cover_what_they_claim():
    cases = pc.header_cases()
    cams = {bytes(fh.idnt_hdr.cameraName).split(b"\0")[0] for _, fh, _, _ in cases}
    assert len(cams) >= 3
    seen = set()
    for label, fh, fps, base in cases:
        ri = fh.rawi_hdr.raw_info
        y1, x1, y2, x2 = (int(v) for v in ri.active_area)
        w, h = int(fh.rawi_hdr.xRes), int(fh.rawi_hdr.yRes)
        inside = x2 <= w and y2 <= h
        if inside and (x1 % 4 or y1 % 4) and x1 and y1:
            seen.add("origin")
        if not inside:
            seen.add("overwrite")
        if int(ri.crop[0]) % 2 and int(ri.crop[1]) % 2:
            seen.add("odd crop")
        if (x2 - x1) / (y2 - y1) > 2.0 and (y2 - y1) <= 720:
            seen.add("5:3")
        elif (x2 - x1) < 2000:
            seen.add("below 2000")
        if w % 4 and h % 4:
            seen.add("dropped")
        # a header recomputed from halved sizes would decide otherwise somewhere: a full-size area of 2000 columns and more whose
        # half is below 2000
        if (x2 - x1) >= 2000 and not ((x2 - x1) / (y2 - y1) > 2.0 and (y2 - y1) <= 720):
            seen.add("halved would bin x3")
    assert seen == {"origin", "overwrite", "odd crop", "5:3", "below 2000", "dropped", "halved would bin x3"}, seen
    assert (0, 100000) in pc.WINDOWS and any(o for o, _ in pc.WINDOWS) and all(o + min(n, 65536) <= 65536 or o == 0 for o, n in pc.WINDOWS)
