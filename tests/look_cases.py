"""A look for the rendered frames (include/mlvfs_amd.h, "a look for the rendered frames"): the cases the CPU and GPU
tests share.  The definition itself is mlvfs_amd/look.py.  tests/test_look_cases.py proves that the cases reach what they claim and
that each of five wrong definitions changes some byte of them."""
import itertools

import numpy as np

from mlvfs_amd import look, render

import render_cases as rc

NS = (2, 3, 17, 33, 65)

# shaper values the chosen triples are made of: both ends, the steps of 4d (with the edge table u = 128 | 129 give v = 128 | 129, and
# u = 65407 | 65408 give v = 65406 | 65407), the step of 4c (f = 32767 | 32768 at N = 2), a cell boundary at N = 3 and its neighbours, thirds (cell boundaries at N = 4, ...), others
U = [0, 1, 128, 129, 0x7FFF, 0x8000, 0x8001, 21845, 43690, 65407, 65408, 0xFFFE, 0xFFFF, 1000, 30000, 50001]


def case_shaper(seed=0):
    """4096 random 16-bit values -- not monotone --, the first len(U) of them U: index k < len(U) reads U[k]"""
    S = np.random.default_rng(7000 + seed).integers(0, 65536, 4096, dtype=np.uint16)
    S[:len(U)] = U
    return S


def case_triples():
    """every triple of indices below len(U): (3, len(U)^3) -- all six orders of three distinct fractions, every pair equal above and
    below the third, all three equal, all zero, each axis at its first and at its last cell"""
    return np.array(list(itertools.product(range(len(U)), repeat=3)), np.int64).T.copy()


def random_triples(count=100000, seed=0):
    return np.random.default_rng(7100 + seed).integers(0, 4096, (3, count), dtype=np.int64)


def random_table(n, seed=0):
    return np.random.default_rng(7200 + 100 * n + seed).integers(0, 65536, (n ** 3, 3), dtype=np.uint16)


def edge_table():
    """N = 2, so that f = u.  Along red from (0, 0, 0) to (1, 0, 0): R goes 0 -> 1, so v_R = (f_r + 32768) >> 16 steps at f_r = 32768
    (4c); G goes 0 -> 65535, so v_G is f_r to within 1 and out_G steps between v = 128 and 129 (4d); B goes 65535 -> 0.  The other
    six vertices are random."""
    T = random_table(2, 9)
    T[0] = (0, 0, 65535)
    T[1] = (1, 65535, 0)
    return T


def looks():
    """[(name, S, N, T)]: a random table at every N behind the case shaper; the edge table; an all-zero and an all-65535 table; 65535
    throughout behind S = 65535 throughout; a random table behind the linear shaper; the identity behind the sRGB shaper"""
    out = [(f"random{n}", case_shaper(n), n, random_table(n)) for n in NS]
    out.append(("edge2", case_shaper(1), 2, edge_table()))
    out.append(("zero3", case_shaper(2), 3, np.zeros((27, 3), np.uint16)))
    out.append(("white17", case_shaper(3), 17, np.full((17 ** 3, 3), 65535, np.uint16)))
    out.append(("allwhite5", np.full(4096, 65535, np.uint16), 5, np.full((125, 3), 65535, np.uint16)))
    out.append(("linear33", look.shaper_linear(), 33, random_table(33, 1)))
    out.append(("identity17", look.shaper_srgb(), 17, look.identity(17)))
    return out


def look_of(name):
    return next(l[1:] for l in looks() if l[0] == name)


# ---- the wrong definitions: each must change some byte of the cases
def _object(a):
    return np.asarray(a).astype(object)


def wrong(kind, t, S, n, T):
    """step 4 done wrongly in one respect: uint8 of t's shape (3, count)"""
    st = look.stages(t, S, n, T)
    i, f = st["i"], st["f"]
    Tl = np.asarray(T, np.int64).reshape(n ** 3, 3)
    base = (i[2] * n + i[1]) * n + i[0]
    stride = (1, n, n * n)
    if kind == "red_slowest":                                    # T[(r N + g) N + b]
        return look.apply(t, S, n, Tl.reshape(n, n, n, 3).transpose(2, 1, 0, 3).reshape(-1, 3))
    if kind == "shift8":                                         # out = v >> 8
        return (st["v"] >> 8).astype(np.uint8)
    if kind == "fixed_order":                                    # a, b, c = r, g, b whatever the fractions
        w = [65536 - f[0], f[0] - f[1], f[1] - f[2], f[2]]
        at = [base, base + 1, base + 1 + n, base + 1 + n + n * n]
        v = np.clip((sum(w[j][:, None] * Tl[at[j]] for j in range(4)) + 32768) >> 16, 0, 65535).T
        return ((v + 128) // 257).astype(np.uint8)
    if kind == "w65535":                                         # weights that sum to 65535, divided by it
        fs = np.take_along_axis(f, st["order"], 0)
        fs = np.minimum(fs, 65535)
        w = [65535 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2]]
        o = st["order"]
        at = [base, base + np.array(stride)[o[0]], base + np.array(stride)[o[0]] + np.array(stride)[o[1]], base + 1 + n + n * n]
        v = ((sum(w[j][:, None] * Tl[at[j]] for j in range(4)) + 32767) // 65535).T
        return ((v + 128) // 257).astype(np.uint8)
    if kind == "trilinear":                                      # all eight vertices, weights the products of the three axes'
        acc = np.zeros(t.shape[1:] + (3,), object)
        for db, dg, dr in itertools.product((0, 1), repeat=3):
            w = _object(f[0] if dr else 65536 - f[0]) * _object(f[1] if dg else 65536 - f[1]) * _object(f[2] if db else 65536 - f[2])
            acc = acc + w[:, None] * _object(Tl[base + dr + dg * n + db * n * n])
        v = ((acc + (1 << 47)) // (1 << 48)).astype(np.int64).T
        return ((v + 128) // 257).astype(np.uint8)
    raise ValueError(kind)


WRONG = ("trilinear", "red_slowest", "w65535", "shift8", "fixed_order")


# ---- frames: the shapes at which each of the six look kernels runs, smallest first (tests/test_gpu_look.py)
HALF_SIZES = [(2, 2), (7, 5), (16, 4), (48, 4), (1040, 4)]
FULL_SIZES = [(4, 4), (7, 5), (16, 4), (528, 33)]
SCALED_SIZES = [((16, 4), (3, 1)), ((48, 8), (24, 4)), ((1040, 6), (100, 2))]
BIG_W, BIG_H = rc.BIG_W, rc.BIG_H

# (frames, source offset, destination offset, aligned strides): each x16 kernel and each generic kernel at every shape either could
# take, batches of 1 and 3 with different parameters per frame.  The middle frame of a batch of 3 takes the largest K a forward matrix
# of shorts can give, which does not fit 32 bits: both matrix paths meet in one batch (tests/test_look_cases.py checks that)
PLACEMENTS = [(3, 0, 0, True), (3, 2, 3, False), (1, 16, 8, True), (1, 2, 1, False)]
BIG_K = render.params(0, 65535, (1, 1) * 3, (32767, -32768, 32767) * 3, 256)[4:]


def frame_cases(w, h, first=0):
    """[(frames with parameters, src_off, dst_off, aligned, look name)]: one look per launch, another for every launch"""
    names = [l[0] for l in looks()]
    out = []
    for k, (n, src_off, dst_off, aligned) in enumerate(PLACEMENTS):
        batch = rc.batch(w, h, n, first + k)
        if n == 3:
            batch[1] = (batch[1][0], batch[1][1][:4] + BIG_K)
        out.append((batch, src_off, dst_off, aligned, names[(first + k + w) % len(names)]))
    return out


def cube_text(n, table, title="a test", digits=10):
    """a .cube file of the table: each value as q / 65535 with enough digits to quantise back to q"""
    rows = ["TITLE \"%s\"" % title, "# written by the test", "", "LUT_3D_SIZE %d" % n, "DOMAIN_MIN 0 0 0", "DOMAIN_MAX 1.0 1.0 1.0"]
    rows += ["%.*f %.*f %.*f" % (digits, r / 65535, digits, g / 65535, digits, b / 65535) for r, g, b in np.asarray(table).reshape(-1, 3).tolist()]
    return "\n".join(rows) + "\n"
