"""The frames the batched LJ92 encoder (csrc/k_lj92enc.hip, csrc/lj92enc.cpp) is tested at, and a numpy model of how its kernels cut a
frame's bit stream; shared by tests/test_lj92_encode_cases.py (CPU: model, oracle and the reference's encoder and decoder agree on
every case, and every case reaches what its class is there to reach) and tests/test_gpu_lj92_encode_seams.py (GPU: every stream byte
for byte, nothing written outside a stream).

The encoder cuts a frame into blocks of BLOCK pixels (one workgroup each; BLOCK comes from the library itself, through
mlvfs_amd_test_lj92_encode_plan, never from a literal here) and stitches the blocks' bits back together.  Nearly all of its index
arithmetic lives at those seams.  What each class of cases is there to reach -- asserted from the model by the CPU test, so that no
case is vacuous:

  phase    constant frames whose first difference has class s = 0 .. 8, three blocks and a last block of 1 to 7 pixels, at 14 bits and
           one at 16.  The table then has two codes, class 0 = `11` and class s, and every seam falls at bit phase (len[s] + s - 2)
           mod 8 inside a byte that is 0xFF: the byte k_lje_scan_ff counts for the block that begins it.  Every phase 0 .. 7 is met.
           A last block of three pixels is six bits: at phase 1 or 2 they lie inside the byte the block before it began (B0 == B1 in
           k_lje_stuff; one dword under both atomicOr rules in k_lje_emit); at phase 3 and beyond, and with more pixels, the last block
           straddles a byte edge.  (The term `(e & ~7u) >= o[b]` of k_lje_scan_ff is false only for such a last block inside one byte;
           the byte it ends in is the stream's zero-padded last one, never 0xFF, so the term changes no count: Facts.double_count.)
  deep    every row holds the same staircase, so only the frame's first pixels have non-zero differences: class j is used
           Fibonacci(j) times, j = 1 .. K, which gives class 0 -- always the LAST code of the reference's list, all ones -- a code of
           K + 1 bits.  K = 7, 10, 14 at 14 bits and K = 15 at 16 bits: codes of 8, 11, 15 and the full 16 bits.  Behind the staircase
           the stream is 0xFF and nothing else: blocks of more than BLOCK and more than 2 x BLOCK unstuffed bytes (two and three trips
           of k_lje_stuff's chunk loop), chunks of BLOCK bytes that are all 0xFF behind three lead bytes (the most k_lje_stuff's LDS
           ever holds: 3 + 2 x BLOCK of its 2 x BLOCK + 8 bytes), streams longer than the w x h x 3 + 200 bytes the reference's
           encoder allocates.
  narrow   the same two kinds of material at widths 1, 3, 15, 17, BLOCK - 1 and BLOCK + 1: the sixteen pixels of a thread at a
           block seam wrap rows not at all, once and many times, and no row but the first begins on a 16-byte edge (odd widths; the
           GPU test also places whole frames at an odd 16-bit offset).
  blocks   frames of 1023, 1024, 1025 and 2049 blocks, the last block full and not: the scan kernels' threads take one block each
           with the last thread idle (1023) and busy (1024), two with half of the threads idle (1025), three (2049).
  mixed    one batch of eight frames of one geometry at 16 bits: phase, deep and noise frames between a frame with 17-bit differences,
           a frame that uses all 17 classes (both refused by the table builder, as the reference would leave its arrays) and a frame
           whose stream does not fit the room the batch is given.  Every frame has its own table and its own place in the bit buffer.
  room     a frame whose stream length L is a multiple of 4 beside a short neighbour: it fits at out_stride = L and is refused at
           L - 4; the neighbour stands either way.

The yardstick of every stream is the reference's own encoder where the stream fits the w x h x 3 + 200 bytes it allocates, and the
oracle's restatement of it where it does not (tests/test_gpu_lossless_dng.py: _expect)."""
import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np

from mlvfs_amd import lib


def plan(npix: int) -> dict:
    """mlvfs_amd_test_lj92_encode_plan: how the kernels cut a frame of npix pixels"""
    out = (C.c_longlong * 4)()
    rc = lib.load().mlvfs_amd_test_lj92_encode_plan(npix, out)
    assert rc == 0, npix
    return dict(block=int(out[0]), blocks=int(out[1]), threads=int(out[2]), per=int(out[3]))


BLOCK = plan(1)["block"]            # pixels per workgroup (LJE_BLOCK), as the library was built
PER_THREAD = 16                     # pixels of one thread (LJE_PER_THREAD; the CPU test checks BLOCK against 256 threads of them)


class Case(NamedTuple):
    name: str
    cls: str                        # phase, deep, narrow, blocks; mixed and room are built from these (MIXED, ROOM)
    w: int
    h: int
    bits: int
    kind: str                       # const, stairs, two, sparse, noise, diff17
    arg: int = 0                    # const: class of the first difference; stairs: K; two / sparse / noise: seed
    refused: Optional[str] = None   # "table", "diff17": what the encoder answers instead of a stream


def fib(j: int) -> int:
    a, b = 1, 1
    for _ in range(j - 1):
        a, b = b, a + b
    return a


# ------------------------------------------------------------------ material
def _sequence(w, h, bits, mags):
    """Pixel by pixel in raster order: the value whose predictor-6 difference is +mags[i], or -mags[i] where that leaves the range;
    zero behind the list.  With the list inside the first row every later row repeats it (difference 0 everywhere)."""
    top = (1 << bits) - 1
    n = w * h
    v = [0] * n
    for i in range(n):
        r, c = divmod(i, w)
        if r == 0:
            px = v[i - 1] if c else 1 << (bits - 1)
        elif c == 0:
            px = v[i - w]
        else:
            px = v[i - w] + ((v[i - 1] - v[i - w - 1]) >> 1)
        d = mags[i] if i < len(mags) else 0
        p = px + d
        if not 0 <= p <= top:
            p = px - d
        v[i] = min(max(p, 0), top)
    return np.array(v, np.uint16).reshape(h, w)


def stairs_steps(K):
    """class j, Fibonacci(j) times, j = 1 .. K: the smallest magnitude of each class"""
    return [0] + [1 << (j - 1) for j in range(1, K + 1) for _ in range(fib(j))]


def image(c: Case) -> np.ndarray:
    mid = 1 << (c.bits - 1)
    if c.kind == "const":                                   # one difference of class arg, then zeros
        return np.full((c.h, c.w), mid + ((1 << (c.arg - 1)) if c.arg else 0), np.uint16)
    if c.kind == "stairs":
        return _sequence(c.w, c.h, c.bits, stairs_steps(c.arg))
    rng = np.random.default_rng(7000 + c.arg)
    if c.kind == "two":                                     # two values
        return np.where(rng.random((c.h, c.w)) < 0.1, 1016, 1000).astype(np.uint16)
    if c.kind == "sparse":                                  # long runs of zero differences (tests/test_lj92_encode.py: material)
        x = np.full((c.h, c.w), 1000, np.uint16)
        m = rng.random((c.h, c.w)) < 0.01
        x[m] = rng.integers(0, 1 << 14, int(m.sum()))
        return x
    if c.kind == "noise":                                   # 12-bit noise: classes up to 13 or so at any precision
        return rng.integers(0, 1 << 12, (c.h, c.w)).astype(np.uint16)
    assert c.kind == "diff17"                               # differences of 17 bits in rows below the first (tests/test_lj92_encode.py)
    x = np.zeros((c.h, c.w), np.uint16)
    x[:, ::2] = 65535
    x[1::2] = 65535 - x[1::2]
    return x


# ------------------------------------------------------------------ the cases
def _phase():
    w = BLOCK + 1                                           # x 3 rows: three blocks and three pixels
    out = [Case(f"phase s{s} {w}x3", "phase", w, 3, 14, "const", s) for s in range(9)]
    out.append(Case(f"phase s3 {w}x3 16b", "phase", w, 3, 16, "const", 3))
    # last blocks of 1, 2, 4, 5, 6 and 7 pixels: 3 x BLOCK + t = w x h with the smallest h > 1 there is (none: one row)
    for t, s in ((2, 1), (4, 5), (6, 2), (7, 7), (5, 3), (1, 4)):
        n = 3 * BLOCK + t
        hh = next((k for k in range(2, 200) if n % k == 0), 1)
        out.append(Case(f"phase s{s} {n // hh}x{hh} tail{t}", "phase", n // hh, hh, 14, "const", s))
    return out


def _deep():
    return [
        Case(f"deep K7 {BLOCK}x4", "deep", BLOCK, 4, 14, "stairs", 7),
        Case(f"deep K10 {BLOCK}x5", "deep", BLOCK, 5, 14, "stairs", 10),
        Case(f"deep K14 {BLOCK}x4", "deep", BLOCK, 4, 14, "stairs", 14),
        Case(f"deep K15 {2 * BLOCK}x3 16b", "deep", 2 * BLOCK, 3, 16, "stairs", 15),
    ]


NARROW_WIDTHS = (1, 3, 15, 17, BLOCK - 1, BLOCK + 1)


def _narrow():
    out = []
    for k, w in enumerate(NARROW_WIDTHS):
        h = -(-(3 * BLOCK + 3) // w)                         # three blocks and a little
        if w == BLOCK + 1:
            h = 4                                           # (x 3 is a phase case already)
        s = (1, 4, 6, 3, 2, 7)[k]
        out.append(Case(f"narrow s{s} {w}x{h}", "narrow", w, h, 14, "const", s))
        K, bits = ((10, 14), (15, 16), (7, 14), (14, 14), (10, 14), (15, 16))[k]
        out.append(Case(f"narrow K{K} {w}x{h}" + (" 16b" if bits == 16 else ""), "narrow", w, h, bits, "stairs", K))
    return out


def _blocks():
    half = BLOCK // 2
    shapes = [(half - 2, half, "two"), (half - 1, half - 2, "sparse"),         # 1023 blocks, full and not
              (half, half, "sparse"), (half - 1, half + 1, "two"),              # 1024
              (half + 2, half, "two"), (half, half + 1, "sparse"),              # 1025
              (BLOCK, half + 1, "sparse"), (BLOCK + 1, half, "two")]            # 2049
    return [Case(f"blocks {w}x{h} {kind}", "blocks", w, h, 14, kind, 10 + k) for k, (w, h, kind) in enumerate(shapes)]


PHASE, DEEP, NARROW, BLOCKS = _phase(), _deep(), _narrow(), _blocks()
CASES = PHASE + DEEP + NARROW + BLOCKS

# one batch of eight frames of one geometry at 16 bits; MIXED_NOFIT is the frame the batch's room is too small for
_MW, _MH = BLOCK + 1, 3
MIXED = [
    Case("mixed phase s3", "mixed", _MW, _MH, 16, "const", 3),
    Case("mixed diff17", "mixed", _MW, _MH, 16, "diff17", refused="diff17"),
    Case("mixed deep K10", "mixed", _MW, _MH, 16, "stairs", 10),
    Case("mixed noise", "mixed", _MW, _MH, 16, "noise", 1),
    Case("mixed 17 classes", "mixed", _MW, _MH, 16, "stairs", 16, refused="table"),
    Case("mixed deep K7", "mixed", _MW, _MH, 16, "stairs", 7),
    Case("mixed deep K15", "mixed", _MW, _MH, 16, "stairs", 15),
    Case("mixed phase s1", "mixed", _MW, _MH, 16, "const", 1),
]
MIXED_NOFIT = 6


def mixed_room(lengths) -> int:
    """The room per stream the mixed batch is given: every stream but MIXED_NOFIT's fits, with 64 bytes to spare"""
    return (max(n for k, n in enumerate(lengths) if n and k != MIXED_NOFIT) + 3) // 4 * 4 + 64


# the frame whose stream length is a multiple of 4, and its short neighbour (one class: a stream of 0xFF bytes, a quarter as long)
ROOM = [Case("room s2", "room", BLOCK + 1, 3, 14, "const", 2), Case("room s0", "room", BLOCK + 1, 3, 14, "const", 0)]


# ------------------------------------------------------------------ the model
def differences(img: np.ndarray, bits: int):
    """Predictor 6 on the pixels themselves (lj92.c:748-776) -> class and value bits of every pixel, in raster order"""
    p = img.astype(np.int32)
    px = np.empty_like(p)
    px[0, 0] = 1 << (bits - 1)
    px[0, 1:] = p[0, :-1]
    px[1:, 0] = p[:-1, 0]
    px[1:, 1:] = p[:-1, 1:] + ((p[1:, :-1] - p[:-1, :-1]) >> 1)
    d = (p - px).reshape(-1)
    ssss = np.frexp(np.abs(d).astype(np.float64))[1].astype(np.int64)          # bit length
    val = np.where(d < 0, d + (1 << ssss) - 1, d).astype(np.int64) & ((1 << ssss) - 1)
    return ssss, val


class Model(NamedTuple):
    refused: Optional[str]          # "diff17", "table", or None
    hist: np.ndarray                # 18 counters
    len0: int = 0                   # length of class 0's code
    head_len: int = 0               # SOI .. SOS
    off: Optional[np.ndarray] = None        # off[0 .. nb]: where each block's bits begin, off[nb] = the frame's bits
    data: Optional[np.ndarray] = None       # the unstuffed bytes
    ffcum: Optional[np.ndarray] = None      # ffcum[i]: 0xFF bytes among data[:i]

    @property
    def stuffed(self):
        return int(self.ffcum[-1])

    @property
    def length(self):
        return self.head_len + len(self.data) + self.stuffed + 2


def model(img: np.ndarray, bits: int, oracle, block: int = 0) -> Model:
    """The encoder's bit stream as its kernels cut it: the oracle's table for the frame's class histogram, len[class] + class bits per
    pixel, block b's bits from off[b] on"""
    block = block or BLOCK
    ssss, val = differences(img, bits)
    npix = ssss.size
    hist = np.bincount(ssss, minlength=18)
    if hist[17]:
        return Model("diff17", hist)
    t = oracle.lj92_encode_table(hist[:17], npix)
    if t is None:
        return Model("table", hist)
    ln, code = np.array(t["len"], np.int64), np.array(t["code"], np.int64)
    nbits = ln[ssss] + ssss
    word = (code[ssss] << ssss) | val
    pos = np.concatenate(([0], np.cumsum(nbits)))
    total = int(pos[-1])
    # class 0 (most pixels of every case) is len[0] one-bits: runs marked at both ends and summed; the rest bit by bit
    marks = np.zeros((total + 7) // 8 * 8 + 1, np.int8)
    zero = np.nonzero(ssss == 0)[0]
    assert code[0] == (1 << ln[0]) - 1 or not zero.size
    marks[pos[zero]] += 1
    marks[pos[zero] + ln[0]] -= 1
    stream = np.cumsum(marks, dtype=np.int8)[:-1].view(np.uint8)
    sel = np.nonzero(ssss)[0]
    for k in range(int(nbits[sel].max()) if sel.size else 0):
        sel = sel[nbits[sel] > k]
        stream[pos[sel] + k] = (word[sel] >> (nbits[sel] - 1 - k)) & 1
    data = np.packbits(stream)
    nb = -(-npix // block)
    off = pos[np.minimum(np.arange(nb + 1) * block, npix)]
    ffcum = np.concatenate(([0], np.cumsum(data == 0xFF)))
    return Model(None, hist, int(ln[0]), 46 + t["nvalues"], off, data, ffcum)


def unstuff(stream: bytes, head_len: int) -> np.ndarray:
    """The entropy-coded segment of a complete stream without the zero behind every 0xFF"""
    body = np.frombuffer(stream, np.uint8)[head_len:-2]
    keep = np.ones(body.size, bool)
    keep[1:] = body[:-1] != 0xFF
    assert not body[~keep].any()
    return body[keep]


class Facts(NamedTuple):
    nb: int
    seam_phases: frozenset          # bit phases of the seams between blocks
    ff_phases: frozenset            # ... of those inside a byte that is 0xFF (phase != 0)
    last_inside: bool               # the last block's bits lie inside one byte begun before it (k_lje_stuff: B0 == B1)
    last_one_dword: bool            # ... and k_lje_emit stores it as one dword under both atomicOr rules
    last_straddles: bool            # the last block begins inside a byte and ends in a later one
    block_bytes: int                # the most unstuffed bytes of a block
    chunks: Tuple[Tuple[int, int, int], ...]    # distinct (lead, bytes, 0xFF bytes) of k_lje_stuff's chunks
    lds_high: int                   # the most bytes a chunk takes of k_lje_stuff's LDS
    scan_ff_term: int               # blocks for which `(e & ~7) >= o[b]` of k_lje_scan_ff is false
    double_count: int               # ... and the byte is 0xFF: what dropping the term would add to the stream's length


def facts(m: Model, block: int = 0) -> Facts:
    block = block or BLOCK
    off = [int(v) for v in m.off]
    nb = len(off) - 1
    seams = off[1:nb]
    ff = frozenset(e & 7 for e in seams if e & 7 and m.data[e >> 3] == 0xFF)
    begin, end = off[nb - 1], off[nb]
    B0, B1 = (begin + 7) >> 3, (end + 7) >> 3
    lead = begin & 31
    chunks, high = set(), 0
    block_bytes = 0
    term = double = 0
    for b in range(nb):
        b0, b1 = (off[b] + 7) >> 3, (off[b + 1] + 7) >> 3
        block_bytes = max(block_bytes, b1 - b0)
        P = m.head_len + b0 + int(m.ffcum[b0])
        for bc in range(b0, b1, block):
            n = min(block, b1 - bc)
            cf = int(m.ffcum[bc + n] - m.ffcum[bc])
            chunks.add((P & 3, n, cf))
            high = max(high, (P & 3) + n + cf)
            P += n + cf
        e = off[b + 1]
        if e & 7 and (e & ~7) < off[b]:
            term += 1
            double += int(m.data[e >> 3] == 0xFF)
    return Facts(nb, frozenset(e & 7 for e in seams), ff, nb > 1 and bool(begin & 7) and B0 == B1,
                 nb > 1 and bool(begin & 7) and B0 == B1 and bool(lead) and bool(end & 31) and (lead + end - begin + 31) >> 5 == 1,
                 nb > 1 and bool(begin & 7) and B1 > B0, block_bytes, tuple(sorted(chunks)), high, term, double)


def seam_wraps(c: Case, block: int = 0):
    """How many times the sixteen pixels of the first thread of each block but the first wrap to another row"""
    block = block or BLOCK
    return {((i0 % c.w) + min(PER_THREAD, c.w * c.h - i0) - 1) // c.w for i0 in range(block, c.w * c.h, block)}


# ------------------------------------------------------------------ yardsticks (made once per session)
_want, _by_reference = {}, set()


def want(c: Case, oracle, reference=None):
    """The stream the encoder must write: the reference's own where its room holds the stream (and the caller hands the fixture in), the
    oracle's restatement where it does not; None for a frame that is refused"""
    if c not in _want:
        _want[c] = oracle.lj92_encode(image(c), c.w, c.h, c.bits)
    s = _want[c]
    if s is not None and reference is not None and len(s) <= c.w * c.h * 3 + 200 and c not in _by_reference:
        assert reference.lj92_encode_tile(image(c), c.w, c.h, c.bits) == s, c.name
        _by_reference.add(c)
    return s
