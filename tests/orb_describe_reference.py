"""The ORB descriptor and Hamming matcher rules of DESIGN.md section 3d, restated
in plain numpy (CPU only): what svo_orb_compute, svo_orb_blur_level,
svo_match_hamming and svo_match_filter must return bit for bit.

Nothing here calls sin, cos or atan2 on the way to a descriptor bit, and no value
depends on whether a multiply-add is fused: the moments are exact integers, c and
s are one correctly rounded f64 square root and division each, the steered
coordinates are exact products and one rounded addition. The reported angle alone
uses atan2 (informational; compared to 1e-3 degree).

Level images come from the oracle's INTER_LINEAR_EXACT resize chain (level l from
level l-1), the pyramid svo_orb_detect builds.
"""
import math

import numpy as np

DESC_BYTES = 32
BLUR_W = np.array([18, 34, 49, 54, 49, 34, 18], np.int64)  # sigma 2, 8-bit weights, sum 256
RNG_SEED = 0x34985739
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


# ------------------------------------------------------------------ tables
def half_patch(patch_size):
    if patch_size % 2 == 0 or not 5 <= patch_size <= 31:
        raise ValueError("patch_size must be odd and in [5, 31]")
    return patch_size // 2


def reach(patch_size):
    """cvRound(hp * sqrt 2): how far a steered pattern point can land from the centre."""
    return int(np.rint(half_patch(patch_size) * math.sqrt(2.0)))


def umax(patch_size):
    """OpenCV's circular patch: row |v| spans |u| <= umax[|v|] (hp + 1 entries)."""
    hp = half_patch(patch_size)
    u = [0] * (hp + 2)
    vmax = int(math.floor(hp * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(hp * math.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        u[v] = int(np.rint(math.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return np.array(u[: hp + 1], np.int32)


class Mwc:
    """cv::RNG: multiply-with-carry; uniform(a, b) = a + next() % (b - a)."""

    def __init__(self, state):
        self.state = state & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a if a == b else a + self.next() % (b - a)


def default_pattern(patch_size):
    """makeRandomPattern: 512 points (x, y) int8, x drawn before y, each in [-hp, hp]."""
    hp = half_patch(patch_size)
    rng = Mwc(RNG_SEED)
    out = np.empty((512, 2), np.int8)
    for i in range(512):
        out[i, 0] = rng.uniform(-hp, hp + 1)
        out[i, 1] = rng.uniform(-hp, hp + 1)
    return out


# ------------------------------------------------------------------ blur
def reflect101(i, n):
    """BORDER_REFLECT_101 index of i (array or int) into [0, n), reflected as often as
    a level narrower than the kernel needs; a one-pixel axis reads its only pixel."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def blur(img):
    """Separable 7-tap blur: h = sum w p (u16), out = (sum w h + 32768) >> 16."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    xs = reflect101(np.arange(w)[:, None] + np.arange(-3, 4)[None, :], w)  # (w, 7)
    hor = (img.astype(np.int64)[:, xs] * BLUR_W).sum(axis=2)               # (h, w)
    assert hor.max() <= 65535
    ys = reflect101(np.arange(h)[:, None] + np.arange(-3, 4)[None, :], h)  # (h, 7)
    ver = (hor[ys, :] * BLUR_W[None, :, None]).sum(axis=1)                 # (h, w)
    return ((ver + 32768) >> 16).astype(np.uint8)


def levels_of(img, scale_factor=1.2, nlevels=8, nfeatures=150):
    """([level images], lscale f32): the scale pyramid svo_orb_detect builds."""
    import oracle as O
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    lw, lh, ls, _ = O.orb_level_info(w, h, scale_factor, nlevels, nfeatures)
    lv = [img]
    for l in range(1, nlevels):
        lv.append(O.resize_linear_exact(lv[-1], int(lw[l]), int(lh[l])))
    return lv, ls.astype(np.float32)


# ------------------------------------------------------------------ descriptor
def level_pixel(x, lscale):
    """cvRound(x * (1.f / lscale)) in f32, half to even."""
    inv = np.float32(1.0) / np.float32(lscale)
    return int(np.rint(np.float32(np.float32(x) * inv)))


def moments(level, cx, cy, patch_size):
    hp = half_patch(patch_size)
    um = umax(patch_size)
    m10 = m01 = 0
    for v in range(-hp, hp + 1):
        d = int(um[abs(v)])
        row = level[cy + v, cx - d: cx + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


def direction(m10, m01):
    """(c, s) f64 and the angle in degrees [0, 360) as f32."""
    r2 = m10 * m10 + m01 * m01
    if r2 == 0:
        c, s = 1.0, 0.0
    else:
        hyp = np.sqrt(np.float64(r2))
        c, s = float(np.float64(m10) / hyp), float(np.float64(m01) / hyp)
    a = math.degrees(math.atan2(float(m01), float(m10)))
    if a < 0:
        a += 360.0
    return c, s, np.float32(a)


def describe_at(level, blurred, cx, cy, pattern, patch_size):
    """(32 descriptor bytes, angle) of the valid level pixel (cx, cy)."""
    c, s, ang = direction(*moments(level, cx, cy, patch_size))
    px = pattern[:, 0].astype(np.float64)
    py = pattern[:, 1].astype(np.float64)
    ix = np.rint(px * c - py * s).astype(np.int64)
    iy = np.rint(px * s + py * c).astype(np.int64)
    smp = blurred[cy + iy, cx + ix]
    bits = (smp[0::2] < smp[1::2]).astype(np.uint8)  # test t compares points 2t and 2t + 1
    return np.packbits(bits, bitorder="little"), ang


def compute(levels, blurred, lscale, kp_xy, octave, patch_size=31, pattern=None):
    """svo_orb_compute: (desc (n, 32) u8, angle (n,) f32, valid (n,) u8)."""
    pattern = default_pattern(patch_size) if pattern is None else np.asarray(pattern, np.int8).reshape(512, 2)
    rch = reach(patch_size)
    n = len(octave)
    desc = np.zeros((n, DESC_BYTES), np.uint8)
    angle = np.full(n, -1.0, np.float32)
    valid = np.zeros(n, np.uint8)
    for i in range(n):
        l = int(octave[i])
        lh, lw = levels[l].shape
        cx, cy = level_pixel(kp_xy[i][0], lscale[l]), level_pixel(kp_xy[i][1], lscale[l])
        if not (rch <= cx <= lw - 1 - rch and rch <= cy <= lh - 1 - rch):
            continue
        desc[i], angle[i] = describe_at(levels[l], blurred[l], cx, cy, pattern, patch_size)
        valid[i] = 1
    return desc, angle, valid


def describe_image(img, kp_xy, octave, scale_factor=1.2, nlevels=8, patch_size=31, pattern=None):
    lv, ls = levels_of(img, scale_factor, nlevels)
    return compute(lv, [blur(a) for a in lv], ls, kp_xy, octave, patch_size, pattern)


# ------------------------------------------------------------------ matcher
def hamming(q, t):
    """(nq, nt) int32 popcounts of the xor."""
    q = np.asarray(q, np.uint8).reshape(-1, DESC_BYTES)
    t = np.asarray(t, np.uint8).reshape(-1, DESC_BYTES)
    return _POP8[q[:, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)


def knn2_scan(d):
    """The rule as stated: scan the train indices upward, strict < for both places."""
    d1, i1, d2, i2 = 257, -1, 257, -1
    for t, v in enumerate(d):
        v = int(v)
        if v < d1:
            d1, i1, d2, i2 = v, t, d1, i1
        elif v < d2:
            d2, i2 = v, t
    return i1, i2, d1, d2


def knn2(q, t):
    """svo_match_hamming of one problem: (idx (nq, 2) i32, dist (nq, 2) i32). The
    lowest index of the minimum, then the lowest index of the minimum of the rest:
    what the upward scan with strict < leaves (knn2_scan; a displaced best has the
    lower index of any equal second)."""
    q = np.asarray(q, np.uint8).reshape(-1, DESC_BYTES)
    t = np.asarray(t, np.uint8).reshape(-1, DESC_BYTES)
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), 257, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    d = hamming(q, t)
    r = np.arange(nq)
    idx[:, 0] = d.argmin(axis=1)
    dist[:, 0] = d[r, idx[:, 0]]
    if nt > 1:
        d2 = d.copy()
        d2[r, idx[:, 0]] = 1 << 20
        idx[:, 1] = d2.argmin(axis=1)
        dist[:, 1] = d2[r, idx[:, 1]]
    return idx, dist


def match_filter(idx_qt, dist_qt, idx_tq=None, ratio_pct=80):
    """svo_match_filter: pairs (q, t) in ascending q, integers only."""
    out = []
    for q in range(len(idx_qt)):
        i1, i2 = int(idx_qt[q][0]), int(idx_qt[q][1])
        if i1 < 0:
            continue
        if ratio_pct != 0 and not (i2 >= 0 and int(dist_qt[q][0]) * 100 < ratio_pct * int(dist_qt[q][1])):
            continue
        if idx_tq is not None and int(idx_tq[i1][0]) != q:
            continue
        out.append((q, i1))
    return np.array(out, np.int32).reshape(-1, 2)
