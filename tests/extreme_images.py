"""Images at the ends of the pixel range (TEST INFRASTRUCTURE): deterministic,
seeded uint8 generators whose gradients reach +-4080 and whose 64 x 32 tiles
hold hundreds of FAST corners, and numpy restatements (int64) of the sums LK
forms on them -- the Scharr normal matrix, the first iteration's right-hand side
and the SAD error -- so that a test can assert that its inputs reach the range it
is there for (2^31, 2^32, 441 * 4080^2, 2048 * 8160) without asking the code
under test. Shared by test_extreme_images_cpu.py and the *_extremes_gpu.py /
test_frontend_saturated_gpu.py tests."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import oracle as O

W_BITS = 14
IX_MAX = 4080          # |Scharr| of a 0 / 255 edge: (3 + 10 + 3) * 255
IVAL_MAX = 8160        # a pixel x32, as LK stores the prev window
MARGIN = 4             # `pair` cuts its two views this far inside the canvas


def _frozen(a):
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- generators
def stripes4(h, w):
    """Columns 0, 0, 255, 255, ...: |Ix| = 4080 and Iy = 0 at every interior pixel."""
    return _frozen(np.broadcast_to(((np.arange(w) // 2) % 2 * 255).astype(np.uint8), (h, w)))


def checker(h, w, k):
    """k x k blocks, alternately 0 and 255."""
    y, x = np.mgrid[0:h, 0:w]
    return _frozen(((y // k + x // k) % 2 * 255).astype(np.uint8))


def blocks(h, w, k, seed):
    """k x k blocks, each 0 or 255 at random."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 2, ((h + k - 1) // k, (w + k - 1) // k), dtype=np.uint8) * np.uint8(255)
    return _frozen(np.kron(cells, np.ones((k, k), np.uint8))[:h, :w])


def noise(h, w, seed):
    """Uniform 0..255."""
    return _frozen(np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8))


def binary_noise(h, w, seed):
    """Uniform over {0, 255}."""
    return _frozen(np.random.default_rng(seed).integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255))


def inverse(img):
    return _frozen(255 - np.asarray(img, np.uint8))


def binarise(frame):
    """255 where the frame is >= 128, else 0: a scene frame's geometry and motion at
    full contrast."""
    return _frozen(np.where(np.asarray(frame) >= 128, 255, 0).astype(np.uint8))


def pair(img, dx, dy):
    """(prev, next) cut from the canvas `img`, MARGIN px inside it: next(x + dx, y + dy)
    = prev(x, y), a true shift by (dx, dy) with real content moving in at the edges.
    Both are (H - 2 MARGIN, W - 2 MARGIN)."""
    m = MARGIN
    assert abs(dx) <= m and abs(dy) <= m
    H, W = img.shape
    return _frozen(img[m:H - m, m:W - m]), _frozen(img[m - dy:H - m - dy, m - dx:W - m - dx])


def canvas(gen, h, w, *args):
    """gen(...) sized so that `pair` returns h x w views."""
    return gen(h + 2 * MARGIN, w + 2 * MARGIN, *args)


# ---------------------------------------------------------------- exact LK sums
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _weights(a, b):
    """LKTrackerInvoker's rounded bilinear weights of the float32 fractions (a, b)."""
    a, b = np.float32(a), np.float32(b)
    one, s = np.float32(1), np.float32(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _sample(P, x0, y0, ww, wh, wts, shift):
    """The (wh, ww) window with top-left (x0, y0) of the padded int64 plane P,
    bilinear in fixed point, descaled by `shift`."""
    w00, w01, w10, w11 = wts
    r0, r1 = P[y0:y0 + wh], P[y0 + 1:y0 + wh + 1]
    return _descale(r0[:, x0:x0 + ww] * w00 + r0[:, x0 + 1:x0 + ww + 1] * w01 +
                    r1[:, x0:x0 + ww] * w10 + r1[:, x0 + 1:x0 + ww + 1] * w11, shift)


def lk_sums(prev, nxt, pts, win):
    """What calcOpticalFlowPyrLK sums at level 0 for features `pts` of `prev`, the
    guess being the feature itself (max_level 0, no initial flow), in int64:
      a11, a12, a22   sum Ix^2, Ix Iy, Iy^2 over the window (Scharr of O.scharr,
                      zero outside the image, as OpenCV's derivative level)
      b1, b2          sum (J - I) Ix, (J - I) Iy of the first iteration (I, J x32)
      sad             sum |J - I| (x32): flags 0's error before any step
      inside          the window's top-left pixel passes OpenCV's bounds test
    At integer positions (odd windows) the bilinear weights are (2^14, 0, 0, 0):
    the samples are the pixels themselves and the sums have no rounding in them."""
    prev, nxt = np.asarray(prev, np.uint8), np.asarray(nxt, np.uint8)
    h, w = prev.shape
    ww, wh = win
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    pad = ((wh, wh), (ww, ww))
    I = np.pad(prev, pad, mode="reflect").astype(np.int64)
    J = np.pad(nxt, pad, mode="reflect").astype(np.int64)
    d = O.scharr(prev).astype(np.int64)
    Dx, Dy = np.pad(d[..., 0], pad), np.pad(d[..., 1], pad)
    n = len(pts)
    out = SimpleNamespace(inside=np.zeros(n, bool), **{k: np.zeros(n, np.int64) for k in
                                                       ("a11", "a12", "a22", "b1", "b2", "sad")})
    half = np.array([(ww - 1) * 0.5, (wh - 1) * 0.5], np.float32)
    for i, p in enumerate(pts):
        q = p - half  # float32
        ix, iy = int(np.floor(q[0])), int(np.floor(q[1]))
        if ix < -ww or ix >= w or iy < -wh or iy >= h:
            continue
        out.inside[i] = True
        wts = _weights(q[0] - np.float32(ix), q[1] - np.float32(iy))
        x0, y0 = ix + ww, iy + wh
        iv = _sample(I, x0, y0, ww, wh, wts, W_BITS - 5)
        jv = _sample(J, x0, y0, ww, wh, wts, W_BITS - 5)
        gx = _sample(Dx, x0, y0, ww, wh, wts, W_BITS)
        gy = _sample(Dy, x0, y0, ww, wh, wts, W_BITS)
        diff = jv - iv
        out.a11[i], out.a12[i], out.a22[i] = (gx * gx).sum(), (gx * gy).sum(), (gy * gy).sum()
        out.b1[i], out.b2[i] = (diff * gx).sum(), (diff * gy).sum()
        out.sad[i] = np.abs(diff).sum()
    return out


FLT_SCALE = np.float32(1.0 / (1 << 20))
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)


def min_eig_f32(a11, a12, a22, win):
    """oracle/lk.c's (LKTrackerInvoker's) float32 evaluation, operation by operation,
    of the exact sums: (minEig, D)."""
    A11 = a11.astype(np.float32) * FLT_SCALE  # int64 -> float32 rounds to nearest even, as (float)int64
    A12 = a12.astype(np.float32) * FLT_SCALE
    A22 = a22.astype(np.float32) * FLT_SCALE
    D = A11 * A22 - A12 * A12
    dif = A11 - A22
    me = (A22 + A11 - np.sqrt(dif * dif + np.float32(4) * A12 * A12)) / np.float32(2 * win[0] * win[1])
    return me, D


# ---------------------------------------------------------------- points
def border_points(w, h, seed=0):
    """test_lk_borders_and_out_of_image's set scaled to (w, h): 400 uniform points
    reaching 40 px outside, the four corners' neighbourhoods and points whose window
    just touches / just misses the image."""
    rng = np.random.default_rng(seed)
    return np.concatenate([
        np.c_[rng.uniform(-40, w + 40, 400), rng.uniform(-40, h + 40, 400)],
        np.array([[0, 0], [w - 1, h - 1], [-21, 5], [5, -21], [-20.5, 3], [w + 19.9, h / 2], [w / 2, h + 19.5]]),
    ]).astype(np.float32)


def integer_points(w, h, n, seed, margin=0):
    rng = np.random.default_rng(seed)
    return np.c_[rng.integers(margin, w - margin, n), rng.integers(margin, h - margin, n)].astype(np.float32)


def subpixel_points(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(0, w, n), rng.uniform(0, h, n)].astype(np.float32)


def half_points(w, h, n, seed, margin=0):
    """Features at k + 0.5: the window's top-left pixel is an integer for an even
    window (half = 15.5 at 32 columns), the weights (2^14, 0, 0, 0)."""
    return integer_points(w, h, n, seed, margin) + np.float32(0.5)


def speckled(img, seed, one_in=40, amp=12):
    """`img` with one pixel in `one_in` moved `amp` grey levels inwards (0 -> amp,
    255 -> 255 - amp): stripes keep |Ix| ~ 4080 and gain the little Iy that lets a
    window pass LK's minimum-eigenvalue test, so its iterations run."""
    rng = np.random.default_rng(seed)
    out = np.array(img, np.int16)
    hit = rng.integers(0, one_in, out.shape) == 0
    out[hit] += np.where(out[hit] < 128, amp, -amp).astype(np.int16)
    return _frozen(out.astype(np.uint8))


# ---------------------------------------------------------------- LK cases
LK_W, LK_H = 320, 240


def _scene(seed=4):
    from svo_amd.scene import Scene
    return Scene(LK_W, LK_H, seed=seed)


def _blocks_pair(k, dx, dy):
    return lambda: pair(canvas(blocks, LK_H, LK_W, k, 10 + k), dx, dy)


def _blocks_inverse(k):
    def make():
        a = blocks(LK_H, LK_W, k, 10 + k)
        return a, inverse(a)
    return make


# name -> () -> (prev, next), all LK_W x LK_H
LK_PAIRS = {
    "stripes4-shift1": lambda: pair(canvas(stripes4, LK_H, LK_W), 1, 0),
    "stripes4-speckled-shift1": lambda: pair(speckled(canvas(stripes4, LK_H, LK_W), 9), 1, 0),
    "checker2-shift1": lambda: pair(canvas(checker, LK_H, LK_W, 2), 1, 0),
    "scene-binary-temporal": lambda: (binarise(_scene().frame(0)), binarise(_scene().frame(1))),
    "scene-binary-stereo": lambda: (binarise(_scene().frame(0)), binarise(_scene().right(0))),
}
for _k in (2, 4, 8):
    LK_PAIRS[f"blocks{_k}-shift(1,1)"] = _blocks_pair(_k, 1, 1)
    LK_PAIRS[f"blocks{_k}-shift(3,-2)"] = _blocks_pair(_k, 3, -2)
    LK_PAIRS[f"blocks{_k}-inverse"] = _blocks_inverse(_k)


@functools.lru_cache(maxsize=None)
def lk_pair(name):
    return LK_PAIRS[name]()


N_INT, N_SUB = 200, 200


@functools.lru_cache(maxsize=None)
def lk_points(w=LK_W, h=LK_H, seed=0):
    """About 200 features at integer positions (the first N_INT), about 200 at random
    sub-pixel positions, then the border / outside set."""
    p = np.concatenate([integer_points(w, h, N_INT, seed + 1), subpixel_points(w, h, N_SUB, seed + 2),
                        border_points(w, h, seed)])
    p.setflags(write=False)
    return p


# ---------------------------------------------------------------- FAST statistics
def tile_stats(corner):
    """(corners in the fullest 64 x 32 tile, adjacent -- 8-connected -- corner pairs)."""
    c = corner.astype(bool)
    h, w = c.shape
    fullest = max(int(c[y:y + 32, x:x + 64].sum()) for y in range(0, h, 32) for x in range(0, w, 64))
    pairs = int((c[:, 1:] & c[:, :-1]).sum() + (c[1:] & c[:-1]).sum() +
                (c[1:, 1:] & c[:-1, :-1]).sum() + (c[1:, :-1] & c[:-1, 1:]).sum())
    return fullest, pairs


# the FAST tests' images by name (each call builds the same array)
IMAGES = {
    "noise-161x121": lambda: noise(121, 161, 1),
    "noise-320x240": lambda: noise(240, 320, 2),
    "noise-401x203": lambda: noise(203, 401, 3),
    "binary-noise-320x240": lambda: binary_noise(240, 320, 4),
    "blocks2-161x121": lambda: blocks(121, 161, 2, 5),
    "blocks3-320x240": lambda: blocks(240, 320, 3, 6),
    "blocks5-401x203": lambda: blocks(203, 401, 5, 7),
    "checker2-161x121": lambda: checker(121, 161, 2),
    "stripes4-161x121": lambda: stripes4(121, 161),
    "scene-binary-320x240": lambda: binarise(_scene_frame(320, 240, 4, 0)),
}
NOISE_IMAGES = ("noise-161x121", "noise-320x240", "noise-401x203")


def _scene_frame(w, h, seed, t):
    from svo_amd.scene import Scene
    return Scene(w, h, seed=seed).frame(t)
