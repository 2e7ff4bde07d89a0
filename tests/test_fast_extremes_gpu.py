"""The fused FAST kernel (fast_detect_q_kernel: the one svo_fast_detect and the front
end run) on images that fill its tiles (tests/extreme_images.py): uniform noise
with more than 500 corners in a 64 x 32 tile -- each wave's private queue takes
several 64-entry compaction passes -- and thousands of adjacent corners, whose NMS
decisions are the only place the packed 16-bit score (corner_score16_pk) shows;
0 / 255 images whose corners all score 254, the top of the range, at every
threshold. Keypoint lists equal the oracle's in x, y and response; the scalar
score kernel's maps are bit-exact; cap < n truncates to the oracle's first rows.
test_extreme_images_cpu.py asserts the corner densities these cases claim."""
import functools

import numpy as np
import pytest

import extreme_images as X
import oracle as O
import svo_amd as S

pytestmark = pytest.mark.gpu

THRESHOLDS = (1, 20, 100, 254, 255)


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@functools.lru_cache(maxsize=None)
def _image(key):
    return X.IMAGES[key]()


@pytest.fixture(scope="module")
def device_image(ctx):
    made = {}

    def get(key):
        if key not in made:
            made[key] = ctx.image(_image(key), 0)
        return made[key]

    return get


@pytest.mark.parametrize("nonmax", [True, False], ids=["nms", "all"])
@pytest.mark.parametrize("key", list(X.IMAGES))
def test_fast_keypoints_identical(ctx, device_image, key, nonmax):
    g = device_image(key)
    total = 0
    for t in THRESHOLDS:
        got = ctx.fast_detect(g, t, nonmax)
        ref = O.fast(_image(key), t, nonmax)
        assert got.shape == ref.shape, f"t={t}: {len(got)} keypoints vs {len(ref)}"
        assert np.array_equal(got, ref), f"t={t}: first difference at row {np.nonzero((got != ref).any(1))[0][:5]}"
        total += len(ref)
    if key.startswith(("stripes", "checker")):
        assert total == 0  # no corner at all, at any threshold
    else:
        assert total > 100


@pytest.mark.parametrize("key", list(X.IMAGES))
def test_fast_score_map_bit_exact(ctx, device_image, key):
    """fast_score_kernel (the scalar score): scores up to 254, never produced by the
    rectangle scenes."""
    g = device_image(key)
    top = 0
    for t in THRESHOLDS:
        s, c = ctx.fast_score_map(g, t)
        so, co = O.fast_score(_image(key), t)
        assert np.array_equal(c, co), f"corner map differs at t={t}"
        assert np.array_equal(s, so), f"score map differs at t={t}"
        top = max(top, int(so.max()))
    if key.startswith(("binary", "blocks", "scene")):
        assert top == 254


@pytest.mark.parametrize("nonmax", [True, False], ids=["nms", "all"])
@pytest.mark.parametrize("key", X.NOISE_IMAGES)
def test_fast_with_mask_identical(ctx, device_image, key, nonmax):
    """A mask_boxes mask from every third keypoint: a masked corner is dropped from
    the list but still suppresses its neighbours (the mask acts after NMS)."""
    img = _image(key)
    h, w = img.shape
    full = O.fast(img, 20, True)
    prev = full[::3, :2] + np.float32(0.37)
    m_gpu = ctx.mask_boxes(w, h, prev, 3.0)
    m_ref = O.mask_boxes(w, h, prev, 3.0)
    assert np.array_equal(m_gpu, m_ref)
    assert 0.2 < (m_ref == 0).mean() < 0.9
    got = ctx.fast_detect(device_image(key), 20, nonmax, m_gpu)
    ref = O.fast(img, 20, nonmax, m_ref)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert 0 < len(ref) < len(O.fast(img, 20, nonmax))
    if nonmax:
        # a masked maximum still suppresses: masking the oracle's unmasked NMS list
        # gives the same rows, and masking before NMS would give more
        keep = m_ref[full[:, 1].astype(int), full[:, 0].astype(int)] != 0
        assert np.array_equal(ref, full[keep])
        s, c = O.fast_score(img, 20)
        s2 = np.where(m_ref != 0, s, 0).astype(np.int16)
        p = np.pad(s2, 1)
        nb = np.max([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy],
                    axis=0)
        assert int(((c > 0) & (m_ref != 0) & (s2 > nb)).sum()) > len(ref)


@pytest.mark.parametrize("nonmax", [True, False], ids=["nms", "all"])
def test_fast_cap_truncates_to_the_first_rows(ctx, device_image, nonmax):
    """cap < n: the rows returned are the oracle's first min(n, cap) (raster order)
    and *n_out is still n."""
    key = "noise-161x121"
    ref = O.fast(_image(key), 20, nonmax)
    n = len(ref)
    assert n > 1000
    for cap in (1, 64, n - 1, n, n + 1):
        got, n_out = ctx.fast_detect(device_image(key), 20, nonmax, cap=cap, return_count=True)
        assert n_out == n, f"cap={cap}: n_out {n_out} vs {n}"
        assert len(got) == min(n, cap) and np.array_equal(got, ref[:cap]), f"cap={cap}"
