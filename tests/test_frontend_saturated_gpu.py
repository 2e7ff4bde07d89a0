"""The batched front end on binarised scenes (starved_cases.Case(binary=True): every
frame 255 where the scene is >= 128, else 0). The geometry and the motion are the
scene's, so the reference loop tracks, fits a pose and tops the set up as ever,
but every edge is a 0 / 255 step: the fused FAST kernel scores 254 on XCD-ordered
tiles under the box mask, and both LK calls sum gradients of +-4080 inside the
step's own launches. Every step against the oracle loop, as
test_frontend_starved_gpu follows its cases: counts, bit-equal feature lists,
poses and map points. (Dense noise frames stay out: they give more corners than
the candidate capacity, which the reference loop does not have.) The oracle-side
conditions (C.assert_saturated_conditions) also run without a GPU, in
test_extreme_images_cpu.py."""
import pytest

import oracle as O
import starved_cases as C
import svo_amd as S
from test_frontend_starved_gpu import _follow, _resident

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


@pytest.fixture
def resident(ctx):
    made = []

    def make(cases, **kw):
        made.append(_resident(ctx, cases, **kw))
        return made[-1]

    yield make
    for fe in made:
        fe.close()


@pytest.mark.parametrize("forward", [False, True], ids=["scene", "forward"])
@pytest.mark.parametrize("n", [64, 300])
def test_saturated_batch(resident, n, forward):
    cases = C.saturated(n, forward)
    C.assert_saturated_conditions(cases)
    _follow(resident(cases), cases)


@pytest.mark.parametrize("forward", [False, True], ids=["scene", "forward"])
@pytest.mark.parametrize("n", [64, 300])
def test_saturated_bucketed(resident, n, forward):
    cases = C.saturated(n, forward, bucket=(50, 4))
    C.assert_saturated_conditions(cases)
    _follow(resident(cases, bucket_size=50, per_bucket=4), cases)


def test_saturated_opencv_order(resident):
    """Both LK calls in OpenCV's float summation order against the oracle loop with
    ACC_SSE (as test_frontend_opencv_order_200_frames_kitti builds it)."""
    cases = C.saturated(300, acc=O.ACC_SSE)
    C.assert_saturated_conditions(cases)
    _follow(resident(cases, lk_flags=S.LK_GET_MIN_EIGENVALS | S.LK_OPENCV_ORDER), cases)
