"""The final fit's sin / cos / acos in plain arithmetic (trig_pa.hpp, svo_trig_pa on
the host) against np.longdouble: correctly rounded as far as a 64-bit significand
can tell, |result - longdouble| <= (1/2 + 2^-9) ulp of the result (half an ulp of
the rounding, and the longdouble's own error of about 2^-11 double ulps), over a
sweep and the edges: acos at |c| -> 1, c = +-1 and c ~ 0; sin / cos at 0, around
every multiple of pi / 2 up to 8 (the reduction's quadrants k = 0 .. 5) and next
to the doubles nearest them. Host code only."""
import numpy as np

import svo_amd as S


def acos_arguments():
    rng = np.random.default_rng(1)
    tiny = 2.0 ** -np.arange(1, 54, dtype=np.float64)
    edge = np.r_[1.0, -1.0, 0.0, -0.0, 1 - tiny, -(1 - tiny), tiny, -tiny, np.nextafter(1.0, 0), np.nextafter(-1.0, 0),
                 np.cos(3.0179), 0.5, -0.5, np.sqrt(0.5), -np.sqrt(0.5)]
    return np.r_[edge, rng.uniform(-1, 1, 20000), 1 - rng.uniform(0, 1e-3, 5000), -1 + rng.uniform(0, 1e-3, 5000),
                 1 - 10.0 ** rng.uniform(-15, -3, 2000), -1 + 10.0 ** rng.uniform(-15, -3, 2000),
                 rng.uniform(-1e-3, 1e-3, 2000)]


def sincos_arguments():
    rng = np.random.default_rng(2)
    near = []
    for k in range(0, 6):
        c = k * (np.pi / 2)
        if c > 8:
            break
        near += [c, np.nextafter(c, 9), np.nextafter(c, 0)] + list(c + rng.uniform(-1e-6, 1e-6, 200)) \
            + list(c + 10.0 ** rng.uniform(-15, -7, 100)) + list((k + 0.5) * (np.pi / 2) + rng.uniform(-1e-9, 1e-9, 50))
    x = np.r_[0.0, 8.0, 2.0 ** -np.arange(1, 60, dtype=np.float64), np.array(near), rng.uniform(0, 8, 30000), 3.0179]
    return x[(x >= 0) & (x <= 8)]


def _ulp_error(got, ref):
    """|got - ref| in ulps of got (ref longdouble)."""
    return np.abs(got.astype(np.longdouble) - ref) / np.spacing(np.abs(got)).astype(np.longdouble)


BOUND = 0.5 + 2.0 ** -9


def test_acos_is_correctly_rounded():
    c = acos_arguments()
    got = S.trig_pa(c, "acos")
    err = _ulp_error(got, np.arccos(c.astype(np.longdouble)))
    print(f"acos: {len(c)} arguments, largest error {float(err.max()):.4f} ulp; "
          f"the maths library's differs on {int((np.arccos(c) != got).sum())}")
    assert float(err.max()) <= BOUND
    assert got[0] == 0.0 and got[1] == np.pi and got[2] == np.pi / 2


def test_sin_and_cos_are_correctly_rounded():
    x = sincos_arguments()
    got = S.trig_pa(x, "sincos")
    xl = x.astype(np.longdouble)
    nz = got != 0
    es = _ulp_error(got[:, 0][nz[:, 0]], np.sin(xl)[nz[:, 0]])
    ec = _ulp_error(got[:, 1][nz[:, 1]], np.cos(xl)[nz[:, 1]])
    print(f"sin / cos: {len(x)} arguments, largest error {float(es.max()):.4f} / {float(ec.max()):.4f} ulp; "
          f"the maths library's differ on {int((np.sin(x) != got[:, 0]).sum())} / {int((np.cos(x) != got[:, 1]).sum())}")
    assert float(es.max()) <= BOUND and float(ec.max()) <= BOUND
    assert got[0, 0] == 0.0 and got[0, 1] == 1.0 and nz[:, 1].all()
    assert np.array_equal(~nz[:, 0], x == 0)  # only sin 0 is 0: no other double is a multiple of pi


def test_outside_the_range_and_refused_arguments():
    x = np.array([-1.0, 9.0, 100.0])
    got = S.trig_pa(x, "sincos")  # the maths library's there
    assert np.array_equal(got[:, 0], np.sin(x)) and np.array_equal(got[:, 1], np.cos(x))
    assert np.isnan(S.trig_pa([np.nan], "acos")[0])
    L = S.lib()
    assert L.svo_trig_pa(None, None, 3, 0, 0, None) == -1 and L.svo_trig_pa(None, None, 0, 0, 0, None) == 0
    one = np.ones(2)
    p = one.ctypes.data_as(S._f64p)
    assert L.svo_trig_pa(None, p, 1, 2, 0, p) == -1 and L.svo_trig_pa(None, p, 1, 0, 1, p) == -1
    assert L.svo_trig_pa(None, p, -1, 0, 0, p) == -1
