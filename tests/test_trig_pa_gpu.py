"""trig_pa.hpp on the device (svo_trig_pa device = 1) against the host: the same
bits on every argument of test_trig_pa_cpu.py -- what the device fit's bit-identity
with the host fit rests on."""
import numpy as np
import pytest

import svo_amd as S
from test_trig_pa_cpu import acos_arguments, sincos_arguments

pytestmark = pytest.mark.gpu


def test_device_bits_are_host_bits():
    ctx = S.Context(0)
    for fn, x in (("acos", acos_arguments()), ("sincos", sincos_arguments())):
        host, dev = S.trig_pa(x, fn), S.trig_pa(x, fn, ctx)
        bad = np.nonzero(host.view(np.uint64) != dev.view(np.uint64))[0]
        assert len(bad) == 0, f"{fn}: {len(bad)} of {len(x)} differ, first at x = {x[bad[0] // (2 if fn == 'sincos' else 1)]!r}"
    assert S.trig_pa([], "acos", ctx).shape == (0,)
