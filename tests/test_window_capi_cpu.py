"""The observation window's C ABI on a CPU-only host: include/svo_gpu.h declares,
the library exports and the Python wrapper binds the four symbols (no compute
calls: there is no GPU here)."""
import ctypes

import svo_amd as S
from test_capi import declared_symbols

NEW = ["svo_ba_stage_lists", "svo_frontend_bundle_adjust", "svo_frontend_window", "svo_frontend_window_enable"]


def test_header_declares_the_window_symbols():
    assert set(NEW) <= set(declared_symbols())


def test_library_exports_the_window_symbols():
    lib = ctypes.CDLL(S.lib_path())
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_binds_the_window_symbols():
    assert set(NEW) <= set(S.SYMBOLS)
    for name in ("window_enable", "window", "bundle_adjust"):
        assert callable(getattr(S.Frontend, name)), name
    assert callable(S.Context.ba_stage_lists)


def test_calls_refuse_null_handles():
    """Argument checks that need no device."""
    lib = S.lib()
    assert lib.svo_frontend_window_enable(None, 4) == -1  # SVO_ERR_ARG
    assert lib.svo_frontend_window(None, 0, 0, None, None, None, None, None, None) == -1
    assert lib.svo_frontend_bundle_adjust(None, 2, 0.0, 5, None, None, None) == -1
    assert lib.svo_ba_stage_lists(None, 1, 1, 1, None, None, None, None, None, None, None, None, None, None, None,
                                  None) == -1
