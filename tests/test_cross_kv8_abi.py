"""The 8-bit cross-KV option's surface, without a GPU: the two C entry points and cross_kv."""
import ctypes
import inspect

import pytest


def test_library_exports_cross_kv8_entry_points():
    from whisper import backend_hip
    lib = ctypes.CDLL(backend_hip.lib_path())
    for name in ("wh_set_cross_kv_format", "wh_read_cross_kv8"):
        assert hasattr(lib, name) and name in backend_hip._EXPORTS, name


def test_python_surface_carries_cross_kv():
    import whisper
    from whisper.backend_hip import HipContext
    for fn in (whisper.load_model, whisper.Whisper.__init__, HipContext.__init__):
        assert inspect.signature(fn).parameters["cross_kv"].default is None, fn
    with pytest.raises(ValueError, match="fp8.*fp32"):
        HipContext({}, dtype="fp32", cross_kv="fp8")
