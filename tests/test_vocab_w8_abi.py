"""vocab="fp8" without a GPU: the two entry points are declared, exported and bound, the keyword
exists with default None, and an fp32 context is refused before the library is touched."""
import ctypes
import inspect

import pytest

from test_abi import _declared

NAMES = ("wh_set_vocab_format", "wh_read_vocab_w8")


def test_symbols_declared_exported_and_bound():
    from whisper import backend_hip
    lib = ctypes.CDLL(backend_hip.lib_path())
    for name in NAMES:
        assert name in _declared() and hasattr(lib, name) and name in backend_hip._EXPORTS, name


def test_vocab_keyword_defaults_to_none():
    import whisper
    from whisper.backend_hip import HipContext
    for f in (whisper.load_model, whisper.Whisper.__init__, HipContext.__init__):
        assert inspect.signature(f).parameters["vocab"].default is None, f


def test_fp32_context_refused_before_the_library(monkeypatch):
    from whisper import backend_hip, synthetic as S
    monkeypatch.setattr(backend_hip, "load_library", lambda: pytest.fail("the library was touched"))
    with pytest.raises(ValueError, match="vocab='fp8' needs dtype='fp16'"):
        backend_hip.HipContext(S.MODEL_DIMS["micro"], dtype="fp32", vocab="fp8")
