"""encoder="fp8" without a GPU: the ABI symbols are in the built library, and the options that
cannot work are refused by name before any context is created."""
import pytest


@pytest.mark.parametrize("symbol", ["wh_set_encoder_format", "wh_encoder_kernels", "wh_fp8_linear"])
def test_symbols_exist(symbol):
    from whisper import backend_hip
    assert hasattr(backend_hip.load_library(), symbol)


@pytest.mark.parametrize("dtype,encoder,match", [("fp32", "fp8", "encoder='fp8'.*fp32"), ("fp16", "int4", "encoder='int4'")])
def test_refused_by_name(dtype, encoder, match):
    import whisper
    from whisper import synthetic as S
    with pytest.raises(ValueError, match=match):
        whisper.Whisper(whisper.ModelDimensions(**S.MODEL_DIMS["micro"]), "micro", dtype=dtype, encoder=encoder)
