"""flac_amd — MI355X-native FLAC encode-analysis for turlando/flac-py's encode() API.

The per-block analysis (fixed predictor search, Tukey-windowed autocorrelation,
Levinson-Durbin, LPC quantisation, candidate residuals, subframe choice and Rice
partition search) runs as HIP kernels in ``libflacmi.so`` behind a C-ABI
(``include/flacmi.h``); the encoder entry point, the Subframe/Residual dataclasses
and the bitstream writer keep flac-py's interface (flac/encoder.py, flac/common.py).  ``flac_amd.decoder``
is flac/decoder.py's ``decode`` over the device stream decoder; ``flac_amd.analyze`` /
``flac_amd.summarize`` (``flac_amd.info``) report what a .flac holds, frame by frame.
"""
__version__ = "0.1.0"

_INFO = ("analyze", "summarize", "StreamReport", "FrameReport", "SubframeReport")
__all__ = list(_INFO)


def __getattr__(name):
    # flac_amd.info loaded on first use: importing the package stays free of numpy and the library
    if name in _INFO:
        from importlib import import_module
        return getattr(import_module(__name__ + ".info"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
