"""MI355X-native per-hop speech-denoising path (STFT -> mel -> GRUUNet2 -> inverse mel -> Griffin-Lim).

Host side in Python on PyTorch-ROCm tensors; all arithmetic in hand-written HIP kernels for gfx950
behind the C ABI of ``include/dn_denoise.h`` (``lib/libdn_denoise.so``).  Import as
``audio_denoising_amd`` (alias module at the repo root) -- or, for the reference's own import line
``from gruunet2 import GRUUNet2`` (app3.py:38), through the repo-root ``gruunet2.py``.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # ``audio_denoising_amd.SessionPool`` / ``SessionState`` (sessions.py), imported on first use: importing the package stays free of torch
    if name in ("SessionPool", "SessionState", "RateBank"):
        import importlib
        return getattr(importlib.import_module(__name__ + ".sessions"), name)
    # ``audio_denoising_amd.Denoiser`` (``denoise_clip``: a whole clip per call) / ``DenoiserStream`` (``push`` / ``push_many``), likewise
    if name in ("Denoiser", "DenoiserStream"):
        import importlib
        return getattr(importlib.import_module(__name__ + ".pipeline"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
