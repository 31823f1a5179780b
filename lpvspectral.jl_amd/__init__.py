"""MI355X-native regression-matrix + ADMM hot path of LPVSpectral.jl.

The product is ``liblpvspectral.so`` (hand-written HIP for gfx950 behind the C-ABI of
``include/lpvspectral.h``); this package is the host-side mirror of the reference's Julia API
(same names / keywords) used by the parity tests and the benchmark.  No CPU fallback exists:
importing without the built library raises ImportError, calling without a GPU raises DeviceError.
"""
from ._lib import DeviceError, DomainError, NumericError, lib as _load

_load()  # fail loudly at import time if the HIP extension is missing

from .api import (MFCC, MelSpectrogram, Spectrogram, dct_matrix, fft_frequencies, freq, hz_to_mel, mel, mel_frequencies, mel_to_hz,  # noqa: E402
                  melspectrogram, mfcc, nextfastfft, spectrogram, stft_last_timing, time,
                  Periodogram, welch_pgram, periodogram, compress, compress_thresholds, heatmap, compress_last_timing,
                  lombscargle, lombscargle_last_timing, lombscargle_terms_last_timing, lombscargle_spectrogram, lombscargle_welch, lombscargle_windows_last_timing, time_windows,
                  WWZ, wwz, wwz_radius, wwz_last_timing, BLS, bls, bls_frequencies, bls_last_timing,
                  PDM, CE, pdm, aov, conditional_entropy, pdm_last_timing, cent_last_timing,
                  CLEAN, clean, clean_loop, clean_restore, clean_sigma, dirty_spectrum, clean_last_timing,
                  bootstrap_indices, lombscargle_bootstrap, lombscargle_bootstrap_last_timing, false_alarm_probability, false_alarm_level,
                  ComplexNormal, SchedFunc, schedfunc, rand, randn, cholesky_upper, cn_last_timing, pdf, affine_transform, detrend, detrend_, Σ,  # noqa: E402
                  cn_V2ΓC, cn_Vxx, cn_Vyy, cn_Vxy, cn_Vyx, cn_fVxx, cn_fVyy, cn_fVxy, cn_fVyx, cn_Vs, cn_fV, cn_V,  # noqa: E402
                  ADMM, Problem, autocor, autocov, autofun_last_timing, isequidistant, SpectralExt, basis_activation_func, check_freq, default_freqs,  # noqa: E402
                  fourier2complex, get_fourier_regressor, lpv_regressor, ls_sparse_spectral,
                  ls_cohere, lambda_max, lambda_grid, ls_sparse_spectral_path, ls_sparse_spectral_lpv_path, ls_sparse_spectral_lpv, ls_sparse_spectral_lpv_multi, ls_sparse_spectral_lpv_rowsharded, lpv_ranges, predict, residual, fva, eval_last_timing, lpv_batch_multi, lpv_signals_multi, ls_spectral, ls_spectral_lpv, tls_spectral, ls_windowcsd, ls_windowpsd, ls_windowpsd_lpv, psd,
                  reshape_params, set_default_option, get_default_option, default_options, windowpsd_sparse_batched, windowpsd_last_timing, windows_estimate, windows_estimate_multi, windowcsd_batched)
from .prox import IndBallL0, LeastSquares, NormL0, NormL1, NormL2, Quadratic, SlicedSeparableSum  # noqa: E402
from . import sharding  # noqa: E402
from .windows import Windows2, Windows3, hanning, mapwindows, merge, rect  # noqa: E402

__all__ = [
    "ComplexNormal", "SchedFunc", "schedfunc", "rand", "randn", "cholesky_upper", "cn_last_timing", "pdf", "affine_transform", "detrend", "detrend_", "Σ",
    "cn_V2ΓC", "cn_Vxx", "cn_Vyy", "cn_Vxy", "cn_Vyx", "cn_fVxx", "cn_fVyy", "cn_fVxy", "cn_fVyx", "cn_Vs", "cn_fV", "cn_V",
    "autocov", "autocor", "autofun_last_timing", "isequidistant",
    "spectrogram", "melspectrogram", "mfcc", "mel", "hz_to_mel", "mel_to_hz", "mel_frequencies", "fft_frequencies", "dct_matrix",
    "nextfastfft", "Spectrogram", "MelSpectrogram", "MFCC", "freq", "time", "stft_last_timing",
    "Periodogram", "welch_pgram", "periodogram", "compress", "compress_thresholds", "heatmap", "compress_last_timing",
    "lombscargle", "lombscargle_last_timing", "lombscargle_terms_last_timing", "lombscargle_spectrogram", "lombscargle_welch", "lombscargle_windows_last_timing", "time_windows",
    "WWZ", "wwz", "wwz_radius", "wwz_last_timing", "BLS", "bls", "bls_frequencies", "bls_last_timing",
    "PDM", "CE", "pdm", "aov", "conditional_entropy", "pdm_last_timing", "cent_last_timing",
    "CLEAN", "clean", "clean_loop", "clean_restore", "clean_sigma", "dirty_spectrum", "clean_last_timing",
    "bootstrap_indices", "lombscargle_bootstrap", "lombscargle_bootstrap_last_timing", "false_alarm_probability", "false_alarm_level",
    "ADMM", "Problem", "SpectralExt", "basis_activation_func", "check_freq", "default_freqs", "fourier2complex",
    "get_fourier_regressor", "lpv_regressor", "ls_sparse_spectral", "ls_sparse_spectral_lpv", "ls_sparse_spectral_lpv_multi", "ls_sparse_spectral_lpv_rowsharded", "lpv_ranges", "predict", "residual", "fva", "eval_last_timing", "lpv_batch_multi", "lpv_signals_multi", "ls_spectral",
    "lambda_max", "lambda_grid", "ls_sparse_spectral_path", "ls_sparse_spectral_lpv_path", "ls_spectral_lpv", "tls_spectral", "ls_windowcsd", "ls_cohere", "ls_windowpsd", "ls_windowpsd_lpv", "psd", "reshape_params", "IndBallL0", "LeastSquares",
    "NormL0", "NormL1", "NormL2", "Quadratic", "SlicedSeparableSum", "Windows2", "Windows3", "hanning",
    "mapwindows", "merge", "rect", "set_default_option", "get_default_option", "default_options", "windowpsd_sparse_batched", "windowpsd_last_timing", "windows_estimate", "windows_estimate_multi", "windowcsd_batched", "DeviceError", "DomainError", "NumericError",
]
