#!/usr/bin/env python3
"""One line per branch and kind of the STFT engine (csrc/melspec.hip, csrc/stft_plan.h): SHA-256 of the output and the plan slots of
stft_last_timing() -- path, fft_length, pairs_per_workgroup, rows, sum_chain, slabs -- at the smallest shape that reaches the branch:
the four paths and the LDS fallback, f64 and f32, windowed and not, host and device output, the multi-chunk four-step loops, and the
frame averages of tests/test_gpu_welch.py (the two-sided ones included).
Two builds of the library compute the same thing exactly when their outputs are identical:

    LPVS_LIBRARY=/path/to/other/liblpvspectral.so tools/stft_hashes.py > a.txt;  tools/stft_hashes.py > b.txt;  cmp a.txt b.txt

Inputs are fixed (seeded); nothing in the output depends on time."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import lpvspectral_jl_amd as L

SLOTS = ("path", "fft_length", "pairs_per_workgroup", "rows", "sum_chain", "slabs")


def noise(seed, size, f32=False):
    return np.random.default_rng(seed).standard_normal(size).astype(np.float32 if f32 else np.float64)


def report(name, out):
    a = out.detach().cpu().numpy() if hasattr(out, "detach") else np.asarray(out)
    tm = L.stft_last_timing()
    sha = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]
    print(f"{name:58s} {sha} {a.dtype} {'x'.join(map(str, a.shape)):12s} " + " ".join(f"{k} {tm[k]}" for k in SLOTS), flush=True)


def stft(name, kind, y, n, nov, nfft, nmels=40, nmfcc=13, window=None):
    if kind == "power":
        report(name, L.spectrogram(y, n, nov, nfft=nfft, window=window).power)
    elif kind == "mel":
        report(name, L.melspectrogram(y, n, nov, nfft=nfft, nmels=nmels, window=window).power)
    else:
        report(name, L.mfcc(y, n, nov, nfft=nfft, nmels=nmels, nmfcc=nmfcc, window=window).mfcc)


def stft_cases():
    import torch
    for f32 in (False, True):
        t = "f32" if f32 else "f64"
        # path 1: pairs per workgroup from the frames, from the cap, from the epilogue's regions
        y = noise(1, 4096, f32)
        for kind in ("power", "mel", "mfcc"):
            stft(f"{t} lds {kind} nfft 256 hanning", kind, y, 256, 192, 256, window=L.hanning(256))
        stft(f"{t} lds power nfft 256 no window", "power", y, 256, 192, 256)
        stft(f"{t} lds power nfft 256 zero-padded from 200", "power", y, 200, 50, 256, window=L.hanning(200))
        stft(f"{t} lds power nfft 8", "power", noise(2, 1000, f32), 8, 0, 8)
        stft(f"{t} lds mel nfft 8192 nmels 40", "mel", noise(3, 16384, f32), 8192, 0, 8192)
        # the fallback through global power columns, plain and Bluestein
        stft(f"{t} fallback mfcc nfft 8192 nmels 4096", "mfcc", noise(4, 16384, f32), 8192, 0, 8192, nmels=4096)
        stft(f"{t} fallback mel nfft 64 nmels 24000", "mel", noise(5, 5 * 64, f32), 64, 0, 64, nmels=24000, window=L.hanning(64))
        stft(f"{t} fallback mel nfft 4093 nmels 6200", "mel", noise(6, 5 * 4093, f32), 4093, 0, 4093, nmels=6200)
        # path 3
        for kind in ("power", "mel", "mfcc"):
            stft(f"{t} bluestein-lds {kind} nfft 1009 hanning", kind, noise(7, 5000, f32), 1000, 500, 1009, window=L.hanning(1000))
        stft(f"{t} bluestein-lds power nfft 11", "power", noise(8, 88, f32), 11, 0, 11)
        # path 2
        y = noise(9, 3 * 16384, f32)
        for kind in ("power", "mel", "mfcc"):
            stft(f"{t} four-step {kind} nfft 16384", kind, y, 16384, 0, 16384)
        stft(f"{t} four-step power nfft 16384 hanning", "power", y, 16384, 0, 16384, window=L.hanning(16384))
        stft(f"{t} four-step power nfft 33614", "power", noise(10, 3 * 33614, f32), 33614, 0, 33614)
        # path 4
        for nfft in (4099, 8191, 16411):
            stft(f"{t} bluestein-four-step power nfft {nfft}", "power", noise(nfft, 3 * nfft, f32), nfft, 0, nfft)
        stft(f"{t} bluestein-four-step mel nfft 4099 hanning", "mel", noise(11, 3 * 4099, f32), 4099, 0, 4099, window=L.hanning(4099))
        stft(f"{t} bluestein-four-step mfcc nfft 4099", "mfcc", noise(11, 3 * 4099, f32), 4099, 0, 4099)
        # device tensors in and out
        d = torch.as_tensor(noise(12, 4096, f32)).cuda()
        stft(f"{t} device lds mel nfft 256", "mel", d, 256, 192, 256, window=L.hanning(256))
        stft(f"{t} device four-step power nfft 16384", "power", torch.as_tensor(y).cuda(), 16384, 0, 16384)
    # the chunk loops (tests/test_gpu_stft_paths.py: test_four_step_chunk_boundaries, test_bluestein_four_step_chunk_boundary)
    y = noise(21, 16 * 4100)
    y[4096 * 16 + 5] = np.nan
    for kind in ("power", "mfcc"):
        stft(f"f64 four-step {kind} nfft 16384 two chunks", kind, y, 16, 0, 16384)
    stft("f64 bluestein-four-step power nfft 4099 two chunks", "power", noise(22, 4099 + 8199), 4099, 4098, 4099)


def welch(name, y, n, nov, nfft, window=None, onesided=True):
    report(name, L.welch_pgram(y, n, nov, nfft=nfft, window=window, onesided=onesided).power)


def welch_cases():
    import torch
    welch("f64 welch lds 65533 frames hanning", noise(1, 2 ** 22), 256, 192, 256, window=L.hanning(256))
    for n, K in ((5000, 37), (8192, 6), (6000, 9)):
        welch(f"f64 welch lds one pair n {n}", noise(n, n + (K - 1) * (n // 2)), n, n - n // 2, n)
    welch("f64 welch lds batches stride over slabs", noise(2, 2048 + 9000), 2048, 2047, 2048, window=L.hanning(2048))
    welch("f64 welch lds longest chain", noise(3, 8 * (40 * 1024 + 7)), 8, 0, 8)
    welch("f64 welch single frame", noise(4, 300), 300, 0, 300)
    welch("f64 welch zero-padded", noise(5, 200 * 9 + 13), 200, 50, 256, window=L.hanning(200))
    welch("f64 welch bluestein-lds", noise(6, 1000 * 40 + 3), 1000, 500, 1009, window=L.hanning(1000))
    welch("f64 welch four-step two chunks", noise(7, 16 * 4100), 16, 0, 16384)
    welch("f64 welch bluestein-four-step", noise(8, 4099 + 6000), 4099, 3099, 4099)
    for Ls in (5000, 2 ** 20, 2 ** 20 + 1, 3 * 2 ** 20):
        for windowed in (False, True):
            p = L.periodogram(noise(Ls, Ls), nfft=Ls, fs=3.0, window=L.hanning(Ls) if windowed else None)
            report(f"f64 periodogram {Ls}{' hanning' if windowed else ''}", p.power)
    welch("f32 welch lds hanning", noise(10, 2 ** 18, True), 256, 192, 256, window=L.hanning(256))
    welch("f32 welch bluestein-lds", noise(11, 20000, True), 1000, 500, 1009)
    report("f32 periodogram 2^20", L.periodogram(noise(12, 2 ** 20, True), nfft=2 ** 20).power)
    for n, nov, nfft, Ls in ((256, 192, 256, 20000), (1000, 500, 1009, 30000), (16384, 8192, 16384, 16384 * 6), (4099, 0, 4099, 4099 * 5)):
        for f32 in (False, True):
            welch(f"{'f32' if f32 else 'f64'} welch two-sided nfft {nfft} hanning", noise(n, Ls, f32), n, nov, nfft, window=L.hanning(n), onesided=False)
    for dt in (torch.float64, torch.float32):
        d = torch.as_tensor(noise(15, 50000)).to(dt).cuda()
        welch(f"{str(dt)[6:]} device welch n 500", d, 500, 100, None, window=L.hanning(500))
        report(f"{str(dt)[6:]} device periodogram two-sided", L.periodogram(d, onesided=False).power)


if __name__ == "__main__":
    stft_cases()
    welch_cases()
