"""Deterministic test signals of the pitch tests (tests/test_pitch_cpu.py, tests/test_pitch_gpu.py)."""
import numpy as np


def speechlike(seed, n, sr):
    """A function of (seed, n, sr) alone: eight harmonics (amplitude 0.6^k, random phases) of an F0 that wanders
    between 40 and 240 Hz, a 2.1 Hz envelope, voiced and noise-only stretches, the first sr / 10 samples exactly zero,
    peak 0.5.  float64."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    phases = rng.uniform(0, 2 * np.pi, 8)
    phi = rng.uniform(0, 2 * np.pi)
    f0 = 140 + 60 * np.sin(2 * np.pi * 1.3 * t + phi) + 40 * np.sin(2 * np.pi * 0.37 * t)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    s = sum(0.6 ** k * np.sin((k + 1) * ph + phases[k]) for k in range(8))
    env = 0.5 * (1 + np.sin(2 * np.pi * 2.1 * t))
    noise = rng.standard_normal(n)
    voiced = np.sin(2 * np.pi * 0.9 * t + 1) > -0.3
    x = np.where(voiced, 0.3 * env * s + 0.01 * noise, 0.05 * noise)
    x[: sr // 10] = 0.0
    return 0.5 * x / np.abs(x).max()


def short(seed, n, sr=22050):
    """n samples from sample 3000 of an 8000-sample signal: past the zero head."""
    return speechlike(seed, 8000, sr)[3000:3000 + n]


def tone(f, n, sr):
    """A steady two-harmonic tone."""
    t = np.arange(n) / sr
    return 0.4 * np.sin(2 * np.pi * f * t + 0.3) + 0.2 * np.sin(2 * np.pi * 2 * f * t + 1.1)


def zero_headed(n=9000, sr=22050):
    """The full signal: its first frames begin in exact zeros."""
    return speechlike(3, n, sr)
