"""Deterministic noisy test signal of the probabilistic-YIN tests (tests/test_pyin_cpu.py); the other signals are those
of tests/pitch_signals.py."""
import numpy as np


def noisy_voice(seed, n, sr, noise=0.10, first=1.0):
    """A function of its arguments alone: eight harmonics (amplitude ``first`` for the fundamental, 0.6^k above it,
    random phases) of an F0 that wanders between 110 and 260 Hz, every second period 8 % stronger (period doubling),
    in stretches that alternate with silence, white noise of standard deviation ``noise`` over all of it.
    -> (samples, F0 in Hz per sample, voiced per sample), float64 / float64 / bool."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    phases = rng.uniform(0, 2 * np.pi, 8)
    phi = rng.uniform(0, 2 * np.pi, 3)
    f0 = 185 + 50 * np.sin(2 * np.pi * 0.7 * t + phi[0]) + 25 * np.sin(2 * np.pi * 0.23 * t + phi[1])
    ph = 2 * np.pi * np.cumsum(f0) / sr
    amp = [first] + [0.6 ** k for k in range(1, 8)]
    s = sum(amp[k] * np.sin((k + 1) * ph + phases[k]) for k in range(8))
    s = s * (1 + 0.08 * np.cos(0.5 * ph))
    voiced = np.sin(2 * np.pi * 0.9 * t + phi[2]) > -0.3
    x = np.where(voiced, 0.25 * s, 0.0) + noise * rng.standard_normal(n)
    return x, f0, voiced
