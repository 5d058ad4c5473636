"""The weight generation, and the one cache for tensors derived from weights.

The fused Adam kernel (and the DDP / style-tuning paths) write parameters through raw pointers, which torch's
version counters never see.  Every such writer calls ``bump_generation()`` afterwards; everything computed from
weights -- the bf16 operand images and captured graphs (``ops.hip``, ``infer.graphs``) and every ``DerivedCache``
below -- is valid for one generation only.  Plain Python: importable without the kernel library.
"""
import torch

from . import IdCache

_gen = 0


def generation() -> int:
    return _gen


def bump_generation():
    """Declare every parameter changed (call after writing parameters through raw pointers)."""
    global _gen
    _gen += 1


class DerivedCache:
    """One value per anchor tensor (by identity, held weakly: nothing is attached to a module, its state dict or
    its deep copies), valid while its source tensors, the weight generation and ``extra`` are unchanged."""

    def __init__(self):
        self._c = IdCache()

    def get(self, anchor, sources, build, extra=()):
        """The value cached under ``anchor``, ``build()`` (under ``no_grad``) when it is missing or any of
        ``sources`` (entries may be None) moved, was written in place, or changed device, dtype or shape."""
        key = (_gen, extra, [t if t is None else (t.data_ptr(), t._version, t.device, t.dtype, t.shape)
                             for t in sources])  # ~0.5 us of host time per tensor: keep it off per-replay paths
        hit = self._c.get(anchor)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, build())
            self._c.put(anchor, hit)
        return hit[1]

    def peek(self, anchor):
        """The stored value (possibly stale) or None; never builds."""
        hit = self._c.get(anchor)
        return None if hit is None else hit[1]
