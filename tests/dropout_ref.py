"""numpy restatement of the device's counter-based dropout masks (test infrastructure only), written from the
formulas in csrc/tgnx_common.h (mix64, hash4) and csrc/tgnx_math.h (fmix32, drop_base, keep32); it calls nothing
of the library.  Every function broadcasts over numpy arrays.

  mix64(z)      splitmix64's output function: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
                z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31   (uint64, wrapping)
  hash4(a,b,c,d) mix64(a ^ mix64(b ^ mix64(c ^ mix64(d))))
  fmix32(h)     murmur3's 32-bit finaliser
  drop_base     the low 32 bits of hash4(seed, stream, key, sub)
  keep32        h = fmix32(base ^ (idx * 0x9E3779B9 mod 2^32)); kept iff (h >> 8) >= ceil(float32(p) * 2^24)
  step_seed     mix64(base_seed ^ mix64(nb)) >> 1, nb = the batch counter after the advance
"""
from __future__ import annotations

import numpy as np

_U64 = np.uint64
_U32 = np.uint32


def _u64(x):
    """Any integer (array) as uint64 with two's-complement wrap-around."""
    a = np.asarray(x)
    if a.dtype == object or a.dtype.kind not in "iu":
        a = np.asarray([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.ravel(x)], dtype=_U64).reshape(np.shape(x))
    return a.astype(_U64)


def mix64(z):
    with np.errstate(over="ignore"):
        z = _u64(z) + _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def hash4(a, b, c, d):
    return mix64(_u64(a) ^ mix64(_u64(b) ^ mix64(_u64(c) ^ mix64(d))))


def fmix32(h):
    with np.errstate(over="ignore"):
        h = (_u64(h) & _U64(0xFFFFFFFF)).astype(_U32)
        h = h ^ (h >> _U32(16))
        h = h * _U32(0x85EBCA6B)
        h = h ^ (h >> _U32(13))
        h = h * _U32(0xC2B2AE35)
        return h ^ (h >> _U32(16))


def drop_base(seed, stream, key, sub):
    return (hash4(seed, stream, key, sub) & _U64(0xFFFFFFFF)).astype(_U32)


def threshold(p) -> int:
    """ceil(float32(p) * 2^24): the product is exact in float32 (a power-of-two scale)."""
    return int(np.ceil(np.float32(p) * np.float32(16777216.0)))


def keep_hash(base, idx):
    """The 24-bit draw (h >> 8) of element idx under `base`."""
    with np.errstate(over="ignore"):
        i = (_u64(idx) & _U64(0xFFFFFFFF)).astype(_U32) * _U32(0x9E3779B9)
    return fmix32(np.asarray(base, dtype=_U32) ^ i) >> _U32(8)


def keep32(base, idx, p):
    """Boolean keep mask: True where the element survives dropout p."""
    return keep_hash(base, idx) >= _U32(threshold(p))


def keep_scale(base, idx, p):
    """float32 mask values: 0 or 1 / (1 - p), as the kernels multiply them in."""
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(keep32(base, idx, p), inv, np.float32(0.0)).astype(np.float32)


def step_seed(base_seed: int, nb: int) -> int:
    return int(mix64(_u64(base_seed) ^ mix64(nb))) >> 1
