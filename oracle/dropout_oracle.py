"""The counter-based dropout generator of ``stonkgs_amd/csrc/common.h``, restated in numpy (no GPU).

The kernels store no mask: forward and backward regenerate it from (seed, row, column). This module states the same
function independently, in 64-bit integers masked to 32 bits after every step, so that a test can say which elements a
kernel must have dropped instead of reading that off the kernel's own output.

    x = (row * G_ROW + seed_mix(seed)) ^ (column * G_COL)            (mod 2^32)
    y = lo24(x) * C1 + x                                            (mod 2^32)
    z = (y >> 8) * C2                                               (mod 2^32; y >> 8 has 24 bits)
    keep iff z >= thr32(p)

Covered: the element form (``stonk_keep``) used by the LayerNorm kernels, the embedding front-ends (row = the output row, in
the packed layout the packed row) and ``stonk_dropout_f32`` (row 0, column = the flat element index).

The attention probabilities use the 4 x 4 BLOCK form (``stonk_blk_round1`` / ``stonk_blk_keep``): one first round per block of
four query rows x four keys, one last round per element with one of sixteen multipliers (``keep_block``):

    rk = (row >> 2) * G_ROW + seed_mix(seed)                        (mod 2^32)
    ck = (key >> 2) * G_COL                                         (mod 2^32)
    x  = rk ^ ck
    y8 = (lo24(x) * C1 + x  mod 2^32) >> 8
    z  = y8 * C2_BLK[4 * (row & 3) + (key & 3)]                     (mod 2^32)
    keep iff z >= thr32(p)

with row = (b * NH + h) * S + q, q the query's row INSIDE its sequence and S the launch's ``S`` argument (in the packed
layout too), and key = the key's row inside its sequence (``attention_keep``).
"""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_M24 = np.uint64(0xFFFFFF)
G_ROW = np.uint64(0x9E3779B1)
G_COL = np.uint64(0x85EBCA77)
C1 = np.uint64(0xB5297B)
C2 = np.uint64(0x68E31D)
# STONK_C2_BLK: the last-round multiplier of block member 4 * (row & 3) + (key & 3)
C2_BLK = np.array([0x45821F, 0xFAC0C5, 0xD90A1B, 0xE6B85B, 0xE11EE7, 0x6E41B9, 0xB8115D, 0xB1494B,
                   0xBF440F, 0xA96C25, 0x7B570F, 0xA2609D, 0x98207D, 0xB5677D, 0x82C471, 0xAC3C19], dtype=np.uint64)


def _hash32(x: np.uint64) -> np.uint64:
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def seed_mix(seed: int) -> int:
    """The seed word the kernels see (computed once per launch on the host)."""
    s = np.uint64(int(seed) & 0xFFFFFFFF)
    return int(_hash32((s * np.uint64(0x9E3779B9) + np.uint64(0x85EBCA6B)) & _M32))


def thr32(p: float) -> int:
    """Drop probability as a 32-bit threshold. The launchers take p as a C float, so it is rounded to float32 first."""
    t = float(np.float32(p)) * 4294967296.0
    t = min(max(t, 0.0), 4294967295.0)
    return int(t + 0.5)


def keep(rows, cols, seed: int, p: float) -> np.ndarray:
    """Keep mask bool[len(rows), len(cols)]: element (i, j) is that of row index rows[i] and column index cols[j]."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 1).astype(np.uint64) & _M32
    c = np.asarray(cols, dtype=np.int64).reshape(1, -1).astype(np.uint64) & _M32
    rowkey = (r * G_ROW + np.uint64(seed_mix(seed))) & _M32
    colkey = (c * G_COL) & _M32
    x = rowkey ^ colkey
    y = ((x & _M24) * C1 + x) & _M32
    z = ((y >> np.uint64(8)) * C2) & _M32
    return z >= np.uint64(thr32(p))


def keep_flat(n: int, seed: int, p: float) -> np.ndarray:
    """Keep mask bool[n] of ``stonk_dropout_f32``: row 0, column = element index."""
    return keep([0], np.arange(n), seed, p)[0]


def keep_block(rows, keys, seed: int, p: float) -> np.ndarray:
    """Keep mask bool[len(rows), len(keys)] of the 4 x 4 block form: element (i, j) is that of row rows[i] and key keys[j]."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 1).astype(np.uint64) & _M32
    k = np.asarray(keys, dtype=np.int64).reshape(1, -1).astype(np.uint64) & _M32
    two, three = np.uint64(2), np.uint64(3)
    rk = ((r >> two) * G_ROW + np.uint64(seed_mix(seed))) & _M32
    ck = ((k >> two) * G_COL) & _M32
    x = rk ^ ck
    y8 = (((x & _M24) * C1 + x) & _M32) >> np.uint64(8)
    c2 = C2_BLK[(np.uint64(4) * (r & three) + (k & three)).astype(np.int64)]
    z = (y8 * c2) & _M32
    return z >= np.uint64(thr32(p))


def attention_keep(b: int, h: int, NH: int, S: int, n_queries: int, n_keys: int, seed: int, p: float) -> np.ndarray:
    """Keep mask bool[n_queries, n_keys] of head h of sequence b in a launch with `NH` heads and the argument `S`:
    the first n_queries query rows of the sequence against its first n_keys keys."""
    return keep_block((b * NH + h) * S + np.arange(n_queries), np.arange(n_keys), seed, p)
