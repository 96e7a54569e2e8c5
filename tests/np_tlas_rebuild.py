"""jpt_scene_rebuild_tlas restated in numpy, from the words of include/jpt.h (jpt_debug_tlas_order, jpt_debug_tlas_template): the keys in
binary32 steps, the sort as np.argsort of the unique 45-bit keys, the template, and the bottom-up union of the boxes."""
import math

import numpy as np

EMPTY = np.int32(-2 ** 31)
F32_MAX = np.float32(3.402823466e38)


def keys(lo, hi):
    """uint64 [n]: Morton code << 15 | index."""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    hi = np.asarray(hi, np.float32).reshape(-1, 3)
    n = len(lo)
    with np.errstate(all="ignore"):
        c = (lo + hi) * np.float32(0.5)
        fin = np.isfinite(c)
        cell = np.zeros((n, 3), np.uint32)
        for k in range(3):
            ck = c[:, k]
            f = ck[fin[:, k]]
            bmin = f.min() if len(f) else F32_MAX
            bmax = f.max() if len(f) else -F32_MAX
            ext = np.float32(bmax - bmin)
            inv = np.float32(1024.0) / ext if ext > 0 else np.float32(0.0)
            t = np.floor((ck - np.float32(bmin)) * np.float32(inv)).astype(np.float32)
            q = np.where(t >= 1024, 1023, np.where(t >= 0, t, 0))   # (a NaN compares false twice: cell 0)
            q = np.where(fin[:, k], q, 0)
            cell[:, k] = np.nan_to_num(q, nan=0.0).astype(np.uint32)
    code = np.zeros(n, np.uint64)
    for bit in range(10):
        for k in range(3):   # x in the highest bit of each triple
            code |= ((cell[:, k].astype(np.uint64) >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + (2 - k))
    return (code << np.uint64(15)) | np.arange(n, dtype=np.uint64)


def order(lo, hi):
    """(keys per instance, the instance at every sorted position)."""
    k = keys(lo, hi)
    return k, np.argsort(k, kind="stable").astype(np.uint32)


def template(n):
    """int32 [R, 4] child words (>= 0 a record, ~position a leaf, EMPTY), the number of levels."""
    rows, level, numbered, levels = [], [(0, n)], 1, 0
    while level:
        nxt = []
        for first, m in level:
            slot = [EMPTY] * 4
            if m <= 4:
                for k in range(m):
                    slot[k] = ~(first + k)
            else:
                at = first
                for k in range(4):
                    part = m // 4 + (1 if k < m % 4 else 0)
                    if part == 1:
                        slot[k] = ~at
                    else:
                        slot[k] = numbered + len(nxt)
                        nxt.append((at, part))
                    at += part
            rows.append(slot)
        numbered += len(nxt)
        levels += 1
        level = nxt
    return np.array(rows, np.int32).reshape(-1, 4), levels


def stack_need(child, r=0):
    """pending entries of a near-first walk: (children - 1) + the deepest child's need."""
    kids = [c for c in child[r] if c != EMPTY]
    return len(kids) - 1 + max([stack_need(child, c) for c in kids if c >= 0], default=0)


def ceil_log4(n):
    l = 0
    while 4 ** l < n:
        l += 1
    return l


NODE4 = np.dtype([("lo", np.float32, (3, 4)), ("child", np.int32, 4), ("hi", np.float32, (3, 4)), ("pad", np.uint32, 4)])
assert NODE4.itemsize == 128


def records(n, sorted_instances, inst_lo, inst_hi):
    """The template over `sorted_instances` as 128-byte records, boxes by the bottom-up union (min and max are exact)."""
    child, _ = template(n)
    out = np.zeros(len(child), NODE4)
    out["lo"][:] = F32_MAX
    out["hi"][:] = -F32_MAX
    for r in range(len(child) - 1, -1, -1):   # breadth-first numbering: every child record has a larger index
        for k in range(4):
            c = int(child[r, k])
            if c == EMPTY:
                out["child"][r, k] = EMPTY
            elif c < 0:
                i = int(sorted_instances[~c])
                out["child"][r, k] = ~i
                out["lo"][r, :, k] = inst_lo[i]
                out["hi"][r, :, k] = inst_hi[i]
            else:
                out["child"][r, k] = c
                used = out["child"][c] != EMPTY
                out["lo"][r, :, k] = out["lo"][c][:, used].min(axis=1)
                out["hi"][r, :, k] = out["hi"][c][:, used].max(axis=1)
    return out
