"""jpt_scene_rebuild_mesh restated in numpy, from the words of include/jpt.h: the triangles' vertex boxes, their codes (the TLAS
rebuild's code of the box: np_tlas_rebuild.keys), the stable order, the template over the sorted triangles and the padded-union boxes
in the record layout test_gpu_mesh_update.records reads."""
import numpy as np

import np_tlas_rebuild as npt

F32_MAX = npt.F32_MAX
EMPTY = npt.EMPTY


def tri_boxes(vertices, indices):
    """(lo, hi) float32 [t, 3]: min and max of the three vertices taken one after the other from +-FLT_MAX -- (b < a) ? b : a and
    (a < b) ? b : a, so a NaN coordinate is skipped and an infinity is taken"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)[np.asarray(indices).reshape(-1, 3)]   # [t, 3 vertices, 3 axes]
    lo = np.full((len(v), 3), F32_MAX, np.float32)
    hi = np.full((len(v), 3), -F32_MAX, np.float32)
    with np.errstate(invalid="ignore"):
        for j in range(3):
            lo = np.where(v[:, j] < lo, v[:, j], lo)
            hi = np.where(hi < v[:, j], v[:, j], hi)
    return lo, hi


def codes(vertices, indices):
    """uint32 [t]: the 30-bit Morton code of every triangle"""
    lo, hi = tri_boxes(vertices, indices)
    return (npt.keys(lo, hi) >> np.uint64(15)).astype(np.uint32)


def order(vertices, indices):
    """(codes per triangle, the triangle at every sorted position): ascending by (code, triangle)"""
    c = codes(vertices, indices)
    return c, np.argsort(c, kind="stable").astype(np.uint32)


def box_pad(vertices, indices):
    """mesh_box_pad (SahBlasBuilder::prepare): from the largest |coordinate| of the triangles' vertices, in binary32"""
    lo, hi = tri_boxes(vertices, indices)
    m = np.float32(max(np.abs(lo.min(axis=0)).max(), np.abs(hi.max(axis=0)).max()))
    return np.float32(np.float32(m * np.float32(2e-6)) + np.float32(1e-30))


def records(sorted_tris, tri_lo, tri_hi, pad, first_record=0, first_tri=0):
    """The template over `sorted_tris` (triangle within the mesh per sorted position) as 128-byte records the way the device stores
    them: internal references counted from `first_record`, a leaf slot ~(first_tri + triangle) with the triangle's vertex box (in the
    order the caller's tri_lo / tri_hi are in) widened by `pad`, an internal slot the union of the record below."""
    n = len(sorted_tris)
    lo = (np.asarray(tri_lo, np.float32) - np.float32(pad)).astype(np.float32)
    hi = (np.asarray(tri_hi, np.float32) + np.float32(pad)).astype(np.float32)
    out = npt.records(n, np.asarray(sorted_tris), lo, hi)
    child = out["child"]
    leaf = (child < 0) & (child != EMPTY)
    child[leaf] = ~(~child[leaf] + np.int32(first_tri))
    child[child >= 0] += np.int32(first_record)
    return out
