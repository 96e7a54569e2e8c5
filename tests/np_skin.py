"""Blend shapes and linear blend skinning as jpt_scene_pose_mesh defines them (include/jpt.h), restated in numpy float32: every + and *
below is one binary32 operation on float32 arrays, in the stated order, no fma.  Written from the definition, not from the C++.

For vertex v, from its bind position p and bind normal n:
  blend shapes   for each shape s with weight w != 0, ascending s:  p = p + dP[s][v] * w  per component;  n = n + dN[s][v] * w when
                 the rig has normal deltas.  Nothing is normalised here; all-zero weights read no delta.
  skinning       K = 4 or 8 (K = 0: skipped):  M = B[b_0] * w_0 per entry (transform12 layout: basis rows xx xy xz yx yy yz zx zy zz,
                 then the origin), then M = M + B[b_i] * w_i for i = 1 .. K-1 in order -- all K influences, zero weights included,
                 weights as given.  x' = M[0]*x + M[1]*y + M[2]*z + M[9] left to right; y' from 3 4 5 10; z' from 6 7 8 11.  The normal
                 takes the same rows without the origin.
  normal         with normals: n * (1 / sqrt(n.n)) with n.n = n.x*n.x + n.y*n.y + n.z*n.z left to right, once, at the end (also K = 0).
"""
import copy

import numpy as np

F = np.float32


def np_skin(bind_positions, bind_normals, bones, weights, influences, position_deltas, normal_deltas, bone_transforms12, blend_weights):
    """(positions, normals) float32 [n, 3]; normals None when bind_normals is None.  bones / weights: [n, K]; deltas: [S, n, 3]."""
    p = np.array(bind_positions, dtype=F).reshape(-1, 3).copy()
    n = None if bind_normals is None else np.array(bind_normals, dtype=F).reshape(-1, 3).copy()
    nv = len(p)
    bw = np.zeros(0, F) if blend_weights is None else np.asarray(blend_weights, dtype=F).reshape(-1)
    for s in range(len(bw)):
        w = bw[s]
        if w == F(0):
            continue
        dp = np.asarray(position_deltas, dtype=F).reshape(len(bw), nv, 3)[s]
        p = (p + (dp * w).astype(F)).astype(F)
        if n is not None and normal_deltas is not None:
            dn = np.asarray(normal_deltas, dtype=F).reshape(len(bw), nv, 3)[s]
            n = (n + (dn * w).astype(F)).astype(F)
    K = int(influences)
    if K:
        B = np.asarray(bone_transforms12, dtype=F).reshape(-1, 12)
        b = np.asarray(bones).reshape(nv, K)
        wt = np.asarray(weights, dtype=F).reshape(nv, K)
        M = (B[b[:, 0]] * wt[:, 0:1]).astype(F)
        for i in range(1, K):
            M = (M + (B[b[:, i]] * wt[:, i:i + 1]).astype(F)).astype(F)

        def rows(v, origin):
            out = np.zeros((nv, 3), F)
            for r in range(3):
                acc = (M[:, 3 * r] * v[:, 0]).astype(F)
                acc = (acc + (M[:, 3 * r + 1] * v[:, 1]).astype(F)).astype(F)
                acc = (acc + (M[:, 3 * r + 2] * v[:, 2]).astype(F)).astype(F)
                if origin:
                    acc = (acc + M[:, 9 + r]).astype(F)
                out[:, r] = acc
            return out

        p = rows(p, True)
        if n is not None:
            n = rows(n, False)
    if n is not None:
        d = (n[:, 0] * n[:, 0]).astype(F)
        d = (d + (n[:, 1] * n[:, 1]).astype(F)).astype(F)
        d = (d + (n[:, 2] * n[:, 2]).astype(F)).astype(F)
        inv = (F(1) / np.sqrt(d).astype(F)).astype(F)
        n = (n * inv[:, None]).astype(F)
    return p, n


# ---- test material: rigs and poses -------------------------------------------------------------------------------------------

class Rig:
    """One surface's rig arrays as the tests make them"""

    def __init__(self, bones, weights, position_deltas, normal_deltas):
        self.bones, self.weights, self.position_deltas, self.normal_deltas = bones, weights, position_deltas, normal_deltas


def random_rig(rng, n_vertices, influences, n_shapes, n_bones, normal_deltas=True, wide_weights=True):
    """bones over all of 0 .. n_bones - 1 (the last one named for certain); wide_weights: weights also outside [0, 1] and some exactly 0"""
    K = influences
    bones = weights = dp = dn = None
    if K:
        bones = rng.randint(0, n_bones, size=(n_vertices, K)).astype(np.int32)
        bones[rng.randint(0, n_vertices), rng.randint(0, K)] = n_bones - 1
        if wide_weights:   # the first in (0.9, 1.3), the others in (-0.08, 0.4) or exactly 0: the sum stays above 0.3, so no normal degenerates
            weights = rng.uniform(-0.08, 0.4, size=(n_vertices, K))
            weights[rng.uniform(size=weights.shape) < 0.2] = 0.0
            weights[:, 0] = rng.uniform(0.9, 1.3, size=n_vertices)
        else:
            weights = rng.dirichlet(np.ones(K), size=n_vertices)
        weights = weights.astype(F)
    if n_shapes:
        dp = rng.uniform(-0.2, 0.2, size=(n_shapes, n_vertices, 3)).astype(F)
        if normal_deltas:
            dn = rng.uniform(-0.3, 0.3, size=(n_shapes, n_vertices, 3)).astype(F)
    return Rig(bones, weights, dp, dn)


def random_palette(rng, n_bones, amount=0.3):
    """near-identity affine bone transforms (transform12 layout): normals stay far from degenerate"""
    B = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (n_bones, 1))
    return (B + rng.uniform(-amount, amount, size=B.shape)).astype(F)


def skin_mesh(mesh, rigs, influences, bone_transforms12, blend_weights, with_normals=True):
    """a copy of scenes.Mesh `mesh` (the bind pose) with every surface posed by np_skin"""
    out = copy.deepcopy(mesh)
    for s, r in zip(out.surfaces, rigs):
        p, n = np_skin(s.vertices, s.normals if with_normals else None, r.bones, r.weights, influences, r.position_deltas,
                       r.normal_deltas if with_normals else None, bone_transforms12, blend_weights)
        s.vertices = p
        if with_normals:
            s.normals = n
    return out


def ring_rig(surface, n_bones, seed=21, wide_weights=True):
    """the rig of the demo scene's blob (a displaced torus; tools/skin_rate.py and the GPU tests): n_bones bones along the torus, each vertex
    bound to the four from its own on, two blend shapes with small deltas"""
    rng = np.random.RandomState(seed)
    rig = random_rig(rng, len(surface.vertices), 4, 2, n_bones, wide_weights=wide_weights)
    u = np.arctan2(surface.vertices[:, 2], surface.vertices[:, 0]) / (2 * np.pi) + 0.5
    rig.bones = ((np.floor(u * n_bones).astype(int)[:, None] + np.arange(4)[None, :]) % n_bones).astype(np.int32)
    rig.position_deltas = (rig.position_deltas * F(0.2)).astype(F)
    return rig


MANY_BONES = 257   # a palette far larger than a character's (12 KB): more bones than a block has threads


def debug_cases():
    """The cases of jpt_debug_skin's tests, host and device: (label, dict of jpt_debug_skin's inputs).  K in {0, 4, 8} x shapes in {0, 1, 3}
    (one zero weight among three) x {no normals, normals, normals + normal deltas} x n_vertices in {1, 63, 64, 65, 263}, weights outside
    [0, 1]; and palettes of 1, 3 and MANY_BONES bones."""
    out = []
    seed = 0
    for K in (0, 4, 8):
        for S in (0, 1, 3):
            if K == 0 and S == 0:
                continue
            for normals, deltas in ((False, False), (True, False), (True, True)):
                if deltas and S == 0:
                    continue
                for nv in (1, 63, 64, 65, 263):
                    for n_bones in ((5,) if (K == 0 or nv != 263) else (5, 1, 3, MANY_BONES)):
                        seed += 1
                        rng = np.random.RandomState(1000 + seed)
                        pos = rng.uniform(-1, 1, size=(nv, 3)).astype(F)
                        nrm = rng.normal(size=(nv, 3))
                        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F) if normals else None
                        rig = random_rig(rng, nv, K, S, n_bones, normal_deltas=deltas)
                        bw = {0: None, 1: np.array([-0.6], F), 3: np.array([0.75, 0.0, 1.4], F)}[S]
                        pal = random_palette(rng, n_bones) if K else None
                        out.append(("K%d S%d n%d d%d nv%d bones%d" % (K, S, normals, deltas, nv, n_bones),
                                    dict(pos=pos, nrm=nrm, rig=rig, K=K, S=S, palette=pal, blend=bw)))
    return out
