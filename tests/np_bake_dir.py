"""Directional lightmaps (jpt_set_bake_directional, csrc/jpt_bake_dir.h) restated in float32 numpy: the three first moments of the
incoming light per texel, M_k.c = sum over the frames, in frame order, of cur_f.c * d_f.k -- cur_f the frame's value as the
accumulation adds it, d_f the bake ray's direction (np_bake.bake_rays).  Test infrastructure, like np_bake: one IEEE binary32 operation
per * and + in source order."""
import numpy as np

import np_bake as nb

F = np.float32


def frame_value(radiance, ldr8):
    """a frame's value as wf2_accumulate adds it: the radiance itself (JPT_ACCUM_HDR_F32), or the rgba8 store of main.glsl:434 read
    back (JPT_ACCUM_REF_LDR8: test_gpu_transmission.np_sum's expression)"""
    cur = np.asarray(radiance, F)
    if ldr8:
        with np.errstate(all="ignore"):
            clipped = np.fmin(np.fmax(cur, F(0)), F(1))          # minNum / maxNum: a NaN operand is ignored
            cur = (np.floor(clipped * F(255) + F(0.5)).astype(F) / F(255)).astype(F)
    return cur


def directions(position4, normal4, frame):
    """ray.d of bake_ray for every texel of frame `frame`: float32 [H, W, 3] (zeros for an invalid texel) and valid [H, W]"""
    h, w = np.asarray(normal4).shape[:2]
    _, _, d, valid = nb.bake_rays(position4, normal4, int(frame))
    return d.reshape(h, w, 3), valid.reshape(h, w)


def moments(position4, normal4, frames, first_frame_index, ldr8, frame_count=1, prev=None):
    """The planes after a render of `frames` (radiance [H, W, 3] each; frame f is frame first_frame_index + f) whose first frame has
    ProgressiveRendering frame count `frame_count`: float32 [3, H, W, 4], plane k = (M_k.r, M_k.g, M_k.b, 0).  frame_count > 1
    continues `prev`; an invalid texel holds +0 in all nine values whatever prev held."""
    h, w = np.asarray(normal4).shape[:2]
    have_prev = frame_count > 1
    m = np.zeros((3, h, w, 3), F) if not have_prev else np.array(np.asarray(prev, F)[..., :3], F)
    valid = nb.texel_valid(normal4)
    with np.errstate(all="ignore"):
        for f, radiance in enumerate(frames):
            cur = frame_value(radiance, ldr8)
            d, _ = directions(position4, normal4, int(first_frame_index) + f)
            for k in range(3):
                prod = (cur * d[..., k:k + 1]).astype(F)
                m[k] = (prod + m[k]).astype(F) if have_prev else prod
            have_prev = True
    out = np.zeros((3, h, w, 4), F)
    out[..., :3] = np.where(valid[None, ..., None], m, F(0.0))
    return out
