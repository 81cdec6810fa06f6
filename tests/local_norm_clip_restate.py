"""numpy restatements of the two clip combines through local-normalisation planes (include/stacker.h, "Locally normalised
clip", "Locally normalised median / MAD clip"): the restatements of the weighted clip (test_cpu_robust.py) and of the
median / MAD clip with participation (test_cpu_robust_clip.py) on u = s * G + O from local_norm_restate._fields, with unit
gains and zero offsets: the construction norm_quantile_restate uses. Like the other restatements they take the fold's
samples and participation flags as inputs, so they restate what this feature adds and nothing else."""
import numpy as np

from local_norm_restate import _fields
from test_cpu_robust import robust_clip_restate
from test_cpu_robust_clip import robust_clip_restate_weighted

F = np.float32


def _normalised(samples, planes, step, g, o, wt):
    s, G, O = _fields(samples, planes, g, o, step)
    n, cn = s.shape[0], s.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        u = (s * G + O).astype(F)
    wt = np.ones(n, F) if wt is None else np.asarray(wt, F).reshape(n)
    # The restatements below form u * 1 + 0 again. That is u, except that a -0 becomes +0, which is harmless: -0 and +0
    # compare equal in every interval test and sort as the same value; d = u - c is the same number for either unless it is
    # a zero itself, and a zero of either sign adds nothing to sums that start at +0 (w * (+-0) = +-0, and +0 + -0 = +0); a
    # median or a centre that is a zero gives out = c + a / sw with a = +0, hence +0 for either sign.
    return u, np.ones((n, cn), F), np.zeros((n, cn), F), wt


def norm_clip_restate(samples, participates, planes, step, kappa_low, kappa_high, iterations, g=None, o=None, wt=None):
    """The locally normalised clip: (out, counts, kept_weight), each H x W x C. participates: N x H x W (kappa == 1 under
    coverage = 1, all true otherwise; w > 0 is applied here); planes: N planes or None entries (then g / o, N x C)."""
    u, g1, o0, wt = _normalised(samples, planes, step, g, o, wt)
    return robust_clip_restate(u, participates, g1, o0, wt, kappa_low, kappa_high, iterations)


def norm_robust_clip_restate(samples, participates, planes, step, kappa_low, kappa_high, sigma_floor, iterations, g=None, o=None,
                             wt=None):
    """The locally normalised median / MAD clip: (out, counts, kept_weight), each H x W x C."""
    u, g1, o0, wt = _normalised(samples, planes, step, g, o, wt)
    return robust_clip_restate_weighted(u, participates, g1, o0, wt, kappa_low, kappa_high, sigma_floor, iterations)


# ---- the planted exact case ---------------------------------------------------------------------------------------
def planted_stack(n=8, h=45, w=150, step=16, trail_frame=3):
    """Frame i = an integer scene + a piecewise-bilinear ramp with integer node values in -8 .. 8 (frame 0: none); frame
    `trail_frame` carries a trail of +2 on 270 pixels. f32 frames, alpha 1, identity warps. The planes that undo the ramps
    are G = 1, O = -ramp nodes: through them every sample is the scene exactly (all values are small integers or dyadic
    fractions: every operation of the chain and of the clip is exact), except on the trail.
    Returns (frames N x H x W x 1 f32, planes (None first), scene H x W x 1 f32, trail mask H x W)."""
    from local_norm_restate import grids, plane_at_pixels
    rng = np.random.default_rng(20)
    scene = rng.integers(40, 200, (h, w, 1)).astype(F)
    gw, gh, _, _ = grids(w, h, step)
    frames, planes = [scene.copy()], [None]
    for i in range(1, n):
        nodes = rng.integers(-8, 9, (gh, gw, 1)).astype(F)
        P = np.concatenate([np.ones((gh, gw, 1), F), -nodes], axis=-1)
        _, O = plane_at_pixels(P, w, h, step)                  # -ramp at every pixel, exact
        frames.append((scene - O).astype(F))
        planes.append(P)
    mask = np.zeros((h, w), bool)
    mask[10:13, 30:120] = True                                  # 3 x 90 = 270 pixels
    frames[trail_frame] = frames[trail_frame] + F(2) * mask[..., None].astype(F)
    return np.stack(frames), planes, scene, mask
