"""Shared pieces of test_render_full_cpu.py and test_gpu_render_full.py: the float64 restatement of the per-face
light (nr.lighting as include/g2s.h states it for g2s_face_light_fwd), its composition with `restate` of
test_gpu_render_rgb_grad.py, the cases and the light they are lit with."""
import numpy as np
import torch

from test_gpu_render_rgb_grad import EPS, make_case, restate

# (S, ts, C, fill_back, implicit)
CASES = [(16, 2, 3, True, True), (20, 2, 3, True, False), (12, 2, 3, False, True), (16, 1, 3, True, True)]

IA, ID = 0.4, 0.6
CA = (1.0, 0.8, 0.6)
CD = (0.7, 0.9, 1.0)
AMBIENT = tuple(IA * c for c in CA)
DIRECTIONAL = tuple(ID * c for c in CD)
# fixed, non-axis; the first one that keeps every face of a case away from the kink of max(0, .) is used
DIRECTIONS = [(0.3, 0.5, -0.8), (-0.5, 0.3, -0.75), (0.6, 0.2, 0.7)]
MIN_DOT = 1e-4      # no face closer to the kink of max(0, dot(n, direction))
MIN_CROSS = 1e-4    # no face closer to the 1e-5 clamp of the normalisation
# |cross| does not depend on the direction: a flat face of make_case's scene (10 degree field of view at depth 1)
# has |cross| = (2 tan 5deg / (S - 1))^2, 8.5e-5 at S = 20, below MIN_CROSS whatever the light.  A case whose faces
# are that small is used at the first of these uniform scales of its camera-space vertices under which it is well
# conditioned.  Powers of two: the fp32 vertices keep their mantissas, the projection x / (z + 1e-9) and with it
# winners, barycentric weights and cube coordinates are those of the unscaled scene up to that 1e-9, depths stay
# inside near / far.
SCALES = [1.0, 2.0]
BG = (1.0, 0.5, -0.25)


def light(verts, faces, fill_back, ambient, directional, direction):
    """float64 per-face light.  verts [B,N,3] float64 (differentiable), faces (F,3) integer array.
    Returns (light [B, F * (1 + fill_back), 3], dot(n, direction) [B, F], |cross| [B, F])."""
    faces = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    v0, v1, v2 = verts[:, faces[:, 0]], verts[:, faces[:, 1]], verts[:, faces[:, 2]]
    cross = torch.linalg.cross(v0 - v1, v2 - v1, dim=-1)
    length = cross.norm(dim=-1)
    # the clamp carries no gradient where it is active (include/g2s.h); the cases stay away from it
    n = cross / length.clamp(min=1e-5)[..., None]
    d = (n * torch.tensor(direction, dtype=torch.float64)).sum(-1)
    amb = torch.tensor(ambient, dtype=torch.float64)
    dc = torch.tensor(directional, dtype=torch.float64)
    out = amb + dc * d.clamp(min=0.0)[..., None]
    if fill_back:       # the reversed copy (v2, v1, v0) has the normal -n
        out = torch.cat([out, amb + dc * (-d).clamp(min=0.0)[..., None]], 1)
    return out, d, length


def restate_lit(verts, faces, tex, face_idx, S, K, fill_back, ambient, directional, direction, background=BG):
    """float64 lit texture pass: the colour `restate` gathers for a sample, times light[b, winner]; background
    samples stay unlit.  `restate` is affine in the textures and a winner reads the cube of face winner % F, so
    the product is formed per orientation: samples won by front copies read textures * light[:, :F], samples won
    by reversed copies textures * light[:, F:], and the background comes from a pass with zero textures."""
    F = tex.shape[1]
    lt, _, _ = light(verts, faces, fill_back, ambient, directional, direction)
    fidx = np.asarray(face_idx)
    zero = (0.0, 0.0, 0.0)
    front = np.where(fidx < F, fidx, -1)
    out = restate(verts, faces, tex * lt[:, :F, None, None, None, :], front, S, K, background=zero)
    if fill_back:
        back = np.where(fidx >= F, fidx, -1)
        out = out + restate(verts, faces, tex * lt[:, F:, None, None, None, :], back, S, K, background=zero)
    return out + restate(verts.detach(), faces, torch.zeros_like(tex), fidx, S, K, background=background)


def conditioning(verts, faces, direction):
    """(min |dot(n, direction)|, min |cross|) over every face, on the float64 restatement."""
    _, d, length = light(torch.tensor(verts, dtype=torch.float64), faces, False, AMBIENT, DIRECTIONAL, direction)
    return float(d.abs().min()), float(length.min())


def pick_conditioning(verts, faces):
    """(scale, direction): the first of SCALES, and under it the first of DIRECTIONS, with which the case is well
    conditioned; (SCALES[0], DIRECTIONS[0]) when nothing is (test_cases_are_well_conditioned then fails).  Chosen
    on the CPU from the restatement alone."""
    for s in SCALES:
        for d in DIRECTIONS:
            dot, cross = conditioning(verts * np.float32(s), faces, d)
            if dot >= MIN_DOT and cross >= MIN_CROSS:
                return s, d
    return SCALES[0], DIRECTIONS[0]


_cache = {}


def lit_case(key):
    """make_case of the unlit tests with C = 3, at the scale and with the light direction pick_conditioning gives
    the case (computed once)."""
    if key not in _cache:
        S, ts, Cc, fill_back, implicit = key
        geo, verts, faces, tex, grad = make_case(S, ts, Cc)
        scale, direction = pick_conditioning(verts, faces)
        _cache[key] = dict(S=S, fill_back=fill_back, implicit=implicit, K=geo.K[0], verts=verts * np.float32(scale),
                           faces=faces, tex=tex, grad=grad, direction=direction, scale=scale)
    return _cache[key]


__all__ = ["CASES", "IA", "ID", "CA", "CD", "AMBIENT", "DIRECTIONAL", "DIRECTIONS", "MIN_DOT", "MIN_CROSS", "BG",
           "EPS", "light", "restate_lit", "conditioning", "pick_conditioning", "SCALES", "lit_case"]
