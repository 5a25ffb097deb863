"""Cases and the float64 oracle of the pseudo-view pass (csrc/sweep.hip: g2s_sweep_pseudo).

The oracle restates the formulas of include/g2s.h in numpy float64 and takes the rasterised depth `warped` as an
INPUT, so that it never disagrees with the rasterizer about silhouettes.  Every case is seeded and is the smallest
shape at which its path can still go wrong: S below one workgroup (8), odd and no multiple of anything (33), several
workgroups per frame (64); one frame and B x V frames; poses up to +-60 degrees of yaw with translations, so that
frames hold samples outside the canonical image.

The nearest-sampled mask is discontinuous where a sampling coordinate is a half-integer.  `ambiguous` marks the pixels
whose oracle coordinate lies within HALF_TOL px of one; they are left out of the mask comparison and must be at most
HALF_SHARE of a case (test_manipulate_cpu.py checks that on the CPU rasterizer's depth for every case).
"""
import math

import numpy as np

import sweep_cases as sc

ROT_CENTER = 1.0
MIN_DEPTH, MAX_DEPTH = 0.9, 1.1
MARGIN = (MAX_DEPTH - MIN_DEPTH) / 2
DEPTH_LO, DEPTH_HI = MIN_DEPTH - MARGIN, MAX_DEPTH + MARGIN       # warp_canon_depth's clamp
RASTER_NEAR, RASTER_FAR = 0.1, 100.0                              # render_depth's near / far
HALF_TOL, HALF_SHARE = 1e-4, 5e-3

intrinsics = sc.intrinsics
rotation = sc.rotation


def rays_of(S, K=None):
    """(S*S, 3) float64 K^-1 (u, v, 1)^T, K = intrinsics(S) unless given."""
    K = intrinsics(S) if K is None else K
    v, u = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    return np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1).reshape(-1, 3)


def view_pose(view, base=None):
    """(12,) float64 A, t of the posed-vertex map of one frame, from the chain applied to the basis:
    p -> R (p - c) + c + t_view, after the same map of `base` when given."""
    c = np.array([0.0, 0.0, ROT_CENTER])

    def chain(p):
        for v in ([] if base is None else [base]) + [view]:
            p = rotation(*v[:3]) @ (p - c) + c + np.asarray(v[3:6], np.float64)
        return p
    t = chain(np.zeros(3))
    A = np.stack([chain(e) - t for e in np.eye(3)], 1)
    return np.concatenate([A.reshape(9), t])


def shade(albedo, normal, light):
    """g2s_shading_fwd in float64: albedo (C,S,S), normal (S,S,3), light (4,) raw -> (C,S,S)."""
    a, b = light[0] / 2 + 0.5, light[1] / 2 + 0.5
    d = np.array([light[2], light[3], 1.0])
    d = d / np.sqrt((d * d).sum())
    return (albedo / 2 + 0.5) * (a + b * np.maximum(normal @ d, 0.0))[None] * 2 - 1


def oracle_pseudo(warped, pose, albedo, normal=None, light=None, mask=None, lo=DEPTH_LO, hi=DEPTH_HI, K=None):
    """g2s_sweep_pseudo in float64.  warped (B*V,S,S), pose (B,V,12), albedo (B,C,S,S), normal (B,S,S,3) and light
    (B*V,4) both or neither, mask (B,S,S) or None.  Returns dict(im (B*V,C,S,S), mask (B*V,S,S), ix, iy (B*V,S,S) the
    sampling coordinates in texels).  K: the intrinsics, intrinsics(S) unless given."""
    warped, pose, albedo = (np.asarray(x, np.float64) for x in (warped, pose, albedo))
    BV, S, _ = warped.shape
    B, V = pose.shape[:2]
    C = albedo.shape[1]
    assert BV == B * V
    K = intrinsics(S) if K is None else np.asarray(K, np.float64)
    rays = rays_of(S, K)
    im = np.zeros((BV, C, S, S))
    mout = np.zeros((BV, S, S))
    IX, IY = np.zeros((BV, S, S)), np.zeros((BV, S, S))
    for f in range(BV):
        b = f // V
        A, t = pose[b, f % V, :9].reshape(3, 3), pose[b, f % V, 9:]
        d = np.clip(warped[f].reshape(-1), lo, hi)
        q = (d[:, None] * rays - t) @ A                      # A^T z per row
        uv = (q / q[:, 2:]) @ K.T
        ix, iy = uv[:, 0], uv[:, 1]
        IX[f], IY[f] = ix.reshape(S, S), iy.reshape(S, S)
        tex = albedo[b] if light is None else shade(albedo[b], np.asarray(normal[b], np.float64),
                                                    np.asarray(light[f], np.float64))
        x0, y0 = np.floor(ix), np.floor(iy)
        acc = np.zeros((C, S * S))
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):      # nw, ne, sw, se
            x, y = x0 + dx, y0 + dy
            w = (1 - np.abs(ix - x)) * (1 - np.abs(iy - y))
            ok = (x >= 0) & (x < S) & (y >= 0) & (y < S)
            xi, yi = np.where(ok, x, 0).astype(int), np.where(ok, y, 0).astype(int)
            acc += np.where(ok, w, 0.0)[None] * tex[:, yi, xi]
        im[f] = np.clip(acc, -1, 1).reshape(C, S, S)
        rx, ry = np.rint(ix), np.rint(iy)                    # round half to even
        ok = (rx >= 0) & (rx <= S - 1) & (ry >= 0) & (ry <= S - 1)
        src = np.ones((S, S)) if mask is None else np.asarray(mask[b], np.float64)
        mout[f] = np.where(ok, src[np.where(ok, ry, 0).astype(int), np.where(ok, rx, 0).astype(int)], 0.0).reshape(S, S)
    return dict(im=im, mask=mout, ix=IX, iy=IY)


def ambiguous(ix, iy):
    """Pixels whose nearest texel hangs on rounding: a coordinate within HALF_TOL px of a half-integer."""
    def near_half(x):
        return np.abs(x - np.floor(x) - 0.5) <= HALF_TOL
    return near_half(ix) | near_half(iy)


def canonical_verts(depth, S):
    """(B,S,S) depth -> (B,S*S,3) float32 canonical mesh, depth * ray."""
    return (depth.reshape(len(depth), -1, 1).astype(np.float64) * rays_of(S)[None]).astype(np.float32)


def posed_verts(verts, pose):
    """(B,N,3), (B,V,12) -> (B*V,N,3) float32: g2s_sweep_verts in float64."""
    v, p = np.asarray(verts, np.float64), np.asarray(pose, np.float64)
    B, V = p.shape[:2]
    out = np.einsum("bvij,bnj->bvni", p[..., :9].reshape(B, V, 3, 3), v) + p[:, :, None, 9:]
    return out.reshape(B * V, -1, 3).astype(np.float32)


def _make(seed, S, B, V, yaw_deg=60.0):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S), indexing="ij")
    depth = np.stack([1.0 - 0.05 * (1.2 - x * x - y * y) * (1 - 0.5 * (b % 2)) + 0.002 * rng.standard_normal((S, S))
                      for b in range(B)]).astype(np.float32)
    views = np.zeros((B, V, 6))
    views[..., 1] = np.linspace(-yaw_deg, yaw_deg, B * V).reshape(B, V) * math.pi / 180 if B * V > 1 else 0.35
    views[..., 0] = rng.uniform(-0.2, 0.2, (B, V))
    views[..., 2] = rng.uniform(-0.1, 0.1, (B, V))
    views[..., 3:] = rng.uniform(-0.03, 0.03, (B, V, 3))
    pose = np.stack([np.stack([view_pose(views[b, v]) for v in range(V)]) for b in range(B)])
    light = np.concatenate([rng.uniform(-0.6, 0.2, (B * V, 2)), rng.uniform(-0.8, 0.8, (B * V, 2))], 1)
    m = (rng.uniform(0, 1, (B, S, S)) > 0.3).astype(np.float32)
    return dict(S=S, B=B, V=V, depth=depth, views=views.astype(np.float32), pose=pose.astype(np.float32),
                albedo={C: rng.uniform(-1, 1, (B, C, S, S)).astype(np.float32) for C in (1, 3)},
                normal=sc.normals_of(depth, S), light=light.astype(np.float32), mask=m)


CASES = {f"S{S}_B{B}V{V}": _make(100 * S + 10 * B + V, S, B, V) for S in (8, 33, 64) for B, V in ((1, 1), (2, 5))}

# (C, light?, mask?, mask_out?) per run of a case: each channel count with and without a light, a mask given and not,
# with mask_out and with mask_out == NULL (for a given mask and for none)
RUNS = ((3, True, True, True), (1, False, False, True), (3, True, False, False), (1, False, True, True),
        (1, True, False, True), (3, False, True, False))


def run_args(c, C, lit, masked):
    return dict(albedo=c["albedo"][C], normal=c["normal"] if lit else None, light=c["light"] if lit else None,
                mask=c["mask"] if masked else None)


def relit_rows(light_a, light_b, dxy, rand, alpha):
    """The raw light rows that reproduce sample_pseudo_imgs' relighting: a' = light_a + alpha * rand and
    b' = light_b + rand, so a = 2 a' - 1, b = 2 b' - 1."""
    rand = np.asarray(rand, np.float64).reshape(-1, 1)
    a = (float(np.asarray(light_a).reshape(-1)[0]) + alpha * rand) * 2 - 1
    b = (float(np.asarray(light_b).reshape(-1)[0]) + rand) * 2 - 1
    return np.concatenate([a, b, np.asarray(dxy, np.float64)], 1)


def view_transformation(views, rot_range=60.0, txy=0.1, tz=0.1):
    """GAN2Shape.get_view_transformation with the model's default ranges."""
    v = np.asarray(views, np.float64)
    return np.concatenate([v[:, :3] * math.pi / 180 * rot_range, v[:, 3:5] * txy, v[:, 5:] * tz], 1)
