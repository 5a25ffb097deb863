"""Cases of the canonical object mask (Renderer.canon_mask, g2s_canon_mask), shared by
tests/golden/make_canon_mask_golden.py (which feeds them to the REFERENCE's Renderer parts) and the tests (which feed
them to this package's): views, canonical depths and input masks as pure functions of the case, so both sides see
identical operands.  The fixture tests/golden/canon_mask.npz stores the operands as well; the tests read them from
there and use this module for the list of cases and the renderer they run through."""
import math

import numpy as np
import torch

ROT_CENTER, FOV, MIN_DEPTH, MAX_DEPTH = 1.0, 10, 0.9, 1.1

# (rx, ry, rz, tx, ty, tz) in the units set_transform_matrices takes: radians and scene units
VIEWS = {
    "identity": (0., 0., 0., 0., 0., 0.),                       # canon_mask must reproduce the mask
    "small": (0.10, -0.15, 0.05, 0.012, -0.008, 0.),            # a small rotation plus translation
    "yaw60": (0., math.pi / 3, 0., 0., 0., 0.),                 # many samples leave the image: the zero padding
    "ztrans": (0.04, 0.08, -0.03, 0.005, 0.004, 0.09),          # a view with z-translation
}

# name: (S, views of the B samples, mask kind, mask shared by the batch)
CASES = {
    "identity_disc_s16_b1": (16, ("identity",), "disc", False),
    "identity_soft_s32_b2": (32, ("identity", "identity"), "soft", False),
    "small_disc_s32_b2": (32, ("small", "ztrans"), "disc", False),
    "small_rect_s16_b3": (16, ("small", "identity", "yaw60"), "rect", False),
    "yaw60_rect_s32_b1": (32, ("yaw60",), "rect", False),
    "yaw60_soft_s16_b2": (16, ("yaw60", "small"), "soft", False),
    "yaw60_ones_s32_b3": (32, ("yaw60", "ztrans", "small"), "ones", False),
    "ztrans_soft_s32_b3": (32, ("ztrans", "small", "yaw60"), "soft", False),
    "ztrans_disc_s16_b1": (16, ("ztrans",), "disc", False),
    "broadcast_disc_s32_b3": (32, ("small", "yaw60", "ztrans"), "disc", True),
}


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)


def depth_of(name):
    """(B, S, S) float64 canonical depth: a tilted, bumpy surface filling [MIN_DEPTH, MAX_DEPTH], one per sample."""
    S, views, _, _ = CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S, dtype=torch.float64), torch.linspace(-1, 1, S, dtype=torch.float64),
                            indexing="ij")
    out = []
    for v in views:
        a, b, p, q = (torch.rand(4, generator=g, dtype=torch.float64) * 2 - 1).tolist()
        if v == "yaw60":    # tilted along x, away from the camera on the right: the yaw pushes both sides out of the image
            a, b = 1.0, 0.1 * b
        relief = 0.6 * (a * xx + b * yy) / (abs(a) + abs(b)) + 0.4 * torch.sin(3 * xx + 3 * p) * torch.cos(2 * yy + 3 * q)
        out.append(1.0 + 0.1 * relief.clamp(-1, 1))
    return torch.stack(out)


def mask_of(name):
    """(B or 1, 1, S, S) float64 input mask in [0, 1]."""
    S, views, kind, shared = CASES[name]
    g = torch.Generator().manual_seed(_seed(name) + 1)
    n = 1 if shared else len(views)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float64), torch.arange(S, dtype=torch.float64), indexing="ij")
    out = []
    for _ in range(n):
        u = torch.rand(4, generator=g, dtype=torch.float64)
        if kind == "disc":          # hard disc, off centre
            cx, cy, r = (0.4 + 0.2 * u[0]) * S, (0.4 + 0.2 * u[1]) * S, (0.25 + 0.1 * u[2]) * S
            m = (((xx - cx) ** 2 + (yy - cy) ** 2) < r * r).double()
        elif kind == "rect":        # hard rectangle touching the left and the top border
            m = ((xx < (0.5 + 0.3 * u[0]) * S) & (yy < (0.4 + 0.4 * u[1]) * S)).double()
        elif kind == "soft":        # soft random field
            low = torch.rand(1, 1, 5, 5, generator=g, dtype=torch.float64)
            m = torch.nn.functional.interpolate(low, size=(S, S), mode="bicubic", align_corners=True)[0, 0].clamp(0, 1)
        elif kind == "ones":
            m = torch.ones(S, S, dtype=torch.float64)
        else:
            raise KeyError(kind)
        out.append(m)
    return torch.stack(out).unsqueeze(1)


def view_of(name):
    """(B, 6) float64."""
    return torch.tensor([VIEWS[v] for v in CASES[name][1]], dtype=torch.float64)


def intrinsics(S):
    """K (3,3) float64 of renderer.py:35-46 at size S."""
    f = (S - 1) / 2 / math.tan(FOV / 2 * math.pi / 180)
    c = (S - 1) / 2
    return torch.tensor([[f, 0., c], [0., f, c], [0., 0., 1.]], dtype=torch.float64)


def package_renderer(S, device, dtype=torch.float32):
    """This package's Renderer at size S; for float64 its intrinsics are rebuilt in float64 (the constructor's are
    float32, and an inverse taken in float32 would cap the float64 route at float32 accuracy)."""
    from gan2shape_amd.renderer import Renderer
    r = Renderer({"rot_center_depth": ROT_CENTER, "fov": FOV}, S, MIN_DEPTH, MAX_DEPTH, device=device)
    if dtype == torch.float64:
        K = intrinsics(S).to(device)
        r.K, r.inv_K = K.unsqueeze(0), torch.inverse(K).unsqueeze(0)
        r._rays.clear()
    return r


def run_package(r, view, depth, mask):
    """Renderer.canon_mask of one case on the device and in the dtype of `depth`."""
    r.set_transform_matrices(view.to(depth))
    return r.canon_mask(depth, mask.to(depth))


def max_err(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))
