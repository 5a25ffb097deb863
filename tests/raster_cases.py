"""Seeded rasterizer test scenes shared by the CPU and GPU parity tests."""
import math

import numpy as np

from oracle import geometry as og


def scene(S, B=2, seed=0, rot=60.0, step=True, noise=0.01):
    """GAN2Shape-like canonical depth in [0.9, 1.1] with a depth discontinuity (object vs
    background plane), viewed from random poses up to +-rot degrees / +-0.1 translation
    (model.py:49-57,330-335).  Returns (geo, verts (B, S*S, 3) f32, faces (F, 3) i32)."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    r2 = ((u - S / 2) ** 2 + (v - S / 2) ** 2) / (0.35 * S) ** 2
    depth = np.where(r2 < 1, 0.92 + 0.08 * r2, 1.08 if step else 1.0)
    depth = depth[None] + noise * rng.standard_normal((B, S, S))
    depth = np.clip(depth, 0.9, 1.1).astype(np.float32)
    view = np.concatenate([rng.uniform(-1, 1, (B, 3)) * rot * math.pi / 180,
                           rng.uniform(-1, 1, (B, 3)) * 0.1], 1).astype(np.float32)
    geo = og.Geometry(S, 0.9, 1.1, rot_center_depth=1.0, fov=10)
    geo.set_transform_matrices(view)
    verts = geo.get_warped_3d_grid(depth).reshape(B, -1, 3).astype(np.float32)
    return geo, verts, og.get_face_idx(1, S, S)[0]


def soup(n_faces=300, n_verts=200, seed=0, B=2):
    """Unstructured triangle soup around z = 1 (explicit-topology path)."""
    rng = np.random.default_rng(seed)
    verts = np.stack([rng.uniform(-0.09, 0.09, (B, n_verts)), rng.uniform(-0.09, 0.09, (B, n_verts)),
                      rng.uniform(0.9, 1.1, (B, n_verts))], -1).astype(np.float32)
    base = rng.integers(0, n_verts, n_faces)
    faces = np.stack([base, (base + rng.integers(1, 6, n_faces)) % n_verts,
                      (base + rng.integers(6, 12, n_faces)) % n_verts], -1).astype(np.int32)
    return verts, faces


def confetti(S, B=2, seed=0, flip_odd=True):
    """One small triangle per quad of the S x S pixel grid at the identity pose, each with three
    vertices of its own: quad-local points (0.1, 0.1), (0.9, 0.3), (0.3, 0.9) (row, column), placed
    bilinearly between the quad's four grid vertices, every vertex then moved along its ray by a
    seeded factor in [0.95, 1.05] (same projection, different depth) and the vertex ids scrambled.
    Odd faces have indices 0 and 2 swapped when `flip_odd`: with fill_back they win through their
    reversed copy (id + F), without it they vanish.  At ssaa 1 the sample centre of every pixel of
    the first S-1 rows and columns lies in exactly its own triangle, so a full 8x8 tile references
    192 distinct vertices.  Returns (geo, verts (B, 3(S-1)^2, 3) f32, faces ((S-1)^2, 3) i32)."""
    rng = np.random.default_rng(seed)
    geo = og.Geometry(S)
    geo.set_transform_matrices(np.zeros((B, 6), np.float32))
    grid = geo.get_warped_3d_grid(np.ones((B, S, S), np.float32)).astype(np.float64)
    v00, v10, v01, v11 = grid[:, :-1, :-1], grid[:, 1:, :-1], grid[:, :-1, 1:], grid[:, 1:, 1:]
    corners = [(1 - s) * (1 - t) * v00 + s * (1 - t) * v10 + (1 - s) * t * v01 + s * t * v11
               for s, t in ((0.1, 0.1), (0.9, 0.3), (0.3, 0.9))]
    F = (S - 1) * (S - 1)
    verts = np.stack(corners, 3).reshape(B, 3 * F, 3)          # vertex 3 f + k = corner k of face f
    verts = verts * rng.uniform(0.95, 1.05, (B, 3 * F, 1))
    faces = np.arange(3 * F).reshape(F, 3)
    if flip_odd:
        faces[1::2] = faces[1::2, ::-1]
    perm = rng.permutation(3 * F)
    scrambled = np.empty_like(verts)
    scrambled[:, perm] = verts
    return geo, scrambled.astype(np.float32), perm[faces].astype(np.int32)


def forward_stats(fw, faces):
    """From an oracle forward result: (share of covered samples, share of the covered samples won by
    a reversed copy, face_idx >= F, largest number of distinct vertices referenced in any 8x8 tile of
    any image)."""
    fi = fw["face_idx"]
    F = faces.shape[0]
    cov = fi >= 0
    most = 0
    for img in fi:
        for y in range(0, img.shape[0], 8):
            for x in range(0, img.shape[1], 8):
                t = img[y:y + 8, x:x + 8]
                most = max(most, np.unique(faces[t[t >= 0] % F]).size)
    return float(cov.mean()), float((fi >= F).sum() / max(int(cov.sum()), 1)), most


# ----------------------------------------------------------------------------- the depth-path case table
FAR = 100.0


class Case:
    """One row of the table the CPU and GPU depth-path tests share.  `grid`: the faces are the regular
    grid's, so the implicit topology (faces = None) must give the same result."""

    def __init__(self, name, S, ssaa, fill_back, make, grid=False):
        self.name, self.S, self.ssaa, self.fill_back, self.grid = name, S, ssaa, fill_back, grid
        self._make = make
        self._data = None

    def __repr__(self):
        return self.name

    @property
    def topologies(self):  # implicit flags to run
        return (False, True) if self.grid else (False,)

    def data(self):
        """verts, faces, K, then everything the oracle says about them, computed once: fw (fp32
        forward), g (upstream gradient: seeded normal, 0 where the oracle depth exceeds 1.2 — the
        clamp of warp_canon_depth), ref32 / ref64 (oracle backward in fp32 / float64 on the fp32
        forward's maps), e32 = max|ref32 - ref64|, scale = max|ref64| and the bound on
        max|kernel - ref64|: 4 e32 + 5e-6 scale (summation order apart, the kernels do the fp32
        oracle's arithmetic; the factor covers the re-association through merges, LDS table and
        atomics, the floor the cases where fp32 lands within an ulp or two of float64)."""
        if self._data is None:
            from oracle import capi
            verts, faces, K = self._make()
            S, ssaa, B = self.S, self.ssaa, verts.shape[0]
            fw = capi.render_depth(verts, faces, S, K, ssaa=ssaa, fill_back=self.fill_back, far=FAR)
            g = np.random.default_rng(len(self.name) + S).standard_normal((B, S, S)).astype(np.float32)
            if self.name != "background":     # there every pixel is at `far`: keep g, the result must still be 0
                g[fw["depth"] > 1.2] = 0
            ref32 = capi.render_depth_bwd(verts, faces, g, fw["face_idx"], fw["bary"], S, K, ssaa=ssaa)
            ref64 = capi.render_depth_bwd(verts.astype(np.float64), faces, g.astype(np.float64),
                                          fw["face_idx"], fw["bary"].astype(np.float64), S,
                                          K.astype(np.float64), ssaa=ssaa, dtype=np.float64)
            e32 = float(np.abs(ref32 - ref64).max())
            scale = float(np.abs(ref64).max())
            self._data = dict(verts=verts, faces=faces, K=K, fw=fw, g=g, ref32=ref32, ref64=ref64,
                              e32=e32, scale=scale, bound=4 * e32 + 5e-6 * scale)
            for a in (verts, faces, K, g, ref32, ref64, *fw.values()):
                a.setflags(write=False)
        return self._data


def _scene_case(name, S, seed, ssaa, fill_back):
    def make():
        geo, verts, faces = scene(S, B=2, seed=seed)
        return verts, faces, geo.K[0]
    return Case(name, S, ssaa, fill_back, make, grid=True)


def _soup_case(name, fill_back):
    def make():
        verts, faces = soup(700, 300)
        return verts, faces, og.Geometry(24).K[0]
    return Case(name, 24, 2, fill_back, make)


def _confetti_case(name, S, fill_back, flip_odd=True):
    def make():
        geo, verts, faces = confetti(S, flip_odd=flip_odd)
        return verts, faces, geo.K[0]
    return Case(name, S, 1, fill_back, make)


def _background_case():
    def make():   # every vertex pushed along its ray to z ~ 150 > far: binned, evaluated, rejected
        geo, verts, faces = scene(13, B=2, seed=15)
        return (verts * np.float32(150.0)).astype(np.float32), faces, geo.K[0]
    return Case("background", 13, 2, True, make, grid=True)


CASES = [
    _scene_case("grid", 32, 34, 2, True),        # baseline, a few reversed winners
    _scene_case("ss1", 16, 17, 1, True),         # ssaa 1
    _scene_case("nofill", 16, 18, 2, False),     # fill_back off
    _scene_case("ragged1", 13, 14, 1, True),     # side 13: 2 x 2 tiles, the outer ones partial
    _scene_case("ragged2", 18, 20, 2, True),     # side 36: 5 x 5 tiles (odd, 25 % 8 != 0), partial
    _soup_case("soup", True),                    # about 60 % reversed winners, long face lists
    _soup_case("soup_nofill", False),
    _confetti_case("confetti", 16, True),        # vertex table overflow, half the winners reversed
    _confetti_case("confetti_nofill", 16, False),             # the flipped half vanishes: 96 vertices in a tile
    _confetti_case("confetti_noflip_nofill", 16, False, False),  # overflow with fill_back off
    _confetti_case("confetti17", 17, True),      # overflow, 3 x 3 tiles: full ones beside 1-sample slivers
]
BACKGROUND = _background_case()                  # nothing drawn: depth = far, face_idx = -1, zero gradient
CASE = {c.name: c for c in CASES + [BACKGROUND]}
