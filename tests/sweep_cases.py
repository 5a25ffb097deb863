"""Cases and the float64 oracle of the viewing path (csrc/sweep.hip: g2s_sweep_verts, g2s_sweep_shade).

The oracle restates the formulas of include/g2s.h in numpy float64, sample by sample, and takes `face_idx` and `bary`
as INPUTS, so that it never disagrees with the rasterizer about winners.  Every case is seeded and is the smallest
shape at which its path can still go wrong.

Error figure of colours and posed vertices: e = |got - want| / (1 + |want|).  Bound: 4 x the largest e that the same
formula in float32 torch ops on the CPU (sweep_shade_torch; `verts_torch_f32` for the vertices) shows against the
oracle over ALL cases, on the same face_idx / bary: the kernel may order its few multiply-adds differently from
torch but does no more work.  Alpha is a count over ssaa^2 samples and must be equal.
"""
import math

import numpy as np

FOV = 10.0
NEAR, FAR = 0.1, 10.0          # the renderer's near / far (renderer_min_depth, renderer_max_depth)
ROT_CENTER = 1.0
MODES = {"texture": 0, "shaded": 1, "shape": 2, "normal": 3}


def intrinsics(S):
    f = (S - 1) / 2 / math.tan(FOV / 2 * math.pi / 180)
    c = (S - 1) / 2
    return np.array([[f, 0, c], [0, f, c], [0, 0, 1]], np.float64)


def grid_verts(depth, S):
    """(B, m, m) depth -> (B, m*m, 3) float32 camera-space points of an m x m mesh spread over the S x S image."""
    B, m, _ = depth.shape
    K = intrinsics(S)
    u = np.linspace(0, S - 1, m)
    vv, uu = np.meshgrid(u, u, indexing="ij")
    rays = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu)], -1)
    return (rays[None] * depth[..., None]).reshape(B, -1, 3).astype(np.float32)


def grid_faces(m):
    idx = np.arange(m * m).reshape(m, m)
    f1 = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:]], -1).reshape(-1, 3)
    f2 = np.stack([idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]], -1).reshape(-1, 3)
    return np.concatenate([f1, f2]).astype(np.int32)


def rotation(rx, ry, rz):
    """Rz Ry Rx, the convention of get_transform_matrices."""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    mx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    my = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    mz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return mz @ my @ mx


def chain_pose(rot, v_before=None, v_after=None):
    """(12,) float64 A, t of ONE frame from the sequential chain, applied to the basis: undo of v_before, the sweep
    rotation about the centre, v_after — written step by step, as Renderer._canonical_mesh / _sweep apply them."""
    c = np.array([0.0, 0.0, ROT_CENTER])

    def chain(p):
        if v_before is not None:
            R0, t0 = rotation(*v_before[:3]), np.asarray(v_before[3:6], np.float64)
            p = R0.T @ (p - t0 - c) + c
        p = rotation(*rot) @ (p - c) + c
        if v_after is not None:
            R2, t2 = rotation(*v_after[:3]), np.asarray(v_after[3:6], np.float64)
            p = R2 @ (p - c) + c + t2
        return p
    t = chain(np.zeros(3))
    A = np.stack([chain(e) - t for e in np.eye(3)], 1)
    return np.concatenate([A.reshape(9), t])


def normals_of(depth, S):
    """Unit normals (B, m, m, 3) float32 of the mesh, central differences of its points, border (0, 0, 1)."""
    B, m, _ = depth.shape
    p = grid_verts(depth, S).astype(np.float64).reshape(B, m, m, 3)
    n = np.zeros_like(p)
    n[..., 2] = 1.0
    tu = p[:, 1:-1, 2:] - p[:, 1:-1, :-2]
    tv = p[:, 2:, 1:-1] - p[:, :-2, 1:-1]
    n[:, 1:-1, 1:-1] = np.cross(tu, tv)
    return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)


def _make(seed, m, S, ssaa, B, poses, v_before=None, v_after=None, faces=None, channels=(3,), modes=tuple(MODES),
          lights=None, background=(1.0, 1.0, 1.0, 1.0), bump=0.04, shift=None):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, m), np.linspace(-1, 1, m), indexing="ij")
    # image 0 is a hill, image 1 a bowl: seen from the side, the near wall of a bowl shows its back (reversed winners)
    depth = np.stack([1.0 - bump * (1.2 - x * x - y * y) * (1 - 2.3 * (b % 2)) + 0.004 * rng.standard_normal((m, m))
                      for b in range(B)])
    poses = np.asarray(poses, np.float64)
    V = poses.shape[-2]
    poses = np.broadcast_to(poses, (B, V, 3))
    pose = np.stack([np.stack([chain_pose(poses[b, v], None if v_before is None else v_before[b],
                                          None if v_after is None else v_after[b]) for v in range(V)])
                     for b in range(B)])
    if shift is not None:                       # frames translated on top of the chain (out of view)
        pose[:, shift[0], 9:] += np.asarray(shift[1], np.float64)
    if lights is None:
        d = rng.standard_normal((B, V, 3)) * np.array([0.4, 0.4, 0.0]) + np.array([0.0, 0.0, 1.0])
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        lights = np.concatenate([rng.uniform(0.2, 0.5, (B, V, 1)), rng.uniform(0.3, 0.7, (B, V, 1)), d], -1)
    lights = np.broadcast_to(np.asarray(lights, np.float64), (B, V, 5))
    return dict(m=m, S=S, ssaa=ssaa, B=B, V=V, depth=depth.astype(np.float32),
                verts=grid_verts(depth.astype(np.float32), S), pose=pose.astype(np.float32),
                rotations=poses.astype(np.float32), v_before=v_before, v_after=v_after, faces=faces,
                attr={C: rng.uniform(-1, 1, (B, C, m, m)).astype(np.float32) for C in channels},
                normal=normals_of(depth.astype(np.float32), S), light=lights.astype(np.float32).reshape(B * V, 5),
                modes=modes, background=background, grey=0.7)


def _masked_faces(m, block):
    """Faces of the m x m grid without those that touch the top-left block x block corner."""
    valid = np.ones((m, m), bool)
    valid[:block, :block] = False
    f = grid_faces(m)
    return f[valid.reshape(-1)[f].all(1)]


_ZERO = [[0.0, 0.0, 0.0]]
_D = math.pi / 180
_YAW_PITCH = [[0, -60 * _D, 0], [0, -25 * _D, 0], [0, 0, 0], [0, 40 * _D, 0], [0, 60 * _D, 0], [-20 * _D, 0, 0],
              [20 * _D, 10 * _D, 0]]
_AWAY = np.array([0.3, 0.6, 0.0, 0.0, -1.0])      # a light facing away from every front-facing normal

CASES = {
    "3x3_ssaa1": _make(1, 3, 3, 1, 1, _ZERO),
    "3x3_ssaa2": _make(2, 3, 3, 2, 1, [[0, 0.2, 0], [0.1, -0.3, 0.05]]),
    "8x8_identity": _make(3, 8, 8, 2, 1, _ZERO),
    "17x17_poses": _make(4, 17, 17, 2, 2, _YAW_PITCH,
                         v_before=np.array([[0.05, -0.1, 0.02, 0.01, -0.005, 0.0], [-0.04, 0.08, 0.0, 0.0, 0.01, 0.005]]),
                         v_after=np.array([[0.03, 0.06, -0.02, 0.004, 0.0, 0.01], [0.0, -0.05, 0.03, -0.003, 0.002, 0.0]]),
                         channels=(1, 3, 4), background=(1.0, -0.5, 0.25, 0.0)),
    "6x6_masked_faces": _make(5, 6, 16, 2, 1, [[0, 0.3, 0], [0.15, -0.2, 0]], faces=_masked_faces(6, 2)),
    "out_of_view": _make(6, 5, 5, 2, 1, [[0, 0.1, 0], [0, 0.1, 0]], shift=(1, [5.0, 0.0, 0.0]),
                         background=(0.25, -0.5, 0.75, 1.0)),
    "light_lb0": _make(7, 5, 5, 2, 1, [[0, 0.2, 0]], modes=("shaded", "shape"), lights=[0.45, 0.0, 0.2, -0.1, 0.97]),
    "light_away": _make(8, 5, 5, 2, 1, _ZERO, modes=("shaded", "shape"), lights=_AWAY),
}


def runs(name):
    """(mode name, C) pairs a case is rendered with: every mode, and every channel count in mode texture."""
    c = CASES[name]
    first = min(c["attr"])
    out = []
    for mode in c["modes"]:
        for C in (sorted(c["attr"]) if mode == "texture" else [3 if 3 in c["attr"] else first]):
            out.append((mode, C))
    return out


def faces_of(c):
    return grid_faces(c["m"]) if c["faces"] is None else c["faces"]


# ------------------------------------------------------------------------------------------------------- the oracle
def oracle_verts(verts, pose):
    """(B, N, 3), (B, V, 12) -> (B*V, N, 3) float64."""
    v, p = verts.astype(np.float64), pose.astype(np.float64)
    B, V = p.shape[:2]
    out = np.empty((B, V) + v.shape[1:])
    for b in range(B):
        for k in range(V):
            A, t = p[b, k, :9].reshape(3, 3), p[b, k, 9:]
            for n in range(v.shape[1]):
                out[b, k, n] = A @ v[b, n] + t
    return out.reshape(B * V, -1, 3)


def oracle_shade(posed, faces, face_idx, bary, attr, normal, pose, light, B, V, S, ssaa, fill_back, mode, background,
                 grey):
    """g2s_sweep_shade in float64, one sample at a time.  Returns (rgb (B*V, Cout, S, S), alpha (B*V, S, S))."""
    mode = MODES.get(mode, mode)
    posed = np.asarray(posed, np.float64)
    F, N, isz = faces.shape[0], posed.shape[1], S * ssaa
    C = attr.shape[1] if mode in (0, 1) else 3
    at = None if attr is None else attr.astype(np.float64).reshape(B, -1, N)
    nm = None if normal is None else normal.astype(np.float64).reshape(B, N, 3)
    po = None if pose is None else pose.astype(np.float64).reshape(B * V, 12)
    li = None if light is None else light.astype(np.float64).reshape(B * V, 5)
    bg = np.array([background[min(i, len(background) - 1)] for i in range(C)], np.float64)
    rgb = np.zeros((B * V, C, S, S))
    alpha = np.zeros((B * V, S, S))
    for f in range(B * V):
        b = f // V
        for r in range(S):
            for c0 in range(S):
                for dy in range(ssaa):
                    for dx in range(ssaa):
                        yi, xi = isz - 1 - (r * ssaa + dy), c0 * ssaa + dx
                        fn = int(face_idx[f, yi, xi])
                        if fn < 0:
                            rgb[f, :, r, c0] += bg
                            continue
                        alpha[f, r, c0] += 1
                        v = [int(x) for x in faces[fn % F]]
                        if fill_back and fn >= F:
                            v = v[::-1]
                        w = bary[f, yi, xi].astype(np.float64)
                        z = posed[f, v, 2]
                        u = w * (1.0 / np.sum(w / z)) / z
                        if mode in (0, 1):
                            a = at[b][:, v] @ u
                        if mode == 0:
                            rgb[f, :, r, c0] += a
                            continue
                        n = po[f, :9].reshape(3, 3) @ (u @ nm[b, v])
                        n = n / max(np.linalg.norm(n), 1e-12)
                        if mode == 3:
                            rgb[f, :, r, c0] += n
                            continue
                        shade = li[f, 0] + li[f, 1] * max(0.0, float(n @ li[f, 2:]))
                        rgb[f, :, r, c0] += ((a / 2 + 0.5) if mode == 1 else grey) * shade * 2 - 1
    return rgb / (ssaa * ssaa), alpha / (ssaa * ssaa)


def verts_torch_f32(verts, pose):
    """The float32 comparator of g2s_sweep_verts: A . v + t in elementwise torch ops on the CPU -> (B*V, N, 3)."""
    import torch
    v, p = torch.from_numpy(verts)[:, None], torch.from_numpy(pose)[:, :, None]          # (B,1,N,3), (B,V,1,12)
    out = [(p[..., 3 * c] * v[..., 0] + p[..., 3 * c + 1] * v[..., 1]) + p[..., 3 * c + 2] * v[..., 2] + p[..., 9 + c]
           for c in range(3)]
    return torch.stack(out, -1).reshape(-1, verts.shape[1], 3).numpy()


def error(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (1 + np.abs(want))).max())


def shade_args(c, mode, C, posed, face_idx, bary):
    """Positional arguments of oracle_shade / sweep_shade_torch for one run of a case (numpy)."""
    m = MODES[mode]
    return dict(posed=posed, faces=faces_of(c), face_idx=face_idx, bary=bary, attr=c["attr"][C] if m in (0, 1) else None,
                normal=c["normal"] if m else None, pose=c["pose"], light=c["light"] if m in (1, 2) else None,
                B=c["B"], V=c["V"], S=c["S"], ssaa=c["ssaa"], fill_back=True, mode=m,
                background=c["background"], grey=c["grey"])


def torch_shade_f32(a):
    """sweep_shade_torch in float32 on the CPU with the arguments of `shade_args` -> (rgb, alpha) numpy."""
    import torch
    from gan2shape_amd.plugins.neural_renderer import sweep_shade_torch
    t = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    rgb, alpha = sweep_shade_torch(t["posed"], t["faces"], t["face_idx"], t["bary"], t["attr"], t["normal"], t["pose"],
                                   t["light"], a["B"], a["V"], a["S"], a["ssaa"], a["fill_back"], a["mode"],
                                   a["background"], a["grey"])
    return rgb.numpy(), alpha.numpy()
