"""Viewing path without a GPU: the float64 oracle of sweep_cases.py against hand-computed values, sweep_shade_torch
and the pose composition against it, and gan2shape_amd.visualize (poses, lights, files, the command with a recording
stub in place of render_sweep: the rasterizer runs on the GPU only)."""
import math
import os

import numpy as np
import pytest
import torch

import sweep_cases as sc


@pytest.fixture(scope="module")
def capi():
    from oracle import capi
    return capi


def _raster(capi, c, posed):
    r = capi.render_depth(posed.astype(np.float32), sc.faces_of(c), c["S"], sc.intrinsics(c["S"]), ssaa=c["ssaa"],
                          near=sc.NEAR, far=sc.FAR)
    return r["face_idx"], r["bary"]


# ------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_on_the_hand_computed_3x3_mesh(capi):
    """Flat 3 x 3 mesh at depth 1 in front of a 3 x 3 image, ssaa 1.  Vertex column j projects to pixel coordinate j,
    the centre of sample x is at pixel coordinate x + 1/2: sample (y, x) sees the CENTRE of quad (y, x) for y, x < 2,
    and nothing at y = 2 or x = 2.  The centre of a quad lies on its diagonal (i, j+1) - (i+1, j): the winner holds
    weights 1/2 on those two vertices and 0 on the third, so the colour is the mean of the two.  Raster rows are
    stored bottom-up (row 2 is the top)."""
    depth = np.ones((1, 3, 3), np.float32)
    verts = sc.grid_verts(depth, 3)
    faces = sc.grid_faces(3)
    # faces2 of quad (i, j) is number 4 + 2 i + j = ((i,j+1), (i+1,j), (i+1,j+1)): weights (1/2, 1/2, 0)
    face_idx = np.array([[[-1, -1, -1], [6, 7, -1], [4, 5, -1]]], np.int32)
    bary = np.zeros((1, 3, 3, 3), np.float32)
    bary[0, 1:, :2] = (0.5, 0.5, 0.0)
    attr = np.arange(27, dtype=np.float32).reshape(1, 3, 3, 3) / 13 - 1
    normal = sc.normals_of(depth, 3)
    pose = np.array([[[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]]], np.float32)
    light = np.array([[0.25, 0.5, 0.0, 0.6, 0.8]], np.float32)
    bg = (1.0, -1.0, 0.5)
    want = np.empty((3, 3, 3))
    want[:] = np.array(bg)[:, None, None]
    for i in range(2):
        for j in range(2):
            want[:, i, j] = (attr[0, :, i, j + 1].astype(np.float64) + attr[0, :, i + 1, j]) / 2
    alpha_want = np.zeros((3, 3))
    alpha_want[:2, :2] = 1

    def run(mode):
        return sc.oracle_shade(verts, faces, face_idx, bary, attr, normal, pose, light, 1, 1, 3, 1, True, mode, bg, 0.7)
    rgb, alpha = run(0)
    np.testing.assert_allclose(rgb[0], want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(alpha[0], alpha_want)
    # flat mesh: every normal is (0, 0, 1); shade = 0.25 + 0.5 * 0.8 = 0.65
    rgb, _ = run(3)
    np.testing.assert_allclose(rgb[0, :, :2, :2], np.broadcast_to(np.array([0, 0, 1.0])[:, None, None], (3, 2, 2)), atol=1e-12)
    rgb, _ = run(2)
    np.testing.assert_allclose(rgb[0, :, :2, :2], 0.7 * 0.65 * 2 - 1, atol=1e-7)
    rgb, _ = run(1)
    np.testing.assert_allclose(rgb[0, :, :2, :2], (want[:, :2, :2] / 2 + 0.5) * 0.65 * 2 - 1, atol=1e-7)
    assert (rgb[0, :, 2, :] == np.array(bg)[:, None]).all() and (rgb[0, :, :, 2] == np.array(bg)[:, None]).all()
    # the rasterizer's own maps: same coverage, same point of the mesh under every sample (the id may differ on the
    # diagonal, where both faces of the quad hold the sample)
    r = capi.render_depth(verts, faces, 3, sc.intrinsics(3), ssaa=1, near=sc.NEAR, far=sc.FAR)
    np.testing.assert_array_equal(r["face_idx"] >= 0, face_idx >= 0)
    for y, x in zip(*np.nonzero(face_idx[0] >= 0)):
        p_hand = bary[0, y, x] @ verts[0, faces[face_idx[0, y, x]]]
        p_rast = r["bary"][0, y, x] @ verts[0, faces[r["face_idx"][0, y, x] % 8]]
        np.testing.assert_allclose(p_hand, p_rast, atol=1e-6)
    rgb_r, alpha_r = sc.oracle_shade(verts, faces, r["face_idx"], r["bary"], attr, normal, pose, light, 1, 1, 3, 1, True,
                                     0, bg, 0.7)
    np.testing.assert_allclose(rgb_r[0], want, atol=1e-6)
    np.testing.assert_array_equal(alpha_r[0], alpha_want)


def test_oracle_verts_is_the_sequential_chain():
    c = sc.CASES["17x17_poses"]
    posed = sc.oracle_verts(c["verts"], c["pose"])
    ctr = np.array([0, 0, sc.ROT_CENTER])
    for b, v, n in ((0, 0, 5), (1, 6, 288), (1, 3, 144)):
        p = c["verts"][b, n].astype(np.float64)
        R0, t0 = sc.rotation(*c["v_before"][b, :3]), c["v_before"][b, 3:]
        p = R0.T @ (p - t0 - ctr) + ctr
        p = sc.rotation(*c["rotations"][b, v].astype(np.float64)) @ (p - ctr) + ctr
        p = sc.rotation(*c["v_after"][b, :3]) @ (p - ctr) + ctr + c["v_after"][b, 3:]
        np.testing.assert_allclose(posed[b * c["V"] + v, n], p, atol=2e-7)     # the pose was rounded to float32


def test_cases_are_what_they_claim(capi):
    c = sc.CASES["8x8_identity"]
    assert np.array_equal(sc.oracle_verts(c["verts"], c["pose"])[0], c["verts"][0].astype(np.float64))
    c = sc.CASES["17x17_poses"]
    fidx, _ = _raster(capi, c, sc.oracle_verts(c["verts"], c["pose"]))
    F = sc.faces_of(c).shape[0]
    assert (fidx >= F).any() and (fidx < 0).any() and ((fidx >= 0) & (fidx < F)).any()    # reversed, background, front
    c = sc.CASES["6x6_masked_faces"]
    assert len(c["faces"]) < len(sc.grid_faces(6)) and not np.isin(c["faces"], [0, 1, 6, 7]).any()
    c = sc.CASES["out_of_view"]
    fidx, _ = _raster(capi, c, sc.oracle_verts(c["verts"], c["pose"]))
    assert (fidx[1] < 0).all() and (fidx[0] >= 0).any()
    assert sorted(sc.CASES["17x17_poses"]["attr"]) == [1, 3, 4]


# ----------------------------------------------------------------------------------- the torch statement, the bound
@pytest.fixture(scope="module")
def cpu_runs(capi):
    """name -> (posed64, face_idx, bary, {(mode, C): (oracle rgb, oracle alpha, torch rgb, torch alpha)}), with the
    CPU rasterizer's maps of the float32 torch vertices."""
    out = {}
    for name, c in sc.CASES.items():
        posed32 = sc.verts_torch_f32(c["verts"], c["pose"])
        fidx, bary = _raster(capi, c, posed32)
        res = {}
        for mode, C in sc.runs(name):
            a = sc.shade_args(c, mode, C, posed32, fidx, bary)
            res[(mode, C)] = sc.oracle_shade(**a) + sc.torch_shade_f32(a)
        out[name] = (posed32, fidx, bary, res)
    return out


def test_sweep_shade_torch_matches_the_oracle(cpu_runs):
    worst_v = worst_c = 0.0
    for name, (posed32, fidx, bary, res) in cpu_runs.items():
        c = sc.CASES[name]
        ev = sc.error(posed32, sc.oracle_verts(c["verts"], c["pose"]))
        worst_v = max(worst_v, ev)
        for key, (rgb64, a64, rgb32, a32) in res.items():
            e = sc.error(rgb32, rgb64)
            worst_c = max(worst_c, e)
            print(f"{name} {key}: colour e = {e:.3g}, vertices e = {ev:.3g}")
            np.testing.assert_array_equal(a32, a64)
            assert rgb32.shape == rgb64.shape == (c["B"] * c["V"], key[1] if key[0] in ("texture", "shaded") else 3,
                                                  c["S"], c["S"])
            assert e < 1e-5, (name, key, e)           # float32: a handful of roundings of O(1) values
    print(f"largest float32 torch figures: colour {worst_c:.3g}, vertices {worst_v:.3g}")
    assert 0 < worst_c and worst_v < 1e-6


def test_special_lights_and_background(cpu_runs):
    c = sc.CASES["light_lb0"]
    rgb64 = cpu_runs["light_lb0"][3][("shape", 3)][0]
    hit = cpu_runs["light_lb0"][3][("shape", 3)][1] == 1
    assert hit.any() and np.allclose(rgb64[:, 0][hit], c["grey"] * 0.45 * 2 - 1, atol=1e-12)
    c = sc.CASES["light_away"]
    rgb64, a64 = cpu_runs["light_away"][3][("shape", 3)][:2]
    assert np.allclose(rgb64[:, 0][a64 == 1], c["grey"] * 0.3 * 2 - 1, atol=1e-12)       # diffuse term 0: la alone
    c = sc.CASES["out_of_view"]
    for key, (rgb64, a64, rgb32, a32) in cpu_runs["out_of_view"][3].items():
        assert (a64[1] == 0).all() and (a32[1] == 0).all()
        bg = np.array(c["background"][:rgb64.shape[1]])
        assert (rgb64[1] == bg[:, None, None]).all() and (rgb32[1] == bg.astype(np.float32)[:, None, None]).all()


def test_pose_composition_matches_the_sequential_chain():
    from gan2shape_amd.renderer.renderer import Renderer, compose_sweep_pose
    c = sc.CASES["17x17_poses"]
    B, V = c["B"], c["V"]
    r = Renderer({"rot_center_depth": sc.ROT_CENTER}, 17, 0.9, 1.1, device="cpu")
    r._centroid = r._centroid.double()
    rot = torch.from_numpy(c["rotations"]).double()
    vb, va = torch.from_numpy(c["v_before"]), torch.from_numpy(c["v_after"])
    verts = torch.from_numpy(c["verts"]).double()
    pose = compose_sweep_pose(rot, vb, va, sc.ROT_CENTER, B)
    assert pose.shape == (B, V, 12) and pose.dtype == torch.float64
    got = torch.einsum("bvij,bnj->bvni", pose[..., :9].view(B, V, 3, 3), verts) + pose[..., None, 9:]
    # the loop of Renderer._canonical_mesh / _sweep, one step after another
    from gan2shape_amd.renderer.utils import get_transform_matrices
    R0, t0 = get_transform_matrices(vb)
    canon = r.rotate_pts(r.translate_pts(verts, -t0), R0.transpose(2, 1))
    for v in range(V):
        Ri, _ = get_transform_matrices(rot[:, v])
        posed = r.rotate_pts(canon, Ri)
        R2, t2 = get_transform_matrices(va)
        posed = r.translate_pts(r.rotate_pts(posed, R2), t2)
        assert float((got[:, v] - posed).abs().max()) < 1e-14
    # (V, 3) rotations shared by the batch, per-frame v_after (V, B, k), no v_before; against the case's own chain
    pose2 = compose_sweep_pose(rot[0], None, va.unsqueeze(0).expand(V, -1, -1), sc.ROT_CENTER, B)
    for b in range(B):
        for v in range(V):
            want = sc.chain_pose(c["rotations"][0, v].astype(np.float64), None, c["v_after"][b])
            np.testing.assert_allclose(pose2[b, v].numpy(), want, atol=1e-14)
    assert np.abs(pose.float().numpy() - c["pose"]).max() < 2e-7
    assert torch.equal(r.sweep_pose(rot, vb, va, B), pose)


def test_render_sweep_refuses_cpu_tensors():
    from gan2shape_amd.renderer.renderer import Renderer
    r = Renderer({}, 8, 0.9, 1.1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.render_sweep(torch.zeros(1, 3, 8, 8), torch.ones(1, 8, 8), torch.zeros(2, 3))


def test_symbols_are_declared():
    from gan2shape_amd import lib
    assert {"g2s_sweep_verts", "g2s_sweep_shade"} <= set(lib.SIGNATURES)
    L = lib.load()
    d = (lib.C.c_float * 16)()
    assert L.g2s_sweep_verts(None, d, d, 1, 1, 1, None) == -1 and b"NULL" in L.g2s_last_error()
    assert L.g2s_sweep_shade(d, None, d, d, d, d, d, d, 1, 1, 9, 8, 3, 1, 3, 1, 4, d, 0.7, d, None, None) == -1
    assert b"mode" in L.g2s_last_error()


# --------------------------------------------------------------------------------------------------------- visualize
def test_turntable_rotations():
    from gan2shape_amd import visualize as vz
    rot = vz.turntable_rotations()
    assert rot.shape == (120, 3) and rot.dtype == torch.float32
    assert (rot[:, 0] == 0).all() and (rot[:, 2] == 0).all()
    yaw = rot[:, 1].double().numpy()
    x = np.arange(-0.75, 0.75, 0.025)
    assert len(x) == 60
    np.testing.assert_allclose(yaw[0], -math.atan2(0.75, 1.5), rtol=1e-6)
    np.testing.assert_allclose(yaw[59], math.atan2(x[59], 1.5), rtol=1e-6)
    np.testing.assert_allclose(yaw[59], math.atan2(0.725, 1.5), rtol=1e-5)
    np.testing.assert_allclose(yaw[60], math.atan2(0.75, 1.5), rtol=1e-6)
    np.testing.assert_allclose(yaw[119], -math.atan2(0.725, 1.5), rtol=1e-5)
    np.testing.assert_allclose(yaw[60:], -yaw[:60], rtol=0, atol=1e-7)          # there and back, mirrored
    assert (np.diff(yaw[:60]) > 0).all() and (np.diff(yaw[60:]) < 0).all()
    assert vz.turntable_rotations(5).shape == (10, 3)
    yp = vz.yaw_pitch_rotations((20, 90), (5, 9))
    assert yp.shape == (14, 3) and (yp[:9, 0] == 0).all() and (yp[9:, 1] == 0).all()
    np.testing.assert_allclose(yp[:9, 1].numpy(), np.linspace(-math.pi / 2, math.pi / 2, 9), atol=1e-6)
    np.testing.assert_allclose(yp[9:, 0].numpy(), np.linspace(-math.pi / 9, math.pi / 9, 5), atol=1e-6)


def test_light_circle():
    from gan2shape_amd import visualize as vz
    li = vz.light_circle(12, 0.3, 0.6, 0.8)
    assert li.shape == (12, 5) and (li[:, 0] == 0.3).all() and (li[:, 1] == 0.6).all()
    np.testing.assert_allclose(li[:, 2:].double().norm(dim=1).numpy(), 1.0, atol=1e-6)
    xy = (li[:, 2:4] / li[:, 4:]).double()
    np.testing.assert_allclose(xy.norm(dim=1).numpy(), 0.8, atol=1e-6)
    np.testing.assert_allclose(xy[3].numpy(), [0.0, 0.8], atol=1e-6)             # a quarter of the way round
    assert (li[:, 4] > 0).all()


def test_write_obj_parses_back(tmp_path):
    from gan2shape_amd import visualize as vz
    from gan2shape_amd.renderer.renderer import Renderer
    r = Renderer({}, 6, 0.9, 1.1, device="cpu")
    depth = 1.0 + 0.01 * torch.arange(36.).reshape(6, 6)
    depth[:2, :2] = float("nan")
    v, f, uv = vz.depth_mesh(r, depth)
    image = torch.rand(3, 6, 6) * 2 - 1
    path = tmp_path / "m.obj"
    vz.write_obj(str(path), v, f, uv, image)
    recs = [line.split() for line in path.read_text().splitlines()]
    assert {rec[0] for rec in recs} == {"mtllib", "usemtl", "v", "vt", "f"}
    vs = np.array([[float(x) for x in rec[1:]] for rec in recs if rec[0] == "v"])
    vts = np.array([[float(x) for x in rec[1:]] for rec in recs if rec[0] == "vt"])
    fs = np.array([[[int(i) for i in tok.split("/")] for tok in rec[1:]] for rec in recs if rec[0] == "f"])
    assert vs.shape == (32, 3) and vts.shape == (32, 2) and np.isfinite(vs).all()
    assert len(fs) == len(sc._masked_faces(6, 2)) == 50 - 7        # the corner block touches 4 + 3 faces ... counted below
    assert fs.min() == 1 and fs.max() == 32 and (fs[..., 0] == fs[..., 1]).all()
    assert vts.min() >= 0 and vts.max() <= 1
    # the same triangles as the masked grid, by position
    want = sc._masked_faces(6, 2)
    grid = r.depth_to_3d_grid(torch.nan_to_num(depth, nan=9.0)[None])[0].reshape(-1, 3).numpy() * [1, -1, -1]
    np.testing.assert_allclose(vs[fs[..., 0] - 1], grid[want], rtol=1e-6)
    assert (tmp_path / "m.mtl").read_text().count("map_Kd m.png") == 1
    from PIL import Image
    assert Image.open(tmp_path / "m.png").size == (6, 6)
    with pytest.raises(ValueError):
        vz.write_obj(str(path), v, f + 40, uv, None)


def test_save_gif_and_pngs_read_back(tmp_path):
    from PIL import Image
    from gan2shape_amd import visualize as vz
    frames = torch.linspace(-1, 1, 7).view(7, 1, 1, 1).expand(7, 3, 5, 9).clone()
    frames[:, :, :2, :2] = 1.0
    vz.save_gif(frames, str(tmp_path / "a.gif"), duration_ms=70)
    with Image.open(tmp_path / "a.gif") as g:
        assert g.n_frames == 7 and g.size == (9, 5)
        for i in range(7):
            g.seek(i)
            assert g.info["duration"] == 70
            rgbf = np.asarray(g.convert("RGB"))
            assert (rgbf[:2, :2] == 255).all()
            assert abs(int(rgbf[4, 8, 0]) - round(i / 6 * 255)) <= 2
    # alpha composites over white
    u8 = vz.to_uint8(torch.full((3, 2, 2), -1.0), torch.tensor([[0.0, 1.0], [0.5, 0.25]]))
    assert u8[..., 0].tolist() == [[255, 0], [128, 191]]
    d = torch.tensor([[1.0, 1.5], [float("nan"), 2.0]])
    vz.depth_to_png(d, str(tmp_path / "d.png"))
    assert np.asarray(Image.open(tmp_path / "d.png")).tolist() == [[0, 128], [255, 255]]
    n = torch.tensor([[[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]])
    vz.normal_to_png(n, str(tmp_path / "n.png"))
    assert np.asarray(Image.open(tmp_path / "n.png")).tolist() == [[[128, 128, 255], [255, 128, 128]]]
    vz.save_png(torch.zeros(1, 3, 4), str(tmp_path / "p.png"))
    assert np.asarray(Image.open(tmp_path / "p.png")).shape == (3, 4, 3)


def tiny_dataset(tmp_path, size=16, block=5):
    """Two images, a config and a depth directory as `evaluate` writes it; b's depth has a NaN corner block."""
    from PIL import Image
    rng = np.random.default_rng(0)
    root = tmp_path / "data" / "face"
    root.mkdir(parents=True)
    y, x = np.meshgrid(np.linspace(-1, 1, size), np.linspace(-1, 1, size), indexing="ij")
    ddir = tmp_path / "eval" / "depth"
    ddir.mkdir(parents=True)
    for i, name in enumerate(["a.png", "b.png"]):
        img = np.stack([x * 60 + 100, y * 60 + 100, x * y * 60 + 100], -1) + rng.integers(0, 20, (size, size, 3))
        Image.fromarray(img.astype(np.uint8)).save(root / name)
        d = (1.0 - 0.05 * (1.2 - x * x - y * y)).astype(np.float32)
        if i == 1:
            d[:block, :block] = np.nan
        np.save(ddir / (name[:-4] + ".npy"), d)
    (root / "list.txt").write_text("a.png\nb.png\n")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(f"category: face\nroot_path: {tmp_path / 'data'}\nimage_size: {size}\n")
    return cfg, ddir


def test_command_with_a_recording_stub(tmp_path, monkeypatch):
    from PIL import Image
    from gan2shape_amd import visualize as vz
    from gan2shape_amd.renderer.renderer import Renderer
    cfg, ddir = tiny_dataset(tmp_path)
    calls = []

    def stub(self, im, depth, rotations, mode="texture", light=None, normal=None, faces=None, **kw):
        calls.append(dict(im=im, depth=depth, rotations=torch.as_tensor(rotations), mode=mode, light=light,
                          normal=normal, faces=faces))
        V = len(rotations)
        return torch.linspace(-1, 1, V).view(1, V, 1, 1, 1).expand(1, V, 3, 16, 16)
    monkeypatch.setattr(Renderer, "render_sweep", stub)
    out = tmp_path / "viz"
    written = vz.main(["--config", str(cfg), "--depth-dir", str(ddir), "--out", str(out), "--device", "cpu",
                       "--frames", "4", "--relight", "--obj", "--modes", "texture", "shape"])
    assert written == [str(out / "a"), str(out / "b")]
    for stem in "ab":
        assert sorted(os.listdir(out / stem)) == sorted(
            ["turntable_texture.gif", "turntable_shape.gif", "relight.gif", "depth.png", "normal.png",
             stem + ".obj", stem + ".mtl", stem + ".png"])                  # no recon.png: no model ran
        with Image.open(out / stem / "turntable_shape.gif") as g:
            assert g.n_frames == 8 and g.size == (16, 16)
    assert [c["mode"] for c in calls] == ["texture", "shape", "shaded"] * 2
    for c in calls:
        assert c["im"].shape == (1, 3, 16, 16) and c["depth"].shape == (1, 16, 16) and c["normal"].shape == (1, 16, 16, 3)
        assert torch.isfinite(c["depth"]).all() and torch.isfinite(c["normal"]).all()
    for c in calls[0:2] + calls[3:5]:
        assert torch.equal(c["rotations"], vz.turntable_rotations(4))
        assert torch.equal(c["light"], torch.tensor([vz.HEADLIGHT]).expand(8, 5))
    for c in (calls[2], calls[5]):
        assert torch.equal(c["rotations"], torch.zeros(8, 3)) and torch.equal(c["light"], vz.light_circle(8))
    assert all(c["faces"] is None for c in calls[:3])                       # a: nothing masked, the implicit grid
    want = sc._masked_faces(16, 5)
    for c in calls[3:]:                                                     # b: faces off the NaN block only
        assert c["faces"].dtype == torch.int32 and np.array_equal(c["faces"].numpy(), want)
        d = np.load(ddir / "b.npy")
        assert float(c["depth"][0, 0, 0]) == np.nanmax(d)                   # the stand-in: farthest finite depth
    assert np.asarray(Image.open(out / "b" / "depth.png"))[:5, :5].min() == 255
    assert np.asarray(Image.open(out / "b" / "normal.png"))[:5, :5].min() == 255
    n_v = sum(line.startswith("v ") for line in (out / "b" / "b.obj").read_text().splitlines())
    assert n_v == 256 - 25


def test_command_with_a_stub_model(tmp_path, monkeypatch):
    from gan2shape_amd import visualize as vz
    from gan2shape_amd.renderer.renderer import Renderer
    cfg, _ = tiny_dataset(tmp_path)

    class StubModel():
        def __init__(self):
            self.device = torch.device("cpu")
            self.renderer = Renderer({}, 16, 0.9, 1.1, device="cpu")

        def evaluate_results(self, image):
            return image * 0.5, 1.0 + 0.02 * image[:, 0]
    monkeypatch.setattr(Renderer, "render_sweep",
                        lambda self, im, depth, rotations, **kw: torch.linspace(-1, 1, len(rotations)).view(
                            1, -1, 1, 1, 1).expand(1, len(rotations), 3, 16, 16))
    out = tmp_path / "viz"
    vz.main(["--config", str(cfg), "--ckpt", "unused", "--out", str(out), "--device", "cpu", "--frames", "2",
             "--images", "1", "--modes", "normal"], model=StubModel())
    assert sorted(os.listdir(out / "b")) == ["depth.png", "normal.png", "recon.png", "turntable_normal.gif"]
    with pytest.raises(SystemExit):
        vz.main(["--config", str(cfg), "--out", str(out)])                  # neither --ckpt nor --depth-dir
