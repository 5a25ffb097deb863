"""The pseudo-view pass and the manipulation path, without a GPU: the float64 oracle of manipulate_cases.py against a
hand-computed case, against the torch statement of the training renderer in float64 and against the reference's own
run (tests/golden/steps.npz); then the host logic (poses, helpers, chunks, argument checks, the command)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import manipulate_cases as mc
import sweep_cases as sc


@pytest.fixture(scope="module")
def capi():
    from oracle import capi
    return capi


def warped_of(capi, c):
    """The CPU rasterizer's depth of the posed meshes of a case, as render_depth calls it."""
    S = c["S"]
    posed = mc.posed_verts(mc.canonical_verts(c["depth"], S), c["pose"])
    return capi.render_depth(posed, sc.grid_faces(S), S, mc.intrinsics(S), near=mc.RASTER_NEAR, far=mc.RASTER_FAR)["depth"]


@pytest.fixture(scope="module")
def warped(capi):
    return {name: warped_of(capi, c) for name, c in mc.CASES.items()}


# ------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_on_the_hand_computed_case():
    """Identity pose, flat depth 1, S = 5: every grid point is a pixel centre.  Then a shift of exactly k pixels.
    Once with the cases' intrinsics (to 1e-12) and once with fx = fy = 4, cx = cy = 2, for which every ray, t_x = k / fx
    and every coordinate is an exact binary fraction: there the results are EQUAL and the vacated columns exactly 0."""
    S, k = 5, 2
    rng = np.random.default_rng(0)
    albedo = rng.uniform(-1, 1, (1, 3, S, S))
    normal = sc.normals_of(np.ones((1, S, S), np.float32), S)
    light = np.array([[-0.3, 0.1, 0.4, -0.2]])
    mask = (rng.uniform(0, 1, (1, S, S)) > 0.4).astype(np.float64)
    flat = np.ones((1, S, S))
    want = mc.shade(albedo[0], normal[0].astype(np.float64), light[0])
    exact_K = np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]])
    for K, tol in ((None, 1e-12), (exact_K, 0.0)):
        fx = mc.intrinsics(S)[0, 0] if K is None else K[0, 0]
        pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).reshape(1, 1, 12)
        r = mc.oracle_pseudo(flat, pose, albedo, normal, light, mask, K=K)
        assert np.abs(r["im"][0] - want).max() <= tol and np.array_equal(r["mask"][0], mask[0])
        r0 = mc.oracle_pseudo(flat, pose, albedo, K=K)                         # no light: the albedo as given
        assert np.abs(r0["im"][0] - albedo[0]).max() <= tol and np.array_equal(r0["mask"][0], np.ones((S, S)))
        pose[0, 0, 9] = 1.0 * k / fx                                           # t_x = d k / fx
        r = mc.oracle_pseudo(flat, pose, albedo, normal, light, mask, K=K)
        assert np.abs(r["im"][0][:, :, k:] - want[:, :, :-k]).max() <= tol
        assert np.array_equal(r["mask"][0][:, k:], mask[0][:, :-k])
        assert (r["mask"][0][:, :k] == 0).all()
        if K is None:   # irrational fx: an integer coordinate may come out as -1 + 1e-16 and leave a tap of that weight
            assert np.abs(r["im"][0][:, :, :k]).max() <= tol
        else:
            assert np.array_equal(r["ix"][0], np.arange(S)[None] - k + np.zeros((S, 1)))
            assert (r["im"][0][:, :, :k] == 0).all()


def _renderer(S, dtype):
    """The package's Renderer on the CPU with every constant in `dtype` (its torch statements, not its kernels)."""
    from gan2shape_amd.renderer.renderer import Renderer
    r = Renderer({"rot_center_depth": mc.ROT_CENTER, "fov": sc.FOV}, S, mc.MIN_DEPTH, mc.MAX_DEPTH, device="cpu")
    K = torch.tensor(mc.intrinsics(S), dtype=dtype)[None]
    r.K, r.inv_K = K, torch.inverse(K.double()).to(dtype)
    r._centroid = r._centroid.to(dtype)
    r._rays[(S, S, "cpu")] = torch.tensor(mc.rays_of(S), dtype=dtype).view(1, S, S, 3)
    r._rays[("wh", S, S, "cpu")] = torch.tensor([S - 1, S - 1], dtype=dtype).view(1, 1, 1, 2)
    return r


def torch_path(c, warped, args, dtype=torch.float64):
    """Shade, Renderer.get_inv_warped_2d_grid, F.grid_sample (bilinear for the image, nearest for the mask): the
    composition render_given_view(grid_sample=True) runs after the relighting, on a GIVEN warped depth."""
    from gan2shape_amd.renderer.utils import get_transform_matrices
    S, B, V = c["S"], c["B"], c["V"]
    r = _renderer(S, dtype)
    r.rot_mat, r.trans_xyz = get_transform_matrices(torch.tensor(c["views"], dtype=dtype).reshape(B * V, 6))
    d = torch.tensor(warped, dtype=dtype).clamp(mc.DEPTH_LO, mc.DEPTH_HI)
    grid = r.get_inv_warped_2d_grid(d)
    albedo = torch.tensor(args["albedo"], dtype=dtype).repeat_interleave(V, 0)
    if args["light"] is not None:
        light = torch.tensor(args["light"], dtype=dtype)
        normal = torch.tensor(args["normal"], dtype=dtype).repeat_interleave(V, 0)
        la, lb = light[:, :1] / 2 + 0.5, light[:, 1:2] / 2 + 0.5
        ld = torch.cat([light[:, 2:], torch.ones(B * V, 1, dtype=dtype)], 1)
        ld = ld / ((ld ** 2).sum(1, keepdim=True)) ** 0.5
        diffuse = (normal * ld.view(-1, 1, 1, 3)).sum(3).clamp(min=0).unsqueeze(1)
        albedo = (albedo / 2 + 0.5) * (la.view(-1, 1, 1, 1) + lb.view(-1, 1, 1, 1) * diffuse) * 2 - 1
    im = F.grid_sample(albedo, grid, mode="bilinear", align_corners=True).clamp(-1, 1)
    m = torch.ones(B, S, S, dtype=dtype) if args["mask"] is None else torch.tensor(args["mask"], dtype=dtype)
    m = F.grid_sample(m.repeat_interleave(V, 0).unsqueeze(1), grid, mode="nearest", align_corners=True)
    return im.numpy(), m[:, 0].numpy()


@pytest.mark.parametrize("name", list(mc.CASES))
def test_oracle_matches_the_torch_path_in_float64(name, warped):
    c = mc.CASES[name]
    # the pose of the float32 views in float64, unrounded: both routes then compute the same map
    pose = np.stack([np.stack([mc.view_pose(v.astype(np.float64)) for v in vb]) for vb in c["views"]])
    for C, lit, masked, _ in mc.RUNS:
        a = mc.run_args(c, C, lit, masked)
        r = mc.oracle_pseudo(warped[name], pose, **a)
        im, m = torch_path(c, warped[name], a)
        sure = ~mc.ambiguous(r["ix"], r["iy"])
        assert np.abs(r["im"] - im).max() <= 1e-9, (name, C, lit)
        assert np.array_equal(r["mask"][sure], m[sure]), (name, C, masked)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_cases_are_what_they_claim(name, warped):
    c = mc.CASES[name]
    r = mc.oracle_pseudo(warped[name], c["pose"], c["albedo"][1])
    assert mc.ambiguous(r["ix"], r["iy"]).mean() <= mc.HALF_SHARE
    if c["B"] * c["V"] > 1:                                  # frames with samples outside the canonical image
        S = c["S"]
        outside = (r["ix"] < 0) | (r["ix"] > S - 1) | (r["iy"] < 0) | (r["iy"] > S - 1)
        assert outside.any() and not outside.all()
        assert abs(c["views"][..., 1]).max() >= math.pi / 3 - 1e-6


def test_oracle_matches_the_reference_run(capi, golden):
    """steps.npz: the reference's own sample_pseudo_imgs run.  The caps are test_step2_vs_reference_run's."""
    g = golden("steps")
    S = g["s1.depth"].shape[-1]
    n = g["s2.draw.views"].shape[0]
    alpha = -0.6                                             # rand_light[6], the model's default
    light = mc.relit_rows(g["s1.light_a"], g["s1.light_b"], g["s2.draw.dxy"], g["s2.draw.rand"], alpha)
    views = mc.view_transformation(g["s2.draw.views"])
    pose = np.stack([mc.view_pose(v) for v in views])[None].astype(np.float32)
    posed = mc.posed_verts(mc.canonical_verts(g["s1.depth"], S), pose)
    w = capi.render_depth(posed, sc.grid_faces(S), S, mc.intrinsics(S), near=mc.RASTER_NEAR, far=mc.RASTER_FAR)["depth"]
    r = mc.oracle_pseudo(w, pose, g["s1.albedo"], g["s1.normal"], light)
    assert r["im"].shape == (n, 3, S, S)
    off = (np.abs(r["im"] - g["s2.pseudo_im"]) > 2e-3).mean()
    flips = (r["mask"] != g["s2.pseudo_mask"][:, 0]).mean()
    print(f"oracle against the reference run: {off:.2e} of the pixels off by more than 2e-3, {flips:.2e} mask flips")
    assert off < 5e-3
    assert flips < 2e-3


# ------------------------------------------------------------------------------------------------------- host logic
def test_pseudo_pose_matches_the_chain():
    from gan2shape_amd.renderer.renderer import Renderer
    r = Renderer({"rot_center_depth": mc.ROT_CENTER}, 8, mc.MIN_DEPTH, mc.MAX_DEPTH, device="cpu")
    c = mc.CASES["S8_B2V5"]
    got = r.pseudo_pose(torch.tensor(c["views"]), None, 2).numpy()
    assert got.shape == (2, 5, 12) and np.abs(got - c["pose"]).max() <= 5e-7
    shared = r.pseudo_pose(torch.tensor(c["views"][0]), None, 2).numpy()       # (V, 6): the same views for every image
    assert np.array_equal(shared[0], got[0]) and np.array_equal(shared[1], got[0])
    base = np.array([[0.1, -0.3, 0.05, 0.02, -0.01, 0.03], [-0.2, 0.2, 0.0, 0.0, 0.01, -0.02]], np.float32)
    got = r.pseudo_pose(torch.tensor(c["views"]), torch.tensor(base), 2).numpy()
    want = np.stack([np.stack([mc.view_pose(c["views"][b, v].astype(np.float64), base[b].astype(np.float64))
                               for v in range(5)]) for b in range(2)])
    assert np.abs(got - want).max() <= 5e-7              # a few float32 roundings of values up to 1.1


def test_rotation_views_and_light_sweep():
    from gan2shape_amd.model import light_sweep, rotation_views
    v = rotation_views(40, 5, pitch_deg=10)
    assert v.shape == (5, 6) and v.dtype == torch.float32
    np.testing.assert_allclose(v[:, 1].numpy(), np.deg2rad([-40, -20, 0, 20, 40]), atol=1e-7)
    np.testing.assert_allclose(v[:, 0].numpy(), np.deg2rad(10), atol=1e-7)
    assert (v[:, 2:] == 0).all()
    assert rotation_views(60, 1).shape == (1, 6)
    s = light_sweep(-0.2, 0.3, 4, 0.5)
    assert s.shape == (4, 4) and s.dtype == torch.float32
    np.testing.assert_allclose(s.numpy(), [[-0.2, 0.3, 0.5, 0], [-0.2, 0.3, 0, 0.5], [-0.2, 0.3, -0.5, 0],
                                           [-0.2, 0.3, 0, -0.5]], atol=1e-7)


def test_chunk_arithmetic():
    from gan2shape_amd.renderer.renderer import sweep_chunks
    assert sweep_chunks(2, 5, None, 1 << 20) == (2, 5)                         # everything fits
    assert sweep_chunks(2, 5, 3, 1) == (2, 1)
    assert sweep_chunks(2, 5, 4, 1) == (2, 2)
    assert sweep_chunks(4, 5, 3, 1) == (3, 1)
    assert sweep_chunks(1, 120, 7, 1) == (1, 7)
    assert sweep_chunks(1, 120, None, 64 << 20) == (1, 4)                      # the 256 MiB budget
    for b, V, m in ((2, 5, 3), (4, 5, 3), (1, 7, 2), (3, 4, 100)):             # the chunks tile b x V exactly once
        bc, vc = sweep_chunks(b, V, m, 1)
        seen = np.zeros((b, V), int)
        for b0 in range(0, b, bc):
            for v0 in range(0, V, vc):
                seen[b0:b0 + bc, v0:v0 + vc] += 1
                assert min(bc, b - b0) * min(vc, V - v0) <= m
        assert (seen == 1).all()
    with pytest.raises(ValueError):
        sweep_chunks(1, 1, 0, 1)


def test_bad_shapes_raise_before_any_launch(monkeypatch):
    from gan2shape_amd import lib
    from gan2shape_amd.plugins import neural_renderer as nr
    from gan2shape_amd.renderer.renderer import Renderer
    monkeypatch.setattr(lib, "load", lambda: pytest.fail("a launch was attempted"))
    S = 8
    good = dict(verts=(2, 64, 3), pose=(2, 5, 12), rays=(64, 3), albedo=(2, 3, S, S), normal=(2, S, S, 3),
                light=(10, 4), mask=(2, S, S), S=S)
    assert nr.check_pseudo_shapes(**good) == (2, 5)
    assert nr.check_pseudo_shapes(**dict(good, normal=None, light=None, mask=None)) == (2, 5)
    for bad in (dict(albedo=(2, 5, S, S)), dict(albedo=(2, 3, S, S + 1)), dict(normal=None), dict(light=None),
                dict(light=(10, 5)), dict(light=(9, 4)), dict(pose=(2, 5, 11)), dict(pose=(1, 5, 12)),
                dict(mask=(2, 1, S, S)), dict(rays=(63, 3)), dict(verts=(2, 63, 3)), dict(normal=(2, S, S))):
        with pytest.raises(ValueError):
            nr.check_pseudo_shapes(**dict(good, **bad))
    # pseudo_frames itself: the shape checks come first, before the device check and long before the first launch
    t = {k: torch.zeros(v) for k, v in good.items() if k != "S"}
    tail = (0.8, 1.2, S, S, True, True)

    def frames(**over):
        a = dict(t, **over)
        return nr.pseudo_frames(a["verts"], a["pose"], a["rays"], (1.0,) * 9, a["albedo"], a["normal"], a["light"],
                                a["mask"], *tail)
    for bad in (dict(albedo=torch.zeros(2, 5, S, S)), dict(light=torch.zeros(9, 4)), dict(normal=None),
                dict(mask=torch.zeros(2, 1, S, S)), dict(pose=torch.zeros(2, 5, 11))):
        with pytest.raises(ValueError):
            frames(**bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # good shapes, CPU tensors: still no launch
        frames()
    r = Renderer({}, S, 0.9, 1.1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # GPU only, like render_sweep
        r.render_pseudo_sweep(torch.zeros(1, 3, S, S), torch.zeros(1, S, S, 3), torch.ones(1, S, S), torch.zeros(2, 6))


def test_symbol_is_declared():
    from gan2shape_amd import lib
    assert len(lib.SIGNATURES["g2s_sweep_pseudo"][1]) == 17
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "g2s.h")) as f:
        assert "int g2s_sweep_pseudo(" in f.read()


class StubModel:
    """Records what the command asks of `manipulate` and answers with frames of the right shapes."""

    def __init__(self, S=16, style_dim=12):
        self.device = torch.device("cpu")
        self.S, self.style_dim, self.calls = S, style_dim, []

    def manipulate(self, image, latent, views, lights=None, relative=False, gan_batch=8):
        self.calls.append(dict(image=image, latent=latent, views=views, lights=lights, relative=relative,
                               gan_batch=gan_batch))
        V = len(views)
        ramp = torch.linspace(-1, 1, V).view(V, 1, 1, 1).expand(V, 3, self.S, self.S)
        return dict(pseudo=ramp, gan=-ramp, mask=torch.ones(V, 1, self.S, self.S),
                    w=latent.reshape(1, -1) + torch.arange(V).view(V, 1), view=torch.zeros(1, 6),
                    light=torch.tensor([[-0.25, 0.5, 0.1, 0.2]]))


def test_command_with_a_recording_stub(tmp_path):
    from PIL import Image
    from gan2shape_amd import manipulate as mp
    from gan2shape_amd.model import light_sweep, rotation_views
    from test_sweep_cpu import tiny_dataset
    cfg, _ = tiny_dataset(tmp_path)
    (tmp_path / "data" / "face" / "latents").mkdir()
    for i, stem in enumerate("ab"):
        torch.save(torch.full((1, 12), float(i)), tmp_path / "data" / "face" / "latents" / (stem + ".pt"))
    model = StubModel()
    out = tmp_path / "manip"
    written = mp.main(["--config", str(cfg), "--out", str(out), "--device", "cpu", "--frames", "4", "--yaw", "30",
                       "--relight", "--relative", "--gan-batch", "3"], model=model)
    assert written == [str(out / "a"), str(out / "b")]
    for i, stem in enumerate("ab"):
        assert sorted(os.listdir(out / stem)) == ["gan_relight.gif", "gan_rotate.gif", "latents.pt",
                                                  "pseudo_relight.gif", "pseudo_rotate.gif"]
        for name in ("gan_rotate", "pseudo_rotate", "gan_relight", "pseudo_relight"):
            with Image.open(out / stem / (name + ".gif")) as gif:
                assert gif.n_frames == 4 and gif.size == (16, 16)
        w = torch.load(out / stem / "latents.pt", weights_only=True)
        assert w.shape == (4, 12) and torch.equal(w[:, 0], i + torch.arange(4.0))
    assert len(model.calls) == 4
    for k, c in enumerate(model.calls):
        assert c["image"].shape == (1, 3, 16, 16) and c["latent"].shape == (12,)
        assert c["relative"] is True and c["gan_batch"] == 3
        if k % 2 == 0:
            assert torch.equal(c["views"], rotation_views(30, 4)) and c["lights"] is None
        else:                                                # the relighting: fixed pose, predicted a and b
            assert torch.equal(c["views"], torch.zeros(4, 6))
            assert torch.equal(c["lights"], light_sweep(-0.25, 0.5, 4, 0.5))
    only = mp.main(["--config", str(cfg), "--out", str(tmp_path / "one"), "--device", "cpu", "--frames", "2",
                    "--images", "1"], model=StubModel())
    assert only == [str(tmp_path / "one" / "b")]
    assert sorted(os.listdir(tmp_path / "one" / "b")) == ["gan_rotate.gif", "latents.pt", "pseudo_rotate.gif"]
    with pytest.raises(ValueError):
        mp.main(["--config", str(cfg), "--out", str(out), "--device", "cpu"])  # no model and no --ckpt
