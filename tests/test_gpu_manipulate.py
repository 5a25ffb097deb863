"""-m gpu: the pseudo-view pass (csrc/sweep.hip: g2s_sweep_pseudo) against the float64 oracle of manipulate_cases.py,
Renderer.render_pseudo_sweep against the existing composition and the reference's run, GAN2Shape.manipulate end to
end against the reference's step 2, and the manipulate command.

Image tolerance of the kernel: per case and run e = max |got - want| against the oracle on the GPU rasterizer's own
`warped`; the bound is 1.5 x the e that the existing float32 composition (g2s_shading_fwd, g2s_inv_warp_grid_fwd,
grid_sample on the same `warped`) shows against the same oracle IN THAT RUN, as test_gpu_golden.py applies the margin.
Both are printed before they are asserted.  The nearest mask is compared outside the pixels manipulate_cases.ambiguous marks.
"""
import os

import numpy as np
import pytest
import torch

import manipulate_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    return lib


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def gpu_warped(g2s, c):
    """g2s_sweep_verts + g2s_raster_depth_fwd of a case, as render_depth calls the rasterizer."""
    L = g2s.load()
    S, B, V = c["S"], c["B"], c["V"]
    N, F = S * S, 2 * (S - 1) * (S - 1)
    verts, pose = _dev(mc.canonical_verts(c["depth"], S)), _dev(c["pose"])
    posed = torch.empty(B * V, N, 3, device="cuda")
    g2s.check(L.g2s_sweep_verts(g2s.ptr(verts), g2s.ptr(pose), g2s.ptr(posed), B, V, N, g2s.stream()))
    warped = torch.empty(B * V, S, S, device="cuda")
    ws = torch.empty(L.g2s_raster_workspace_bytes(B * V, N, F, S), dtype=torch.uint8, device="cuda")
    K = (g2s.C.c_float * 9)(*mc.intrinsics(S).reshape(9))
    g2s.check(L.g2s_raster_depth_fwd(g2s.ptr(posed), None, B * V, N, F, S, K, float(S), 2, 1, mc.RASTER_NEAR,
                                     mc.RASTER_FAR, g2s.ptr(warped), None, None, g2s.ptr(ws), ws.numel(), g2s.stream()))
    return warped


def kernel(g2s, c, warped, albedo, normal=None, light=None, mask=None, want_mask=True, pose=None, out=None, C=None):
    """One g2s_sweep_pseudo call on device tensors -> (return code, im, mask_out)."""
    L = g2s.load()
    S = c["S"]
    pose = _dev(c["pose"]) if pose is None else pose
    B, V = pose.shape[:2]
    C = albedo.shape[1] if C is None else C
    im, mout = out if out is not None else (torch.empty(B * V, albedo.shape[1], S, S, device="cuda"),
                                            torch.empty(B * V, S, S, device="cuda") if want_mask else None)
    K = (g2s.C.c_float * 9)(*mc.intrinsics(S).reshape(9))
    rays = _dev(mc.rays_of(S))
    rc = L.g2s_sweep_pseudo(g2s.ptr(warped), g2s.ptr(rays), g2s.ptr(pose), K, g2s.ptr(albedo), g2s.ptr(normal),
                            g2s.ptr(light), g2s.ptr(mask), mc.DEPTH_LO, mc.DEPTH_HI, B, V, S, C, g2s.ptr(im),
                            g2s.ptr(mout), g2s.stream())
    return rc, im, mout


def composed(c, warped, a):
    """The existing float32 composition on the same warped depth: fused shading, inverse-warp grid, grid_sample."""
    from gan2shape_amd import fused_geometry as fg
    from gan2shape_amd.op import grid_sample
    S, B, V = c["S"], c["B"], c["V"]
    R, t = fg.view_transform(_dev(c["views"]).reshape(B * V, 6))
    d = warped.clamp(mc.DEPTH_LO, mc.DEPTH_HI)
    grid = fg.inv_warp_grid(d, _dev(mc.rays_of(S)), R, t, tuple(float(v) for v in mc.intrinsics(S).reshape(9)), mc.ROT_CENTER)
    tex = _dev(a["albedo"]).repeat_interleave(V, 0)
    if a["light"] is not None:
        # g2s_shading_fwd is a 3-channel kernel and every channel goes through the same arithmetic: a 1-channel
        # albedo is shaded as three copies of itself, of which one is kept
        C = tex.shape[1]
        _, tex = fg.shading(_dev(a["normal"]).repeat_interleave(V, 0), _dev(a["light"]),
                            tex if C == 3 else tex.expand(-1, 3, -1, -1).contiguous())
        tex = tex[:, :C]
    return grid_sample(tex.contiguous(), grid, -1, 1)


@pytest.fixture(scope="module")
def results(g2s):
    """Everything once: per case and run the kernel's outputs, the oracle's and the composition's error."""
    out = {}
    for name, c in mc.CASES.items():
        warped = gpu_warped(g2s, c)
        wh = warped.cpu().numpy()
        res = []
        for C, lit, masked, want_mask in mc.RUNS:
            a = mc.run_args(c, C, lit, masked)
            want = mc.oracle_pseudo(wh, c["pose"], **a)
            e32 = float(np.abs(composed(c, warped, a).cpu().numpy() - want["im"]).max())
            rc, im, mout = kernel(g2s, c, warped, _dev(a["albedo"]), _dev(a["normal"]), _dev(a["light"]),
                                  _dev(a["mask"]), want_mask)
            assert rc == 0, g2s.load().g2s_last_error()
            res.append(((C, lit, masked), im.cpu().numpy(), None if mout is None else mout.cpu().numpy(), want, e32))
        out[name] = res
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(mc.CASES))
def test_kernel_matches_the_float64_oracle(name, results):
    out = results
    for key, im, mout, want, e32 in out[name]:
        print(f"{name} {key}: g2s_sweep_pseudo e = {np.abs(im - want['im']).max():.3g}, composition e = {e32:.3g} "
              f"(bound {1.5 * e32:.3g})")
    for key, im, mout, want, e32 in out[name]:
        assert np.isfinite(im).all()
        assert np.abs(im - want["im"]).max() <= 1.5 * e32, key
        if mout is not None:
            unsure = mc.ambiguous(want["ix"], want["iy"])
            assert unsure.mean() <= mc.HALF_SHARE
            assert np.array_equal(mout[~unsure], want["mask"][~unsure]), key


def test_chunks_determinism_and_rejected_calls(g2s):
    c = mc.CASES["S33_B2V5"]
    a = mc.run_args(c, 3, True, True)
    dev = {k: _dev(v) for k, v in a.items()}
    warped = gpu_warped(g2s, c)
    _, im, mout = kernel(g2s, c, warped, **dev)
    _, im2, mout2 = kernel(g2s, c, warped, **dev)
    assert torch.equal(im, im2) and torch.equal(mout, mout2)
    pose, light = _dev(c["pose"]), dev["light"].view(2, 5, 4)
    S, V = c["S"], c["V"]
    w5 = warped.view(2, V, S, S)
    for v0 in range(0, V, 2):                               # V in chunks of 2 (the last holds one frame)
        sv = slice(v0, v0 + 2)
        n = len(range(V)[sv])
        _, im_c, m_c = kernel(g2s, c, w5[:, sv].reshape(2 * n, S, S).contiguous(), dev["albedo"], dev["normal"],
                              light[:, sv].reshape(-1, 4).contiguous(), dev["mask"], pose=pose[:, sv].contiguous())
        assert torch.equal(im_c.view(2, n, 3, S, S), im.view(2, V, 3, S, S)[:, sv])
        assert torch.equal(m_c.view(2, n, S, S), mout.view(2, V, S, S)[:, sv])
    # rejected calls: a non-zero code, outputs untouched
    sentinel = (torch.full_like(im, 7.0), torch.full_like(mout, 7.0))
    rc, _, _ = kernel(g2s, c, warped, dev["albedo"], dev["normal"], dev["light"], dev["mask"], out=sentinel, C=5)
    assert rc != 0 and b"C = 5" in g2s.load().g2s_last_error()
    rc2, _, _ = kernel(g2s, c, warped, dev["albedo"], None, dev["light"], dev["mask"], out=sentinel)
    assert rc2 != 0
    rc3, _, _ = kernel(g2s, c, warped, dev["albedo"], dev["normal"], None, dev["mask"], out=sentinel)
    assert rc3 != 0
    torch.cuda.synchronize()
    assert bool((sentinel[0] == 7).all()) and bool((sentinel[1] == 7).all())


def test_pseudo_frames_checks_shapes_before_any_launch(g2s, monkeypatch):
    from gan2shape_amd.plugins import neural_renderer as nr
    c = mc.CASES["S8_B2V5"]
    S = c["S"]
    a = {k: _dev(v) for k, v in mc.run_args(c, 3, True, True).items()}
    verts, pose, rays = _dev(mc.canonical_verts(c["depth"], S)), _dev(c["pose"]), _dev(mc.rays_of(S))
    K = tuple(float(v) for v in mc.intrinsics(S).reshape(9))

    def frames(**over):
        b = dict(a, verts=verts, pose=pose, rays=rays)
        b.update(over)
        return nr.pseudo_frames(b["verts"], b["pose"], b["rays"], K, b["albedo"], b["normal"], b["light"], b["mask"],
                                mc.DEPTH_LO, mc.DEPTH_HI, S, S, True, True)
    im, mout = frames()                                     # the good call runs
    assert im.shape == (2, 5, 3, S, S) and mout.shape == (2, 5, S, S)
    monkeypatch.setattr(g2s, "load", lambda: pytest.fail("a launch was attempted"))
    for bad in (dict(albedo=a["albedo"][:, :1].expand(2, 5, S, S)), dict(light=a["light"][:9]), dict(normal=None),
                dict(mask=a["mask"][:, None]), dict(pose=pose[..., :11]), dict(rays=rays[:-1])):
        with pytest.raises(ValueError):
            frames(**bad)


# ------------------------------------------------------------------------------- the renderer, the model, the command
@pytest.fixture(scope="module")
def step_model(g2s, golden):
    from test_gpu_golden import build_step_model
    g = golden("steps")
    return build_step_model(g), g


def _s1(g):
    return tuple(_dev(g[f"s1.{k}"]) for k in ("normal", "light_a", "light_b", "albedo", "depth"))


def _lights(m, g):
    return _dev(mc.relit_rows(g["s1.light_a"], g["s1.light_b"], g["s2.draw.dxy"], g["s2.draw.rand"], m.rand_light[6]))


def test_render_pseudo_sweep_vs_the_existing_path_and_the_reference(step_model):
    m, g = step_model
    normal, la, lb, albedo, depth = _s1(g)
    draws = tuple(_dev(g[f"s2.draw.{k}"]) for k in ("dxy", "rand", "views"))
    n = draws[2].shape[0]
    with torch.no_grad():
        want_im, want_mask = m.sample_pseudo_imgs(n, normal, la, lb, albedo, depth, None, _draws=draws)
    views = m.get_view_transformation(draws[2])
    im, mask = m.renderer.render_pseudo_sweep(albedo, normal, depth, views, _lights(m, g))
    assert im.shape == (1, n, 3, 128, 128) and mask.shape == (1, n, 1, 128, 128)
    for tag, ref_im, ref_mask in (("sample_pseudo_imgs", want_im.cpu().numpy(), want_mask.cpu().numpy()),
                                  ("the reference run", g["s2.pseudo_im"], g["s2.pseudo_mask"])):
        off = (np.abs(im[0].cpu().numpy() - ref_im) > 2e-3).mean()
        flips = (mask[0].cpu().numpy() != ref_mask).mean()
        print(f"render_pseudo_sweep against {tag}: {off:.2e} of the pixels off by more than 2e-3, {flips:.2e} mask flips")
        assert off < 5e-3 and flips < 2e-3
    # the chunking does not show: three images x two views, at most 3 frames per chunk, against one call
    al3 = torch.cat([albedo, albedo.flip(2), albedo.flip(3)])
    n3, d3 = normal.expand(3, -1, -1, -1).contiguous(), depth.expand(3, -1, -1).contiguous()
    cm = (al3[:, 0] > 0).float()
    one = m.renderer.render_pseudo_sweep(al3, n3, d3, views, _lights(m, g), cm)
    for mf in (3, 1):
        part = m.renderer.render_pseudo_sweep(al3, n3, d3, views, _lights(m, g), cm, max_frames=mf)
        assert torch.equal(one[0], part[0]) and torch.equal(one[1], part[1])
    assert torch.equal(one[0][0], im[0])                    # the images of a batch do not see each other
    with pytest.raises(ValueError):
        m.renderer.render_pseudo_sweep(albedo, normal, depth, views[:, :5], _lights(m, g))
    with pytest.raises(ValueError):
        m.renderer.render_pseudo_sweep(albedo, normal, depth, views, _lights(m, g)[:1])


def test_manipulate_vs_reference_run(step_model):
    m, g = step_model
    image, latent = _dev(g["image"]), _dev(g["latent"])
    views = m.get_view_transformation(_dev(g["s2.draw.views"]))
    lights = _lights(m, g)
    d = m.decompose(image)
    _, c1 = m.forward_step1(image, latent, None)
    # the decomposition is forward_step1's, to the tolerances test_step1_vs_reference_run holds `collected` to (the
    # paired and the single forwards of the nets differ in rounding; normals amplify depth differences)
    for key, got, want in zip(("normal", "light_a", "light_b", "albedo", "depth"), d["collected"][:5], c1[:5]):
        tol = 1e-3 if key == "normal" else 2e-5
        assert float((got - want).detach().abs().max()) <= tol * float(want.detach().abs().max()), key
    out = m.manipulate(image, latent, views, lights)
    n = views.shape[0]
    assert out["gan"].shape == (n, 3, 128, 128) and out["w"].shape == (n, 512)
    assert out["pseudo"].shape == (n, 3, 128, 128) and out["mask"].shape == (n, 1, 128, 128)
    proj, ref = out["gan"].cpu().numpy(), g["s2.projected"]
    rel = np.linalg.norm(proj - ref) / np.linalg.norm(ref)
    flips = (out["mask"].cpu().numpy() != g["s2.mask"]).mean()
    print(f"manipulate against the reference's step 2: |d| / |ref| = {rel:.2e}, mask flips {flips:.2e}")
    assert rel <= 2e-3
    assert flips < 2e-3


def test_decompose_is_forward_step1_behind_the_nets(step_model):
    """With every net called on its own in both (paired_nets off) and reproducible launch partitions, decompose and
    forward_step1 run the same code on the same numbers: the same bits."""
    from gan2shape_amd import lib, zeropool
    m, g = step_model
    image, latent = _dev(g["image"]), _dev(g["latent"])
    paired, m.paired_nets = m.paired_nets, False
    prev = lib.set_deterministic(True)
    try:
        with torch.no_grad():
            d = m.decompose(image)
            _, c1 = m.forward_step1(image, latent, None)
            view = m.viewpoint_net(image) + m.view_light_sampler.view_mean.unsqueeze(0)
            light = m.lighting_net(image) + m.view_light_sampler.light_mean.unsqueeze(0)
        for key, got, want in zip(("normal", "light_a", "light_b", "albedo", "depth"), d["collected"][:5], c1[:5]):
            assert torch.equal(got, want), key
        assert torch.equal(d["view"], view) and torch.equal(d["light"], light)
    finally:
        lib.set_deterministic(prev)
        m.paired_nets = paired
        zeropool.end()


def test_manipulate_gan_batch_and_relative(step_model):
    m, g = step_model
    image, latent = _dev(g["image"]), _dev(g["latent"])
    from gan2shape_amd.model import rotation_views
    views = rotation_views(40, 5).cuda()
    from gan2shape_amd import lib
    prev = lib.set_deterministic(True)                      # the nets of the decomposition: the same bits in both calls
    try:
        a = m.manipulate(image, latent, views, gan_batch=8)
        b = m.manipulate(image, latent, views, gan_batch=3)
    finally:
        lib.set_deterministic(prev)
    assert torch.equal(a["pseudo"], b["pseudo"])
    assert torch.equal(a["w"], b["w"])                      # the encoder sees all frames at once either way
    # batched against split generator forwards: tests/test_gpu_synth_batch.py's bound, 2e-6 of the largest value of
    # the generator's output (there the raw images; here `invert` clamps them to [-1, 1] afterwards, which cannot
    # increase a difference, so the scale is taken from the raw images of the same latents)
    with torch.no_grad():
        raw, _ = m.generator([a["w"]], input_is_w=True, truncation_latent=m.mean_latent, truncation=m.truncation,
                             randomize_noise=False)
    top = float(raw.abs().max())
    e = float((a["gan"] - b["gan"]).abs().max())
    print(f"gan_batch 3 against 8: max |d| = {e:.3g}, largest raw value {top:.3g}, bound {2e-6 * top:.3g}")
    assert e <= 2e-6 * top
    # relative, zero rotation, predicted light: the step-1 reconstruction's warp of the canonical image
    r = m.manipulate(image, latent, torch.zeros(1, 6), relative=True)
    d = m.decompose(image)
    normal, la, lb, albedo, depth, _ = d["collected"]
    _, _, _, texture = m._shade(normal, d["light"], albedo)
    with torch.no_grad():
        want, wmask = m.renderer.render_given_view(texture, depth, m.get_view_transformation(d["view"]),
                                                   mask=torch.ones_like(texture))
    off = ((r["pseudo"] - want.clamp(-1, 1)).abs() > 2e-3).float().mean().item()
    flips = (r["mask"] != wmask[:, :1]).float().mean().item()
    print(f"relative zero pose against render_given_view: {off:.2e} pixels off by more than 2e-3, {flips:.2e} flips")
    assert off < 5e-3 and flips < 2e-3


def test_command_on_the_gpu(step_model, tmp_path):
    from PIL import Image
    from gan2shape_amd import manipulate as mp
    from test_sweep_cpu import tiny_dataset
    m, g = step_model
    cfg, _ = tiny_dataset(tmp_path, size=128)
    (tmp_path / "data" / "face" / "latents").mkdir()
    for stem in "ab":
        torch.save(torch.from_numpy(g["latent"]), tmp_path / "data" / "face" / "latents" / (stem + ".pt"))
    out = tmp_path / "manip"
    written = mp.main(["--config", str(cfg), "--out", str(out), "--frames", "4", "--relight"], model=m)
    assert written == [str(out / "a"), str(out / "b")]
    for stem in "ab":
        for name in ("gan_rotate", "pseudo_rotate", "gan_relight", "pseudo_relight"):
            with Image.open(out / stem / (name + ".gif")) as gif:
                assert gif.n_frames == 4 and gif.size == (128, 128)
        assert torch.load(out / stem / "latents.pt", weights_only=True).shape == (4, 512)
