"""-m gpu: the viewing path (csrc/sweep.hip) against the float64 oracle of sweep_cases.py.

Per case: g2s_sweep_verts against the oracle, g2s_raster_depth_fwd on its output, the oracle shade on THOSE face_idx /
bary (copied to the host), g2s_sweep_shade against it.  Alpha must be equal.  Colours and posed vertices: e = |got -
want| / (1 + |want|) <= 4 x the largest e the float32 torch statements show on the CPU against the oracle over all
cases (sweep_cases.py).  The figures are printed before they are asserted.  Then Renderer.render_sweep end to end,
the argument checks and the visualize command.
"""
import os

import numpy as np
import pytest
import torch

import sweep_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    return lib


def _dev(x, dtype=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _kernel_verts(g2s, c):
    L = g2s.load()
    verts, pose = _dev(c["verts"]), _dev(c["pose"])
    B, N, V = c["B"], verts.shape[1], c["V"]
    posed = torch.empty(B * V, N, 3, device="cuda")
    g2s.check(L.g2s_sweep_verts(g2s.ptr(verts), g2s.ptr(pose), g2s.ptr(posed), B, V, N, g2s.stream()))
    return posed


def _kernel_raster(g2s, c, posed):
    L = g2s.load()
    S, ssaa, BV, N = c["S"], c["ssaa"], posed.shape[0], posed.shape[1]
    faces = _dev(c["faces"])
    F = sc.faces_of(c).shape[0]
    depth = torch.empty(BV, S, S, device="cuda")
    fidx = torch.empty(BV, S * ssaa, S * ssaa, dtype=torch.int32, device="cuda")
    bary = torch.empty(BV, S * ssaa, S * ssaa, 3, device="cuda")
    ws = torch.empty(L.g2s_raster_workspace_bytes(BV, N, F, S), dtype=torch.uint8, device="cuda")
    K = (g2s.C.c_float * 9)(*sc.intrinsics(S).reshape(9))
    g2s.check(L.g2s_raster_depth_fwd(g2s.ptr(posed), g2s.ptr(faces), BV, N, F, S, K, float(S), ssaa, 1, sc.NEAR, sc.FAR,
                                     g2s.ptr(depth), g2s.ptr(fidx), g2s.ptr(bary), g2s.ptr(ws), ws.numel(), g2s.stream()))
    return depth, fidx, bary


def _kernel_shade(g2s, c, mode, C, posed, fidx, bary, want_alpha=True):
    L = g2s.load()
    m = sc.MODES[mode]
    S, BV, N = c["S"], posed.shape[0], posed.shape[1]
    faces = _dev(c["faces"])
    attr = _dev(c["attr"][C]) if m in (0, 1) else None
    normal = _dev(c["normal"]) if m else None
    pose = _dev(c["pose"])
    light = _dev(c["light"]) if m in (1, 2) else None
    Cout = C if m in (0, 1) else 3
    rgb = torch.empty(BV, Cout, S, S, device="cuda")
    alpha = torch.empty(BV, S, S, device="cuda") if want_alpha else None
    bg = (g2s.C.c_float * 4)(*c["background"])
    g2s.check(L.g2s_sweep_shade(g2s.ptr(posed), g2s.ptr(faces), g2s.ptr(fidx), g2s.ptr(bary), g2s.ptr(attr),
                                g2s.ptr(normal), g2s.ptr(pose), g2s.ptr(light), c["B"], c["V"], N,
                                sc.faces_of(c).shape[0], S, c["ssaa"], C, 1, m, bg, c["grey"], g2s.ptr(rgb),
                                g2s.ptr(alpha), g2s.stream()))
    return rgb, alpha


@pytest.fixture(scope="module")
def results(g2s):
    """Everything once: per case the kernel's outputs, the oracle's and the float32 torch statement's on the kernel
    rasterizer's maps; the two bounds."""
    out, worst_c, worst_v = {}, 0.0, 0.0
    for name, c in sc.CASES.items():
        posed = _kernel_verts(g2s, c)
        _, fidx, bary = _kernel_raster(g2s, c, posed)
        posed_h, fidx_h, bary_h = posed.cpu().numpy(), fidx.cpu().numpy(), bary.cpu().numpy()
        want_v = sc.oracle_verts(c["verts"], c["pose"])
        worst_v = max(worst_v, sc.error(sc.verts_torch_f32(c["verts"], c["pose"]), want_v))
        res = {}
        for mode, C in sc.runs(name):
            a = sc.shade_args(c, mode, C, posed_h, fidx_h, bary_h)
            rgb64, alpha64 = sc.oracle_shade(**a)
            rgb32, _ = sc.torch_shade_f32(a)
            worst_c = max(worst_c, sc.error(rgb32, rgb64))
            rgb, alpha = _kernel_shade(g2s, c, mode, C, posed, fidx, bary)
            res[(mode, C)] = (rgb.cpu().numpy(), alpha.cpu().numpy(), rgb64, alpha64)
        out[name] = (posed_h, want_v, fidx_h, res)
    print(f"float32 torch on the CPU against the oracle: colour e = {worst_c:.3g}, vertices e = {worst_v:.3g}")
    return out, 4 * worst_c, 4 * worst_v


@pytest.mark.parametrize("name", list(sc.CASES))
def test_kernels_match_the_float64_oracle(name, results):
    out, bound_c, bound_v = results
    posed, want_v, fidx, res = out[name]
    c = sc.CASES[name]
    ev = sc.error(posed, want_v)
    print(f"{name}: g2s_sweep_verts e = {ev:.3g} (bound {bound_v:.3g})")
    for key, (rgb, alpha, rgb64, alpha64) in res.items():
        print(f"{name} {key}: g2s_sweep_shade e = {sc.error(rgb, rgb64):.3g} (bound {bound_c:.3g})")
    assert ev <= bound_v
    for key, (rgb, alpha, rgb64, alpha64) in res.items():
        assert rgb.shape == rgb64.shape
        np.testing.assert_array_equal(alpha, alpha64)
        assert sc.error(rgb, rgb64) <= bound_c, key
    if name == "8x8_identity":
        assert np.array_equal(posed[0], c["verts"][0])                       # the unposed mesh, bit for bit
    if name == "out_of_view":
        for key, (rgb, alpha, _, _) in res.items():
            assert (alpha[1] == 0).all() and (alpha[0] > 0).any()
            assert (rgb[1] == np.array(c["background"][:rgb.shape[1]], np.float32)[:, None, None]).all()
    if name == "17x17_poses":
        F = sc.faces_of(c).shape[0]
        assert (fidx >= F).any() and (fidx < 0).any()                        # reversed winners and background
    if name == "light_lb0":
        rgb, alpha = res[("shape", 3)][:2]
        assert np.allclose(rgb[:, 0][alpha == 1], c["grey"] * 0.45 * 2 - 1, atol=2e-7)
    if name == "light_away":
        rgb, alpha = res[("shape", 3)][:2]
        assert np.allclose(rgb[:, 0][alpha == 1], c["grey"] * 0.3 * 2 - 1, atol=2e-7)


def _renderer(S):
    from gan2shape_amd.renderer.renderer import Renderer
    return Renderer({"rot_center_depth": sc.ROT_CENTER, "fov": sc.FOV}, S, 0.9, 1.1, device="cuda")


def test_render_sweep_end_to_end(g2s, results):
    c = sc.CASES["17x17_poses"]
    r = _renderer(17)
    im, depth = _dev(c["attr"][3]), _dev(c["depth"])
    rot, vb, va = _dev(c["rotations"]), _dev(c["v_before"]).float(), _dev(c["v_after"]).float()
    light = _dev(c["light"]).view(2, 7, 5)
    bg = c["background"]
    # step by step with the renderer's own vertices, pose and normals
    verts = r.depth_to_3d_grid(depth).reshape(2, -1, 3).contiguous()
    pose = r.sweep_pose(rot, vb, va, 2)
    assert float((pose - _dev(c["pose"])).abs().max()) < 1e-6
    normal = r.get_normal_from_depth(depth)
    cc = dict(c, verts=verts.cpu().numpy(), pose=pose.cpu().numpy(), normal=normal.cpu().numpy())
    posed = _kernel_verts(g2s, cc)
    dmap, fidx, bary = _kernel_raster(g2s, cc, posed)
    for mode in sc.MODES:
        want, want_a = _kernel_shade(g2s, cc, mode, 3, posed, fidx, bary)
        kw = dict(v_before=vb, v_after=va, mode=mode, light=light, background=bg)
        got, alpha, d = r.render_sweep(im, depth, rot, return_alpha=True, return_depth=True, **kw)
        assert got.shape == (2, 7, 3, 17, 17) and alpha.shape == d.shape == (2, 7, 17, 17)
        assert torch.equal(got.view(14, 3, 17, 17), want) and torch.equal(alpha.view(14, 17, 17), want_a)
        assert torch.equal(d.view(14, 17, 17), dmap)
        again = r.render_sweep(im, depth, rot, **kw)
        assert torch.equal(again, got)                                        # two runs
        for mf in (1, 3, 5):
            one, a1 = r.render_sweep(im, depth, rot, max_frames=mf, return_alpha=True, **kw)
            assert torch.equal(one, got) and torch.equal(a1, alpha), (mode, mf)
    # non-contiguous image and depth
    wide = torch.zeros(2, 3, 17, 34, device="cuda")
    wide[..., ::2] = im
    tall = torch.zeros(2, 34, 17, device="cuda")
    tall[:, ::2] = depth
    assert not wide[..., ::2].is_contiguous() and not tall[:, ::2].is_contiguous()
    kw = dict(v_before=vb, v_after=va, mode="shaded", light=light, background=bg)
    assert torch.equal(r.render_sweep(wide[..., ::2], tall[:, ::2], rot, **kw), r.render_sweep(im, depth, rot, **kw))
    # (V, 3) rotations and (V, 5) lights are shared by the batch
    a = r.render_sweep(im, depth, rot[0], mode="shape", light=light[0])
    b = r.render_sweep(im, depth, rot[:1].expand(2, -1, -1), mode="shape", light=light[:1].expand(2, -1, -1))
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        r.render_sweep(im, depth, rot, mode="shaded")                         # no light
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.render_sweep(im.cpu(), depth.cpu(), rot.cpu())


def test_frontal_view_reproduces_the_image_and_covers_the_mesh():
    r = _renderer(17)
    c = sc.CASES["17x17_poses"]
    im, depth = _dev(c["attr"][3])[:1], _dev(c["depth"])[:1]
    rgb, alpha = r.render_sweep(im, depth, torch.zeros(1, 3), return_alpha=True)
    # the mesh ends half a pixel inside the image on the right and at the bottom (vertex j sits at pixel coordinate j,
    # sample centres at k/2 + 1/4): all four samples of a pixel are covered exactly for rows and columns < 16
    a = alpha[0, 0]
    assert (a[:16, :16] == 1).all() and (a[16, :] < 1).all() and (a[:, 16] < 1).all()


def test_rejected_arguments_leave_the_outputs_untouched(g2s, results):
    L = g2s.load()
    c = sc.CASES["8x8_identity"]
    posed = _kernel_verts(g2s, c)
    _, fidx, bary = _kernel_raster(g2s, c, posed)
    attr, normal, pose, light = _dev(c["attr"][3]), _dev(c["normal"]), _dev(c["pose"]), _dev(c["light"])
    SENTINEL = -7.5
    rgb = torch.full((1, 4, 8, 8), SENTINEL, device="cuda")
    alpha = torch.full((1, 8, 8), SENTINEL, device="cuda")
    bg = (g2s.C.c_float * 4)(1, 1, 1, 1)
    ptr = g2s.ptr

    def call(attr_=attr, N=64, F=98, C=3, mode=0, normal_=normal, light_=light, fidx_=fidx, ssaa=2, rgb_=rgb):
        return L.g2s_sweep_shade(ptr(posed), None, ptr(fidx_), ptr(bary), ptr(attr_), ptr(normal_), ptr(pose), ptr(light_),
                                 1, 1, N, F, 8, ssaa, C, 1, mode, bg, 0.7, ptr(rgb_), ptr(alpha), g2s.stream())
    for kw in ({"N": 63}, {"F": 97}, {"C": 5}, {"C": 0}, {"mode": 4}, {"mode": -1}, {"attr_": None},
               {"attr_": None, "mode": 1}, {"normal_": None, "mode": 3}, {"light_": None, "mode": 2}, {"fidx_": None},
               {"ssaa": 3}, {"rgb_": None}):
        rc = call(**kw)
        assert rc == -1, (kw, rc)
        with pytest.raises(g2s.G2SError):
            g2s.check(rc)
    out = torch.full((1, 64, 3), SENTINEL, device="cuda")
    for args in ((None, ptr(pose), ptr(out), 1, 1, 64), (ptr(posed), None, ptr(out), 1, 1, 64),
                 (ptr(posed), ptr(pose), None, 1, 1, 64), (ptr(posed), ptr(pose), ptr(out), 0, 1, 64),
                 (ptr(posed), ptr(pose), ptr(out), 1, 0, 64), (ptr(posed), ptr(pose), ptr(out), 1, 1, 0),
                 (ptr(posed), ptr(pose), ptr(out), 65536, 1, 64)):
        assert L.g2s_sweep_verts(*args, g2s.stream()) == -1
    torch.cuda.synchronize()
    assert bool((rgb == SENTINEL).all()) and bool((alpha == SENTINEL).all()) and bool((out == SENTINEL).all())
    # a valid call afterwards: NULL attr is fine in mode 2, NULL alpha anywhere
    assert call(attr_=None, mode=2) == 0
    torch.cuda.synchronize()
    want = results[0]["8x8_identity"][3][("shape", 3)][0]
    assert np.array_equal(rgb[:, :3].reshape(-1)[:192].cpu().numpy().reshape(1, 3, 8, 8), want)


def test_command_from_a_depth_directory(tmp_path):
    from PIL import Image
    from gan2shape_amd import visualize as vz
    from test_sweep_cpu import tiny_dataset
    cfg, ddir = tiny_dataset(tmp_path, size=32, block=10)
    out = tmp_path / "viz"
    vz.main(["--config", str(cfg), "--depth-dir", str(ddir), "--out", str(out), "--relight", "--obj"])
    for stem in "ab":
        names = set(os.listdir(out / stem))
        assert names == {f"turntable_{m}.gif" for m in vz.MODES} | {"relight.gif", "depth.png", "normal.png",
                                                                     stem + ".obj", stem + ".mtl", stem + ".png"}
        for m in vz.MODES:
            with Image.open(out / stem / f"turntable_{m}.gif") as g:
                assert g.n_frames == 120 and g.size == (32, 32), (stem, m)
        with Image.open(out / stem / "relight.gif") as g:
            assert g.n_frames == 120 and g.size == (32, 32)
    with Image.open(out / "b" / "turntable_shape.gif") as g:
        frames = []
        for i in range(g.n_frames):
            g.seek(i)
            frames.append(np.asarray(g.convert("RGB")).astype(np.int32))
    frames = np.stack(frames)
    assert np.abs(frames[0] - frames[30]).max() > 8                          # first pose against the middle one
    # the 10 x 10 masked corner: a yaw of at most atan2(0.75, 1.5) moves a vertex by (z - c) sin(yaw) in x, and the
    # depths here stay within 0.04 of the rotation centre c = 1: 0.018 of a half width of 0.0875 = 15.5 pixels, 3.2
    # pixels; rows shift by less than one (z changes by < 4 %).  The inner 6 x 6 of the block stays uncovered.
    assert (frames[:, :6, :6] == 255).all()
    assert (frames[:, 12:20, 12:20] < 255).any()
