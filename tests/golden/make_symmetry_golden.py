"""Golden vectors of the symmetry flips (flip1_cfg / flip3_cfg / lam_flip): tests/golden/symmetry.npz.

    python tests/golden/make_symmetry_golden.py

The reference stops at `# TODO: add flips?` (GAN2Shape/model.py:102,124), so the oracle is built here from the
reference model's OWN parts: its nets, get_clamped_depth, get_view_transformation, get_lighting_directions,
get_shading, its Renderer's geometry methods and its loss classes, composed as the flipped step 1 and step 3 are
specified.  The model is the one of make_golden.steps_golden (model_cases.STEP_CFG, seeded nets,
model_cases.fake_perceptual, the C oracle behind the rasterizer boundary); image, latent and the step-2 hand-off
(projected samples and masks, n_proj = 2) come from tests/golden/steps.npz.  Every pass runs once in float64 — the
stored values — and once in float32: `e32_<key>` is max |float32 run - float64 run|, the reference's own float32
error, from which the GPU tests take their bounds.  Only data is written.
"""
import math
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import make_golden as mg        # noqa: E402
import model_cases as mc        # noqa: E402
import symmetry_cases as sc     # noqa: E402

IMAGE_SEED = None       # None: the image of steps.npz; an int: another seeded image (if the mirrored rows fold)


def build_reference_model(steps, dtype):
    """The reference's GAN2Shape in the state of make_golden.steps_golden, in `dtype`."""
    import types
    sys.modules["neural_renderer"] = types.ModuleType("neural_renderer")
    sys.modules["neural_renderer"].Renderer = lambda **k: None      # replaced below: the reference only stores it
    for name in [m for m in sys.modules if m.startswith("GAN2Shape.renderer")]:
        del sys.modules[name]
    ref_model, ref_losses, _ = mg._import_reference_model()
    from GAN2Shape import networks as ref_nets
    from GAN2Shape.renderer import Renderer as RefRenderer
    cfg = mc.STEP_CFG
    S = cfg["image_size"]
    M = object.__new__(ref_model.GAN2Shape)
    torch.nn.Module.__init__(M)
    M.debug, M.image_size = False, S
    for name, cls in (("lighting", "LightingNet"), ("viewpoint", "ViewpointNet"), ("depth", "DepthNet"),
                      ("albedo", "AlbedoNet")):
        net = getattr(ref_nets, cls)(S)
        mc.fill_scaled(net, cfg["seeds"][name])
        if name == "depth":     # the well-conditioned surface of steps.npz `s3s.*`: no view of the fixture folds it
            mc.smooth_depth_net(net)
        setattr(M, f"{name}_net", net.to(dtype))
    M.max_depth, M.min_depth = 1.1, 0.9
    M.border_depth = 0.7 * M.max_depth + 0.3 * M.min_depth
    M.lam_perc, M.lam_smooth, M.lam_flip = 1, 0.01, sc.LAM_FLIP
    M.xyz_rotation_range, M.xy_translation_range, M.z_translation_range = 60, 0.1, 0.1
    M.renderer = RefRenderer({"rot_center_depth": 1.0, "fov": 10, "tex_cube_size": 2}, S, M.min_depth, M.max_depth)
    M.renderer.renderer = sc.OracleRasterizer(mg.np_(M.renderer.K), S)
    M.renderer.K, M.renderer.inv_K = M.renderer.K.to(dtype), M.renderer.inv_K.to(dtype)
    with tempfile.TemporaryDirectory() as tmp:
        torch.save({"mean": torch.tensor(steps["vls.vm"]), "cov": torch.tensor(steps["vls.vc"])}, os.path.join(tmp, "v.pth"))
        torch.save({"mean": torch.tensor(steps["vls.lm"]), "cov": torch.tensor(steps["vls.lc"])}, os.path.join(tmp, "l.pth"))
        M.view_light_sampler = ref_model.ViewLightSampler(os.path.join(tmp, "v.pth"), os.path.join(tmp, "l.pth"), 1)
    M.smooth_loss, M.photometric_loss = ref_losses.SmoothLoss(), ref_losses.PhotometricLoss()
    M.perceptual_loss = mc.fake_perceptual
    return M


def flipped_step1(M, images, step1, b=1):
    """forward_step1 (model.py:95-173) with the flip: 2B rows behind the nets -> (terms, tensors, collected)."""
    B, (h, w) = len(images), (M.image_size, M.image_size)
    with torch.no_grad() if step1 else torch.enable_grad():
        depth_raw = M.depth_net(images)
        view = M.viewpoint_net(images)
        lighting = M.lighting_net(images)
    albedo = M.albedo_net(images)
    depth = M.get_clamped_depth(depth_raw.squeeze(1), h, w)             # the centre over the B unflipped maps
    view = view + M.view_light_sampler.view_mean.unsqueeze(0)
    lighting = lighting + M.view_light_sampler.light_mean.unsqueeze(0)
    depth2, albedo2 = torch.cat([depth, depth.flip(2)]), torch.cat([albedo, albedo.flip(3)])
    view2, lighting2 = torch.cat([view, view]), torch.cat([lighting, lighting])
    M.renderer.set_transform_matrices(M.get_view_transformation(view2))
    la, lb, ld = M.get_lighting_directions(lighting2)
    normal2 = M.renderer.get_normal_from_depth(depth2)
    diffuse2, texture2 = M.get_shading(normal2, la, lb, ld, albedo2)
    recon_depth = M.renderer.warp_canon_depth(depth2)
    grid = M.renderer.get_inv_warped_2d_grid(recon_depth)
    margin = (M.max_depth - M.min_depth) / 2
    mask = (recon_depth < M.max_depth + margin).to(recon_depth.dtype).unsqueeze(1).detach()
    recon_im = F.grid_sample(texture2, grid, mode='bilinear').clamp(min=-1, max=1)
    rb, mb, rf, mf = recon_im[:b], mask[:b], recon_im[B:B + b], mask[B:B + b]
    terms = dict(l1=M.photometric_loss(rb, images, mask=mb), l1_flip=M.photometric_loss(rf, images, mask=mf),
                 perc=torch.mean(M.perceptual_loss(rb * mb, images * mb)),
                 perc_flip=torch.mean(M.perceptual_loss(rf * mf, images * mf)),
                 smooth_depth=M.smooth_loss(depth2), smooth_shading=M.smooth_loss(diffuse2))
    loss = (terms["l1"] + M.lam_flip * terms["l1_flip"] + M.lam_perc * (terms["perc"] + M.lam_flip * terms["perc_flip"])
            + M.lam_smooth * (terms["smooth_depth"] + terms["smooth_shading"]))
    return loss, terms, dict(recon_im=rb, recon_im_flip=rf), (normal2[:B], la[:B], lb[:B], albedo, depth, None)


def flipped_step3(M, images, c2):
    """forward_step3 (model.py:225-280) with the flip: the inner step-1 pass above, then 2b rows for the b samples."""
    projected, masks = c2
    step1_loss, _, _, collected = flipped_step1(M, images, step1=False)
    _, _, _, albedo, depth, _ = collected
    b, S = len(projected), M.image_size
    view = M.viewpoint_net(projected) + M.view_light_sampler.view_mean.unsqueeze(0)
    light = M.lighting_net(projected) + M.view_light_sampler.light_mean.unsqueeze(0)
    depth2 = torch.cat([depth.expand(b, S, S), depth.flip(2).expand(b, S, S)])
    albedo2 = torch.cat([albedo.expand(b, 3, S, S), albedo.flip(3).expand(b, 3, S, S)])
    view2, light2, masks2 = torch.cat([view, view]), torch.cat([light, light]), torch.cat([masks, masks])
    M.renderer.set_transform_matrices(M.get_view_transformation(view2))
    la, lb, ld = M.get_lighting_directions(light2)
    normal2 = M.renderer.get_normal_from_depth(depth2)
    _, texture2 = M.get_shading(normal2, la, lb, ld, albedo2)
    recon_depth = M.renderer.warp_canon_depth(depth2)
    grid = M.renderer.get_inv_warped_2d_grid(recon_depth)
    margin = (M.max_depth - M.min_depth) / 2
    mask = (recon_depth < M.max_depth + margin).to(recon_depth.dtype).unsqueeze(1).detach() * masks2
    recon_im = F.grid_sample(texture2, grid, mode='bilinear').clamp(min=-1, max=1)
    rb, mb, rf, mf = recon_im[:b], mask[:b], recon_im[b:], mask[b:]
    terms = dict(step1=step1_loss, l1=M.photometric_loss(rb, projected, mask=mb),
                 l1_flip=M.photometric_loss(rf, projected, mask=mf),
                 perc=torch.mean(M.perceptual_loss(rb * mb, projected * mb)),
                 perc_flip=torch.mean(M.perceptual_loss(rf * mf, projected * mf)))
    loss = (step1_loss + terms["l1"] + M.lam_flip * terms["l1_flip"]
            + M.lam_perc * (terms["perc"] + M.lam_flip * terms["perc_flip"]))
    return loss, terms, dict(recon_im=rb, recon_im_flip=rf), collected


def run(dtype, steps, image):
    out, folds = {}, {}
    with mg._cuda_is_identity(), mg._torch12_grid_sample():
        M = build_reference_model(steps, dtype)
        # the reference builds its rotation matrices, border masks and constants with torch.zeros / torch.ones of the
        # DEFAULT dtype (renderer/utils.py:34-36, model.py:342,351): the float64 run makes that float64 too, after the
        # seeded weights are drawn (torch.randn follows the default dtype as well)
        torch.set_default_dtype(dtype)
        image = image.to(dtype)
        c2 = (torch.tensor(steps["s2.projected"]).to(dtype), torch.tensor(steps["s2.mask"]).to(dtype))
        for name, (kind, _switch, step1) in sc.PASSES.items():
            for p in M.parameters():
                p.grad = None
            n0 = len(M.renderer.renderer.maps)
            if kind == 1:
                loss, terms, tensors, collected = flipped_step1(M, image, step1)
            else:
                loss, terms, tensors, collected = flipped_step3(M, image, c2)
            loss.backward()
            out[f"{name}.loss"] = loss
            for k, v in list(terms.items()) + list(tensors.items()) + list(zip(sc.COLLECTED, collected[:5])):
                out.update({k2: torch.tensor(v2) for k2, v2 in sc.stored(name, k, v.detach().double().numpy()).items()})
            for net in sc.TRAINED[name]:
                tnorm, proj = mc.grad_evidence(getattr(M, f"{net}_net"))
                out[f"{name}.gnorm.{net}"] = torch.tensor(float(np.linalg.norm(tnorm)), dtype=torch.float64)
                out[f"{name}.gtnorm.{net}"], out[f"{name}.gproj.{net}"] = torch.tensor(tnorm), torch.tensor(proj)
            for net in set(("lighting", "viewpoint", "depth", "albedo")) - set(sc.TRAINED[name]):
                assert all(p.grad is None for p in getattr(M, f"{net}_net").parameters()), (name, net)
            folds[name] = [mg.fold_report(f, b_, M.image_size) for f, b_ in M.renderer.renderer.maps[n0:]]
        torch.set_default_dtype(torch.float32)
    return {k: v.detach().double().numpy() for k, v in out.items()}, folds


def main():
    steps = dict(np.load(os.path.join(OUT, "steps.npz")))
    if IMAGE_SEED is None:
        image = torch.tensor(steps["image"])
    else:
        g = torch.Generator().manual_seed(IMAGE_SEED)
        image = torch.tanh(F.interpolate(torch.randn(1, 3, 32, 32, generator=g), scale_factor=4, mode="bilinear"))
    v64, folds = run(torch.float64, steps, image)
    v32, _ = run(torch.float32, steps, image)
    out = {"image": image.numpy(), "lam_flip": np.array(sc.LAM_FLIP)}
    for k, v in v64.items():
        out[k] = v
        out[f"e32_{k}"] = np.array(sc.distance(v32[k], v))
    # (a) the mirrored depth rows are as well conditioned as the plain ones (fold_report: discontinuous pairs, edge
    # samples, edge samples at a discontinuity, max quad jump)
    for name, reports in folds.items():
        print(name, "fold_report per rasterizer call:", reports)
        out[f"{name}.fold_report"] = np.array(reports)
    # (b) a test can tell the halves apart: the flipped L1 term is not the plain one
    for name in sc.PASSES:
        d = abs(float(out[f"{name}.l1_flip"]) - float(out[f"{name}.l1"]))
        e = max(float(out[f"e32_{name}.l1_flip"]), float(out[f"e32_{name}.l1"]))
        print(f"{name}: |l1_flip - l1| = {d:.3e}, e32 = {e:.3e}, loss = {float(out[name + '.loss']):.6f}")
        assert d > 100 * e, (name, d, e)
    for name, reports in folds.items():
        for r in reports:
            # as make_golden.steps_golden asserts of the plain rows of this surface: no supersample within the edge
            # tolerance sits at a depth discontinuity, and the mesh shows none inside
            assert r[2] == 0 and r[3] <= 2, (name, "the mirrored rows are ill-conditioned: change IMAGE_SEED", reports)
    np.savez_compressed(os.path.join(OUT, "symmetry.npz"), **out)
    print("symmetry.npz", os.path.getsize(os.path.join(OUT, "symmetry.npz")))
    for k in sorted(out):
        if k.startswith("e32_") and out[k].ndim == 0 and ("loss" in k or ".l1" in k or ".perc" in k or "gnorm" in k):
            print(f"  {k} = {float(out[k]):.3e}  (value {float(np.max(np.abs(out[k[4:]]))):.6f})")


if __name__ == "__main__":
    main()
