"""Shared by tests/golden/make_symmetry_golden.py (the reference side) and the symmetry tests (this package's side):
the cases of tests/golden/symmetry.npz, a CPU rasterizer stand-in that keeps the precision of its input, and the
comparison of a run with the stored float64 one."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAM_FLIP = 0.5
# pass name -> (step kind, the switch that is on, step1 argument of the inner / only forward_step1)
PASSES = {"f1s1": (1, "flip1", True), "f3s1": (1, "flip3", False), "f3s3": (3, "flip3", False)}
TERMS = {"f1s1": ("l1", "l1_flip", "perc", "perc_flip", "smooth_depth", "smooth_shading"),
         "f3s1": ("l1", "l1_flip", "perc", "perc_flip", "smooth_depth", "smooth_shading"),
         "f3s3": ("step1", "l1", "l1_flip", "perc", "perc_flip")}
COLLECTED = ("normal", "light_a", "light_b", "albedo", "depth")
TRAINED = {"f1s1": ("albedo",), "f3s1": ("lighting", "viewpoint", "depth", "albedo"),
           "f3s3": ("lighting", "viewpoint", "depth", "albedo")}


class _RenderDepth(torch.autograd.Function):
    """oracle/raster_body.inc behind the render_depth boundary, in the precision of the vertices (the helper of
    make_golden.py returns float32 whatever it computed in)."""

    @staticmethod
    def forward(ctx, verts, faces, S, K, maps):
        from oracle import capi
        dt = np.float64 if verts.dtype == torch.float64 else np.float32
        v = verts.detach().numpy().astype(dt)
        f = faces[0].numpy().astype(np.int32)
        ref = capi.render_depth(v, f, S, K.astype(dt), dtype=dt)
        ctx.save_for_backward(verts)
        ctx.aux = (f, S, K, ref["face_idx"], ref["bary"], dt)
        maps.append((ref["face_idx"], ref["bary"]))
        return torch.from_numpy(np.asarray(ref["depth"], dt))

    @staticmethod
    def backward(ctx, g):
        from oracle import capi
        (verts,) = ctx.saved_tensors
        f, S, K, fidx, bary, dt = ctx.aux
        gv = capi.render_depth_bwd(verts.detach().numpy().astype(dt), f, g.contiguous().numpy().astype(dt), fidx, bary,
                                   S, K.astype(dt), dtype=dt)
        return torch.from_numpy(np.asarray(gv, dt)), None, None, None, None


class OracleRasterizer:
    """What a Renderer calls `self.renderer`: render_depth(vertices [B,V,3], faces [B,F,3]) -> [B,S,S] on the CPU."""

    def __init__(self, K, image_size):
        self.K = np.asarray(K, np.float64).reshape(-1, 3, 3)[0]
        self.image_size = image_size
        self.maps = []          # (face_idx, bary) of every call, in call order

    def render_depth(self, vertices, faces):
        return _RenderDepth.apply(vertices, faces, self.image_size, self.K, self.maps)


MAPS = ("recon_im", "recon_im_flip", "normal", "albedo", "depth")
N_MAP_PROBES = 4


def stored(name, key, value):
    """What symmetry.npz keeps of quantity `key` of pass `name`: everything, except for the image-sized maps (the file
    stays under the size limit for a committed fixture): every 4th pixel of every 4th row from (1, 1), whole in
    `<key>`, and the WHOLE map's projections on N_MAP_PROBES fixed probe directions (model_cases.probe_direction)
    in `<key>.proj` — every element enters those."""
    import model_cases as mc
    v = np.asarray(value, np.float64)
    if key not in MAPS:
        return {f"{name}.{key}": v}
    sub = v[:, 1::4, 1::4] if key in ("normal", "depth") else v[:, :, 1::4, 1::4]
    flat = v.reshape(-1)
    proj = np.array([float(flat @ mc.probe_direction(flat.size, 100 + k)) for k in range(N_MAP_PROBES)])
    return {f"{name}.{key}": np.ascontiguousarray(sub), f"{name}.{key}.proj": proj}


def rounding(value, dtype=np.float32):
    """One rounding of a quantity of this size: eps * the largest magnitude in it."""
    return float(np.finfo(dtype).eps) * float(np.max(np.abs(value)))


def distance(value, ref):
    """max |value - ref|: the distance every `e32_<key>` of symmetry.npz is stored in."""
    return float(np.max(np.abs(np.asarray(value, np.float64) - np.asarray(ref, np.float64))))


def run_pass(model, name, image, latent, c2, evidence, zero_grads):
    """One pass of PASSES on this package's GAN2Shape -> {key: float64 numpy} with the keys of symmetry.npz
    (`<name>.<quantity>`).  `evidence(net)` -> (per-tensor norms, probe projections) (model_cases.grad_evidence);
    the loss terms are recorded from the calls of the model's own loss objects, in call order."""
    kind, switch, step1 = PASSES[name]
    out = {}
    model.flip1 = model.flip3 = False
    setattr(model, switch, True)
    zero_grads(model)
    calls = {"l1": [], "perc": [], "smooth": [], "recon": []}
    orig = (model.photometric_loss, model.perceptual_loss, model.smooth_loss)

    def photometric(a, b, mask=None, **k):
        v = orig[0](a, b, mask=mask, **k)
        calls["l1"].append(v)
        calls["recon"].append(a)
        return v

    def perceptual(a, b):
        v = orig[1](a, b)
        calls["perc"].append(v)
        return v

    def smooth(x):
        v = orig[2](x)
        calls["smooth"].append(v)
        return v
    object.__setattr__(model, "photometric_loss", photometric)
    object.__setattr__(model, "perceptual_loss", perceptual)
    object.__setattr__(model, "smooth_loss", smooth)
    try:
        if kind == 1:
            loss, collected = model.forward_step1(image, latent, None, step1=step1)
        else:
            inner = {}
            f1 = model._step1_terms       # the inner step-1 pass of step 3 -> (terms, collected, LPIPS groups)

            def keep(*a, **k):
                r = f1(*a, **k)
                inner["collected"] = r[1]
                return r
            model._step1_terms = keep
            try:
                loss, _ = model.forward_step3(image, latent, c2)
            finally:
                del model._step1_terms
            collected = inner["collected"]
        loss.backward()
    finally:
        object.__setattr__(model, "photometric_loss", orig[0])
        object.__setattr__(model, "perceptual_loss", orig[1])
        object.__setattr__(model, "smooth_loss", orig[2])
        model.flip1 = model.flip3 = False

    def f64(t):
        return t.detach().double().cpu().numpy()
    out[f"{name}.loss"] = f64(loss)
    perc = torch.cat([p.reshape(-1) for p in calls["perc"]])      # one trunk pass or several: the same values in order
    lam = model.lam_flip
    if kind == 1:
        B = len(image)
        terms = dict(l1=calls["l1"][0], l1_flip=calls["l1"][1], perc=perc[:B].mean(), perc_flip=perc[B:2 * B].mean(),
                     smooth_depth=calls["smooth"][0], smooth_shading=calls["smooth"][1])
        recon = calls["recon"][0], calls["recon"][1]
    else:
        b = len(c2[0])
        s1 = (calls["l1"][0] + lam * calls["l1"][1] + model.lam_perc * (perc[0] + lam * perc[1])
              + model.lam_smooth * (calls["smooth"][0] + calls["smooth"][1]))
        terms = dict(step1=s1, l1=calls["l1"][2], l1_flip=calls["l1"][3], perc=perc[2:2 + b].mean(),
                     perc_flip=perc[2 + b:2 + 2 * b].mean())
        recon = calls["recon"][2], calls["recon"][3]
    for key in TERMS[name]:
        out[f"{name}.{key}"] = f64(terms[key])
    for key, t in list(zip(("recon_im", "recon_im_flip"), recon)) + list(zip(COLLECTED, collected[:5])):
        out.update(stored(name, key, f64(t)))
    for net in TRAINED[name]:
        tnorm, proj = evidence(getattr(model, f"{net}_net"))
        out[f"{name}.gnorm.{net}"] = np.array(float(np.linalg.norm(tnorm)))
        out[f"{name}.gtnorm.{net}"], out[f"{name}.gproj.{net}"] = tnorm, proj
    zero_grads(model)
    return out
