"""Reference results of the parsing networks -> tests/golden/parsing.npz (run where the reference is; only DATA is
written, and no weights: tests/parsing_cases.py regenerates them from a seed).

    python tests/golden/make_parsing_golden.py [--search]

The reference's resnet.py / networks.py are loaded by path under the package name `GAN2Shape` (networks.py imports
`GAN2Shape.resnet`), with empty placeholders for torchvision and the gradient-debugging helper.  --search prints,
per net, the first weight seeds whose masks are non-trivial; the seed in parsing_cases.NETS must be one of them
(asserted below).

Stored per net (BiSeNet at 128 x 128, PSPNet at 97 x 97, B = 2 images of parsing_cases.images):
  names            ordered 'name shape' list of the state dict (PSPNet: without the training-only `aux` branch, which
                   the reference's constructor creates and its strict=False load tolerates)
  low              float64 logits BEFORE the net's final bilinear align_corners=True up-sampling.  The full-resolution
                   float64 logits would be 5 MB; they are that interpolation of `low` (checked here to 1e-12), which
                   the tests redo in float64 on the CPU (parsing_cases.upsample64).
  norm.*           float64 L2 norms of feat8 / feat16 / feat32 (layer1..4 for PSPNet), to localise a failure
  ref_fp32_err     the reference's own float32-vs-float64 L2-relative error of the full logits, maximum over 16 inputs
  mm.*             MaskingModel at size = 128 / 97 on 32 x 32 images: image_mask, confidence_mask, the packed
                   full-resolution hard mask and the float64 top-2 margin (stored as float32) after the class
                   rule's channel drop, mm.max_abs = max|logit|, mm.conf_range = per-sample max - min of the confidence sum.  The reference hard-codes its sizes (512 / 473), so
                   its rules are applied as restated in parsing_cases (hard_oracle, confidence_oracle) to the
                   REFERENCE nets' float64 logits of the reference-resized image (GAN2Shape/utils.py resize)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                      # noqa: E402  helpers only
import parsing_cases as pc                    # noqa: E402


def load_reference():
    pkg_dir = os.path.join(mg.REF, "GAN2Shape")
    for name in ("torchvision", "torchvision.transforms", "torchvision.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    pkg = types.ModuleType("GAN2Shape")
    pkg.__path__ = []
    sys.modules["GAN2Shape"] = pkg
    sys.modules["GAN2Shape.debug_grad_updates"] = types.ModuleType("GAN2Shape.debug_grad_updates")
    pkg.debug_grad_updates = sys.modules["GAN2Shape.debug_grad_updates"]
    for sub in ("resnet", "networks"):
        mod = mg._load_by_path(f"GAN2Shape.{sub}", os.path.join(pkg_dir, f"{sub}.py"))
        sys.modules[f"GAN2Shape.{sub}"] = mod
        setattr(pkg, sub, mod)
    utils = mg._load_by_path("ref_utils", os.path.join(pkg_dir, "utils.py"))
    return pkg.networks, utils


def build(nets, name, seed, dtype):
    if name == "bisenet":
        net = nets.BiSeNet(n_classes=19)
    else:
        net = nets.PSPNet(layers=50, classes=21, pretrained=False)
        del net.aux
    return pc.fill(net.eval().to(dtype), seed)


def run(net, name, x):
    """(full logits, low-resolution logits, stage features) of the reference net."""
    grabbed = {}
    head = net.conv_out if name == "bisenet" else net.cls
    handle = head.register_forward_hook(lambda m, i, o: grabbed.__setitem__("low", o))
    with torch.no_grad():
        full = net(x)
        if name == "bisenet":
            stages = dict(zip(("feat8", "feat16", "feat32"), net.cp.resnet(x)))
        else:
            y, stages = net.layer0(x), {}
            for i in (1, 2, 3, 4):
                y = getattr(net, f"layer{i}")(y)
                stages[f"layer{i}"] = y
    handle.remove()
    return full, grabbed["low"], stages


def masking_case(net, utils, name, dtype):
    cfg = pc.NETS[name]
    x = utils.resize(pc.images(name + ".mm", pc.S).to(dtype), [cfg["side"]] * 2)
    full, _, _ = run(net, name, x)
    drop, classes, channels = pc.rule_of(cfg["category"])
    mask, empty, margin, soft = pc.hard_oracle(full, drop, classes, pc.S)
    return full, mask, empty, margin, soft, pc.confidence_oracle(full, channels, pc.S)


def coverage_ok(net, utils, name, dtype=torch.float32):
    full, mask, empty, margin, _, _ = masking_case(net, utils, name, dtype)
    cover = mask.double().flatten(1).mean(1)
    excluded = float(pc.excluded_pixels(full, margin).double().mean())
    ok = bool(((cover >= 0.05) & (cover <= 0.95)).all()) and not bool(empty.any()) and excluded <= 0.8 * pc.EXCLUDED_CAP
    return ok, cover.tolist(), excluded


def main():
    nets, utils = load_reference()
    if "--search" in sys.argv:
        for name in pc.NETS:
            for seed in range(40):
                ok, cover, excluded = coverage_ok(build(nets, name, seed, torch.float32), utils, name)
                print(name, "seed", seed, "coverage", cover, "excluded", excluded, "ok" if ok else "")
                if ok:
                    break
        return
    out = {}
    for name, cfg in pc.NETS.items():
        side, seed = cfg["side"], cfg["weight_seed"]
        net64, net32 = build(nets, name, seed, torch.float64), build(nets, name, seed, torch.float32)
        ref = nets.BiSeNet(n_classes=19) if name == "bisenet" else nets.PSPNet(layers=50, classes=21, pretrained=False)
        out[f"{name}.names"] = pc.state_list(ref.state_dict(), skip=("aux.",))
        err, flips = 0.0, 0
        for s in range(pc.N_SEEDS):
            x = pc.images(name, side, s)
            full64, low64, stages = run(net64, name, x.double())
            full32, _, _ = run(net32, name, x)
            err = max(err, pc.l2_rel(full32, full64))
            flips += int((full32.argmax(1) != full64.argmax(1)).sum())
            if s == 0:
                assert float((pc.upsample64(low64, full64.shape[-1]) - full64).abs().max()) <= 1e-12 * float(full64.abs().max())
                out[f"{name}.low"] = mg.np_(low64)
                for k, v in stages.items():
                    out[f"{name}.norm.{k}"] = np.array(float(v.norm()))
        out[f"{name}.ref_fp32_err"] = np.array(err)
        ok, cover, excluded = coverage_ok(net32, utils, name)
        assert ok, (name, "the weight seed gives a trivial mask or too many near-ties", cover, excluded)
        full, mask, empty, margin, soft, conf = masking_case(net64, utils, name, torch.float64)
        cover = mask.double().flatten(1).mean(1)
        assert bool(((cover >= 0.05) & (cover <= 0.95)).all()) and not bool(empty.any()), (name, cover)
        share = float(pc.excluded_pixels(full, margin).double().mean())
        assert share <= pc.EXCLUDED_CAP, (name, share)
        out[f"{name}.mm.image_mask"] = mg.np_(soft)
        out[f"{name}.mm.confidence_mask"] = mg.np_(conf)
        out[f"{name}.mm.full_mask"] = np.packbits(mg.np_(mask))
        out[f"{name}.mm.margin"] = mg.np_(margin).astype(np.float32)
        out[f"{name}.mm.max_abs"] = np.array(float(full.abs().max()))
        v = full[:, list(pc.rule_of(cfg["category"])[2])].sum(1).flatten(1)
        out[f"{name}.mm.conf_range"] = mg.np_(v.amax(1) - v.amin(1))
        out[f"{name}.weight_seed"] = np.array(seed)
        print(f"{name}: fp32 L2-relative logit error {err:.2e}, fp32-vs-fp64 argmax flips {flips}, mask coverage "
              f"{cover.tolist()}, share of pixels with margin < {pc.MARGIN_REL} max|logit|: {100 * share:.3f} %")
    path = os.path.join(HERE, "parsing.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size)
    assert size < 1 << 20


if __name__ == "__main__":
    main()
