"""-m "not gpu": the parsing networks and MaskingModel (gan-2d-to-3d_amd/parsing.py) on the CPU route — the
architecture restatement against the reference's float64 results (tests/golden/parsing.npz, weights regenerated from
the seed recipe of parsing_cases), BatchNorm folding, the polyphase form of the dilated convolutions, checkpoint
layouts, and what the new C entry points refuse before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gan2shape_amd  # noqa: F401
from gan2shape_amd import lib, parsing

import parsing_cases as pc

NEW_SYMBOLS = ["g2s_conv_stem7", "g2s_maxpool3x3s2", "g2s_adaptive_avgpool", "g2s_resize_bilinear", "g2s_gate_add_act",
               "g2s_parse_head_workspace_bytes", "g2s_parse_head"]


def make_net(name, dtype=torch.float64):
    net = parsing.BiSeNet(19) if name == "bisenet" else parsing.PSPNet(50, 21)
    return pc.fill(net.to(dtype), pc.NETS[name]["weight_seed"])


@pytest.fixture(scope="module")
def nets64():
    return {name: make_net(name) for name in pc.NETS}


@pytest.mark.parametrize("name", list(pc.NETS))
def test_state_dict_names_and_shapes(golden, name):
    net = parsing.BiSeNet(19) if name == "bisenet" else parsing.PSPNet(50, 21)
    assert list(pc.state_list(net.state_dict())) == list(golden("parsing")[f"{name}.names"])


@pytest.mark.parametrize("name", list(pc.NETS))
def test_cpu_route_reproduces_the_float64_logits(golden, nets64, name):
    """1e-10 relative in float64: pins the architecture restatement, stage by stage."""
    g, net, side = golden("parsing"), nets64[name], pc.NETS[name]["side"]
    x = pc.images(name, side).double()
    stages = net.features(x)
    keys = ("feat8", "feat16", "feat32") if name == "bisenet" else ("layer1", "layer2", "layer3", "layer4")
    for key, feat in zip(keys, stages):
        assert abs(float(feat.norm()) / float(g[f"{name}.norm.{key}"]) - 1) < 1e-10, key
    low = net.logits_lowres(x)
    ref = torch.from_numpy(g[f"{name}.low"])
    assert low.shape == ref.shape
    assert pc.l2_rel(low, ref) < 1e-10
    full = net(x)
    assert full.shape == (pc.B, ref.shape[1], side, side)
    assert pc.l2_rel(full, pc.upsample64(ref, side)) < 1e-10


def test_bn_folding_equals_conv_then_bn():
    torch.manual_seed(0)
    for bias in (False, True):
        conv = nn.Conv2d(5, 7, 3, 1, 1, bias=bias).double()
        bn = nn.BatchNorm2d(7).double().eval()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
        x = torch.randn(2, 5, 6, 7, dtype=torch.float64)
        w, b = parsing.fold_bn(conv, bn, torch.float64)
        with torch.no_grad():
            torch.testing.assert_close(F.conv2d(x, w, b, padding=1), bn(conv(x)), rtol=1e-12, atol=1e-12)
        w, b = parsing.fold_bn(conv, None, torch.float64)
        assert torch.equal(w, conv.weight) and (b is None) == (not bias)


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("hw", [(8, 8), (9, 10)])
def test_polyphase_form_of_a_dilated_convolution(d, hw):
    torch.manual_seed(d)
    x = torch.randn(2, 3, *hw, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, dtype=torch.float64)
    b = torch.randn(4, dtype=torch.float64)
    got = parsing.dilated_conv3x3(x, w, b, d)
    torch.testing.assert_close(got, F.conv2d(x, w, b, padding=d, dilation=d), rtol=1e-12, atol=1e-12)
    sub = parsing.polyphase_split(x, d)
    assert sub.shape == (d * d * 2, 3, -(-hw[0] // d), -(-hw[1] // d))
    assert torch.equal(parsing.polyphase_merge(sub, d, 2, *hw), x)


@pytest.mark.parametrize("name", list(pc.NETS))
def test_masking_model_on_cpu_reproduces_the_fixture(golden, nets64, name):
    g, cfg = golden("parsing"), pc.NETS[name]
    mm = parsing.MaskingModel(cfg["category"], device="cpu", size=cfg["side"], net=nets64[name])
    image = pc.images(name + ".mm", pc.S).double()
    got = mm.image_mask(image)
    assert got.shape == (pc.B, 1, pc.S, pc.S)
    # float64 against float64: an argmax can differ only on an exact tie
    np.testing.assert_allclose(got.numpy(), g[f"{name}.mm.image_mask"], rtol=0, atol=1e-12)
    assert mm.last_fallback.tolist() == [0, 0]
    np.testing.assert_allclose(mm.confidence_mask(image).numpy(), g[f"{name}.mm.confidence_mask"], rtol=0, atol=1e-10)
    # the plotting variant: NaN exactly where the full-resolution mask of that sample is empty over the whole bin
    depth = torch.ones(pc.B, pc.S, pc.S, dtype=torch.float64)
    masked = mm.image_mask(image, depth)
    assert masked.shape == (pc.B, 1, pc.S, pc.S)
    full = np.unpackbits(g[f"{name}.mm.full_mask"])[:pc.B * cfg["side"] ** 2].reshape(pc.B, 1, cfg["side"], cfg["side"])
    all_in = F.adaptive_avg_pool2d(torch.from_numpy(full).double(), pc.S) == 1
    assert torch.equal(~torch.isnan(masked), all_in)
    assert parsing.mask_depth(mm, image, depth).shape == masked.shape


def test_masking_model_rules():
    """The rules on hand-made logits: channel 17 never wins, classes 1..13 are the face, a sample without the class
    becomes all ones with its flag set, other samples keep theirs."""
    class Fixed(nn.Module):
        def __init__(self, out):
            super().__init__()
            self.out = out

        def forward(self, x, native=False):
            return self.out

    out = torch.zeros(2, 19, 4, 4)
    out[0, 17] = 5.0                    # dropped: the runner-up decides
    out[0, 3, :2] = 1.0                 # face class on the top half
    out[0, 16, 2:] = 1.0                # class 16 (not face) on the bottom half
    out[1, 0] = 1.0                     # background everywhere: the fallback
    mm = parsing.MaskingModel("face", device="cpu", size=4, net=Fixed(out))
    m = mm.image_mask(torch.zeros(2, 3, 4, 4))
    assert torch.equal(m[0, 0], torch.tensor([[1.0] * 4] * 2 + [[0.0] * 4] * 2))
    assert torch.equal(m[1], torch.ones(1, 4, 4)) and mm.last_fallback.tolist() == [0, 1]
    out21 = torch.zeros(1, 21, 4, 4)
    out21[0, 7, 1] = 2.0
    mm = parsing.MaskingModel("car", device="cpu", size=4, net=Fixed(out21))
    assert torch.equal(mm.image_mask(torch.zeros(1, 3, 4, 4))[0, 0, :, 0], torch.tensor([0.0, 1.0, 0.0, 0.0]))
    assert torch.equal(mm.confidence_mask(torch.zeros(1, 3, 4, 4))[0, 0, :, 0], torch.tensor([0.0, 1.0, 0.0, 0.0]))


def test_checkpoint_layouts_and_missing_file(tmp_path):
    net = pc.fill(parsing.PSPNet(50, 21), 3)
    state = {"module." + k: v for k, v in net.state_dict().items()}
    state["module.aux.0.weight"] = torch.zeros(256, 1024, 3, 3)      # the training-only branch of the public file
    torch.save({"state_dict": state, "epoch": 1}, tmp_path / "pspnet_voc.pth")
    face = pc.fill(parsing.BiSeNet(19), 4)
    torch.save(face.state_dict(), tmp_path / "bisenet.pth")
    mm = parsing.MaskingModel("car", device="cpu", ckpt_dir=str(tmp_path), size=9)
    for k, v in net.state_dict().items():
        assert torch.equal(mm.mask_net.state_dict()[k], v), k
    assert mm.size == 9 and parsing.MaskingModel("cat", device="cpu", ckpt_dir=str(tmp_path)).size == 473
    mf = parsing.MaskingModel("face", device="cpu", ckpt_dir=str(tmp_path))
    assert mf.size == 512 and torch.equal(mf.mask_net.conv_out.conv_out.weight, face.conv_out.conv_out.weight)
    with pytest.raises(FileNotFoundError, match="bisenet.pth"):
        parsing.MaskingModel("face", device="cpu", ckpt_dir=str(tmp_path / "nowhere"))
    with pytest.raises(RuntimeError):        # anything but the aux branch must match by name
        torch.save({"state_dict": {k: v for k, v in state.items() if "cls.4" not in k}}, tmp_path / "pspnet_voc.pth")
        parsing.MaskingModel("car", device="cpu", ckpt_dir=str(tmp_path))
    assert parsing.masking_model_from_config({"category": "car"}) is None
    assert parsing.masking_model_from_config({"category": "car", "parsing_ckpt_dir": str(tmp_path / "nowhere")}) is None


def test_trainer_builds_the_masking_model_only_on_request():
    from gan2shape_amd.trainer import Trainer
    from gan2shape_amd.priors import synthetic_mask
    from model_cases import TOY_CFG, ToyStepModel
    t = Trainer(ToyStepModel, dict(TOY_CFG), device="cpu")
    assert t.prior_generator.masking_model is synthetic_mask and t.prior_generator.mask_accepts_batch is False


def test_libg2s_route_refuses_cpu_tensors():
    x = torch.zeros(1, 3, 8, 8)
    for call in (lambda: parsing.maxpool3x3s2(x), lambda: parsing.adaptive_avgpool(x, 2),
                 lambda: parsing.resize_bilinear(x, 4, True), lambda: parsing.gate_add_act(x),
                 lambda: parsing.conv_stem7(x, torch.zeros(4, 3, 7, 7), None),
                 lambda: parsing.parse_head(x, 16, 8, 0, -1, 2)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()


def test_new_symbols_are_declared_and_exported():
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert name in lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.g2s_abi_version() == 1
    assert L.g2s_parse_head_workspace_bytes(5) == 80 and L.g2s_parse_head_workspace_bytes(0) == 0


def test_validation_precedes_any_launch():
    """A host buffer stands in for device memory: a launch would fault, a rejected call never gets that far."""
    L = lib.load()
    d = (C.c_float * 4)()

    def err():
        return L.g2s_last_error().decode()
    assert L.g2s_conv_stem7(None, d, d, d, 1, 64, 9, 9, 1, None) == -1 and "NULL" in err()
    assert L.g2s_conv_stem7(d, d, d, d, 1, 0, 9, 9, 1, None) == -1 and "positive" in err()
    assert L.g2s_conv_stem7(d, d, d, d, 70000, 64, 9, 9, 1, None) == -1 and "large" in err()
    assert L.g2s_maxpool3x3s2(d, None, 1, 5, 5, None) == -1 and "NULL" in err()
    assert L.g2s_maxpool3x3s2(d, d, 1, 0, 5, None) == -1
    assert L.g2s_adaptive_avgpool(d, d, 1, 5, 5, 0, 1, None) == -1 and "positive" in err()
    assert L.g2s_adaptive_avgpool(None, d, 1, 5, 5, 1, 1, None) == -1 and "NULL" in err()
    assert L.g2s_resize_bilinear(d, d, 1, 5, 5, 1, 0, 1, None) == -1
    assert L.g2s_resize_bilinear(d, None, 1, 5, 5, 7, 7, 1, None) == -1 and "NULL" in err()
    assert L.g2s_resize_bilinear(d, d, 1 << 20, 1 << 6, 1 << 6, 7, 7, 1, None) == -1 and "large" in err()
    assert L.g2s_gate_add_act(d, None, None, None, d, 1, 4, 1, 0, 0, None) == -1 and "gate" in err()
    assert L.g2s_gate_add_act(d, None, None, None, d, 1, 4, 0, 1, 0, None) == -1 and "gate" in err()
    assert L.g2s_gate_add_act(None, None, None, None, d, 1, 4, 0, 0, 0, None) == -1 and "NULL" in err()
    big = 1 << 20
    ok = dict(B=1, C=19, h=8, w=8, size=32, S=8, mode=0, drop=17, cs=0x3ffe)

    def head(logits=d, out=d, full=None, ws=d, ws_bytes=big, **kw):
        a = dict(ok, **kw)
        return L.g2s_parse_head(logits, a["B"], a["C"], a["h"], a["w"], a["size"], a["S"], a["mode"], a["drop"], a["cs"],
                                out, full, None, ws, ws_bytes, None)
    assert head(C=33) == -1 and "C" in err()
    assert head(S=33) == -1 and "S" in err()
    assert head(S=0) == -1
    assert head(mode=2) == -1 and "mode" in err()
    assert head(drop=19) == -1 and "drop" in err()
    assert head(mode=1, drop=17) == -1 and "confidence" in err()
    assert head(cs=0) == -1 and "class_set" in err()
    assert head(cs=1 << 19) == -1 and "class_set" in err()
    assert head(mode=1, drop=-1, full=d) == -1 and "hard" in err()
    assert head(logits=None) == -1 and "NULL" in err()
    assert head(out=None) == -1 and "NULL" in err()
    assert head(ws=None, ws_bytes=0) == -3 and "workspace" in err()
    assert head(ws_bytes=8) == -3 and "workspace" in err()
    assert head(B=-1) == -1
    # an empty batch is a no-op, NULL pointers and all
    assert head(B=0, logits=None, out=None, ws=None, ws_bytes=0) == 0
    assert L.g2s_conv_stem7(None, None, None, None, 0, 64, 9, 9, 1, None) == 0
    assert L.g2s_maxpool3x3s2(None, None, 0, 5, 5, None) == 0
    assert L.g2s_adaptive_avgpool(None, None, 0, 5, 5, 1, 1, None) == 0
    assert L.g2s_resize_bilinear(None, None, 0, 5, 5, 7, 7, 1, None) == 0
    assert L.g2s_gate_add_act(None, None, None, None, None, 0, 4, 0, 0, 0, None) == 0
