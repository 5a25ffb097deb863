"""The training monitor on the device: g2s_image_grid_u8 and g2s_ppl_latents against the float64 statements of
monitor_cases.py, perceptual_path_length against the same modules in float64 on the CPU, the 256 x 256 resize table, and
`train` with monitoring on.

Bounds.  Grid: the oracle's bytes, one off only where the float64 value is within 2^-16 of an integer, at no more than
1 % of the pixels.  Latents: 4 x the float32 torch composition's own maximum error on the same inputs (the multiple of
the pointwise kernels).  Path length: per-pair distances within 8 x the largest error of the float32 CPU route over the
case's pairs (results that pass through the whole convolution stack); at eps = 1e-4 that route must
itself be within 10 % of the oracle, which holds at the seeds of monitor_cases.py.  The scale is the largest of the six
errors and not each pair's own: one pair's float32 error is a single draw of rounding noise that can fall near zero by
chance (the six of one case spread over a factor of 4 to 65 on the side-16 generator), while all pairs of a case pass through the same layers at
distances of one magnitude, so the largest is the estimate of that noise's size that six draws give."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import gan2shape_amd  # noqa: F401
from gan2shape_amd import lib, monitor, train
from gan2shape_amd import stylegan2 as sg2
from gan2shape_amd.op import resample

import canary_buffers as cb
import dataprep_cases
import monitor_cases as mc

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------- grid
@pytest.mark.parametrize("case", mc.GRID_SHAPES, ids=lambda c: "x".join(map(str, c[:6])))
def test_image_grid_kernel(case):
    N, C, H, W, nrow, padding, pad_value = case
    x = mc.grid_inputs(N, C, H, W)
    want, pre = mc.grid64(x, nrow, padding, pad_value=pad_value)
    got = monitor.image_grid(torch.from_numpy(x).cuda(), nrow, padding, pad_value=pad_value)
    differing = mc.check_grid(got.cpu().numpy(), want, pre, str(case))
    print(f"grid {case}: {differing} pixels differ from float64")
    # the same launch into a canary-bracketed buffer, through the C ABI, 4-byte aligned (dword stores where Wg % 4 == 0)
    # and one byte off (byte stores)
    nbytes = want.size
    for shift in (0, 1):
        bufs = cb.Buffers()
        xin = bufs.view("x", arr=x)
        room = bufs.view("out", like=np.empty((nbytes + 8) // 4, np.float32))
        raw = room.view(torch.uint8)
        out = raw[shift:shift + nbytes]
        lib.check(lib.load().g2s_image_grid_u8(lib.ptr(xin), lib.ptr(out), N, C, H, W, nrow, padding, -1.0, 1.0,
                                               pad_value, lib.stream()))
        torch.cuda.synchronize()
        bufs.check()
        assert torch.equal(out.view(want.shape), got), shift
        beside = torch.ones(len(raw), dtype=torch.bool, device="cuda")
        beside[shift:shift + nbytes] = False
        canary = torch.full_like(room, cb.CANARY).view(torch.uint8)
        assert torch.equal(raw[beside], canary[beside]), "bytes beside the grid changed"


def test_image_grid_launch_checks():
    x = torch.zeros(2, 3, 4, 4, device="cuda")
    out = torch.empty(8, 14, 3, dtype=torch.uint8, device="cuda")
    L = lib.load()
    assert L.g2s_image_grid_u8(lib.ptr(x), lib.ptr(out), 2, 2, 4, 4, 8, 2, -1.0, 1.0, 0.0, lib.stream()) != 0
    assert L.g2s_image_grid_u8(lib.ptr(x), None, 2, 3, 4, 4, 8, 2, -1.0, 1.0, 0.0, lib.stream()) != 0
    assert L.g2s_image_grid_u8(lib.ptr(x), lib.ptr(out), 2, 3, 4, 4, 0, 2, -1.0, 1.0, 0.0, lib.stream()) != 0
    assert L.g2s_image_grid_u8(lib.ptr(x), lib.ptr(out), 2, 3, 4, 4, 8, -1, -1.0, 1.0, 0.0, lib.stream()) != 0
    assert L.g2s_ppl_latents(lib.ptr(x), lib.ptr(x), 1e-4, 2, lib.ptr(out), 1, 4, lib.stream()) != 0
    assert L.g2s_ppl_latents(lib.ptr(x), lib.ptr(x), 1e-4, 0, lib.ptr(x), 1, 4, lib.stream()) != 0
    assert L.g2s_ppl_latents(lib.ptr(x), lib.ptr(x), 1e-4, 0, lib.ptr(out), 0, 4, lib.stream()) != 0
    flat = x.view(-1)       # out one row into pairs: a partial overlap
    assert L.g2s_ppl_latents(lib.ptr(flat), lib.ptr(x), 1e-4, 0, lib.ptr(flat[4:]), 1, 4, lib.stream()) != 0
    assert L.g2s_ppl_latents(lib.ptr(flat[4:]), lib.ptr(x), 1e-4, 0, lib.ptr(flat), 1, 4, lib.stream()) != 0
    assert b"overlaps" in L.g2s_last_error()


# -------------------------------------------------------------------------------------------------------- latents
@pytest.mark.parametrize("space", monitor.SPACES)
@pytest.mark.parametrize("B,D", mc.LATENT_SHAPES)
def test_ppl_latents_kernel(B, D, space):
    pairs, t = mc.latent_inputs(B, D)
    want = mc.latents64(pairs, t, mc.t1_of(t, mc.EPS), space)
    composed = monitor.ppl_latents(torch.from_numpy(pairs), torch.from_numpy(t), mc.EPS, space).numpy()
    scale = np.abs(composed - want).max()
    assert scale > 0
    p, tt = torch.from_numpy(pairs).cuda(), torch.from_numpy(t).cuda()
    got = monitor.ppl_latents(p, tt, mc.EPS, space)
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"latents B={B} D={D} {space}: kernel error {err:.3e}, float32 composition {scale:.3e}, ratio {err / scale:.3f}")
    assert err <= 4 * scale
    again = monitor.ppl_latents(p, tt, mc.EPS, space)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    # rows that are not 16-byte aligned (a view one float into a buffer) and canaries around the output
    bufs = cb.Buffers()
    pin, tin = bufs.view("pairs", arr=pairs, shift=1), bufs.view("t", arr=t)
    out = bufs.view("out", like=pairs, shift=1)
    lib.check(lib.load().g2s_ppl_latents(lib.ptr(pin), lib.ptr(tin), mc.EPS, monitor.SPACES.index(space), lib.ptr(out),
                                         B, D, lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    assert np.abs(out.cpu().numpy().reshape(want.shape) - want).max() <= 4 * scale
    # both launches captured in one graph on a side stream: the replay gives the eager bits
    o1, o2 = torch.zeros_like(p), torch.zeros_like(p)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            monitor.ppl_latents(p, tt, mc.EPS, space, out=o1)
            monitor.ppl_latents(p, tt, mc.EPS, space, out=o2)
        graph.replay()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(o1.view(torch.int32), got.view(torch.int32)) and torch.equal(o2.view(torch.int32), got.view(torch.int32))


def test_image_grid_is_capturable():
    N, C, H, W, nrow, padding, pad_value = mc.GRID_SHAPES[3]
    x = torch.from_numpy(mc.grid_inputs(N, C, H, W)).cuda()
    eager = monitor.image_grid(x, nrow, padding, pad_value=pad_value)
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            monitor.image_grid(x, nrow, padding, pad_value=pad_value, out=out)
        graph.replay()
    side.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------ the path length
@pytest.fixture(scope="module")
def ppl_modules():
    """Per generator: the CPU float32 modules, their float64 copies and the device copies; one PerceptualLoss."""
    import copy
    percept = mc.ppl_percept()
    out = {"percept": (percept, copy.deepcopy(percept).double(), copy.deepcopy(percept).cuda())}
    for name in mc.PPL_GENERATORS:
        G = mc.ppl_generator(sg2, name)
        out[name] = (G, copy.deepcopy(G).double(), copy.deepcopy(G).cuda().eval().requires_grad_(False))
    return out


_reference = {}


def ppl_reference(modules, name, space, crop, eps):
    """(float64 oracle, float32 CPU route) distances of a case, computed once."""
    key = (name, space, crop, eps)
    if key not in _reference:
        G32, G64, _ = modules[name]
        p32, p64, _ = modules["percept"]
        draws = mc.ppl_draws(G32)
        oracle = mc.ppl_loop(G64, p64, draws, space, eps, crop)
        route = monitor.perceptual_path_length(G32, p32, mc.PPL_N, mc.PPL_BATCH, space, "full", eps, crop,
                                               draws=draws)["distances"]
        _reference[key] = (oracle, route)
    return _reference[key]


# crop leaves a quarter of the image: 8 x 8 of g16, which the LPIPS trunk (four pools) does not take; g32 covers it
PPL_CASES = [(name, space, crop, eps) for name in mc.PPL_GENERATORS for space in monitor.SPACES
             for crop in ((False, True) if name == "g32" else (False,)) for eps in (1e-2, 1e-4)]


@pytest.mark.parametrize("name,space,crop,eps", PPL_CASES)
def test_path_length_on_the_device(ppl_modules, name, space, crop, eps):
    oracle, route = ppl_reference(ppl_modules, name, space, crop, eps)
    scale = np.abs(route - oracle).max()
    rel = scale / np.abs(oracle).max()
    assert scale > 0 and (oracle > 0).all()
    if eps == 1e-4:
        assert rel < 0.1, f"the float32 route is {rel:.3f} off at eps = 1e-4: choose other seeds"
    G, percept = ppl_modules[name][2], ppl_modules["percept"][2]
    draws = mc.draws_to(mc.ppl_draws(ppl_modules[name][0]), device="cuda")
    r = monitor.perceptual_path_length(G, percept, mc.PPL_N, mc.PPL_BATCH, space, "full", eps, crop, draws=draws)
    err = np.abs(r["distances"] - oracle).max()
    print(f"ppl {name} {space} crop={crop} eps={eps:g}: device error {err:.3e}, float32 CPU route {scale:.3e} "
          f"({rel:.2e} relative), ratio {err / scale:.3f}")
    assert r["n"] == mc.PPL_N and (np.abs(r["distances"] - oracle) <= 8 * scale).all()
    assert r["ppl"] == mc.trimmed_mean64(r["distances"])[0]


def test_resize_table_against_interpolate():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 520, 520, generator=g)
    want = torch.nn.functional.interpolate(x.double(), size=256, mode="bilinear", align_corners=False)
    scale = (torch.nn.functional.interpolate(x, size=256, mode="bilinear", align_corners=False).double() - want).abs().max()
    yb, xb = monitor.ppl_resize_tables(520, False, "cuda")
    got = resample.resample_sep(x.cuda(), yb, xb)
    err = (got.cpu().double() - want).abs().max()
    print(f"resize 520 -> 256: kernel error {err:.3e}, float32 interpolate {scale:.3e}, ratio {err / scale:.3f}")
    assert tuple(got.shape) == (2, 3, 256, 256) and err <= 4 * scale
    assert torch.equal(monitor.ppl_images(x.cuda()), got)
    # with the crop: the table reads rows 3c .. 7c and columns 2c .. 6c of a 1024 image
    big = torch.randn(1, 3, 1024, 1024, generator=g)
    want = torch.nn.functional.interpolate(big[:, :, 384:896, 256:768].double(), size=256, mode="bilinear", align_corners=False)
    scale = (torch.nn.functional.interpolate(big[:, :, 384:896, 256:768], size=256, mode="bilinear",
                                             align_corners=False).double() - want).abs().max()
    err = (monitor.ppl_images(big.cuda(), crop=True).cpu().double() - want).abs().max()
    assert err <= 4 * scale


# ---------------------------------------------------------------------------------------------------------- train
@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("packed"))
    np.save(os.path.join(out, "8.npy"), dataprep_cases.packed_dataset(5, 8, seed=8))
    return out


def train_argv(packed, out, *more):
    return ["--size", "8", *mc.TRAIN_NET, "--data", packed, "--iter", "3", "--batch", "4", "--log-every", "0",
            "--mixing", "0", "--seed", "3", "--lr", "0.02", "--deterministic", "--out", out, *more]


def test_train_on_the_device_writes_the_grids_of_g_ema(packed, tmp_path, monkeypatch):
    """The PNG of iteration i is grid64 of the forward of a NEW generator holding g_ema's weights of iteration i (no
    value of these images lies within 2^-16 of a quantisation boundary, so the bytes are equal), and a run with
    monitoring on ends on the weights of a run without."""
    off, on = str(tmp_path / "off" / "train.pt"), str(tmp_path / "on" / "train.pt")
    states, images = mc.spy_on_monitor(monkeypatch, train)
    prev = lib.set_deterministic(False)
    try:
        train.main(train_argv(packed, off))
        train.main(train_argv(packed, on, "--sample-every", "1", "--n-sample", "4"))
    finally:
        lib.set_deterministic(prev)
    assert [i for i, _ in states] == [0, 1, 2] and len(images) == 3
    sample_z = torch.randn(4, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    fresh = []
    for (i, state), seen in zip(states, images):
        lib.set_deterministic(True)         # as the run was: the launch partitions, and with them the roundings, are its
        try:
            with torch.no_grad():
                fresh.append(mc.fresh_generator(sg2, 8, state, "cuda")([sample_z])[0])
        finally:
            lib.set_deterministic(prev)
        assert seen.is_cuda and tuple(seen.shape) == (4, 3, 8, 8)
        assert torch.equal(seen, fresh[-1]), f"iteration {i}: the monitored images are not those of the current g_ema"
        png = np.asarray(Image.open(os.path.join(os.path.dirname(on), "sample", "%06d.png" % i)))
        want, pre = mc.grid64(fresh[-1].cpu().numpy(), nrow=2)
        assert png.shape == (22, 22, 3) and mc.check_grid(png, want, pre, f"iteration {i}") == 0
        assert np.array_equal(png, want)
    assert not torch.equal(fresh[0], fresh[2])          # the run moved g_ema
    a, b = (torch.load(p, map_location="cpu", weights_only=True) for p in (off, on))
    for key in ("g", "d", "g_ema"):
        for k in a[key]:
            assert torch.equal(a[key][k], b[key][k]), (key, k)


def test_train_ppl_branch_on_the_device(tmp_path, monkeypatch):
    """--ppl-every on the device: every jsonl line is the path length of a NEW generator holding g_ema's weights of that
    iteration, over the same seeded pairs."""
    import json
    data = str(tmp_path / "packed16")
    os.makedirs(data)
    np.save(os.path.join(data, "16.npy"), dataprep_cases.packed_dataset(5, 16, seed=16))
    states, _ = mc.spy_on_monitor(monkeypatch, train)
    percept = mc.ppl_percept()
    out = str(tmp_path / "run" / "train.pt")
    prev = lib.set_deterministic(False)
    try:
        train.main(["--size", "16", *mc.TRAIN_NET, "--data", data, "--iter", "3", "--batch", "4", "--log-every", "0",
                    "--mixing", "0", "--seed", "3", "--lr", "0.02", "--deterministic", "--out", out,
                    "--ppl-every", "2", "--ppl-samples", "3"], percept=percept)
        lines = [json.loads(line) for line in open(os.path.join(os.path.dirname(out), "ppl.jsonl"))]
        assert [r["iter"] for r in lines] == [0, 2]
        for record, (i, state) in zip(lines, [states[0], states[2]]):
            G = mc.fresh_generator(sg2, 16, state, "cuda")
            g = torch.Generator(device="cuda").manual_seed(3)
            want = monitor.perceptual_path_length(G, percept.cuda(), 3, generator=g)
            assert record == {"iter": i, **{k: want[k] for k in ("ppl", "n", "kept", "lo", "hi")}}, i
    finally:
        lib.set_deterministic(prev)
    assert lines[0]["ppl"] != lines[1]["ppl"]
