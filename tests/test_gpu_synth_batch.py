"""-m gpu: the one-node generator with ONE NOISE MAP PER SAMPLE (synthesis.per_sample_noise) — its three entry points
against float64 and bit for bit against their shared-map siblings, the node against the reference's float64 run
(tests/golden/projector_batch.npz; bounds are 4 x the reference's own float32 error, as in test_gpu_projector.py) and
against the layer loop, and what is built on it: generate.sample(batched=True) and projector.project_batch."""
import numpy as np
import pytest
import torch

import projector_cases as pc
import projector_batch_cases as pb

pytestmark = pytest.mark.gpu

MARGIN = 4.0     # x the reference's own float32 error
ALPHA, GAIN = 0.2, 2 ** 0.5


@pytest.fixture(scope="module")
def L():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def fx(golden):
    return golden("projector_batch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def offset_by_one_float(t):
    """The same values at an address 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _lrelu64(pre):
    return GAIN * np.where(pre > 0, pre, pre * ALPHA)


# ----------------------------------------------------------------------------------------- (a) g2s_noise_bias_act_ps
def _nba_inputs(B, C, HW):
    rng = np.random.default_rng([B, C, HW])
    x = rng.standard_normal((B, C, HW)).astype(np.float32)
    noise = rng.standard_normal((B, HW)).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    # pre-activations that are exactly 0 (noise 0, x = -bias: x + nw * 0 + bias == 0 in any order) and negative ones
    noise[:, 1] = 0.0
    x[:, :, 1] = -bias[None, :]
    x[:, :, 2] = -4.0
    return x, noise, bias


@pytest.mark.parametrize("B,C,HW,unaligned", [(2, 3, 16, False), (3, 5, 25, False), (2, 1, 4, False), (1, 4, 64, False),
                                               (2, 3, 16, True)])
def test_noise_bias_act_ps_against_float64(L, B, C, HW, unaligned):
    """y = gain * lrelu(x + noise_w * noise[b] + bias[c]) against the expression in numpy float64 under
    test_noise_bias_act's tolerance (rtol 1e-6, atol 1e-6).  HW = 16, 4, 64: 16-byte accesses; 25: the scalar path;
    `unaligned`: a vector-eligible shape at a pointer one float past alignment, which must take the scalar path (for
    x and y, and for the maps).  In place as well."""
    from gan2shape_amd import lib
    x, noise, bias = _nba_inputs(B, C, HW)
    nw = -0.37
    pre = x.astype(np.float64) + np.float64(np.float32(nw)) * noise.astype(np.float64)[:, None] + bias.astype(np.float64)[None, :, None]
    exp = _lrelu64(pre)
    assert (pre == 0).any() and (pre < 0).any()
    xd, nd, bd, nwd = dev(x), dev(noise), dev(bias), dev([nw])
    variants = [(xd, nd)] if not unaligned else [(offset_by_one_float(xd), nd), (xd, offset_by_one_float(nd))]
    for xv, nv in variants:
        y = offset_by_one_float(torch.full_like(xd, float("nan"))) if xv.data_ptr() % 16 else torch.full_like(xd, float("nan"))
        lib.check(L.g2s_noise_bias_act_ps(lib.ptr(xv), lib.ptr(nv), lib.ptr(nwd), lib.ptr(bd), lib.ptr(y), B, C, HW,
                                          ALPHA, GAIN, lib.stream()))
        err = float(np.abs(y.double().cpu().numpy() - exp).max())
        print(f"[noise_bias_act_ps B {B} C {C} HW {HW} unaligned {unaligned}] max |err| {err:.2e}")
        np.testing.assert_allclose(y.double().cpu().numpy(), exp, rtol=1e-6, atol=1e-6)
        if B > 1:
            assert not torch.equal(y[0], y[1])
        inplace = xv.clone() if not xv.data_ptr() % 16 else offset_by_one_float(xv)
        lib.check(L.g2s_noise_bias_act_ps(lib.ptr(inplace), lib.ptr(nv), lib.ptr(nwd), lib.ptr(bd), lib.ptr(inplace), B, C,
                                          HW, ALPHA, GAIN, lib.stream()))
        assert torch.equal(inplace, y)


def test_noise_bias_act_ps_a_sample_reads_its_own_map(L):
    """The same x for every sample: the results differ only through the maps, and sample b equals the shared-map entry
    given map b."""
    from gan2shape_amd import lib
    B, C, HW = 3, 5, 64
    x, noise, bias = _nba_inputs(B, C, HW)
    x[:] = x[0]
    xd, nd, bd, nwd = dev(x), dev(noise), dev(bias), dev([0.8])
    y = torch.empty_like(xd)
    lib.check(L.g2s_noise_bias_act_ps(lib.ptr(xd), lib.ptr(nd), lib.ptr(nwd), lib.ptr(bd), lib.ptr(y), B, C, HW, ALPHA, GAIN,
                                      lib.stream()))
    for b in range(B):
        one = torch.empty_like(xd[0])
        lib.check(L.g2s_noise_bias_act(lib.ptr(xd[b]), lib.ptr(nd[b]), lib.ptr(nwd), lib.ptr(bd), lib.ptr(one), 1, C, HW,
                                       ALPHA, GAIN, lib.stream()))
        assert torch.equal(y[b], one), b
    assert not torch.equal(y[0], y[1]) and not torch.equal(y[1], y[2])


# ------------------------------------------------------------------------------------------ (b) g2s_upfirdn2d_nba_ps
def _blur_inputs(B, C, H):
    from gan2shape_amd import stylegan2 as sg2
    rng = np.random.default_rng([7, B, C, H])
    x = rng.standard_normal((B, C, H, H)).astype(np.float32)
    k = (sg2.make_kernel([1, 3, 3, 1]) * 4).numpy().astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    oh = H + 2 - 4 + 1
    noise = rng.standard_normal((B, oh, oh)).astype(np.float32)
    return x, k, bias, noise, oh


def _blur_ps(L, xd, kd, bd, nd, nwd, B, C, H, oh):
    from gan2shape_amd import lib
    y = torch.full((B, C, oh, oh), float("nan"), device="cuda")
    lib.check(L.g2s_upfirdn2d_nba_ps(lib.ptr(xd), lib.ptr(kd), lib.ptr(y), B * C, C, H, H, 4, 4, 1, 1, 1, 1, 1, 1,
                                     lib.ptr(bd), lib.ptr(nd), lib.ptr(nwd), ALPHA, GAIN, lib.stream()))
    return y


@pytest.mark.parametrize("B,C,H", [(2, 3, 9), (3, 5, 17), (2, 8, 35)])
def test_blur_tail_ps_against_the_oracle(L, B, C, H):
    """g2s_upfirdn2d_nba_ps (the Blur of an up-sampling StyledConv, kernel [1,3,3,1] x 4, pad (1, 1)) against the C
    oracle's upfirdn2d and the tail in float64 with one map per sample, under test_blur_with_the_styledconv_tail_vs_
    oracle's tolerance (rtol 1e-5, atol 2e-6).  Output sides 8, 16 and 34: one 32 x 32 tile, and a second tile column
    and row with a two-wide tail."""
    from oracle import capi
    x, k, bias, noise, oh = _blur_inputs(B, C, H)
    nw = -0.8
    pre = capi.upfirdn2d(x, k, (1, 1), (1, 1), (1, 1, 1, 1)).astype(np.float64)
    assert pre.shape == (B, C, oh, oh)
    exp = _lrelu64(pre + bias.astype(np.float64)[None, :, None, None] + np.float64(np.float32(nw)) * noise.astype(np.float64)[:, None])
    y = _blur_ps(L, dev(x), dev(k), dev(bias), dev(noise), dev([nw]), B, C, H, oh)
    print(f"[upfirdn2d_nba_ps B {B} C {C} H {H}] max |err| {float(np.abs(y.double().cpu().numpy() - exp).max()):.2e}")
    np.testing.assert_allclose(y.double().cpu().numpy(), exp, rtol=1e-5, atol=2e-6)
    assert not torch.equal(y[0], y[1])


# ----------------------------------------------------------------------------------------- (c) g2s_synth_bwd_rows_ps
def _rows_inputs(B, C, H, per_sample=True):
    g = torch.Generator().manual_seed(B * 100 + C * 10 + H)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)       # noqa: E731
    slope, gain, nw = 0.2, 2 ** 0.5, 0.6
    yconv = r(B, C, H, H)
    noise, bias = r(B if per_sample else 1, 1, H, H), r(C)
    pre = yconv + nw * noise + bias.view(1, C, 1, 1)
    x = torch.where(pre > 0, pre, pre * slope) * gain
    g1, g2 = r(B, C, H, H), r(B, C, H, H)
    s1, s2, demod = r(B, C), r(B, C), 0.5 + torch.rand(B, C, dtype=torch.float64, generator=g)
    return dict(yconv=yconv, noise=noise, bias=bias, x=x, g1=g1, g2=g2, s1=s1, s2=s2, demod=demod, slope=slope, gain=gain,
                nw=nw)


def _rows_call(L, entry, t, B, C, H, two, with_gdot, noise):
    from gan2shape_amd import lib
    f = lambda v: v.float().cuda().contiguous()      # noqa: E731
    keep = [f(t[k]) for k in ("x", "g1", "s1", "g2", "s2")] + [f(noise), f(torch.tensor([t["nw"]])), f(t["bias"]), f(t["demod"])]
    xd, g1d, s1d, g2d, s2d, nzd, nwd, bd, dmd = keep
    out = torch.full_like(xd, float("nan"))
    dot1, dot2, gdot = (torch.full((B, C), float("nan"), device="cuda") for _ in range(3))
    lib.check(entry(lib.ptr(xd), lib.ptr(g1d), lib.ptr(s1d), lib.ptr(g2d if two else None), lib.ptr(s2d if two else None),
                    lib.ptr(nzd), lib.ptr(nwd), lib.ptr(bd), lib.ptr(dmd), lib.ptr(out), lib.ptr(dot1),
                    lib.ptr(dot2 if two else None), lib.ptr(gdot if with_gdot else None), B * C, C, H * H, t["slope"],
                    t["gain"], lib.stream()))
    torch.cuda.synchronize()
    return out, dot1, dot2 if two else None, gdot if with_gdot else None


@pytest.mark.parametrize("B,C,H,two,with_gdot", [(3, 5, 4, False, True), (2, 7, 9, True, True), (2, 7, 9, True, False),
                                                 (2, 4, 5, False, True)])
def test_synth_bwd_rows_ps_against_float64(L, B, C, H, two, with_gdot):
    """g2s_synth_bwd_rows_ps against the float64 chain of test_synth_bwd_rows_vs_float64 with one map per sample, under
    its bounds: out 2e-6 of max; dots rtol 1e-4, atol 2e-5 sqrt(n); gdot rtol 1e-4, atol 1e-4 sqrt(n).  n = 16: 16-byte
    loads; 81 and 25: the scalar path.  Both modes of g2s_set_deterministic give the same bits."""
    from gan2shape_amd import lib
    t = _rows_inputs(B, C, H)
    x, g1, g2, gain, slope = t["x"], t["g1"], t["g2"], t["gain"], t["slope"]
    joined = g1 * t["s1"][:, :, None, None] + (g2 * t["s2"][:, :, None, None] if two else 0)
    out_ref = joined * torch.where(x > 0, gain, gain * slope)
    prev = lib.set_deterministic(True)
    try:
        out, dot1, dot2, gdot = _rows_call(L, L.g2s_synth_bwd_rows_ps, t, B, C, H, two, with_gdot, t["noise"])
        lib.set_deterministic(False)
        other = _rows_call(L, L.g2s_synth_bwd_rows_ps, t, B, C, H, two, with_gdot, t["noise"])
    finally:
        lib.set_deterministic(prev)
    for a, b in zip((out, dot1, dot2, gdot), other):
        assert (a is None and b is None) or torch.equal(a, b)
    n = H * H
    assert float((out.double().cpu() - out_ref).abs().max()) <= 2e-6 * float(out_ref.abs().max())
    np.testing.assert_allclose(dot1.double().cpu().numpy(), (x * g1).sum((2, 3)).numpy(), rtol=1e-4, atol=2e-5 * n ** 0.5)
    if two:
        np.testing.assert_allclose(dot2.double().cpu().numpy(), (x * g2).sum((2, 3)).numpy(), rtol=1e-4, atol=2e-5 * n ** 0.5)
    if with_gdot:
        ref = (out_ref * t["yconv"]).sum((2, 3)) / t["demod"]
        print(f"[synth_bwd_rows_ps B {B} C {C} H {H}] gdot max |err| {float((gdot.double().cpu() - ref).abs().max()):.2e}")
        np.testing.assert_allclose(gdot.double().cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4 * n ** 0.5)
        assert not torch.equal(gdot[0], gdot[1])
        # a kernel that reads the first map for every sample gives another gdot for samples 1..: the float64 chain
        # with map 0 everywhere is out of the bound
        wrong = (out_ref * (t["yconv"] + t["nw"] * (t["noise"] - t["noise"][:1]))).sum((2, 3)) / t["demod"]
        assert float((wrong - ref)[1:].abs().max()) > 10 * (1e-4 * n ** 0.5)
    else:
        assert not torch.equal(out[0], out[1])


# -------------------------------------------------------------------------- bit identity with the shared-map entries
def test_ps_entries_with_equal_maps_give_the_shared_map_entries_bits(L):
    """B copies of one map: each _ps entry equals its sibling under torch.equal — vector and scalar path of (a) and (c),
    two tile columns of (b)."""
    from gan2shape_amd import lib
    for B, C, HW in ((3, 5, 64), (2, 3, 25)):
        x, noise, bias = _nba_inputs(B, C, HW)
        xd, bd, nwd = dev(x), dev(bias), dev([-0.37])
        one = dev(noise[0])
        many = one[None].repeat(B, 1).contiguous()
        y0, y1 = torch.empty_like(xd), torch.empty_like(xd)
        lib.check(L.g2s_noise_bias_act(lib.ptr(xd), lib.ptr(one), lib.ptr(nwd), lib.ptr(bd), lib.ptr(y0), B, C, HW, ALPHA, GAIN,
                                       lib.stream()))
        lib.check(L.g2s_noise_bias_act_ps(lib.ptr(xd), lib.ptr(many), lib.ptr(nwd), lib.ptr(bd), lib.ptr(y1), B, C, HW, ALPHA,
                                          GAIN, lib.stream()))
        assert torch.equal(y0, y1), (B, C, HW)
    B, C, H = 2, 8, 35
    x, k, bias, noise, oh = _blur_inputs(B, C, H)
    xd, kd, bd, nwd = dev(x), dev(k), dev(bias), dev([-0.8])
    one = dev(noise[0])
    y0 = torch.empty((B, C, oh, oh), device="cuda")
    lib.check(L.g2s_upfirdn2d_nba(lib.ptr(xd), lib.ptr(kd), lib.ptr(y0), B * C, C, H, H, 4, 4, 1, 1, 1, 1, 1, 1, lib.ptr(bd),
                                  lib.ptr(one), lib.ptr(nwd), ALPHA, GAIN, lib.stream()))
    y1 = _blur_ps(L, xd, kd, bd, one[None].repeat(B, 1, 1).contiguous(), nwd, B, C, H, oh)
    assert torch.equal(y0, y1)
    for B, C, H in ((3, 5, 4), (2, 7, 9)):
        t = _rows_inputs(B, C, H, per_sample=False)
        shared = _rows_call(L, L.g2s_synth_bwd_rows, t, B, C, H, True, True, t["noise"])
        copies = _rows_call(L, L.g2s_synth_bwd_rows_ps, t, B, C, H, True, True, t["noise"].repeat(B, 1, 1, 1))
        assert all(torch.equal(a, b) for a, b in zip(shared, copies)), (B, C, H)


# ------------------------------------------------------------------------------------------------------- the node
def _agree(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    return float((a - ref).norm() / ref.norm()), float((a * ref).sum() / (a.norm() * ref.norm()))


@pytest.fixture(scope="module")
def G16(L):
    from gan2shape_amd import stylegan2 as sg2
    return pc.fixture_generator(sg2).cuda()


class _count_synthesize:
    """Counts the entries of synthesis.synthesize and records what eligible answered."""

    def __enter__(self):
        from gan2shape_amd import synthesis
        self.mod, self.calls, self.answers = synthesis, [], []
        self.synthesize, self.eligible = synthesis.synthesize, synthesis.eligible
        synthesis.synthesize = lambda *a: self.calls.append(1) or self.synthesize(*a)
        synthesis.eligible = lambda *a: self.answers.append(self.eligible(*a)) or self.answers[-1]
        return self

    def __exit__(self, *exc):
        self.mod.synthesize, self.mod.eligible = self.synthesize, self.eligible


def _run(G, latent, maps, gy, one_node=True, switch=True, mask=None):
    """(image, [latent gradient, map gradients]) of sum(image * gy)."""
    from gan2shape_amd import stylegan2 as sg2, synthesis
    lat = latent.clone().requires_grad_(True)
    nz = [m.clone().requires_grad_(mask is None or mask[i]) for i, m in enumerate(maps)]
    try:
        sg2.Generator.ONE_NODE = one_node
        with synthesis.per_sample_noise(switch):
            img, _ = G([lat], input_is_w=True, noise=nz)
    finally:
        sg2.Generator.ONE_NODE = True
    img.backward(gy)                                # outside the block: backward follows what forward recorded
    return img.detach(), [lat.grad] + [n.grad for n in nz]


@pytest.mark.parametrize("mode", pb.MODES)
def test_node_with_per_sample_maps_against_the_reference_float64(G16, fx, mode):
    """Size-16 generator of the fixture, B = 3, per-sample maps of sides 4, 8, 8, 16, 16 on the one-node path: image,
    latent gradient and every map gradient against the reference's float64 run, each within 4 x the reference's own
    float32 error; and against the layer loop on the same inputs under test_gpu_projector.py's bounds (image 2e-6 of
    max; gradients rel <= 1.5e-3, cosine >= 0.999999)."""
    w, noises, gy = pb.generator_inputs(mode)
    w, maps, gy = dev(w), [dev(n) for n in noises], dev(gy)
    with _count_synthesize() as c:
        img, grads = _run(G16, w, maps, gy)
    assert c.calls == [1] and c.answers == [True]
    keys = pb.generator_keys()
    for key, a in zip(keys, [img] + grads):
        ref = torch.from_numpy(fx[f"g16b.{mode}.{key}"]).cuda()
        assert a.shape == ref.shape, key
        e = float((a.double() - ref).abs().max() / ref.abs().max()) if key == "img" else pc.l2_rel(a, ref)
        allowed = MARGIN * float(fx[f"g16b.{mode}.ref_fp32_err.{key}"])
        print(f"[G(16) B 3 per-sample, {mode}] {key} {e:.2e} / {allowed:.2e}")
        assert e <= allowed, key
    img0, grads0 = _run(G16, w, maps, gy, one_node=False)
    e_img = float((img - img0).abs().max() / img0.abs().max())
    print(f"[G(16) B 3 per-sample, {mode}] vs the layer loop: image {e_img:.2e}")
    assert e_img <= 2e-6
    for key, a, b in zip(keys[1:], grads, grads0):
        rel, cos = _agree(a, b)
        print(f"    {key}: rel {rel:.2e} cosine {cos:.9f}")
        assert a.shape == b.shape and rel <= 1.5e-3 and cos >= 0.999999, key


def test_node_is_entered_once_for_the_batch_under_the_switch(G16):
    """With the switch on the per-sample call is ONE synthesize and eligible says True (on the parent commit eligible
    refuses [B > 1, 1, H, W] maps and there is no switch); with it off — the default — the same call takes the layer
    loop and synthesize is not entered."""
    from gan2shape_amd import synthesis
    w, noises, _ = pb.generator_inputs("w")
    w, maps = dev(w), [dev(n) for n in noises]
    assert synthesis.PER_SAMPLE is False
    with torch.no_grad():
        with _count_synthesize() as c:
            with synthesis.per_sample_noise():
                assert synthesis.PER_SAMPLE is True
                on, _ = G16([w], input_is_w=True, noise=maps)
            assert synthesis.PER_SAMPLE is False
        assert c.calls == [1] and c.answers == [True]
        with _count_synthesize() as c:
            off, _ = G16([w], input_is_w=True, noise=maps)
        assert c.calls == [] and c.answers == [False]
    assert float((on - off).abs().max()) <= 2e-6 * float(off.abs().max())
    assert float((on[0] - on[1]).abs().max()) > 1e-3 * float(off.abs().max())


def test_map_gradient_is_per_sample(G16):
    """A map's gradient is [B, 1, s, s], and row b changes when only sample b's cotangent changes: the rows of the other
    samples stay, row 1 moves by more than a tenth of the gradient's maximum.  In deterministic mode, where every sum
    has one order: a row of another sample is then the same instructions on the same data, so it is held to 1e-6 of the
    maximum (nothing of sample 1 is summed into it).  Outside that mode the split sums of the data-gradient convolutions
    change their order from run to run, and these gradients — differences of large terms — move by 1e-4 .. 1e-3 of
    their maximum between two runs on the SAME inputs, which would hide what this test looks for."""
    from gan2shape_amd import lib
    w, noises, gy = pb.generator_inputs("w")
    w, maps, gy = dev(w), [dev(n) for n in noises], dev(gy)
    gy2 = gy.clone()
    gy2[1] = gy2[1] * -0.5 + 0.25
    prev = lib.set_deterministic(True)
    try:
        _, g_a = _run(G16, w, maps, gy)
        _, g_b = _run(G16, w, maps, gy2)
    finally:
        lib.set_deterministic(prev)
    for m, a, b in zip(maps, g_a[1:], g_b[1:]):
        assert a.shape == m.shape == b.shape
        top = float(a.abs().max())
        moved = [float((a[i] - b[i]).abs().max()) / top for i in range(3)]
        print(f"[map gradient rows, side {m.shape[-1]}] moved {moved}")
        assert moved[0] <= 1e-6 and moved[2] <= 1e-6 and moved[1] > 0.1, moved


def test_mixed_shared_and_per_sample_maps(G16):
    """Maps 1 and 4 shared ([1, 1, s, s]: the fused epilogues), the others per sample, one of them without a gradient:
    the layer loop's image and gradients within the same bounds; a shared map's gradient is [1, 1, s, s]."""
    w, noises, gy = pb.generator_inputs("wp")
    w, gy = dev(w), dev(gy)
    maps = [dev(n[:1] if i in (1, 4) else n) for i, n in enumerate(noises)]
    mask = [i != 2 for i in range(len(maps))]
    with _count_synthesize() as c:
        img, grads = _run(G16, w, maps, gy, mask=mask)
    assert c.calls == [1]
    img0, grads0 = _run(G16, w, maps, gy, one_node=False, mask=mask)
    assert float((img - img0).abs().max()) <= 2e-6 * float(img0.abs().max())
    assert grads[3] is None and grads0[3] is None
    for i, (a, b) in enumerate(zip(grads, grads0)):
        if a is None:
            continue
        rel, cos = _agree(a, b)
        print(f"[mixed maps] input {i}: rel {rel:.2e} cosine {cos:.9f}")
        assert a.shape == b.shape and rel <= 1.5e-3 and cos >= 0.999999, i
    assert grads[2].shape == (1, 1, 8, 8) and grads[1].shape == (3, 1, 4, 4)


def test_node_with_per_sample_maps_is_deterministic(G16):
    from gan2shape_amd import lib
    w, noises, gy = pb.generator_inputs("wp")
    w, maps, gy = dev(w), [dev(n) for n in noises], dev(gy)
    prev = lib.set_deterministic(True)
    try:
        img1, g1 = _run(G16, w, maps, gy)
        img2, g2 = _run(G16, w, maps, gy)
    finally:
        lib.set_deterministic(prev)
    assert torch.equal(img1, img2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


# ----------------------------------------------------------------------------------------------------- sample
def test_batched_sample_is_one_forward_with_the_same_draws(G16):
    """n = 3 with fixed draws: batched=True is ONE Generator.forward on the one-node path; its images are within 2e-6 of
    max of the layer loop on the same draws and of batched=False (one forward per sample); w is the same tensor bit
    for bit."""
    from gan2shape_amd import generate, stylegan2 as sg2
    gen = torch.Generator(device="cuda").manual_seed(9)
    draws = generate.draw(G16, 3, gen)
    with _count_synthesize() as c:
        img_b, w_b = generate.sample(G16, 3, draws=draws, batched=True)
    assert c.calls == [1]
    with _count_synthesize() as c:
        img_s, w_s = generate.sample(G16, 3, draws=draws)
    assert c.calls == [1, 1, 1]
    try:
        sg2.Generator.ONE_NODE = False
        with torch.no_grad():
            loop, _ = G16([w_b], input_is_w=True, noise=list(draws[1]))
    finally:
        sg2.Generator.ONE_NODE = True
    top = float(loop.abs().max())
    assert img_b.shape == (3, 3, 16, 16) and torch.equal(w_b, w_s)
    assert float((img_b - loop).abs().max()) <= 2e-6 * top
    assert float((img_b - img_s).abs().max()) <= 2e-6 * top
    assert float((img_b[0] - img_b[1]).abs().max()) > 1e-3 * top


# ------------------------------------------------------------------------------------------------ project_batch
def _percept():
    """LPIPS with a seeded random trunk (no pretrained weights offline) and non-negative `lin` weights: a distance —
    as test_gpu_projector.py builds it."""
    from gan2shape_amd.lpips import PerceptualLoss
    torch.manual_seed(7)
    p = PerceptualLoss()
    with torch.no_grad():
        for k in range(5):
            getattr(p.net, f"lin{k}").model[-1].weight.abs_()
    return p.cuda()


@pytest.fixture(scope="module")
def G16wide(L):
    """Size 16 with the checkpoint's style_dim 512 and 8 mapping layers, as the projector tests of test_gpu_projector.py."""
    from gan2shape_amd import stylegan2 as sg2
    return pc.fixture_generator(sg2, size=16, style_dim=512, n_mlp=8, seed=77).cuda()


def test_one_batched_projector_step_against_the_op_by_op_step(G16wide):
    """Step 0 of project_batch at G(16), B = 2 (jitter strength 0): loss, latent gradient and every map gradient of the
    fused form (one node with per-sample maps, g2s_noise_regularize) against the op-by-op form (ONE_NODE off, the torch
    noise functions of tests/projector_cases.py), under test_one_projector_step_against_the_op_by_op_step's bounds:
    loss 1e-5; gradients rel <= 1.5e-3, cosine >= 0.999999."""
    from gan2shape_amd import projector, stylegan2 as sg2, synthesis
    G = G16wide
    percept = _percept()
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        target, _ = G([(0.5 * torch.randn(2, 512, generator=g)).cuda()], input_is_w=True)
    latent0 = (0.1 * torch.randn(2, 512, generator=g)).cuda()
    noises0 = [torch.randn(2, 1, s, s, generator=g).cuda() for s in pb.SIDES]
    projector.noise_normalize_(noises0)
    res = {}
    try:
        for fused in (True, False):
            sg2.Generator.ONE_NODE = fused
            leaf = latent0.clone().requires_grad_(True)
            lat = projector.latent_noise(leaf, 0.0)
            nz = [n.clone().requires_grad_(True) for n in noises0]
            reg = projector.noise_regularize(nz) if fused else pc.noise_regularize(nz)
            with _count_synthesize() as c, synthesis.per_sample_noise():
                img = projector._generate(G, lat, nz)
            assert c.calls == ([1] if fused else [])
            loss = percept(img, target).sum() + 1e5 * reg
            res[fused] = (loss.detach(), torch.autograd.grad(loss, [leaf] + nz))
    finally:
        sg2.Generator.ONE_NODE = True
    (l1, g1), (l0, g0) = res[True], res[False]
    e_loss = abs(float(l1) - float(l0)) / abs(float(l0))
    print(f"[batched projector step 0] loss {float(l1):.6e} vs {float(l0):.6e}: rel {e_loss:.2e}")
    assert e_loss <= 1e-5
    for i, (a, b) in enumerate(zip(g1, g0)):
        rel, cos = _agree(a, b)
        print(f"    {'latent' if i == 0 else f'map {i - 1}'}: rel {rel:.2e} cosine {cos:.9f}")
        assert a.shape == b.shape and rel <= 1.5e-3 and cos >= 0.999999, i


def test_batched_projection_lowers_its_loss(G16wide):
    """Five steps at G(16), B = 2, targets G(mean + 0.5 randn): the perceptual term of the un-jittered result is below
    that of the start (mean latent, the maps project_batch draws first); shapes carry the leading B; the maps end
    normalised over the batch; the generator ran as one node per step."""
    from gan2shape_amd import projector
    G = G16wide
    percept = _percept()
    gen = torch.Generator(device="cuda").manual_seed(5)
    stats = projector.mean_latent_stats(G, n=2000, generator=gen)
    with torch.no_grad():
        target, _ = G([stats[0][None] + 0.5 * torch.randn(2, 512, device="cuda", generator=gen)], input_is_w=True)
    state = gen.get_state()
    start = [torch.empty(2, 1, s, s, device="cuda").normal_(generator=gen) for s in pb.SIDES]
    before = float(projector.evaluate(G, percept, target, stats[0][None].repeat(2, 1), start))
    gen.set_state(state)
    with _count_synthesize() as c:
        res = projector.project_batch(G, percept, target, steps=5, latent_stats=stats, generator=gen)
    assert c.calls == [1] * 6 and all(c.answers)                   # five steps and the final image
    after = float(projector.evaluate(G, percept, target, res["latent"], res["noise"]))
    print(f"[batched projection G(16), B 2, 5 steps] perceptual {before:.5f} -> {after:.5f}")
    assert np.isfinite(after) and after < before
    assert res["latent"].shape == (2, 512) and res["img"].shape == (2, 3, 16, 16) and res["history"] == []
    assert [tuple(n.shape) for n in res["noise"]] == [(2, 1, s, s) for s in pb.SIDES]
    for n in res["noise"]:
        d = n.double()
        assert abs(float(d.mean())) <= 1e-5 and abs(float(d.std()) - 1) <= 1e-5
    single = projector.split_projection(res)
    assert len(single) == 2 and single[1]["latent"].shape == (512,) and single[1]["noise"][3].shape == (1, 1, 16, 16)
    assert torch.equal(single[1]["img"][0], res["img"][1])


@pytest.mark.parametrize("w_plus", [False, True])
def test_project_batch_of_one_equals_project_bit_for_bit(G16wide, w_plus):
    """B = 1 with the same seeded torch.Generator: the draws, their order and shapes are project's, and in deterministic
    mode so is every bit of the result."""
    from gan2shape_amd import lib, projector
    G = G16wide
    percept = _percept()
    gen = torch.Generator(device="cuda").manual_seed(11)
    stats = projector.mean_latent_stats(G, n=500, generator=gen)
    with torch.no_grad():
        target, _ = G([stats[0][None] + 0.5 * torch.randn(1, 512, device="cuda", generator=gen)], input_is_w=True)
    state = gen.get_state()
    prev = lib.set_deterministic(True)
    try:
        one = projector.project(G, percept, target, steps=3, mse=0.1, w_plus=w_plus, latent_stats=stats, generator=gen)
        gen.set_state(state)
        many = projector.project_batch(G, percept, target, steps=3, mse=0.1, w_plus=w_plus, latent_stats=stats, generator=gen)
    finally:
        lib.set_deterministic(prev)
    assert many["latent"].shape == (1,) + tuple(one["latent"].shape)
    assert torch.equal(many["latent"][0], one["latent"]) and torch.equal(many["img"], one["img"])
    assert all(torch.equal(a, b) for a, b in zip(many["noise"], one["noise"]))
