"""CPU side of the lit renderer (Renderer.render / lit render_rgb): properties of the float64 restatement the GPU
tests of test_gpu_render_full.py compare against, the conditioning of their cases, and the plugin's argument
check that needs no GPU.

Conditioning.  The light has a kink at dot(n, direction) = 0 and the normalisation a clamp at |cross| = 1e-5;
the comparisons want every face at least 1e-4 from the first and |cross| >= 1e-4.  Figures of the float64
restatement (scale, min |dot| under the direction the case uses, min |cross|):

    (16, 2, 3, True, True)     1    3.64e-3    1.216e-4
    (20, 2, 3, True, False)    2    2.27e-3    2.900e-4    (7.250e-5 at scale 1: 4.2 % of the faces below 1e-4)
    (12, 2, 3, False, True)    1    6.15e-3    2.167e-4
    (16, 1, 3, True, True)     1    1.96e-3    1.208e-4

|cross| does not depend on the light: the scene of make_case has a 10 degree field of view at depth 1, so a flat face
of the S = 20 grid has |cross| = (2 tan 5deg / 19)^2 = 8.5e-5, under the threshold for every direction.  That case's
camera-space vertices are therefore used at twice their size (render_full_cases.SCALES; exact in fp32, same
projection, same winners), chosen like the direction: on the CPU, from the restatement alone."""
import numpy as np
import pytest
import torch

from render_full_cases import (AMBIENT, BG, CA, CASES, DIRECTIONAL, IA, MIN_CROSS, MIN_DOT, conditioning, light, lit_case,
                               restate_lit)
from test_gpu_render_rgb_grad import restate


def _winners(d):
    """Winners for a CPU-only property: any fixed map will do; the oracle's float64 rasterization is at hand."""
    from oracle import capi
    from test_gpu_render_rgb_grad import FAR, NEAR
    maps = capi.render_depth(d["verts"], d["faces"], d["S"], d["K"], fill_back=d["fill_back"], near=NEAR, far=FAR,
                             dtype=np.float64)
    assert (maps["face_idx"] >= 0).mean() > 0.1
    return maps["face_idx"]


@pytest.mark.parametrize("key", CASES, ids=str)
def test_cases_are_well_conditioned(key):
    d = lit_case(key)
    dot, cross = conditioning(d["verts"], d["faces"], d["direction"])
    print(f"conditioning {key}: scale {d['scale']}  direction {d['direction']}  min |dot| {dot:.3e}  "
          f"min |cross| {cross:.3e}")
    assert dot >= MIN_DOT
    assert cross >= MIN_CROSS


@pytest.mark.parametrize("key", CASES, ids=str)
def test_ambient_only_light_is_a_colour_scale(key):
    """id = 0: every face's light is ia * ca, so the lit rendering is ia * ca * (the unlit one) on covered samples
    and the plain background elsewhere."""
    d = lit_case(key)
    fidx = _winners(d)
    v = torch.tensor(d["verts"], dtype=torch.float64)
    t = torch.tensor(d["tex"], dtype=torch.float64)
    lit = restate_lit(v, d["faces"], t, fidx, d["S"], d["K"], d["fill_back"], AMBIENT, (0.0, 0.0, 0.0), d["direction"])
    zero = (0.0, 0.0, 0.0)
    scale = torch.tensor([IA * c for c in CA], dtype=torch.float64)[None, :, None, None]
    want = scale * restate(v, d["faces"], t, fidx, d["S"], d["K"], background=zero) \
        + restate(v, d["faces"], torch.zeros_like(t), fidx, d["S"], d["K"], background=BG)
    assert float((lit - want).abs().max()) <= 1e-12
    # with a black background the statement needs no second term
    lit0 = restate_lit(v, d["faces"], t, fidx, d["S"], d["K"], d["fill_back"], AMBIENT, zero, d["direction"],
                       background=zero)
    assert float((lit0 - scale * restate(v, d["faces"], t, fidx, d["S"], d["K"], background=zero)).abs().max()) <= 1e-12


def test_reversing_a_face_negates_its_normal():
    d = lit_case(CASES[0])
    v = torch.tensor(d["verts"], dtype=torch.float64)
    faces = np.asarray(d["faces"])
    lt, dot, _ = light(v, faces, True, AMBIENT, DIRECTIONAL, d["direction"])
    lt_r, dot_r, _ = light(v, faces[:, ::-1].copy(), True, AMBIENT, DIRECTIONAL, d["direction"])
    F = faces.shape[0]
    assert float((dot + dot_r).abs().max()) <= 1e-15
    # hence the reversed list's front copies are lit like this list's reversed copies, and vice versa
    assert float((lt_r[:, :F] - lt[:, F:]).abs().max()) <= 1e-15
    assert float((lt_r[:, F:] - lt[:, :F]).abs().max()) <= 1e-15
    assert bool(((dot > 0) != (dot_r > 0)).all())


def test_lit_single_channel_textures_are_refused():
    """A light has three colour channels: C = 1 with a directional light (or a coloured ambient one) is a
    ValueError before anything touches the GPU."""
    from gan2shape_amd.plugins import neural_renderer as nr
    S = 4
    K = torch.eye(3)[None]
    verts = torch.zeros(1, S * S, 3)
    tex = torch.zeros(1, 2 * (S - 1) ** 2, 2, 2, 2, 1)
    for kw in (dict(light_intensity_directional=0.5), dict(light_intensity_directional=0.0, light_color_ambient=[1, 0, 0])):
        r = nr.Renderer(camera_mode='projection', K=K, image_size=S, orig_size=S, **kw)
        with pytest.raises(ValueError, match="3 colour channels"):
            r.render_rgb(verts, None, tex)
        with pytest.raises(ValueError, match="3 colour channels"):
            r.render(verts, None, tex)


def test_entry_points_check_their_arguments_before_any_launch():
    """include/g2s.h: a bad argument is G2S_ERR_INVALID (-1) with its message and nothing is launched (the pointers
    here are not device memory)."""
    import ctypes as C
    from gan2shape_amd import lib
    L = lib.load()
    one = C.c_void_p(256)
    f3 = (C.c_float * 3)(0, 0, 1)
    K = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    # light with C != 3, forward and backward
    assert L.g2s_raster_rgba_fwd(one, None, one, one, one, one, 1, 16, 18, 4, 2, 2, 1, 1, f3, 1e-3, one, None, None) == -1
    assert "a light factor needs 3 channels" in L.g2s_last_error().decode()
    assert L.g2s_raster_rgba_bwd(one, None, one, one, one, one, one, 1, 16, 18, 4, K, 4.0, 2, 2, 4, 1, 1e-3, one, one,
                                 None, None, 0, 0, None) == -1
    assert "a light factor needs 3 channels" in L.g2s_last_error().decode()
    assert L.g2s_raster_rgba_bwd(one, None, one, one, one, None, one, 1, 16, 18, 4, K, 4.0, 2, 2, 3, 1, 1e-3, one, one,
                                 one, None, 0, 0, None) == -1
    assert "grad_light needs light" in L.g2s_last_error().decode()
    # implicit topology sizes of the light
    assert L.g2s_face_light_fwd(one, None, 1, 15, 18, 4, 1, f3, f3, f3, one, None) == -1
    assert "implicit topology" in L.g2s_last_error().decode()
    assert L.g2s_face_light_bwd(one, None, None, 1, 16, 18, 4, 1, f3, f3, one, None, 0, 0, None) == -1
    assert "NULL pointer argument" in L.g2s_last_error().decode()
    unlit = L.g2s_raster_rgb_bwd_workspace_bytes(2, 16, 18, 2, 3)
    assert L.g2s_raster_rgba_bwd_workspace_bytes(2, 16, 18, 2, 3, 1) == unlit + 2 * 36 * 3 * 8
    assert L.g2s_raster_rgba_bwd_workspace_bytes(2, 16, 18, 2, 3, 0) == unlit + 2 * 18 * 3 * 8
    assert L.g2s_raster_rgba_bwd_workspace_bytes(0, 16, 18, 2, 3, 1) == 0
