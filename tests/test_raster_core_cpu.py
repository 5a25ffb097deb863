"""CPU check of the product's rasterizer arithmetic + tile culling logic.

tests/raster_tile_emulation.cpp runs the structure of gan-2d-to-3d_amd/csrc/raster.hip (chunk
boxes -> face boxes -> candidate list -> covering faces -> lexicographic (depth, id) minimum, flip +
pooling) serially on the host with the SAME header (csrc/raster_core.h) the HIP kernels compile,
and must agree bit for bit with the brute-force oracle.  (The wavefront-specific parts — ballots,
LDS lists — are covered by the -m gpu tests.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import capi
from raster_cases import BACKGROUND, CASES, forward_stats, scene, soup

HERE = os.path.dirname(os.path.abspath(__file__))
FAR = 100.0


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    so = os.path.join(HERE, "_build", "libraster_emul.so")
    flags = ["-O2"]
    if os.environ.get("G2S_ORACLE_LIB"):   # the sanitizer pass (tests/test_sanitizers_cpu.py)
        so = os.path.join(HERE, "_build", "libraster_emul_san.so")
        flags = capi.SANITIZE
    subprocess.check_call(["g++"] + flags + ["-fPIC", "-shared", "-ffp-contract=off", "-o", so,
                                             os.path.join(HERE, "raster_tile_emulation.cpp")])
    return C.CDLL(so)


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def run_emul(lib, verts, faces, S, K, ssaa, fill_back, near=0.1, far=FAR, implicit=False):
    B, N, _ = verts.shape
    F = faces.shape[0]
    isz = S * ssaa
    depth = np.empty((B, S, S), np.float32)
    fidx = np.empty((B, isz, isz), np.int32)
    bary = np.empty((B, isz, isz, 3), np.float32)
    stats = (C.c_long * 4)()
    Kf = np.ascontiguousarray(K, np.float32).reshape(9)
    rc = lib.g2s_emul_render_depth(_f(verts), _i(None if implicit else faces), B, N, F, S, _f(Kf),
                                   C.c_float(S), ssaa, int(fill_back), C.c_float(near),
                                   C.c_float(far), _f(depth), _i(fidx), _f(bary), stats)
    assert rc == 0
    return dict(depth=depth, face_idx=fidx, bary=bary, candidates=stats[0], fragments=stats[1],
                max_candidates=stats[2], max_chunks=stats[3])


@pytest.mark.parametrize("S,ssaa,fill_back,implicit", [
    (16, 2, True, True), (16, 2, True, False), (20, 2, True, True), (32, 2, True, True),
    (16, 1, True, True), (16, 2, False, True), (12, 1, False, False),
    # raster sides 13 and 36: partial tiles, an odd number of tiles per side
    (13, 1, True, True), (13, 1, True, False), (18, 2, True, True), (18, 2, True, False)])
def test_tile_algorithm_equals_bruteforce(emul, S, ssaa, fill_back, implicit):
    geo, verts, faces = scene(S, B=2, seed=S + ssaa)
    ref = capi.render_depth(verts, faces, S, geo.K[0], ssaa=ssaa, fill_back=fill_back, far=FAR)
    out = run_emul(emul, verts, faces, S, geo.K[0], ssaa, fill_back, implicit=implicit)
    np.testing.assert_array_equal(out["face_idx"], ref["face_idx"])
    np.testing.assert_array_equal(out["bary"], ref["bary"])
    np.testing.assert_array_equal(out["depth"], ref["depth"])
    isz = S * ssaa
    n_faces = faces.shape[0] * (2 if fill_back else 1)
    brute = 2 * isz * isz * n_faces
    assert out["candidates"] * 64 < brute / 4  # culling actually culls


def test_triangle_soup_explicit_topology(emul):
    verts, faces = soup()
    S = 16
    from oracle import geometry as og
    K = og.Geometry(S).K[0]
    for fill_back in (True, False):
        ref = capi.render_depth(verts, faces, S, K, fill_back=fill_back, far=FAR)
        out = run_emul(emul, verts, faces, S, K, 2, fill_back)
        np.testing.assert_array_equal(out["face_idx"], ref["face_idx"])
        np.testing.assert_array_equal(out["depth"], ref["depth"])
        assert (ref["face_idx"] >= 0).mean() > 0.3


def test_backward_arithmetic(emul):
    S = 16
    geo, verts, faces = scene(S, B=2, seed=3)
    fw = capi.render_depth(verts, faces, S, geo.K[0], far=FAR)
    rng = np.random.default_rng(0)
    g = rng.standard_normal((2, S, S)).astype(np.float32)
    g[fw["depth"] > 1.2] = 0  # what the clamp in warp_canon_depth does (renderer.py:123-124)
    ref = capi.render_depth_bwd(verts, faces, g, fw["face_idx"], fw["bary"], S, geo.K[0])
    ref64 = capi.render_depth_bwd(verts.astype(np.float64), faces, g.astype(np.float64),
                                  fw["face_idx"], fw["bary"].astype(np.float64), S,
                                  geo.K[0].astype(np.float64), dtype=np.float64)
    gv = np.empty_like(verts)
    Kf = np.ascontiguousarray(geo.K[0], np.float32).reshape(9)
    for fptr in (faces, None):
        rc = emul.g2s_emul_render_depth_bwd(_f(verts), _i(fptr), _f(g), _i(fw["face_idx"]),
                                            _f(fw["bary"]), 2, S * S, faces.shape[0], S, _f(Kf),
                                            C.c_float(S), 2, _f(gv))
        assert rc == 0
        scale = np.abs(ref64).max()
        assert scale > 0
        np.testing.assert_allclose(gv, ref64, atol=2e-5 * scale)
        np.testing.assert_allclose(gv, ref, atol=2e-5 * scale)


# ----------------------------------------------------------------------------- the texture pass (shade_core.h)
def test_winner_verts_on_a_grid_with_reversed_copies(emul):
    """Every id of an S = 5 grid with fill_back, through the face list and through the implicit topology: the
    triple is the grid's face, flipped for the reversed copy (ids >= F); without reversed copies nothing flips."""
    import torch
    from gan2shape_amd.plugins.neural_renderer import _regular_grid_faces
    S = 5
    faces = np.ascontiguousarray(_regular_grid_faces(S, torch.device("cpu")).numpy(), np.int32)
    F = faces.shape[0]
    assert F == 2 * (S - 1) ** 2
    ids = np.arange(2 * F)
    want = np.where((ids >= F)[:, None], faces[ids % F][:, ::-1], faces[ids % F])
    for fptr in (faces, None):
        for reversible in (1, 0):
            g, rev, v = np.empty(2 * F, np.int32), np.empty(2 * F, np.int32), np.empty((2 * F, 3), np.int32)
            emul.g2s_emul_winner_verts(2 * F, F, S, _i(fptr), reversible, _i(g), _i(rev), _i(v))
            np.testing.assert_array_equal(g, ids % F)
            np.testing.assert_array_equal(rev, (ids >= F) if reversible else np.zeros(2 * F))
            np.testing.assert_array_equal(v, want if reversible else faces[ids % F])


# keys of test_gpu_render_rgb_grad.CASES (S, ts, C, fill_back, implicit): both topologies, fill_back on and off,
# C of 1 and 3; each runs with ssaa 2 and 1
RGB_CASES = [(16, 2, 3, True, True), (20, 2, 3, True, False), (12, 2, 1, False, True)]


@pytest.mark.parametrize("key", RGB_CASES, ids=str)
def test_texture_forward_from_the_shared_header(emul, key):
    """g2s_emul_render_rgb — winner_verts, persp_weights, CubeCoord and resolve_pixel as the kernels compile them —
    on the maps the emulated depth pass produced, against the float64 restatement of test_gpu_render_rgb_grad on
    the same winners.  Yardstick: the restatement evaluated in float32, another fp32 evaluation of the same
    formula that may associate differently; the emulation's relative L2 error may be at most twice its error.

    The scenes of these cases have no reversed winner, so each fill_back case runs a second time on the same maps
    with every winner replaced by its reversed copy: the id plus F and the three weights in the opposite order, which
    is what the depth pass stores for the triple (v2, v1, v0) at the same sample.

    Measured, emulation / yardstick (ratio); the reversed maps give the same figures to three digits:
        (16, 2, 3, True, True)    ssaa 2  2.86e-6 / 2.76e-6 (1.04)   ssaa 1  4.81e-6 / 4.77e-6 (1.01)
        (20, 2, 3, True, False)   ssaa 2  1.73e-6 / 1.73e-6 (1.00)   ssaa 1  1.35e-5 / 9.96e-6 (1.36)
        (12, 2, 1, False, True)   ssaa 2  8.49e-7 / 8.29e-7 (1.02)   ssaa 1  1.17e-6 / 1.12e-6 (1.04)"""
    import torch
    import test_gpu_render_rgb_grad as rg
    assert key in rg.CASES
    S, ts, Cc, fill_back, implicit = key
    geo, verts, faces, tex, _ = rg.make_case(S, ts, Cc)
    B, N, _ = verts.shape
    F = faces.shape[0]
    bg = np.array([1.0, 0.5, -0.25][:Cc], np.float32)
    for ssaa in (2, 1):
        maps = run_emul(emul, verts, faces, S, geo.K[0], ssaa, fill_back, near=rg.NEAR, far=rg.FAR, implicit=implicit)
        assert (maps["face_idx"] >= 0).mean() > 0.1
        for reverse in ((False, True) if fill_back else (False,)):
            fidx, bary = maps["face_idx"], maps["bary"]
            if reverse:
                assert (fidx < F).all()
                fidx = np.where(fidx >= 0, fidx + F, fidx).astype(np.int32)
                bary = np.ascontiguousarray(bary[..., ::-1])
            rgb = np.full((B, Cc, S, S), np.nan, np.float32)
            alpha = np.full((B, S, S), np.nan, np.float32)
            rc = emul.g2s_emul_render_rgb(_f(verts), _i(None if implicit else faces), _i(fidx), _f(bary), _f(tex),
                                          B, N, F, S, ssaa, ts, Cc, _f(bg), C.c_float(rg.EPS), _f(rgb), _f(alpha))
            assert rc == 0
            ref = {dt: rg.restate(torch.tensor(verts, dtype=dt), faces, torch.tensor(tex, dtype=dt), fidx, S, geo.K[0],
                                  ssaa=ssaa, background=bg.tolist(), eps=rg.EPS)
                   for dt in (torch.float64, torch.float32)}
            assert ref[torch.float32].dtype == torch.float32
            want = ref[torch.float64].numpy()
            err = float(np.linalg.norm(rgb.astype(np.float64) - want) / np.linalg.norm(want))
            yard = float(np.linalg.norm(ref[torch.float32].numpy().astype(np.float64) - want) / np.linalg.norm(want))
            print(f"texture forward {key} ssaa={ssaa} reversed={reverse}: emulation rel L2 {err:.3e}  float32 "
                  f"restatement {yard:.3e}  ratio {err / yard:.2f}")
            assert yard > 0
            assert err <= 2 * yard, (key, ssaa, reverse, err, yard)
            # alpha: the share of a pixel's samples with a winner, exactly
            cov = (fidx >= 0)[:, ::-1].reshape(B, S, ssaa, S, ssaa).sum((2, 4)) / float(ssaa * ssaa)
            np.testing.assert_array_equal(alpha, cov.astype(np.float32))


# ----------------------------------------------------------------------------- the depth-path case table
def test_case_table_reaches_its_paths():
    """What keeps the GPU tests of tests/test_gpu_raster_paths.py from passing with a path unvisited,
    shown on the oracle alone: enough coverage, reversed winners (face_idx >= F) where the case is there
    for them, more distinct vertices in one tile than the backward's LDS table has slots (128), and a
    finite non-zero float64 gradient."""
    for case in CASES:
        d = case.data()
        covered, reversed_, most = forward_stats(d["fw"], d["faces"])
        print(f"{case.name:16s} covered {covered:.3f} reversed {reversed_:.3f} vertices/tile {most:3d} "
              f"e32/scale {d['e32'] / d['scale']:.2e}")
        assert covered >= 0.15, case
        if case.name in ("soup", "confetti", "confetti17"):
            assert reversed_ >= 0.25, case
        if not case.fill_back:
            assert reversed_ == 0, case
        if case.name == "confetti_nofill":
            # by counting: the flipped half of the faces is not drawn, 32 triangles of a tile remain
            assert most == 96, case
        elif case.name.startswith("confetti"):
            assert most >= 129, case
        assert np.isfinite(d["ref64"]).all() and d["scale"] > 0, case
        assert d["e32"] > 0, case           # the bound is measured, not just its floor
    isz = np.array([c.S * c.ssaa for c in CASES])
    assert (isz % 8 != 0).any() and (((isz + 7) // 8) % 2 == 1).any()      # partial tiles, odd tiles_side
    assert ((((isz + 7) // 8) ** 2) % 8 != 0).any()                        # no XCD band remap of the tiles
    # reversed winners on the regular grid too (the implicit topology's vertex swap)
    assert forward_stats(CASES[0].data()["fw"], CASES[0].data()["faces"])[1] > 0.01
    d = BACKGROUND.data()
    assert (d["fw"]["face_idx"] == -1).all() and (d["fw"]["depth"] == np.float32(FAR)).all()
    assert not d["ref64"].any() and np.abs(d["g"]).min() > 0


@pytest.mark.parametrize("case", CASES + [BACKGROUND], ids=repr)
def test_tile_algorithm_equals_bruteforce_on_the_case_table(emul, case):
    d = case.data()
    for implicit in case.topologies:
        out = run_emul(emul, d["verts"], d["faces"], case.S, d["K"], case.ssaa, case.fill_back, implicit=implicit)
        np.testing.assert_array_equal(out["face_idx"], d["fw"]["face_idx"])
        np.testing.assert_array_equal(out["bary"], d["fw"]["bary"])
        np.testing.assert_array_equal(out["depth"], d["fw"]["depth"])


@pytest.mark.parametrize("case", CASES + [BACKGROUND], ids=repr)
def test_backward_arithmetic_on_the_case_table(emul, case):
    """g2s_emul_render_depth_bwd (the kernel's per-sample arithmetic, serial adds) against the float64
    oracle within the bound the GPU tests use: 4 e32 + 5e-6 scale (raster_cases.Case.data)."""
    d = case.data()
    verts, faces, fw = d["verts"], d["faces"], d["fw"]
    B, N, _ = verts.shape
    Kf = np.ascontiguousarray(d["K"], np.float32).reshape(9)
    for implicit in case.topologies:
        gv = np.full_like(verts, np.nan)
        rc = emul.g2s_emul_render_depth_bwd(_f(verts), _i(None if implicit else faces), _f(d["g"]),
                                            _i(fw["face_idx"]), _f(fw["bary"]), B, N, faces.shape[0], case.S,
                                            _f(Kf), C.c_float(case.S), case.ssaa, _f(gv))
        assert rc == 0
        err = float(np.abs(gv - d["ref64"]).max())
        print(f"{case.name} implicit={implicit}: err {err:.3e} e32 {d['e32']:.3e} bound {d['bound']:.3e}")
        assert err <= d["bound"], (case, err, d["bound"])
        if case is BACKGROUND:
            assert not gv.any()
