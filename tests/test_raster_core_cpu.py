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
