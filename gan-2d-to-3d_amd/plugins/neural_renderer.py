"""Drop-in for the external CUDA package `neural_renderer` at the boundary GAN2Shape uses.

The reference binds it by name — `import neural_renderer as nr` (GAN2Shape/renderer/renderer.py:6),
builds `nr.Renderer(camera_mode='projection', light_intensity_ambient=1.0,
light_intensity_directional=0., K=K, R=R, t=t, near=.., far=.., image_size=S, orig_size=S,
fill_back=True, background_color=[1,1,1])` (renderer.py:47-54) and calls
`.render_depth(vertices [B,N,3] f32, faces [B,F,3] i32) -> [B,S,S] f32` (renderer.py:120),
differentiable w.r.t. `vertices`.  `.render_rgb(vertices, faces, textures [B,F,T,T,T,C])`
(renderer.py:196,230,248,272,275) is the texture pass (g2s_raster_rgb_fwd / g2s_raster_rgb_bwd),
differentiable w.r.t. `textures` (exact) and `vertices`.  The vertex gradient is the gradient of the
texture lookup with the winning face of every sample held fixed: it has NO SILHOUETTE TERM (the
package approximates the effect of moving silhouettes with an edge-sweep heuristic that nothing here
can pin and that is not rebuilt).  `.render(vertices, faces, textures) -> (rgb, depth, alpha)` returns
all three from ONE rasterization (RenderFunction: g2s_raster_depth_fwd, g2s_face_light_fwd when lit,
g2s_raster_rgba_fwd); rgb and depth are differentiable as in render_rgb / render_depth, the per-face
light (ambient + directional, nr.lighting) is differentiable w.r.t. the vertices, and ALPHA CARRIES NO
GRADIENT, for the reason above.  `.render_silhouettes(vertices, faces) -> alpha` is that alpha alone,
without a texture pass and without a gradient.

Semantics follow SURVEY.md Appendix A (the package itself is un-vendored and un-pinned, so parity
is checked against the oracle's restatement, not against the CUDA original):
`render_depth` rasterizes with the package defaults near=0.1 / far=100 (the constructor's near/far
only reach render_rgb/render_silhouettes), anti_aliasing=True (2x supersampling + average pool),
vertical flip, background = far.
"""
import torch
from torch.autograd import Function

from gan2shape_amd import lib as _lib
from gan2shape_amd import zeropool as _zp

DEFAULT_NEAR = 0.1
DEFAULT_FAR = 100.0


def _workspace(device, nbytes):
    """Rasterizer scratch (projected vertices + chunk boxes), allocated PER CALL: under torch's
    caching allocator this is a free-list hit, and during a HIP-graph capture the block comes from
    the graph's private pool and stays reserved for every replay.  (A grown-on-demand shared
    buffer would be freed when a larger batch arrives while captured graphs still hold its
    address.)"""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _rasterise(verts, faces, F, K, orig_size, S, ssaa, fill_back, near, far, maps=True):
    """g2s_raster_depth_fwd over verts (B,N,3) contiguous; `faces` (F,3) int32 or None (implicit grid); K the nine
    host floats.  Returns (depth (B,S,S), face_idx (B,is,is), bary (B,is,is,3)), is = S * ssaa; without `maps` the
    two saved maps are None and the kernel does not write them."""
    B, N, _ = verts.shape
    L = _lib.load()
    dev = verts.device
    depth = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    fidx = torch.empty((B, S * ssaa, S * ssaa), dtype=torch.int32, device=dev) if maps else None
    bary = torch.empty((B, S * ssaa, S * ssaa, 3), dtype=torch.float32, device=dev) if maps else None
    ws = _workspace(dev, L.g2s_raster_workspace_bytes(B, N, F, S))
    _lib.check(L.g2s_raster_depth_fwd(_lib.ptr(verts), _lib.ptr(faces), B, N, F, S, (_lib.C.c_float * 9)(*K),
                                      float(orig_size), ssaa, int(bool(fill_back)), float(near), float(far),
                                      _lib.ptr(depth), _lib.ptr(fidx), _lib.ptr(bary), _lib.ptr(ws), ws.numel(),
                                      _lib.stream()))
    return depth, fidx, bary


def _scatter_targets(shapes, ws_bytes, device):
    """Where a backward scatters into: one float32 tensor per entry of `shapes` (None = that gradient is not
    wanted -> None) -> (targets, workspace, workspace bytes, acc_is_zero).  Whatever the kernels accumulate in
    must start at zero: in default mode the targets themselves, in deterministic mode the fixed-point workspace of
    `ws_bytes()` bytes (include/g2s.h).  It is a slice of the step's cleared pool when there is one (acc_is_zero =
    1), else the call clears it with a memset of its own.  One flag covers every target: if any of them missed the
    pool, all are allocated uncleared and the call clears them, rather than split the call."""
    def fresh():
        return [None if s is None else torch.empty(s, dtype=torch.float32, device=device) for s in shapes]
    if _lib.load().g2s_get_deterministic():
        nbytes = ws_bytes()
        ws = _zp.take(((nbytes + 3) // 4,), device)
        pre = ws is not None
        if ws is None:
            ws = _workspace(device, nbytes)
        return fresh(), ws, nbytes, int(pre)
    targets = [None if s is None else _zp.take(tuple(s), device) for s in shapes]
    pre = all(t is not None for s, t in zip(shapes, targets) if s is not None)
    return (targets if pre else fresh()), None, 0, int(pre)


def _regular_grid_faces(S, device):
    key = (S, device)
    f = _regular_grid_faces.cache.get(key)
    if f is None:
        idx = torch.arange(S * S, device=device).reshape(S, S)
        f1 = torch.stack([idx[:S - 1, :S - 1], idx[1:, :S - 1], idx[:S - 1, 1:]], -1).reshape(-1, 3)
        f2 = torch.stack([idx[:S - 1, 1:], idx[1:, :S - 1], idx[1:, 1:]], -1).reshape(-1, 3)
        f = torch.cat([f1, f2], 0).int()
        _regular_grid_faces.cache[key] = f
    return f


_regular_grid_faces.cache = {}


class RenderDepthFunction(Function):
    """vertices (B,N,3) camera space -> depth (B,S,S).  `faces` is (F,3) int32 or None (implicit
    regular grid of renderer/utils.py:76-80)."""

    @staticmethod
    def forward(ctx, vertices, faces, K, orig_size, image_size, anti_aliasing, fill_back, near, far):
        _lib.require_cuda(vertices)
        if vertices.dtype != torch.float32:
            raise RuntimeError("render_depth: vertices must be float32")
        verts = vertices.contiguous()
        B, N, _ = verts.shape
        S = int(image_size)
        ssaa = 2 if anti_aliasing else 1
        F = 2 * (S - 1) * (S - 1) if faces is None else faces.shape[0]
        need_grad = ctx.needs_input_grad[0]
        depth, fidx, bary = _rasterise(verts, faces, F, K, orig_size, S, ssaa, fill_back, near, far, maps=need_grad)
        if need_grad:
            ctx.save_for_backward(verts, faces, fidx, bary)
        ctx.meta = (K, float(orig_size), S, ssaa, F)
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        verts, faces, fidx, bary = ctx.saved_tensors
        K, orig_size, S, ssaa, F = ctx.meta
        B, N, _ = verts.shape
        g = grad_depth.contiguous().float()
        L = _lib.load()
        Kc = (_lib.C.c_float * 9)(*K)
        (gv,), ws, ws_bytes, pre = _scatter_targets([verts.shape], lambda: L.g2s_raster_bwd_workspace_bytes(B, N),
                                                    verts.device)
        _lib.check(L.g2s_raster_depth_bwd_ex(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(g),
                                             _lib.ptr(fidx), _lib.ptr(bary), B, N, F, S, Kc, orig_size,
                                             ssaa, _lib.ptr(gv), _lib.ptr(ws), ws_bytes, pre, _lib.stream()))
        return gv, None, None, None, None, None, None, None, None


class RenderRgbFunction(Function):
    """vertices (B,N,3) camera space, textures (B,F,T,T,T,C) -> rgb (B,C,S,S).  `faces` is (F,3) int32
    or None (implicit regular grid).  Backward: g2s_raster_rgb_bwd — the adjoint of the trilinear read
    for the textures, the derivative of the texture lookup (winners fixed, no silhouette term) for the
    vertices; only the gradients `ctx.needs_input_grad` names are computed."""

    @staticmethod
    def forward(ctx, vertices, textures, faces, K, orig_size, image_size, anti_aliasing, fill_back, near, far,
                background, eps):
        verts = vertices.contiguous()
        tex = textures.contiguous()
        B, N, _ = verts.shape
        S = int(image_size)
        ssaa = 2 if anti_aliasing else 1
        F, ts, C = tex.shape[1], tex.shape[2], tex.shape[5]
        L = _lib.load()
        _, fidx, bary = _rasterise(verts, faces, F, K, orig_size, S, ssaa, fill_back, near, far)
        rgb = torch.empty((B, C, S, S), dtype=torch.float32, device=verts.device)
        _lib.check(L.g2s_raster_rgb_fwd(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(fidx), _lib.ptr(bary), _lib.ptr(tex),
                                        B, N, F, S, ssaa, ts, C, (_lib.C.c_float * C)(*background),
                                        float(eps), _lib.ptr(rgb), _lib.stream()))
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(verts, faces, fidx, bary, tex)
        ctx.meta = (K, float(orig_size), S, ssaa, float(eps))
        return rgb

    @staticmethod
    def backward(ctx, grad_rgb):
        verts, faces, fidx, bary, tex = ctx.saved_tensors
        K, orig_size, S, ssaa, eps = ctx.meta
        B, N, _ = verts.shape
        F, ts, C = tex.shape[1], tex.shape[2], tex.shape[5]
        want_v, want_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = grad_rgb.contiguous().float()
        L = _lib.load()
        Kc = (_lib.C.c_float * 9)(*K)
        (gv, gt), ws, ws_bytes, pre = _scatter_targets(
            [verts.shape if want_v else None, tex.shape if want_t else None],
            lambda: L.g2s_raster_rgb_bwd_workspace_bytes(B, N, F, ts, C), verts.device)
        _lib.check(L.g2s_raster_rgb_bwd(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(fidx), _lib.ptr(bary),
                                        _lib.ptr(tex), _lib.ptr(g), B, N, F, S, Kc, orig_size, ssaa, ts, C, eps,
                                        _lib.ptr(gt), _lib.ptr(gv), _lib.ptr(ws), ws_bytes, pre, _lib.stream()))
        return gv, gt, None, None, None, None, None, None, None, None, None, None


class RenderFunction(Function):
    """nr.Renderer.render: vertices (B,N,3) camera space, textures (B,F,T,T,T,C) -> rgb (B,C,S,S), depth (B,S,S),
    alpha (B,S,S) from ONE rasterization.  `light` is None (unlit: the texture pass of RenderRgbFunction) or the
    host triple (ambient rgb, directional rgb, direction) of g2s_face_light_fwd, which needs C == 3.
    Backward: depth path (g2s_raster_depth_bwd_ex), texture path (g2s_raster_rgba_bwd, colour gradient scaled by
    the light) and light path (grad_light of the texture path through g2s_face_light_bwd) summed into one
    grad_verts; alpha is non-differentiable (no silhouette term)."""

    @staticmethod
    def forward(ctx, vertices, textures, faces, K, orig_size, image_size, anti_aliasing, fill_back, near, far,
                background, eps, light):
        verts = vertices.contiguous()
        tex = textures.contiguous()
        B, N, _ = verts.shape
        S = int(image_size)
        ssaa = 2 if anti_aliasing else 1
        F, ts, C = tex.shape[1], tex.shape[2], tex.shape[5]
        fb = int(bool(fill_back))
        L = _lib.load()
        st = _lib.stream()
        depth, fidx, bary = _rasterise(verts, faces, F, K, orig_size, S, ssaa, fb, near, far)
        lit = None
        if light is not None:
            lit = torch.empty((B, F * (1 + fb), 3), dtype=torch.float32, device=verts.device)
            f3 = _lib.C.c_float * 3
            _lib.check(L.g2s_face_light_fwd(_lib.ptr(verts), _lib.ptr(faces), B, N, F, S, fb, f3(*light[0]),
                                            f3(*light[1]), f3(*light[2]), _lib.ptr(lit), st))
        rgb = torch.empty((B, C, S, S), dtype=torch.float32, device=verts.device)
        alpha = torch.empty((B, S, S), dtype=torch.float32, device=verts.device)
        _lib.check(L.g2s_raster_rgba_fwd(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(fidx), _lib.ptr(bary),
                                         _lib.ptr(tex), _lib.ptr(lit), B, N, F, S, ssaa, ts, C, fb,
                                         (_lib.C.c_float * C)(*background), float(eps), _lib.ptr(rgb),
                                         _lib.ptr(alpha), st))
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(verts, faces, fidx, bary, tex, lit)
        ctx.meta = (K, float(orig_size), S, ssaa, float(eps), fb, light)
        ctx.mark_non_differentiable(alpha)
        ctx.set_materialize_grads(False)
        return rgb, depth, alpha

    @staticmethod
    def backward(ctx, grad_rgb, grad_depth, grad_alpha):
        verts, faces, fidx, bary, tex, lit = ctx.saved_tensors
        K, orig_size, S, ssaa, eps, fb, light = ctx.meta
        B, N, _ = verts.shape
        F, ts, C = tex.shape[1], tex.shape[2], tex.shape[5]
        want_v, want_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        L = _lib.load()
        st = _lib.stream()
        Kc = (_lib.C.c_float * 9)(*K)
        dev = verts.device
        gv = gt = None
        if want_v and grad_depth is not None:
            g = grad_depth.contiguous().float()
            (gv,), ws, ws_bytes, pre = _scatter_targets([verts.shape], lambda: L.g2s_raster_bwd_workspace_bytes(B, N),
                                                        dev)
            _lib.check(L.g2s_raster_depth_bwd_ex(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(g), _lib.ptr(fidx),
                                                 _lib.ptr(bary), B, N, F, S, Kc, orig_size, ssaa, _lib.ptr(gv),
                                                 _lib.ptr(ws), ws_bytes, pre, st))
        if grad_rgb is not None and (want_v or want_t):
            g = grad_rgb.contiguous().float()
            # the light moves with the vertices only through its directional term
            want_l = want_v and lit is not None and any(float(x) != 0.0 for x in light[1])
            (gc, gt, gl), ws, ws_bytes, pre = _scatter_targets(
                [verts.shape if want_v else None, tex.shape if want_t else None,
                 (B, F * (1 + fb), 3) if want_l else None],
                lambda: L.g2s_raster_rgba_bwd_workspace_bytes(B, N, F, ts, C, fb), dev)
            _lib.check(L.g2s_raster_rgba_bwd(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(fidx), _lib.ptr(bary),
                                             _lib.ptr(tex), _lib.ptr(lit), _lib.ptr(g), B, N, F, S, Kc, orig_size,
                                             ssaa, ts, C, fb, eps, _lib.ptr(gt), _lib.ptr(gc), _lib.ptr(gl),
                                             _lib.ptr(ws), ws_bytes, pre, st))
            if want_l:
                # added to the texture path's camera-space gradient (acc_is_zero = 1: nothing is cleared); the
                # fixed-point sums of deterministic mode need a cleared workspace of their own
                ws, ws_bytes = None, 0
                if L.g2s_get_deterministic():
                    ws_bytes = L.g2s_raster_bwd_workspace_bytes(B, N)
                    ws = _zp.zeros(((ws_bytes + 3) // 4,), dev)
                f3 = _lib.C.c_float * 3
                _lib.check(L.g2s_face_light_bwd(_lib.ptr(verts), _lib.ptr(faces), _lib.ptr(gl), B, N, F, S, fb,
                                                f3(*light[1]), f3(*light[2]), _lib.ptr(gc), _lib.ptr(ws),
                                                ws_bytes, 1, st))
            if want_v:
                # the projection backward of either path runs in place over that path's own sums, so the two
                # camera-space gradients meet here and not inside one accumulator
                gv = gc if gv is None else gv.add_(gc)
        return gv, gt, None, None, None, None, None, None, None, None, None, None, None


class Renderer:
    """`nr.Renderer` for camera_mode='projection' (the only mode GAN2Shape uses)."""

    def __init__(self, image_size=256, anti_aliasing=True, background_color=[0, 0, 0],
                 fill_back=True, camera_mode='projection', K=None, R=None, t=None,
                 dist_coeffs=None, orig_size=1024, perspective=True, viewing_angle=30,
                 camera_direction=[0, 0, 1], near=0.1, far=100, light_intensity_ambient=0.5,
                 light_intensity_directional=0.5, light_color_ambient=[1, 1, 1],
                 light_color_directional=[1, 1, 1], light_direction=[0, 1, 0], **unknown):
        if camera_mode != 'projection':
            raise ValueError("only camera_mode='projection' is supported (renderer.py:47)")
        self.image_size = image_size
        self.anti_aliasing = anti_aliasing
        self.background_color = background_color
        self.fill_back = fill_back
        self.camera_mode = camera_mode
        self.K, self.R, self.t = K, R, t
        self.dist_coeffs = dist_coeffs
        self.orig_size = orig_size
        self.near, self.far = near, far
        self.light_intensity_ambient = light_intensity_ambient
        self.light_intensity_directional = light_intensity_directional
        self.light_color_ambient = light_color_ambient
        self.light_color_directional = light_color_directional
        self.light_direction = light_direction
        self.rasterizer_eps = 1e-3
        self._K_host = None

    def _host_K(self, K):
        """K lives on the device in the reference; one D2H copy, cached per tensor version."""
        key = (K.data_ptr(), K._version)
        if self._K_host is None or self._K_host[0] != key:
            k = K.detach().float().reshape(-1, 3, 3)
            if k.shape[0] != 1:
                raise NotImplementedError("per-sample intrinsics are not supported (GAN2Shape uses K[1,3,3])")
            self._K_host = (key, tuple(k[0].reshape(9).cpu().tolist()))
        return self._K_host[1]

    def _camera(self, vertices, K, R, t, dist_coeffs, orig_size):
        """The camera of one call: K, R, t, dist_coeffs and orig_size default to the constructor's; lens distortion
        is refused, before anything touches the device.  Returns (vertices in camera space, the nine host floats of
        K, orig_size)."""
        K = self.K if K is None else K
        R = self.R if R is None else R
        t = self.t if t is None else t
        orig_size = self.orig_size if orig_size is None else orig_size
        dist_coeffs = self.dist_coeffs if dist_coeffs is None else dist_coeffs
        if dist_coeffs is not None and bool((dist_coeffs != 0).any()):
            raise NotImplementedError("lens distortion is not supported (GAN2Shape never sets it)")
        if K is None:
            raise ValueError("camera_mode='projection' needs K")
        # R, t: identity / zero at GAN2Shape's call site (renderer.py:30-34); applied as torch ops
        # otherwise so that the kernel keeps the R = I, t = 0 form and autograd carries them.
        if self._needs_transform(R, t):
            if R is not None:
                vertices = torch.matmul(vertices, R.reshape(-1, 3, 3).transpose(2, 1))
            if t is not None:
                vertices = vertices + t.reshape(-1, 1, 3)
        return vertices, self._host_K(K), orig_size

    def render_depth(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        vertices, K9, orig_size = self._camera(vertices, K, R, t, dist_coeffs, orig_size)
        S = self.image_size
        f = self._shared_faces(faces, vertices.shape[1], S)
        return RenderDepthFunction.apply(vertices, f, K9, orig_size, S, self.anti_aliasing, self.fill_back,
                                         DEFAULT_NEAR, DEFAULT_FAR)

    def _needs_transform(self, R, t):
        key = tuple(None if x is None else (x.data_ptr(), x._version) for x in (R, t))
        cache = getattr(self, "_rt_cache", None)
        if cache is None or cache[0] != key:
            ident = True
            if R is not None:
                r = R.detach().reshape(-1, 3, 3).float().cpu()
                ident = ident and bool((r == torch.eye(3)).all())
            if t is not None:
                ident = ident and bool((t.detach().cpu() == 0).all())
            self._rt_cache = cache = (key, not ident)
        return cache[1]

    def _shared_faces(self, faces, n_verts, S):
        """Returns None for the regular-grid topology (fast path: the kernel derives the vertex
        ids of renderer/utils.py:76-80 from the face number and reads no face buffer), else one
        (F,3) int32 face list shared by the batch.  `faces=None` or a tensor tagged by
        gan2shape_amd.renderer.utils.get_face_idx skips the comparison."""
        if faces is None or getattr(faces, "_g2s_regular_grid", None) == S:
            if n_verts != S * S:
                raise ValueError("regular-grid faces need S*S vertices")
            return None
        if faces.dim() == 2:
            faces = faces.unsqueeze(0)
        F = faces.shape[1]
        if n_verts == S * S and F == 2 * (S - 1) * (S - 1):
            ref = _regular_grid_faces(S, faces.device)
            if bool((faces.int() == ref.unsqueeze(0)).all()):
                return None
        f0 = faces[0].int().contiguous()
        if faces.shape[0] > 1 and not bool((faces.int() == f0.unsqueeze(0)).all()):
            raise NotImplementedError("per-sample face lists are not supported: call per sample")
        return f0

    def _light(self):
        """None while today's unlit path computes the same thing (no directional light, white ambient: the
        ambient intensity is then a scale of the textures), else the host triple of g2s_face_light_fwd:
        (intensity_ambient * color_ambient, intensity_directional * color_directional, direction)."""
        ia, idr = float(self.light_intensity_ambient), float(self.light_intensity_directional)
        ca = [float(v) for v in self.light_color_ambient]
        cd = [float(v) for v in self.light_color_directional]
        direction = [float(v) for v in self.light_direction]
        if len(ca) != 3 or len(cd) != 3 or len(direction) != 3:
            raise ValueError("light colours and light_direction have 3 components")
        if idr == 0 and ca == [1.0, 1.0, 1.0]:
            return None
        return tuple(ia * v for v in ca), tuple(idr * v for v in cd), tuple(direction)

    def _texture_args(self, vertices, faces, textures, K, R, t, dist_coeffs, orig_size):
        """Argument checks and the positional arguments that RenderRgbFunction and RenderFunction share."""
        light = self._light()
        if light is not None and textures.shape[-1] != 3:
            raise ValueError(f"lighting needs 3 colour channels, got textures with C = {textures.shape[-1]}")
        vertices, K9, orig_size = self._camera(vertices.float(), K, R, t, dist_coeffs, orig_size)
        _lib.require_cuda(vertices, textures)
        B, N, _ = vertices.shape
        S = self.image_size
        f = self._shared_faces(faces, N, S)
        F = 2 * (S - 1) * (S - 1) if f is None else f.shape[0]
        tex = textures.float()
        if tex.dim() != 6 or tex.shape[0] != B or tex.shape[1] != F or not (tex.shape[2] == tex.shape[3] == tex.shape[4]):
            raise ValueError(f"textures must be [B={B}, F={F}, T, T, T, C], got {tuple(tex.shape)}")
        C = tex.shape[5]
        if light is None and self.light_intensity_ambient != 1:
            tex = tex * float(self.light_intensity_ambient)
        bg = [float(v) for v in self.background_color][:C]
        bg += [bg[-1]] * (C - len(bg))
        return (vertices, tex, f, K9, orig_size, S, self.anti_aliasing, self.fill_back, self.near,
                self.far, tuple(bg), self.rasterizer_eps), light

    def render_rgb(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """[B, C, S, S] image of the textured mesh: rasterize with the constructor's near / far
        (renderer.py:51), read each winning face's texture cube trilinearly at perspective-corrected
        barycentric coordinates, background colour elsewhere, flip + 2x2 average.  Lighting: with
        light_intensity_directional = 0 and a white ambient colour (GAN2Shape builds the renderer with
        ambient 1, directional 0) the ambient intensity scales the textures; otherwise every face's colour
        is multiplied by its light (g2s_face_light_fwd: ambient + directional, flat shading; C must be 3).

        Differentiable w.r.t. `textures` and `vertices` (RenderRgbFunction; RenderFunction when lit):
        gradient of the texture lookup and of the light, no silhouette term.  R, t and the unlit ambient
        intensity are torch ops around the function, so autograd carries them.  When neither input
        requires grad the result has no history."""
        args, light = self._texture_args(vertices, faces, textures, K, R, t, dist_coeffs, orig_size)
        if light is None:
            return RenderRgbFunction.apply(*args)
        return RenderFunction.apply(*args, light)[0]

    def render(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """(rgb [B, C, S, S], depth [B, S, S], alpha [B, S, S]) from ONE rasterization with the constructor's
        near / far: rgb as render_rgb; depth as render_depth's kernel gives it with those near / far (background =
        far); alpha = the share of a pixel's 2x2 samples that a face covers.  rgb and depth are differentiable
        w.r.t. `vertices` (and rgb w.r.t. `textures`); ALPHA HAS NO GRADIENT: the package's silhouette-edge
        heuristic is not rebuilt (nothing pins it)."""
        args, light = self._texture_args(vertices, faces, textures, K, R, t, dist_coeffs, orig_size)
        return RenderFunction.apply(*args, light)

    def render_silhouettes(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """alpha [B, S, S] of `render`, from one rasterization and no texture pass.  NO GRADIENT (see `render`)."""
        with torch.no_grad():
            verts, K9, orig_size = self._camera(vertices.float(), K, R, t, dist_coeffs, orig_size)
            _lib.require_cuda(verts)
            verts = verts.contiguous()
            B, N, _ = verts.shape
            S = self.image_size
            f = self._shared_faces(faces, N, S)
            F = 2 * (S - 1) * (S - 1) if f is None else f.shape[0]
            ssaa = 2 if self.anti_aliasing else 1
            _, fidx, _ = _rasterise(verts, f, F, K9, orig_size, S, ssaa, self.fill_back, self.near, self.far)
            alpha = torch.empty((B, S, S), dtype=torch.float32, device=verts.device)
            _lib.check(_lib.load().g2s_raster_rgba_fwd(None, None, _lib.ptr(fidx), None, None, None, B, N, F, S, ssaa, 1, 1,
                                             int(bool(self.fill_back)), None, 0.0, None, _lib.ptr(alpha),
                                             _lib.stream()))
        return alpha


# ------------------------------------------------------------------------------------------ viewing path
SWEEP_MODES = {"texture": 0, "shaded": 1, "shape": 2, "normal": 3}


def _sweep_mode(mode):
    if mode in SWEEP_MODES:
        return SWEEP_MODES[mode]
    if mode in SWEEP_MODES.values():
        return int(mode)
    raise ValueError(f"mode must be one of {list(SWEEP_MODES)} (or 0..3), got {mode!r}")


def sweep_frames(verts, pose, faces, attr, normal, light, K, orig_size, image_size, anti_aliasing, fill_back, near,
                 far, background, grey, mode, want_alpha=False, want_depth=False):
    """The three launches of the viewing path beside RenderRgbFunction, without autograd (there is no backward):
    g2s_sweep_verts (verts (B,N,3), pose (B,V,12) -> (B*V,N,3)), g2s_raster_depth_fwd over the B*V posed meshes,
    g2s_sweep_shade (include/g2s.h).  attr (B,C,N...) / normal (B,N...,3) / light (B*V,5) may be None where the
    mode does not read them; `faces` is (F,3) int32 or None (implicit regular grid).  Returns (rgb (B,V,Cout,S,S),
    alpha (B,V,S,S) or None, depth (B,V,S,S) or None)."""
    mode = _sweep_mode(mode)
    _lib.require_cuda(verts, pose, faces, attr, normal, light)
    with torch.no_grad():
        verts = verts.float().contiguous()
        pose = pose.float().contiguous()
        B, N, _ = verts.shape
        V = pose.shape[1]
        if pose.shape != (B, V, 12):
            raise ValueError(f"pose must be [B={B}, V, 12], got {tuple(pose.shape)}")
        S = int(image_size)
        ssaa = 2 if anti_aliasing else 1
        fb = int(bool(fill_back))
        if faces is not None:
            faces = faces.int().contiguous()
        elif N != S * S:
            raise ValueError("regular-grid faces need S*S vertices")
        F = 2 * (S - 1) * (S - 1) if faces is None else faces.shape[0]
        C = 3
        if mode in (0, 1):
            if attr is None:
                raise ValueError("modes texture and shaded read the image")
            attr = attr.float().contiguous()
            C = attr.shape[1]
            if attr.shape[0] != B or attr[0, 0].numel() != N:
                raise ValueError(f"attr must be [B={B}, C, Ha, Wa] with Ha*Wa = {N}, got {tuple(attr.shape)}")
        else:
            attr = None
        if mode != 0:
            if normal is None:
                raise ValueError("modes shaded, shape and normal read the normals")
            normal = normal.float().contiguous()
            if normal.shape[0] != B or normal.numel() != B * N * 3:
                raise ValueError(f"normal must be [B={B}, Ha, Wa, 3] with Ha*Wa = {N}, got {tuple(normal.shape)}")
        else:
            normal = None
        if mode in (1, 2):
            if light is None:
                raise ValueError("modes shaded and shape need a light")
            light = light.float().contiguous()
            if light.numel() != B * V * 5:
                raise ValueError(f"light must hold B*V = {B * V} rows of (la, lb, lx, ly, lz), got {tuple(light.shape)}")
        else:
            light = None
        Cout = C if mode in (0, 1) else 3
        bg = [float(v) for v in background][:Cout]
        bg += [bg[-1]] * (Cout - len(bg))
        L = _lib.load()
        st = _lib.stream()
        dev = verts.device
        posed = torch.empty((B * V, N, 3), dtype=torch.float32, device=dev)
        _lib.check(L.g2s_sweep_verts(_lib.ptr(verts), _lib.ptr(pose), _lib.ptr(posed), B, V, N, st))
        depth, fidx, bary = _rasterise(posed, faces, F, K, orig_size, S, ssaa, fb, near, far)
        rgb = torch.empty((B, V, Cout, S, S), dtype=torch.float32, device=dev)
        alpha = torch.empty((B, V, S, S), dtype=torch.float32, device=dev) if want_alpha else None
        _lib.check(L.g2s_sweep_shade(_lib.ptr(posed), _lib.ptr(faces), _lib.ptr(fidx), _lib.ptr(bary), _lib.ptr(attr),
                                     _lib.ptr(normal), _lib.ptr(pose), _lib.ptr(light), B, V, N, F, S, ssaa, C, fb,
                                     mode, (_lib.C.c_float * Cout)(*bg), float(grey), _lib.ptr(rgb), _lib.ptr(alpha),
                                     st))
    return rgb, alpha, depth.view(B, V, S, S) if want_depth else None


def pseudo_frames(verts, pose, rays, K, albedo, normal, light, mask, depth_lo, depth_hi, orig_size, image_size,
                  anti_aliasing, fill_back, want_mask=True):
    """The three launches of the pseudo-view path, without autograd (there is no backward): g2s_sweep_verts,
    g2s_raster_depth_fwd over the B*V posed meshes with render_depth's near / far and no saved maps, g2s_sweep_pseudo
    (include/g2s.h).  verts (B,S*S,3), pose (B,V,12), rays (S*S,3), albedo (B,C,S,S), normal (B,S,S,3) and light
    (B*V,4) both or neither, mask (B,S,S) or None.  Every shape is checked before the first launch.  Returns
    (im (B,V,C,S,S), mask (B,V,S,S) or None)."""
    S = int(image_size)
    B, V = check_pseudo_shapes(verts.shape, pose.shape, rays.shape, albedo.shape, None if normal is None else normal.shape,
                               None if light is None else light.shape, None if mask is None else mask.shape, S)
    _lib.require_cuda(verts, pose, rays, albedo, normal, light, mask)
    with torch.no_grad():
        verts, pose, rays, albedo = (t.float().contiguous() for t in (verts, pose, rays, albedo))
        normal, light, mask = (None if t is None else t.float().contiguous() for t in (normal, light, mask))
        C, N = albedo.shape[1], S * S
        ssaa = 2 if anti_aliasing else 1
        F = 2 * (S - 1) * (S - 1)
        L = _lib.load()
        st = _lib.stream()
        dev = verts.device
        posed = torch.empty((B * V, N, 3), dtype=torch.float32, device=dev)
        _lib.check(L.g2s_sweep_verts(_lib.ptr(verts), _lib.ptr(pose), _lib.ptr(posed), B, V, N, st))
        warped, _, _ = _rasterise(posed, None, F, K, orig_size, S, ssaa, fill_back, DEFAULT_NEAR, DEFAULT_FAR, maps=False)
        Kc = (_lib.C.c_float * 9)(*K)
        im = torch.empty((B, V, C, S, S), dtype=torch.float32, device=dev)
        mout = torch.empty((B, V, S, S), dtype=torch.float32, device=dev) if want_mask else None
        _lib.check(L.g2s_sweep_pseudo(_lib.ptr(warped), _lib.ptr(rays), _lib.ptr(pose), Kc, _lib.ptr(albedo),
                                      _lib.ptr(normal), _lib.ptr(light), _lib.ptr(mask), float(depth_lo),
                                      float(depth_hi), B, V, S, C, _lib.ptr(im), _lib.ptr(mout), st))
    return im, mout


def check_pseudo_shapes(verts, pose, rays, albedo, normal, light, mask, S):
    """The argument checks of `pseudo_frames` on plain shapes (no device needed) -> (B, V); ValueError otherwise."""
    verts, pose, rays, albedo = tuple(verts), tuple(pose), tuple(rays), tuple(albedo)
    B = verts[0]
    if S < 2 or verts != (B, S * S, 3):
        raise ValueError(f"verts must be [B, S*S = {S * S}, 3] with S >= 2, got {verts}")
    if len(pose) != 3 or pose[0] != B or pose[2] != 12 or pose[1] < 1:
        raise ValueError(f"pose must be [B={B}, V, 12], got {pose}")
    V = pose[1]
    if rays != (S * S, 3):
        raise ValueError(f"rays must be [S*S = {S * S}, 3], got {rays}")
    if len(albedo) != 4 or albedo[0] != B or not 1 <= albedo[1] <= 4 or albedo[2:] != (S, S):
        raise ValueError(f"albedo must be [B={B}, C in 1..4, {S}, {S}], got {albedo}")
    if (normal is None) != (light is None):
        raise ValueError("normal and light go together: both, or neither for no relighting")
    if normal is not None and tuple(normal) != (B, S, S, 3):
        raise ValueError(f"normal must be [B={B}, {S}, {S}, 3], got {tuple(normal)}")
    if light is not None and tuple(light) != (B * V, 4):
        raise ValueError(f"light must be [B*V = {B * V}, 4] rows of (a, b, dx, dy), got {tuple(light)}")
    if mask is not None and tuple(mask) != (B, S, S):
        raise ValueError(f"mask must be [B={B}, {S}, {S}], got {tuple(mask)}")
    return B, V


def sweep_shade_torch(verts, faces, face_idx, bary, attr, normal, pose, light, B, V, S, ssaa, fill_back, mode,
                      background, grey=0.7):
    """g2s_sweep_shade (include/g2s.h) written in torch ops, on any device and in the dtype of `verts`: the float32
    comparator of the tests and the statement of what the kernel computes, operation by operation.  Arguments as the
    kernel's: posed verts (B*V,N,3), faces (F,3) or None, face_idx (B*V,is,is), bary (B*V,is,is,3), attr (B,C,...),
    normal (B,...,3), pose (B,V,12), light (B*V,5).  Returns (rgb (B*V,Cout,S,S), alpha (B*V,S,S))."""
    mode = _sweep_mode(mode)
    dev, dt = verts.device, verts.dtype
    N = verts.shape[1]
    if faces is None:
        faces = _regular_grid_faces(S, dev)
    faces = faces.long()
    F = faces.shape[0]
    isz = S * ssaa
    fn = face_idx.long()
    hit = fn >= 0
    g = fn.clamp(min=0) % F
    rev = (fn >= F) if fill_back else torch.zeros_like(hit)
    vid = faces[g]                                                    # (BV, is, is, 3)
    vid = torch.where(rev[..., None], vid.flip(-1), vid)
    frame = torch.arange(B * V, device=dev).view(-1, 1, 1, 1)
    image = frame // V
    z = verts[..., 2][frame, vid]                                     # (BV, is, is, 3)
    w = bary.to(dt)
    depth = 1.0 / (w[..., 0] / z[..., 0] + w[..., 1] / z[..., 1] + w[..., 2] / z[..., 2])
    u = w * depth[..., None] / z
    C = 3
    a = None
    if mode in (0, 1):
        C = attr.shape[1]
        at = attr.reshape(B, C, N).to(dt)
        src = at[image[..., None], torch.arange(C, device=dev).view(1, 1, 1, 1, C), vid[..., None]]   # (BV,is,is,3,C)
        a = (u[..., 0, None] * src[..., 0, :] + u[..., 1, None] * src[..., 1, :]) + u[..., 2, None] * src[..., 2, :]
    if mode == 0:
        col = a
    else:
        nm = normal.reshape(B, N, 3).to(dt)[image, vid]                # (BV, is, is, 3 vertices, 3)
        m = (u[..., 0, None] * nm[..., 0, :] + u[..., 1, None] * nm[..., 1, :]) + u[..., 2, None] * nm[..., 2, :]
        A = pose.reshape(B * V, 12)[:, :9].to(dt).view(B * V, 1, 1, 3, 3)
        n = (A[..., 0] * m[..., None, 0] + A[..., 1] * m[..., None, 1]) + A[..., 2] * m[..., None, 2]
        length = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).sqrt()
        n = n / length.clamp(min=1e-12)[..., None]
        if mode == 3:
            col = n
        else:
            lt = light.reshape(B * V, 5).to(dt).view(B * V, 1, 1, 5)
            dot = (n[..., 0] * lt[..., 2] + n[..., 1] * lt[..., 3]) + n[..., 2] * lt[..., 4]
            shade = lt[..., 0] + lt[..., 1] * dot.clamp(min=0)
            if mode == 1:
                col = (a / 2.0 + 0.5) * shade[..., None] * 2.0 - 1.0
            else:
                col = (grey * shade * 2.0 - 1.0)[..., None].expand(-1, -1, -1, 3)
    Cout = col.shape[-1]
    bg = [float(v) for v in background][:Cout]
    bg += [bg[-1]] * (Cout - len(bg))
    col = torch.where(hit[..., None], col, torch.tensor(bg, dtype=dt, device=dev))
    col = col.flip(1).view(B * V, S, ssaa, S, ssaa, Cout)              # vertical flip, then ssaa x ssaa blocks
    cov = hit.flip(1).view(B * V, S, ssaa, S, ssaa).to(dt)
    total = torch.zeros(B * V, S, S, Cout, dtype=dt, device=dev)
    count = torch.zeros(B * V, S, S, dtype=dt, device=dev)
    for dy in range(ssaa):                                            # the kernel's order: dy, then dx
        for dx in range(ssaa):
            total = total + col[:, :, dy, :, dx]
            count = count + cov[:, :, dy, :, dx]
    inv = 1.0 / float(ssaa * ssaa)
    return (total * inv).permute(0, 3, 1, 2).contiguous(), count * inv
