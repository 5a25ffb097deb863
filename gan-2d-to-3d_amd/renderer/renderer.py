"""Mirror of the training-path methods of GAN2Shape/renderer/renderer.py:13-139,252-264.

Same constructor and method names / argument meaning as the reference `Renderer`; the rasterizer
behind `warp_canon_depth` is the libg2s kernel (through the neural_renderer drop-in).  Differences
that do not change results: tensors are created on `device` directly (the reference hard-codes
.cuda()); the pixel grid, face list and rotation centre are built once; `grid_sample` gets
`align_corners=True` explicitly (the reference targets torch 1.2 where that was the only
behaviour).  render_yaw, render_view, the grid_sample=False branch of
render_given_view (renderer.py:141-277) and downscale_K go through the texture path of the
rasterizer (`render_rgb`); their pose sweeps share one helper (`_sweep`).  That path is
differentiable: everything around `render_rgb` is torch ops, so render_given_view(im, depth, view,
grid_sample=False) carries gradients to `im`, `depth` and `view` (gradient of the texture lookup,
no silhouette term — plugins/neural_renderer.py).  render_sweep is the batched viewing path beside them (no gradient):
all poses of a sweep in three launches (csrc/sweep.hip).  render_pseudo_sweep is the batched form of the training
renderer itself (relight + render_given_view(grid_sample=True)), for manipulation through the GAN: also three
launches, no gradient.
"""
import math

import torch
import torch.nn as nn

from .. import fused_geometry as fg
from ..plugins import neural_renderer as nr
from .utils import get_face_idx, get_grid, get_textures_from_im, get_transform_matrices

EPS = 1e-7


class Renderer():
    def __init__(self, cfgs, image_size, min_depth, max_depth, device="cuda"):
        self.device = torch.device(device)
        self.image_size = image_size
        self.min_depth = min_depth
        self.max_depth = max_depth
        self.rot_center_depth = cfgs.get('rot_center_depth', (self.min_depth + self.max_depth) / 2)
        self.fov = cfgs.get('fov', 10)
        self.tex_cube_size = cfgs.get('tex_cube_size', 2)
        self.renderer_min_depth = cfgs.get('renderer_min_depth', 0.1)
        self.renderer_max_depth = cfgs.get('renderer_max_depth', 10.)

        # pinhole intrinsics (renderer.py:35-46):  d * K^-1 (u, v, 1)^T = (x, y, z)^T
        R = torch.eye(3, device=self.device).unsqueeze(0)
        t = torch.zeros(1, 3, dtype=torch.float32, device=self.device)
        fx = (self.image_size - 1) / 2 / (math.tan(self.fov / 2 * math.pi / 180))
        fy = (self.image_size - 1) / 2 / (math.tan(self.fov / 2 * math.pi / 180))
        cx = (self.image_size - 1) / 2
        cy = (self.image_size - 1) / 2
        K = torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]], dtype=torch.float32,
                         device=self.device)
        self.inv_K_origin = torch.inverse(K).unsqueeze(0)
        self.K_origin = K.unsqueeze(0)
        self.inv_K = self.inv_K_origin.clone()
        self.K = self.K_origin.clone()
        self.renderer = nr.Renderer(camera_mode='projection',
                                    light_intensity_ambient=1.0,
                                    light_intensity_directional=0.,
                                    K=self.K, R=R, t=t,
                                    near=self.renderer_min_depth, far=self.renderer_max_depth,
                                    image_size=self.image_size, orig_size=self.image_size,
                                    fill_back=True,
                                    background_color=[1, 1, 1])
        self._centroid = torch.tensor([0., 0., self.rot_center_depth], device=self.device).view(1, 1, 3)
        self._rays = {}
        self._K9 = (fx, 0., cx, 0., fy, cy, 0., 0., 1.)  # host copy of K for the fused kernels
        # fused = True: on CUDA tensors the geometry chains below run as single libg2s kernels
        # (csrc/geometry.hip); the torch code in each method is the specification they are tested
        # against and the path for CPU tensors.
        self.fused = True

    def _use_fused(self, t):
        return self.fused and t.is_cuda and t.dtype == torch.float32

    def _const(self, key, make):
        """Device constants are built once: a host->device copy inside the hot loop would also make
        the iteration impossible to record into a HIP graph."""
        v = self._rays.get(key)
        if v is None:
            v = self._rays[key] = make()
        return v

    def set_transform_matrices(self, view):
        if self._use_fused(view) and view.size(1) == 6:
            self.rot_mat, self.trans_xyz = fg.view_transform(view)
        else:
            self.rot_mat, self.trans_xyz = get_transform_matrices(view)

    def set_view(self, view, rot_scale, txy_scale, tz_scale):
        """set_transform_matrices(get_view_transformation(view)) of GAN2Shape/model.py:119-120,330-335
        in one step: angles = view[:, :3] * rot_scale, t = (view[:, 3:5] * txy, view[:, 5] * tz)."""
        if self._use_fused(view):
            self.rot_mat, self.trans_xyz = fg.view_transform(view, rot_scale, txy_scale, tz_scale)
        else:
            self.set_transform_matrices(torch.cat([view[:, :3] * rot_scale, view[:, 3:5] * txy_scale,
                                                   view[:, 5:] * tz_scale], 1))

    def rotate_pts(self, pts, rot_mat):
        centroid = self._centroid.to(pts.device)
        pts = pts - centroid          # move to centroid
        pts = pts.matmul(rot_mat.transpose(2, 1))  # rotate
        return pts + centroid         # move back

    def translate_pts(self, pts, trans_xyz):
        return pts + trans_xyz

    def _pixel_rays(self, h, w, device):
        """K^-1 (u, v, 1)^T for every pixel, (1, h, w, 3): constant, built once."""
        key = (h, w, str(device))
        r = self._rays.get(key)
        if r is None:
            grid_2d = get_grid(1, h, w, normalize=False, device=device)
            grid_3d = torch.cat((grid_2d, torch.ones(1, h, w, 1, device=device)), dim=3)
            inv_K = self.inv_K.to(device)
            r = grid_3d.to(inv_K.dtype).matmul(inv_K.transpose(2, 1))    # (a float64 check sets K / inv_K to double)
            self._rays[key] = r
        return r

    def depth_to_3d_grid(self, depth):
        b, h, w = depth.shape
        return self._pixel_rays(h, w, depth.device) * depth.unsqueeze(-1)

    def grid_3d_to_2d(self, grid_3d):
        b, h, w, _ = grid_3d.shape
        grid_2d = grid_3d / grid_3d[..., 2:]
        grid_2d = grid_2d.matmul(self.K.to(grid_3d.device).transpose(2, 1))[:, :, :, :2]
        WH = self._const(("wh", h, w, str(grid_3d.device)), lambda: torch.tensor(
            [w - 1, h - 1], dtype=torch.float32, device=grid_3d.device).view(1, 1, 1, 2))
        return grid_2d / WH * 2. - 1.  # normalize to -1~1

    def get_warped_3d_grid(self, depth):
        b, h, w = depth.shape
        if self._use_fused(depth):
            rays = self._pixel_rays(h, w, depth.device).reshape(-1, 3)
            return fg.warp_verts(depth, rays, self.rot_mat, self.trans_xyz,
                                 self.rot_center_depth).reshape(b, h, w, 3)
        grid_3d = self.depth_to_3d_grid(depth).reshape(b, -1, 3)
        grid_3d = self.rotate_pts(grid_3d, self.rot_mat)
        grid_3d = self.translate_pts(grid_3d, self.trans_xyz)
        return grid_3d.reshape(b, h, w, 3)

    def get_inv_warped_3d_grid(self, depth):
        b, h, w = depth.shape
        grid_3d = self.depth_to_3d_grid(depth).reshape(b, -1, 3)
        grid_3d = self.translate_pts(grid_3d, -self.trans_xyz)
        grid_3d = self.rotate_pts(grid_3d, self.rot_mat.transpose(2, 1))
        return grid_3d.reshape(b, h, w, 3)

    def get_warped_2d_grid(self, depth):
        return self.grid_3d_to_2d(self.get_warped_3d_grid(depth))

    def canon_mask(self, depth, mask):
        """The object mask of the input image carried into the canonical frame (added; the reference leaves the
        place open, model.py:165-172): every canonical pixel reads `mask` where the view set by set_view /
        set_transform_matrices puts it in the input image,
            grid_sample(mask, get_warped_2d_grid(depth), bilinear, zeros padding, align_corners=True).detach().
        depth (B,S,S) canonical; mask (B,1,S,S) or (1,1,S,S) (shared by the batch), float in [0, 1] -> (B,1,S,S), no
        gradient.  One launch on the GPU (g2s_canon_mask, csrc/canon_mask.hip); the torch composition below is its
        specification and the route of CPU and float64 tensors."""
        b, h, w = depth.shape
        if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[0] not in (1, b) or tuple(mask.shape[2:]) != (h, w):
            raise ValueError(f"canon_mask: mask must be ({b},1,{h},{w}) or (1,1,{h},{w}), got {tuple(mask.shape)}")
        mask = mask.detach().to(device=depth.device, dtype=depth.dtype)
        if self._use_fused(depth):
            rays = self._pixel_rays(h, w, depth.device).reshape(-1, 3)
            return fg.canon_mask(depth.detach(), rays, self.rot_mat, self.trans_xyz, self._K9,
                                 self.rot_center_depth, mask)
        with torch.no_grad():
            grid = self.get_warped_2d_grid(depth)
            return nn.functional.grid_sample(mask.expand(b, 1, h, w), grid, mode='bilinear', padding_mode='zeros',
                                             align_corners=True)

    def get_inv_warped_2d_grid(self, depth):
        if self._use_fused(depth):
            b, h, w = depth.shape
            rays = self._pixel_rays(h, w, depth.device).reshape(-1, 3)
            return fg.inv_warp_grid(depth, rays, self.rot_mat, self.trans_xyz, self._K9,
                                    self.rot_center_depth)
        return self.grid_3d_to_2d(self.get_inv_warped_3d_grid(depth))

    def warp_canon_depth(self, canon_depth):
        b, h, w = canon_depth.shape
        grid_3d = self.get_warped_3d_grid(canon_depth).reshape(b, -1, 3)
        faces = get_face_idx(b, h, w, device=canon_depth.device)
        warped_depth = self.renderer.render_depth(grid_3d, faces)
        # allow some margin out of valid range
        margin = (self.max_depth - self.min_depth) / 2
        from ..op import clamp
        return clamp(warped_depth, self.min_depth - margin, self.max_depth + margin)

    def get_normal_from_depth(self, depth):
        b, h, w = depth.shape
        if self._use_fused(depth):
            return fg.normal_from_depth(depth, self._pixel_rays(h, w, depth.device).reshape(-1, 3))
        grid_3d = self.depth_to_3d_grid(depth)
        tu = grid_3d[:, 1:-1, 2:] - grid_3d[:, 1:-1, :-2]
        tv = grid_3d[:, 2:, 1:-1] - grid_3d[:, :-2, 1:-1]
        normal = torch.linalg.cross(tu, tv, dim=3)
        # border pixels get (0, 0, 1)
        normal = nn.functional.pad(normal.permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1)
        def make_border():
            border = torch.zeros(1, h, w, 3, device=depth.device)
            border[..., 2] = 1
            border[:, 1:-1, 1:-1] = 0
            return border
        normal = normal + self._const(("border", h, w, str(depth.device)), make_border)
        return normal / (((normal ** 2).sum(3, keepdim=True)) ** 0.5 + EPS)

    def downscale_K(self, downscale):
        """renderer.py:56-59."""
        if downscale > 1:
            self.K = torch.cat((self.K_origin[:, 0:2] / downscale, self.K_origin[:, 2:]), dim=1)
            self.inv_K = torch.inverse(self.K[0]).unsqueeze(0)
            self._rays.clear()
            self._K9 = tuple(float(v) for v in self.K[0].reshape(9).tolist())
            # like the reference, the nr.Renderer built in __init__ keeps the original intrinsics

    # ------------------------------------------------------------------ texture path (differentiable)
    def _render_textured(self, verts, im):
        """render_rgb of the grid mesh `verts` (b, h*w, 3) coloured by `im` (b, c, h, w), clamped to
        [-1, 1] (renderer.py:196,272)."""
        b, c, h, w = im.shape
        faces = get_face_idx(b, h, w, device=im.device)
        textures = get_textures_from_im(im, tx_size=self.tex_cube_size)
        return self.renderer.render_rgb(verts, faces, textures).clamp(min=-1., max=1.)

    def _warp_by_grid_sample(self, im, depth, view):
        self.set_transform_matrices(view)
        recon_depth = self.warp_canon_depth(depth)
        grid = self.get_inv_warped_2d_grid(recon_depth)
        return nn.functional.grid_sample(im, grid, mode='bilinear', align_corners=True)

    def _canonical_mesh(self, depth, v_before):
        """Vertices of the depth mesh, taken back to the canonical pose when the depth was predicted
        under view `v_before` (renderer.py:166-170,208-212)."""
        b = depth.shape[0]
        verts = self.depth_to_3d_grid(depth).reshape(b, -1, 3)
        if v_before is not None:
            rot_mat, trans_xyz = get_transform_matrices(v_before)
            verts = self.rotate_pts(self.translate_pts(verts, -trans_xyz), rot_mat.transpose(2, 1))
        return verts

    def _sweep(self, im, depth, poses, v_before, v_after, grid_sample, verts):
        """One rendering per pose = (rx, ry, rz) angle triple -> (b, len(poses), c, h, w)."""
        b = im.shape[0]
        frames = []
        for i, angles in enumerate(poses):
            if grid_sample:
                view = torch.tensor([list(angles) + [0., 0., 0.]], dtype=torch.float32, device=im.device)
                if v_before is not None:
                    view = view - v_before
                frames.append(self._warp_by_grid_sample(im, depth, view))
                continue
            rot_i, _ = get_transform_matrices(torch.tensor([list(angles)], dtype=torch.float32, device=im.device))
            posed = self.rotate_pts(verts, rot_i.repeat(b, 1, 1))
            if v_after is not None:
                v_i = v_after[i] if v_after.dim() == 3 else v_after
                rot_mat, trans_xyz = get_transform_matrices(v_i)
                posed = self.translate_pts(self.rotate_pts(posed, rot_mat), trans_xyz)
            frames.append(self._render_textured(posed, im))
        return torch.stack(frames, 1)

    def render_yaw(self, im, depth, v_before=None, v_after=None, rotations=None, maxr=90, nsample=9,
                   grid_sample=False, crop_mesh=None):
        """Yaw sweep of the textured depth mesh (renderer.py:141-198)."""
        grid_3d = self.depth_to_3d_grid(depth)
        if crop_mesh is not None:   # flatten the border band onto its inner neighbour (renderer.py:145-158)
            grid_3d = grid_3d.clone()
            top, bottom, left, right = crop_mesh
            if top > 0:
                grid_3d[:, :top, :, 1:] = grid_3d[:, top:top + 1, :, 1:]
            if bottom > 0:
                grid_3d[:, -bottom:, :, 1:] = grid_3d[:, -bottom - 1:-bottom, :, 1:]
            if left > 0:
                grid_3d[:, :, :left, 0::2] = grid_3d[:, :, left:left + 1, 0::2]
            if right > 0:
                grid_3d[:, :, -right:, 0::2] = grid_3d[:, :, -right - 1:-right, 0::2]
        b = im.shape[0]
        verts = grid_3d.reshape(b, -1, 3)
        if v_before is not None:
            rot_mat, trans_xyz = get_transform_matrices(v_before)
            verts = self.rotate_pts(self.translate_pts(verts, -trans_xyz), rot_mat.transpose(2, 1))
        if rotations is None:
            rotations = torch.linspace(-math.pi / 180 * maxr, math.pi / 180 * maxr, nsample)
        poses = [(0., float(r), 0.) for r in rotations]
        return self._sweep(im, depth, poses, v_before, v_after, grid_sample, verts)

    def render_view(self, im, depth, v_before=None, rotations=None, maxr=[20, 90], nsample=[5, 9],
                    grid_sample=False):
        """Yaw sweep followed by a pitch sweep (renderer.py:200-250)."""
        verts = self._canonical_mesh(depth, v_before)
        pitch = torch.linspace(-math.pi / 180 * maxr[0], math.pi / 180 * maxr[0], nsample[0])
        yaw = torch.linspace(-math.pi / 180 * maxr[1], math.pi / 180 * maxr[1], nsample[1])
        poses = [(0., float(y), 0.) for y in yaw] + [(float(p), 0., 0.) for p in pitch]
        return self._sweep(im, depth, poses, v_before, None, grid_sample, verts)

    # ------------------------------------------------------------------ viewing path (batched, no gradient)
    def sweep_pose(self, rotations, v_before=None, v_after=None, b=1):
        """(b, V, 12) = row-major A, then t, of every frame: the chain `_canonical_mesh` and `_sweep` apply one
        step after another (undo of `v_before`, the sweep rotation about the rotation centre, `v_after`) composed
        into one affine map per frame — see `compose_sweep_pose`."""
        return compose_sweep_pose(rotations, v_before, v_after, self.rot_center_depth, b)

    def render_sweep(self, im, depth, rotations, v_before=None, v_after=None, mode="texture", light=None,
                     normal=None, faces=None, grey=0.7, background=None, return_alpha=False, return_depth=False,
                     max_frames=None):
        """All frames of a pose sweep of the depth mesh in three launches per chunk (g2s_sweep_verts,
        g2s_raster_depth_fwd, g2s_sweep_shade; csrc/sweep.hip) -> (B, V, Cout, S, S), S = image_size.

        im (B,C,h,w) and `normal` (B,h,w,3; default get_normal_from_depth(depth)) are read in place as per-vertex
        attributes shared by the V frames of an image.  rotations: (V,3) or (B,V,3) angle triples in the convention
        of get_transform_matrices; v_before (B,k) / v_after (B,k) or (V,B,k) as in render_yaw.  mode: "texture"
        (the interpolated image), "shaded" ((im/2+0.5) * (la + lb max(0, n.l)) * 2 - 1, model.py get_shading with
        `im` as albedo), "shape" (the same with the constant `grey`), "normal" (the rotated unit normal).  light:
        (V,5) or (B,V,5) rows (la, lb, lx, ly, lz), direction in the frame's camera space, used as given.  faces:
        None (the grid of get_face_idx; needs h = w = image_size) or one (F,3) int32 list for the batch.
        background: Cout floats (default: the renderer's, white).  Runs under no_grad; frames are processed in
        chunks of at most `max_frames` (default: what keeps the saved raster maps of a chunk under 256 MiB), and the
        result does not depend on the chunking.  Returns rgb, then alpha (B,V,S,S) and depth (B,V,S,S) on request."""
        from .. import lib as _lib
        _lib.require_cuda(im, depth)
        with torch.no_grad():
            b, c, h, w = im.shape
            dev = im.device
            S = self.image_size
            r = self.renderer
            verts = self.depth_to_3d_grid(depth.float()).reshape(b, -1, 3)
            pose = self.sweep_pose(torch.as_tensor(rotations, dtype=torch.float32, device=dev),
                                   v_before, v_after, b)
            V = pose.shape[1]
            m = nr._sweep_mode(mode)
            if m != 0 and normal is None:
                normal = self.get_normal_from_depth(depth.float().contiguous())
            if m in (1, 2):
                if light is None:
                    raise ValueError("modes shaded and shape need `light`: (V, 5) or (B, V, 5)")
                light = torch.as_tensor(light, dtype=torch.float32, device=dev)
                light = light.expand(b, V, 5) if light.dim() == 2 else light
                if light.shape != (b, V, 5):
                    raise ValueError(f"light must be (V, 5) or (B, V, 5) with V = {V}, got {tuple(light.shape)}")
            else:
                light = None
            if faces is not None and faces.dim() == 3:
                faces = r._shared_faces(faces, h * w, S)
            bg = r.background_color if background is None else background
            ssaa = 2 if r.anti_aliasing else 1
            bc, vc = sweep_chunks(b, V, max_frames, (S * ssaa) ** 2 * 16 + h * w * 12)
            K = r._host_K(r.K)
            result = sweep_assemble(b, V, bc, vc, lambda sb, sv: nr.sweep_frames(
                verts[sb], pose[sb, sv], faces, im[sb], None if normal is None else normal[sb],
                None if light is None else light[sb, sv].reshape(-1, 5), K, r.orig_size, S,
                r.anti_aliasing, r.fill_back, r.near, r.far, bg, grey, m, return_alpha, return_depth))
        result = tuple(x for x in result if x is not None)     # rgb, then alpha and depth where asked for
        return result[0] if len(result) == 1 else result

    def pseudo_pose(self, views, base_view=None, b=1):
        """(b, V, 12) = row-major A, then t, of the posed-vertex map of `get_warped_3d_grid` for every frame: with c
        the rotation centre and (R, t_view) the view's transform, p -> R (p - c) + c + t_view, so A = R and
        t = c + t_view - R c (`compose_sweep_pose` with the view's translation as its `v_after`, written out: a handful
        of small products on the device, no host synchronisation).  base_view (b,6): each frame's view is applied
        AFTER it, A = R R0 and t = c + t_view + R t0 - A c.  views: (V,6) or (b,V,6)."""
        if views.dim() == 2:
            views = views.unsqueeze(0).expand(b, -1, -1)
        V = views.shape[1]

        def transform(v):
            v = v.contiguous()
            return fg.view_transform(v) if self._use_fused(v) else get_transform_matrices(v)
        R, t = transform(views.reshape(b * V, 6))
        A, t = R.view(b, V, 3, 3), t.view(b, V, 3)
        c = self._centroid.to(device=views.device, dtype=views.dtype).view(1, 1, 3)
        if base_view is not None:
            R0, t0 = transform(base_view.to(views.dtype))
            t = t + t0.view(b, 1, 1, 3).matmul(A.transpose(3, 2)).squeeze(2)                  # R t0
            A = A.matmul(R0.view(b, 1, 3, 3))
        t = (c + t) - c.unsqueeze(0).matmul(A.transpose(3, 2)).squeeze(2)                     # - A c
        return torch.cat([A.reshape(b, V, 9), t], 2).contiguous()

    def render_pseudo_sweep(self, albedo, normal, depth, views, lights=None, mask=None, max_frames=None,
                            base_view=None):
        """The pseudo images of `sample_pseudo_imgs` for GIVEN views and lights, all frames in three launches per
        chunk (g2s_sweep_verts, g2s_raster_depth_fwd, g2s_sweep_pseudo; csrc/sweep.hip) ->
        (im (B,V,C,S,S), mask (B,V,1,S,S)).

        Per frame this is relight + render_given_view(grid_sample=True): the canonical depth mesh posed by the view
        and rasterised, the clamp of warp_canon_depth, the inverse warp, the bilinear read of the relit canonical
        image clamped to [-1, 1] and the nearest read of the mask.  albedo (B,C,S,S); normal (B,S,S,3) canonical unit
        normals; depth (B,S,S); views (V,6) or (B,V,6) in the units `set_transform_matrices` takes; lights (V,4) or
        (B,V,4) raw (a, b, dx, dy) as the lighting net gives them (g2s_shading_fwd's convention), None = `albedo` is
        sampled as given; mask (B,S,S) or (B,1,S,S), None = all ones.  base_view (B,6): every view is composed after
        it (`pseudo_pose`).  Runs under no_grad, GPU only; frames go in chunks of at most `max_frames` (default: what
        keeps the posed vertices of a chunk under 256 MiB) and the result does not depend on the chunking."""
        from .. import lib as _lib
        _lib.require_cuda(albedo, normal, depth, mask)
        with torch.no_grad():
            b, c, h, w = albedo.shape
            dev = albedo.device
            S = self.image_size
            if (h, w) != (S, S) or tuple(depth.shape) != (b, S, S):
                raise ValueError(f"albedo must be (B,C,{S},{S}) and depth (B,{S},{S}), got {tuple(albedo.shape)} and "
                                 f"{tuple(depth.shape)}")
            views = torch.as_tensor(views, dtype=torch.float32, device=dev)
            if views.dim() not in (2, 3) or views.shape[-1] != 6 or (views.dim() == 3 and views.shape[0] != b):
                raise ValueError(f"views must be (V, 6) or (B={b}, V, 6), got {tuple(views.shape)}")
            V = views.shape[-2]
            if lights is not None:
                lights = torch.as_tensor(lights, dtype=torch.float32, device=dev)
                lights = lights.expand(b, V, 4) if lights.dim() == 2 and lights.shape == (V, 4) else lights
                if lights.shape != (b, V, 4):
                    raise ValueError(f"lights must be (V, 4) or (B, V, 4) with V = {V}, got {tuple(lights.shape)}")
                if normal is None:
                    raise ValueError("relighting reads the canonical normals")
            if mask is not None:
                mask = mask.reshape(b, S, S) if mask.numel() == b * S * S else mask
                if tuple(mask.shape) != (b, S, S):
                    raise ValueError(f"mask must be (B,{S},{S}) or (B,1,{S},{S}), got {tuple(mask.shape)}")
            bc, vc = sweep_chunks(b, V, max_frames, S * S * 12 + S * S * 4)
            r = self.renderer
            margin = (self.max_depth - self.min_depth) / 2
            rays = self._pixel_rays(S, S, dev).reshape(-1, 3)
            verts = (rays.unsqueeze(0) * depth.float().reshape(b, -1, 1)).contiguous()
            pose = self.pseudo_pose(views, base_view, b)
            K = self._K9
            out, mout = sweep_assemble(b, V, bc, vc, lambda sb, sv: nr.pseudo_frames(
                verts[sb], pose[sb, sv], rays, K, albedo[sb], None if lights is None else normal[sb],
                None if lights is None else lights[sb, sv].reshape(-1, 4), None if mask is None else mask[sb],
                self.min_depth - margin, self.max_depth + margin, r.orig_size, S, r.anti_aliasing, r.fill_back))
        return out, mout.unsqueeze(2)

    def render_given_view(self, im, depth, view, mask=None, grid_sample=True):
        """renderer.py:252-277: warp `im` (and `mask`) to `view` — by inverse-warp sampling
        (grid_sample=True, the training path) or by rendering the textured mesh."""
        if not grid_sample:
            b = im.shape[0]
            rot_mat, trans_xyz = get_transform_matrices(view)
            verts = self.depth_to_3d_grid(depth).reshape(b, -1, 3)
            verts = self.translate_pts(self.rotate_pts(verts, rot_mat), trans_xyz)
            warped_images = self._render_textured(verts, im)
            if mask is not None:
                return warped_images, self._render_textured(verts, mask)
            return warped_images
        self.set_transform_matrices(view)
        recon_depth = self.warp_canon_depth(depth)
        grid_2d_from_canon = self.get_inv_warped_2d_grid(recon_depth)
        warped_images = nn.functional.grid_sample(im, grid_2d_from_canon, mode='bilinear',
                                                  align_corners=True)
        if mask is not None:
            warped_mask = nn.functional.grid_sample(mask, grid_2d_from_canon, mode='nearest',
                                                    align_corners=True)
            return warped_images, warped_mask
        return warped_images


def sweep_chunks(b, V, max_frames, bytes_per_frame, budget=256 << 20):
    """(images, frames per image) of one chunk of a b x V sweep: at most `max_frames` frames (default: what keeps
    `bytes_per_frame` x frames under `budget`), whole images first."""
    if max_frames is None:
        max_frames = max(1, budget // bytes_per_frame)
    max_frames = int(max_frames)
    if max_frames < 1:
        raise ValueError("max_frames must be at least 1")
    bc = min(b, max_frames)
    return bc, min(V, max(1, max_frames // bc))


def sweep_assemble(b, V, bc, vc, run):
    """The (b, V, ...) results of a sweep from its chunks of bc images x vc frames: run(sb, sv) renders the chunk
    of the image slice sb and the frame slice sv and returns a tuple of (len sb, len sv, ...) tensors, or None where
    a result is not wanted.  A single chunk's tensors are returned as they are, without a copy."""
    outs = None
    for b0 in range(0, b, bc):
        for v0 in range(0, V, vc):
            sb, sv = slice(b0, b0 + bc), slice(v0, v0 + vc)
            parts = run(sb, sv)
            if bc >= b and vc >= V:
                return parts
            if outs is None:
                outs = [None if p is None else torch.empty((b, V) + tuple(p.shape[2:]), dtype=p.dtype, device=p.device)
                        for p in parts]
            for o, p in zip(outs, parts):
                if o is not None:
                    o[sb, sv] = p
    return tuple(outs)


def compose_sweep_pose(rotations, v_before, v_after, rot_center_depth, b=1):
    """The pose chain of Renderer._canonical_mesh / Renderer._sweep as ONE affine map per frame -> (b, V, 12):
    row-major A (3x3), then t.  With c the rotation centre (0, 0, rot_center_depth), (R0, t0) = v_before, Ri the
    sweep rotation of frame i and (R2, t2) = v_after (of that frame), the chain is
        p1 = R0^T (p - t0 - c) + c,   p2 = Ri (p1 - c) + c,   p3 = R2 (p2 - c) + c + t2
    so  A = R2 Ri R0^T  and  t = c + t2 - A (c + t0).  rotations: (V,3) or (b,V,3); v_before: (b,k) or None; v_after:
    (b,k), (V,b,k) or None.  Small (b,V,3,3) torch products in the dtype and on the device of `rotations`: no host
    synchronisation."""
    rot = rotations
    if rot.dim() == 2:
        rot = rot.unsqueeze(0).expand(b, -1, -1)
    V = rot.shape[1]
    dt, dev = rot.dtype, rot.device
    Ri, _ = get_transform_matrices(rot.reshape(b * V, 3))
    A = Ri.view(b, V, 3, 3)
    c = torch.zeros(3, dtype=dt, device=dev)
    c[2] = rot_center_depth
    inner = c.view(1, 1, 3).expand(b, V, 3)          # c + t0
    outer = inner                                    # c + t2
    if v_before is not None:
        R0, t0 = get_transform_matrices(v_before.to(dt))
        A = A.matmul(R0.transpose(2, 1).unsqueeze(1))
        inner = inner + t0.view(b, 1, 3)
    if v_after is not None:
        va = v_after.to(dt)
        va = va.unsqueeze(0).expand(V, -1, -1) if va.dim() == 2 else va          # (V, b, k)
        R2, t2 = get_transform_matrices(va.reshape(V * b, -1))
        A = R2.view(V, b, 3, 3).transpose(0, 1).matmul(A)
        outer = outer + t2.view(V, b, 3).transpose(0, 1)
    t = outer - A.matmul(inner.unsqueeze(-1)).squeeze(-1)
    return torch.cat([A.reshape(b, V, 9), t], 2).contiguous()
