/*
 * g2s.h — C ABI of libg2s.so, the MI355X (gfx950) native kernels behind the GAN2Shape
 * inner loop.  This header is the drop-in boundary: every entry point replaces one native
 * (CUDA) interface the reference binds by name.  Reference citations are relative to
 * /root/reference (alessioGalatolo/GAN-2D-to-3D).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless stated;
 *   - the caller owns and allocates every buffer (the library never allocates device memory,
 *     never synchronises, never throws);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - returns G2S_OK (0) or a negative error code; g2s_last_error() gives a thread-local message;
 *   - re-entrant.  Thread-local state: the error string and the two tuning overrides
 *     g2s_modconv_tune / g2s_raster_tune (off by default; they select among launch configurations
 *     that produce the same results, and only affect the calling thread).  Process-global state:
 *     ONE flag, g2s_set_deterministic (off by default).  No environment variable is read.
 */
#ifndef G2S_H
#define G2S_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G2S_ABI_VERSION 1

#define G2S_OK 0
#define G2S_ERR_INVALID (-1)   /* bad argument (shape / pointer / dtype / unsupported combination) */
#define G2S_ERR_LAUNCH (-2)    /* hipLaunchKernel / hipMemsetAsync reported an error              */
#define G2S_ERR_WORKSPACE (-3) /* workspace too small                                              */

#define G2S_F32 0
#define G2S_F16 1

typedef void *g2s_stream_t; /* hipStream_t */

int g2s_abi_version(void);
const char *g2s_last_error(void);

/* Reproducible launches (no reference counterpart: torch.use_deterministic_algorithms is the
 * analogue a maintainer would reach for).  on = 1: every convolution launch of the process takes a
 * partition in which ONE workgroup owns each output element — direct kernel split-K 1
 * (conv_launch in csrc/modconv.hip, for the fp32 kernel and the fp16-operand one of csrc/modconv_f16.hip),
 * weight-gradient GEMM without its pixel split (csrc/conv_wgrad_core.h),
 * Winograd split-K / stream-K only with stored slices (workspace given), else whole tiles — so the
 * forward values of every network are bit-identical from run to run and independent of how many
 * workgroups race.  Slower (small layers no longer fill 256 CUs); results differ from the default
 * mode by fp32 summation order only.  What remains order-dependent at the 1e-7 level: the scalar
 * loss accumulators and the gradient scatter of the rasterizer / geometry backward kernels (float
 * atomics over tiles).  Takes effect for launches issued after the call, from any thread. */
int g2s_set_deterministic(int on);
int g2s_get_deterministic(void);

/* Caller-cleared accumulators (no reference counterpart).  The functions below that accumulate into small outputs
 * or workspaces clear them first with a memset of their own — one more launch each (14 of step 3's).  With
 * acc_is_zero = 1 the caller guarantees that the buffer the call adds into is already zero (the Python side carves
 * them from the step's one cleared pool, zeropool.py) and the memset is skipped; it holds for that call only:
 * g2s_warp_verts_bwd / g2s_inv_warp_grid_bwd (gRt), g2s_smooth_loss_fwd (loss), g2s_shading_bwd (glight),
 * g2s_depth_head_bwd (gsum), g2s_grid_sample_bwd (gx, or the deterministic mode's fixed-point workspace),
 * g2s_raster_depth_bwd_ex (grad_verts, or its fixed-point workspace; g2s_raster_depth_bwd passes 0),
 * g2s_raster_rgb_bwd (grad_textures and grad_verts, or its fixed-point workspace), g2s_raster_rgba_bwd (the same and
 * grad_light), g2s_face_light_bwd (there it also means: add to what grad_verts holds). */

/* ------------------------------------------------------------------------------------------
 * Differentiable depth rasterizer.
 * Replaces neural_renderer.Renderer.render_depth(vertices, faces) as called from
 * GAN2Shape/renderer/renderer.py:47-54 (constructor: camera_mode='projection', K, R=I, t=0,
 * fill_back=True, anti_aliasing=True) and :116-125 (warp_canon_depth).  neural_renderer is an
 * external, un-vendored CUDA package (README.md:32-37); semantics per SURVEY.md Appendix A.
 *
 * verts      [B, n_verts, 3] f32, camera-space xyz (after the view transform)
 * faces      [n_faces, 3] i32 vertex ids shared by the whole batch, or NULL = the implicit
 *            regular-grid topology of renderer/utils.py:76-80 get_face_idx(b, S, S) with
 *            n_verts == S*S and n_faces == 2*(S-1)*(S-1)
 * K          HOST pointer, 9 floats row-major, pinhole intrinsics (third row must be 0 0 1)
 * orig_size  neural_renderer `orig_size` (== S here)
 * S          output image size; the raster runs at ssaa*S (ssaa 1 or 2; 2 == anti_aliasing)
 * fill_back  1: each face is also rendered with reversed vertex order (face id + n_faces)
 * depth_out  [B, S, S] f32  after vertical flip and ssaa x ssaa average pooling (un-clamped;
 *            background = far)
 * face_idx_out [B, ssaa*S, ssaa*S] i32 winning face id (-1 background) in UNFLIPPED raster rows,
 *            or NULL when no backward is needed
 * bary_out   [B, ssaa*S, ssaa*S, 3] f32 clamped+renormalised barycentric weights of the winner,
 *            or NULL (must be NULL iff face_idx_out is NULL)
 * workspace  >= g2s_raster_workspace_bytes(B, n_verts, n_faces, S) bytes of device scratch
 * ---------------------------------------------------------------------------------------- */
size_t g2s_raster_workspace_bytes(int B, int n_verts, int n_faces, int S);

int g2s_raster_depth_fwd(const float *verts, const int32_t *faces, int B, int n_verts, int n_faces,
                         int S, const float *K, float orig_size, int ssaa, int fill_back,
                         float near, float far, float *depth_out, int32_t *face_idx_out,
                         float *bary_out, void *workspace, size_t workspace_bytes,
                         g2s_stream_t stream);

/* Tuning hook (tools/bench_raster.py): waves_per_tile = 4 runs the 4 waves of a workgroup on ONE
 * 8x8-sample tile, 1 gives every wave its own tile, 0 restores the built-in choice (4 when
 * B * tiles <= 4096).  Calling thread only; outputs are bit-identical either way.  Any other value is
 * G2S_ERR_INVALID and leaves the setting as it was; g2s_raster_get_tune returns the current one. */
int g2s_raster_tune(int waves_per_tile);
int g2s_raster_get_tune(void);

/* Backward of the above w.r.t. verts (neural_renderer backward_depth_map + vertices_to_faces +
 * projection backward).
 * grad_depth [B, S, S] f32 (gradient of depth_out); grad_verts [B, n_verts, 3] f32 is zero-filled
 * by the callee, then accumulated with float atomics. */
int g2s_raster_depth_bwd(const float *verts, const int32_t *faces, const float *grad_depth,
                         const int32_t *face_idx, const float *bary, int B, int n_verts,
                         int n_faces, int S, const float *K, float orig_size, int ssaa,
                         float *grad_verts, g2s_stream_t stream);

/* The same with the scratch deterministic mode needs (g2s_set_deterministic): the per-vertex sums are
 * then accumulated as 2^-40 fixed point with 64-bit integer atomics in `workspace`
 * (>= g2s_raster_bwd_workspace_bytes(B, n_verts) bytes of device memory), whose result does not depend
 * on the order the tiles arrive in — the gradient is bit-identical from run to run — and converted to
 * grad_verts at the end (range +-8.4e6 per component, resolution 9e-13; non-finite contributions are
 * dropped).  In deterministic mode a NULL / short workspace is G2S_ERR_WORKSPACE — also through
 * g2s_raster_depth_bwd, which passes none; otherwise the workspace is ignored.  acc_is_zero = 1: the buffer the
 * sums go to (the workspace in deterministic mode, else grad_verts) is already zero, no memset. */
size_t g2s_raster_bwd_workspace_bytes(int B, int n_verts);
int g2s_raster_depth_bwd_ex(const float *verts, const int32_t *faces, const float *grad_depth,
                            const int32_t *face_idx, const float *bary, int B, int n_verts,
                            int n_faces, int S, const float *K, float orig_size, int ssaa,
                            float *grad_verts, void *workspace, size_t workspace_bytes, int acc_is_zero,
                            g2s_stream_t stream);

/* Texture path: nr.Renderer.render_rgb(vertices, faces, textures [B,F,ts,ts,ts,C]) as the reference's
 * helpers call it (GAN2Shape/renderer/renderer.py:196,230,248,272,275).
 * Second pass over the maps g2s_raster_depth_fwd saves (run it with the constructor's near / far,
 * renderer.py:51): trilinear read of the winning face's texture cube at perspective-corrected
 * barycentric coordinates (eps = rasterizer_eps, 1e-3 in the package), `background` (HOST pointer, C
 * floats) where no face covers the sample, then the vertical flip + ssaa x ssaa average.
 * rgb_out [B, C, S, S].  PARITY UNPINNED like the depth path. */
int g2s_raster_rgb_fwd(const float *verts, const int32_t *faces, const int32_t *face_idx,
                       const float *bary, const float *textures, int B, int n_verts, int n_faces, int S,
                       int ssaa, int ts, int C, const float *background, float eps, float *rgb_out,
                       g2s_stream_t stream);

/* Backward of the texture pass (replaces the autograd of neural_renderer's render_rgb at the call sites above,
 * renderer.py:265-276 render_given_view(grid_sample=False) among them): GRADIENT OF THE TEXTURE LOOKUP, NO
 * SILHOUETTE TERM.  The winner of every raster sample (face_idx) is held fixed.
 * grad_rgb       [B, C, S, S] gradient of rgb_out
 * grad_textures  [B, F, ts, ts, ts, C]: adjoint of the trilinear read (exact, the forward is affine in the
 *                textures); a reversed fill_back copy adds to the cube of its geometric face with axes 0 and 2
 *                swapped; background samples add nothing.  NULL: not computed.
 * grad_verts     [B, n_verts, 3]: colour -> cube coordinates t_k (zero where a clamp is active) -> barycentric
 *                weights and vertex depths -> projected vertices (the weights are the screen-space barycentrics of
 *                the sample centre) -> camera xyz.  The external package instead approximates the effect of moving
 *                silhouettes with an edge-sweep heuristic that is not rebuilt here (nothing pins it).  NULL: not
 *                computed, and its arithmetic is skipped.  Both NULL is G2S_ERR_INVALID.
 * K, orig_size   as g2s_raster_depth_fwd; the other arguments as g2s_raster_rgb_fwd (same requirements: ts 1..8,
 *                C 1..4, ssaa 1 or 2, implicit-topology sizes when faces is NULL).
 * Sums use float atomics.  In deterministic mode (g2s_set_deterministic) they are 2^-40 fixed point with 64-bit
 * integer atomics in `workspace` (>= g2s_raster_rgb_bwd_workspace_bytes bytes of device memory; range +-8.4e6,
 * resolution 9e-13, non-finite contributions dropped) and both gradients are bit-identical from run to run; a NULL
 * / short workspace is then G2S_ERR_WORKSPACE; otherwise the workspace is ignored.  acc_is_zero = 1: the buffers
 * the sums go to (the workspace in deterministic mode, else every non-NULL gradient) are already zero, no memset. */
size_t g2s_raster_rgb_bwd_workspace_bytes(int B, int n_verts, int n_faces, int ts, int C);
int g2s_raster_rgb_bwd(const float *verts, const int32_t *faces, const int32_t *face_idx, const float *bary,
                       const float *textures, const float *grad_rgb, int B, int n_verts, int n_faces, int S,
                       const float *K, float orig_size, int ssaa, int ts, int C, float eps,
                       float *grad_textures, float *grad_verts, void *workspace, size_t workspace_bytes,
                       int acc_is_zero, g2s_stream_t stream);

/* Per-face light factor: replaces nr.lighting(faces, textures, intensity_ambient, intensity_directional,
 * color_ambient, color_directional, direction) as nr.Renderer.render / render_rgb apply it (flat shading per
 * face), evaluated on the camera-space vertices (after R, t, before projection).  PARITY UNPINNED, as recalled
 * (SURVEY.md Appendix A), like the rasterizer entries.  For the face (v0, v1, v2):
 *     n = cross(v0 - v1, v2 - v1) / max(|cross|, 1e-5),  light[c] = ambient[c] + directional[c] * max(0, dot(n, direction))
 * and the reversed fill_back copy (v2, v1, v0) has the normal -n.
 * verts, faces, B, n_verts, n_faces   as g2s_raster_depth_fwd (faces NULL: implicit regular grid of side S;
 *                                     S is not read otherwise)
 * ambient, directional, direction     HOST pointers, 3 floats each: intensity_ambient * color_ambient,
 *                                     intensity_directional * color_directional, light direction (used as given)
 * light_out  [B, n_faces * (1 + fill_back), 3], indexed like the ids in face_idx (reversed copies at f + n_faces) */
int g2s_face_light_fwd(const float *verts, const int32_t *faces, int B, int n_verts, int n_faces, int S,
                       int fill_back, const float *ambient, const float *directional, const float *direction,
                       float *light_out, g2s_stream_t stream);

/* Backward of the above w.r.t. verts (replaces the autograd of nr.lighting; PARITY UNPINNED, as recalled): through
 * the max, the dot product, the normalisation (no gradient while its 1e-5 clamp is active) and the cross product.
 * grad_light [B, n_faces * (1 + fill_back), 3].  The gradient is ADDED to grad_verts [B, n_verts, 3] (camera xyz):
 *   acc_is_zero = 0  the call clears what it adds into first: grad_verts ends as the light's gradient alone.
 *   acc_is_zero = 1  no memset: grad_verts holds zeros or a camera-space gradient this one joins (Renderer.render adds
 *                    it to the texture pass's), and in deterministic mode the workspace is already zero.
 * Float atomics; in deterministic mode (g2s_set_deterministic) the sums are 2^-40 fixed point in `workspace`
 * (>= g2s_raster_bwd_workspace_bytes(B, n_verts) bytes, as g2s_raster_depth_bwd_ex; NULL / short:
 * G2S_ERR_WORKSPACE) and reach grad_verts in one rounding per element: bit-identical from run to run. */
int g2s_face_light_bwd(const float *verts, const int32_t *faces, const float *grad_light, int B, int n_verts,
                       int n_faces, int S, int fill_back, const float *directional, const float *direction,
                       float *grad_verts, void *workspace, size_t workspace_bytes, int acc_is_zero,
                       g2s_stream_t stream);

/* Texture pass with light and alpha: the superset of g2s_raster_rgb_fwd that nr.Renderer.render needs (rgb and
 * alpha of one rasterization; PARITY UNPINNED, as recalled).  Arguments as g2s_raster_rgb_fwd, plus
 * light      NULL, or [B, n_faces * (1 + fill_back), 3] (g2s_face_light_fwd; C must be 3): the sample's colour is
 *            multiplied channel-wise by light[b, winner] before background selection; background samples stay unlit.
 * fill_back  what g2s_raster_depth_fwd was given for these maps (read only with light)
 * alpha_out  NULL, or [B, S, S]: the share of the pixel's ssaa^2 samples that have a winner, flipped and averaged
 *            like rgb.
 * textures, light and rgb_out all NULL: alpha alone (nr.Renderer.render_silhouettes), no texture is read; only
 * face_idx, B, S, ssaa and alpha_out are used. */
int g2s_raster_rgba_fwd(const float *verts, const int32_t *faces, const int32_t *face_idx, const float *bary,
                        const float *textures, const float *light, int B, int n_verts, int n_faces, int S,
                        int ssaa, int ts, int C, int fill_back, const float *background, float eps,
                        float *rgb_out, float *alpha_out, g2s_stream_t stream);

/* Backward of the above (alpha has no gradient: NO SILHOUETTE TERM, as g2s_raster_rgb_bwd).  grad_textures and
 * grad_verts as g2s_raster_rgb_bwd with the incoming colour gradient scaled by the light;
 * grad_light [B, n_faces * (1 + fill_back), 3] (NULL: not computed; needs light) is the sum over the face's samples
 * of grad_colour * unlit colour — feed it to g2s_face_light_bwd.  acc_is_zero and the deterministic mode's fixed-point
 * workspace (>= g2s_raster_rgba_bwd_workspace_bytes bytes) cover all three gradients.  light = grad_light = NULL is
 * g2s_raster_rgb_bwd, bit for bit. */
size_t g2s_raster_rgba_bwd_workspace_bytes(int B, int n_verts, int n_faces, int ts, int C, int fill_back);
int g2s_raster_rgba_bwd(const float *verts, const int32_t *faces, const int32_t *face_idx, const float *bary,
                        const float *textures, const float *light, const float *grad_rgb, int B, int n_verts,
                        int n_faces, int S, const float *K, float orig_size, int ssaa, int ts, int C, int fill_back,
                        float eps, float *grad_textures, float *grad_verts, float *grad_light, void *workspace,
                        size_t workspace_bytes, int acc_is_zero, g2s_stream_t stream);

/* Viewing path (Renderer.render_sweep): V poses per image of the same mesh in three launches — g2s_sweep_verts,
 * g2s_raster_depth_fwd over the B*V posed meshes, g2s_sweep_shade.  No backward.
 *
 * g2s_sweep_verts: out[b*V + v, n] = A[b,v] . verts[b, n] + t[b,v].
 * verts [B, n_verts, 3] canonical camera space; pose [B, V, 12]: row-major 3x3 A, then t; out [B*V, n_verts, 3].
 * B <= 65535. */
int g2s_sweep_verts(const float *verts, const float *pose, float *out, int B, int V, int n_verts,
                    g2s_stream_t stream);

/* g2s_sweep_shade: attribute pass over the maps g2s_raster_depth_fwd saved for the B*V posed meshes (face_idx, bary at
 * ssaa*S, as g2s_raster_rgb_fwd takes them; same flip and ssaa x ssaa average), without texture cubes: the image and
 * the normals are per-vertex attributes of image b = f / V, shared by its V frames.
 * verts      [B*V, n_verts, 3] posed (the output of g2s_sweep_verts)
 * faces      [n_faces, 3] or NULL = implicit regular grid (n_verts == S*S, n_faces == 2*(S-1)*(S-1))
 * attr       [B, C, n_verts] image or albedo (C 1..4); read in modes 0 and 1, may be NULL otherwise
 * normal     [B, n_verts, 3] unit normals in the canonical frame; NULL allowed in mode 0
 * pose       [B, V, 12] as above; only A is read, to rotate the normals; NULL allowed in mode 0
 * light      [B*V, 5] = la, lb, lx, ly, lz, direction in the frame's camera space, used as given; modes 1 and 2
 * fill_back  what g2s_raster_depth_fwd was given (winner ids >= n_faces are the reversed copies: v0 and v2 swapped)
 * background HOST pointer, Cout floats;  grey: the constant albedo of mode 2
 * rgb_out    [B*V, Cout, S, S], Cout = C in modes 0 and 1, 3 in modes 2 and 3;  alpha_out [B*V, S, S] or NULL
 * Per sample with winner (v0, v1, v2), saved weights w and z of the POSED vertices:
 *     D = 1 / sum_k w_k / z_k,  u_k = w_k D / z_k  (no clamp, no renormalisation)
 *     a = sum_k u_k attr[b, :, v_k],  m = sum_k u_k normal[b, v_k],  n = A m / max(|A m|, 1e-12)
 *     mode 0 texture  a
 *     mode 1 shaded   (a / 2 + 0.5) * (la + lb * max(0, n . l)) * 2 - 1   (get_shading, GAN2Shape/model.py:355-358)
 *     mode 2 shape    the same with `grey` in place of a / 2 + 0.5
 *     mode 3 normal   n
 * Samples without a winner take `background` and count 0 for alpha.  No atomics: bit-identical from run to run.
 * Every check precedes the launch: a rejected call leaves the outputs untouched. */
int g2s_sweep_shade(const float *verts, const int32_t *faces, const int32_t *face_idx, const float *bary,
                    const float *attr, const float *normal, const float *pose, const float *light, int B, int V,
                    int n_verts, int n_faces, int S, int ssaa, int C, int fill_back, int mode,
                    const float *background, float grey, float *rgb_out, float *alpha_out, g2s_stream_t stream);

/* g2s_sweep_pseudo: the last launch of the pseudo-view path (Renderer.render_pseudo_sweep: g2s_sweep_verts,
 * g2s_raster_depth_fwd, this).  It is the inverse-warp renderer of render_given_view(grid_sample=True) applied to the
 * relit canonical image (GAN2Shape/model.py:291-328, renderer.py:252-264) for B*V frames in one pass, without forming
 * the relit images, the sampling grid or a 3-channel mask.
 * warped     [B*V, S, S] depth_out of g2s_raster_depth_fwd for the posed meshes, unclamped
 * rays       [S*S, 3] K^-1 (u, v, 1)^T
 * pose       [B, V, 12] the SAME affine map g2s_sweep_verts was given: row-major A, then t
 * K          HOST pointer, 9 floats row-major (rows 0 and 1 are read)
 * albedo     [B, C, S, S], C 1..4;  normal [B, S, S, 3] canonical unit normals, NULL iff light == NULL
 * light      [B*V, 4] raw (a, b, dx, dy) as g2s_shading_fwd takes them, or NULL = no relighting
 * mask       [B, S, S] canonical mask or NULL = all ones
 * im_out     [B*V, C, S, S];  mask_out [B*V, S, S] or NULL
 * Per output pixel p of frame f = b*V + v:
 *     d = clamp(warped[f, p], depth_lo, depth_hi)                    (warp_canon_depth's clamp)
 *     q = A^T (d ray_p - t)                                           (= R^T(d ray - t_view - c) + c of g2s_inv_warp_grid_fwd)
 *     (gx, gy) = (K q / q.z)_xy * 2 / (S - 1) - 1                     (grid_3d_to_2d; q and K q / q.z are computed in double
 *                                                                      and go to texel coordinates directly: the
 *                                                                      normalisation cancels against grid_sample's)
 *     im_out  = clamp(bilinear sample at (gx, gy), -1, 1), align_corners = True, zero padding, taps in the order
 *               nw, ne, sw, se; a tap's value is (albedo / 2 + 0.5) * (a' + b' max(0, n . l)) * 2 - 1 with
 *               a' = a / 2 + 0.5, b' = b / 2 + 0.5, l = (dx, dy, 1) / |(dx, dy, 1)| (g2s_shading_fwd's arithmetic),
 *               or albedo as given when light == NULL
 *     mask_out = nearest sample (round half to even, zero padding) of mask, or of an all-ones image
 * One thread per output pixel; pose and light are wave-uniform loads; S need not be a multiple of anything.  No
 * atomics: bit-identical from run to run and independent of how the caller chunks the frames.
 * Every check precedes the launch: a rejected call leaves the outputs untouched. */
int g2s_sweep_pseudo(const float *warped, const float *rays, const float *pose, const float *K, const float *albedo,
                     const float *normal, const float *light, const float *mask, float depth_lo, float depth_hi,
                     int B, int V, int S, int C, float *im_out, float *mask_out, g2s_stream_t stream);

/* Sample generator (generate.py): the mapping network in one launch, the ordered mean, the image quantiser.
 * No backward.
 *
 * g2s_mapping_fwd: per row of z, in this order
 *     h = z * rsqrt(mean_d(z^2) + 1e-8)                      if pixel_norm
 *     L times:  h = gain * leaky_relu(h W_l^T + b_l, alpha)
 *     out = center + truncation * (h - center)               if center != NULL
 * z [N, D];  w [L, D, D] already multiplied by EqualLinear.scale, row = output feature (as F.linear takes it);
 * b [L, D] already multiplied by lr_mul;  center [D] or NULL;  out [N, D].
 * partial: NULL, or [ceil(N / T), D] with T the tile height the mapping-tile query below returns; row t receives
 * the column sums of `out` over the rows of tile t (rows t*T .. min(N, (t+1)*T) - 1, ascending).
 * D a multiple of 32 in 32..512, 1 <= L <= 16, N >= 1; z, w and out 16-byte aligned.  Rows past N are neither read
 * nor stored.  No atomics: a row's result depends on that row alone, and is the same from run to run. */
int g2s_mapping_tile(void);
int g2s_mapping_fwd(const float *z, const float *w, const float *b, const float *center, float *out,
                    float *partial, int64_t N, int D, int L, int pixel_norm, float alpha, float gain,
                    float truncation, g2s_stream_t stream);

/* g2s_rows_mean: out[d] = (partial[0][d] + partial[1][d] + ... in ascending tile order) / N.  partial [tiles, D]
 * as g2s_mapping_fwd wrote it; out [D].  One launch; the same bits on every run and in either mode of
 * g2s_set_deterministic. */
int g2s_rows_mean(const float *partial, float *out, int64_t tiles, int D, int64_t N, g2s_stream_t stream);

/* g2s_image_to_u8: x [B, 3, H, W] f32 -> out [B, H, W, 3] uint8 with the arithmetic of torchvision's
 * save_image(normalize=True, range=(-1, 1)), every step rounded to f32:
 *     clamp(x, -1, 1);  (x + 1) / 2;  * 255 + 0.5;  clamp(0, 255);  truncate.
 * NaN inputs give an unspecified byte. */
int g2s_image_to_u8(const float *x, uint8_t *out, int64_t B, int H, int W, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fused bias + activation.
 * Replaces fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)
 * (GAN2Shape/stylegan2/stylegan2-pytorch/op/fused_bias_act.cpp:11-20,
 *  op/fused_bias_act_kernel.cu:19-99).
 *   y[i] = f(x[i] + bias[(i / step_b) % size_b]) * scale
 *   act*10+grad: 10,11 -> identity ; 12 -> 0 ; 30 -> lrelu(alpha) ; 31 -> ref>0 ? x : x*alpha ;
 *   32 -> 0 ; anything else -> identity.
 * bias / ref may be NULL (== the reference's 0-element tensors). dtype G2S_F32 or G2S_F16.
 * ---------------------------------------------------------------------------------------- */
int g2s_fused_bias_act(const void *x, const void *bias, const void *ref, void *y, int64_t n,
                       int64_t step_b, int64_t size_b, int act, int grad, float alpha,
                       float scale, int dtype, g2s_stream_t stream);

/* nn.MaxPool2d(2, 2) of the VGG16 trunk (lpips/pretrained_networks.py:97-135): x [planes, H, W] ->
 * y [planes, H/2, W/2]; backward from the saved INPUT (first maximum of a window in row-major order
 * wins, NaN wins: torch's rule), gx fully written.  H even, W a multiple of 8, 16-byte aligned. */
int g2s_maxpool2x2_fwd(const float *x, float *y, int64_t planes, int H, int W, g2s_stream_t stream);
int g2s_maxpool2x2_bwd(const float *x, const float *gy, float *gx, int64_t planes, int H, int W,
                       g2s_stream_t stream);

/* Residual joins of the frozen nets in one pass: y = (a + b + bias[c]) * scale, c = (i / hw) % C.
 * ToRGB: conv + bias + upsample(skip) (stylegan2-pytorch/model.py:371-377); discriminator ResBlock:
 * (out + skip) / sqrt(2) (model.py:693-697).  a, b, y [n] f32; b and bias [C] may be NULL. */
int g2s_add_bias_scale(const float *a, const float *b, const float *bias, float *y, int64_t n, int64_t hw, int C,
                       float scale, g2s_stream_t stream);

/* The mask pyramid of DiscriminatorLoss (GAN2Shape/losses.py:24-30): n_levels (1..4) successive
 * avg_pool2d(., 2, 2) of x [planes, H, W] in one launch; levels: HOST array of n_levels device pointers,
 * level l [planes, H / 2^(l+1), W / 2^(l+1)].  H, W multiples of 2^n_levels.  ATen's arithmetic per window.
 * x is read as float2: 8-byte aligned. */
int g2s_avg_pyramid(const float *x, float *const *levels, int n_levels, int64_t planes, int H, int W,
                    g2s_stream_t stream);

/* Entry of the offset encoder's residual block (GAN2Shape/networks.py:170-194): relu_out = relu(x) for the
 * residual path and pool_out = avg_pool2d(x, 2, 2) for the identity path in one pass over x [planes, H, W]
 * (H, W even); backward gx = (x <= 0 ? 0 : g_relu) + g_pool / 4 in one pass (torch's rule: a NaN in x passes g_relu;
 * either gradient may be NULL).  x, relu_out, g_relu and gx are accessed as float2: 8-byte aligned. */
int g2s_res_split_fwd(const float *x, float *relu_out, float *pool_out, int64_t planes, int H, int W,
                      g2s_stream_t stream);
int g2s_res_split_bwd(const float *x, const float *g_relu, const float *g_pool, float *gx, int64_t planes, int H,
                      int W, g2s_stream_t stream);

/* The depth head (GAN2Shape/model.py:337-345 get_clamped_depth with :323-324 rescale_depth) on the depth net's
 * raw map, raw [n = B*H*W] f32:  t = tanh(raw - mean[0]);  d = (1 + t) / 2 * hi + (1 - t) / 2 * lo;
 * clamp_border: out = d * (1 - b) + b * border_depth with b = 1.02 in the two left / right columns of every
 * row of W, else 0.  mean: device float (the whole-batch mean of raw, reduced by the caller — under data
 * parallelism the all-reduced one).  _bwd: g_raw = gc - mean(gc), gc = g * d out / d (raw - mean) — the
 * centring's own backward included (mean taken over these n elements); gsum: one device float of scratch
 * (acc_is_zero = 1: already zero, no memset). */
int g2s_depth_head_fwd(const float *raw, const float *mean, float *out, int64_t n, int W, float lo, float hi,
                       int clamp_border, float border_depth, g2s_stream_t stream);
int g2s_depth_head_bwd(const float *raw, const float *mean, const float *g, float *g_raw, float *gsum, int64_t n,
                       int W, float lo, float hi, int clamp_border, float border_depth, int acc_is_zero,
                       g2s_stream_t stream);

/* The reconstruction warp: torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='zeros',
 * align_corners=True) as GAN2Shape/model.py:147,267 calls it, optionally followed by .clamp(lo, hi)
 * (model.py:150,270) in the same pass (clamp = 1).  ATen's arithmetic (corner order nw, ne, sw, se).
 *   x [B, C, IH, IW], grid [B, H, W, 2] (x then y in [-1, 1]), y / gy [B, C, H, W], all f32.
 * Backward: gx [B, C, IH, IW] (zero-filled by the callee unless acc_is_zero = 1, then scattered) and
 * ggrid [B, H, W, 2]; either may be NULL.  With clamp = 1 the gradient passes where lo <= sample <= hi
 * (torch's rule), the sample being recomputed.  The scatter uses float atomics; in deterministic mode
 * (g2s_set_deterministic) it accumulates 2^-40 fixed point with 64-bit integer atomics in `workspace`
 * (>= g2s_grid_sample_bwd_workspace_bytes) and converts at the end — bit-identical from run to run, which
 * ATen's grid_sampler_2d_backward cannot offer; there a NULL / short workspace is G2S_ERR_WORKSPACE, and
 * acc_is_zero = 1 promises a cleared workspace instead of a cleared gx. */
int g2s_grid_sample_fwd(const float *x, const float *grid, float *y, int B, int C, int IH, int IW, int H, int W,
                        int clamp, float lo, float hi, g2s_stream_t stream);
size_t g2s_grid_sample_bwd_workspace_bytes(int B, int C, int IH, int IW);
int g2s_grid_sample_bwd(const float *gy, const float *x, const float *grid, float *gx, float *ggrid, int B, int C,
                        int IH, int IW, int H, int W, int clamp, float lo, float hi, void *workspace,
                        size_t workspace_bytes, int acc_is_zero, g2s_stream_t stream);

/* torch.clamp(x, lo, hi) of the step's image / depth clamps (GAN2Shape/model.py:150,270, renderer.py:123-124)
 * and its backward as ONE launch each (autograd's ClampBackward is five: ge, le, logical_and, where, fill).
 * backward = 0: y = min(max(x, lo), hi);  backward = 1: y = g where lo <= x <= hi, else 0 (torch's rule;
 * NaN in x: forward gives NaN like torch, backward 0).  x, g, y [n] f32. */
int g2s_clamp(const float *x, const float *g, float *y, int64_t n, float lo, float hi, int backward,
              g2s_stream_t stream);

/* StyledConv tail in one pass (stylegan2-pytorch/model.py:349-355: NoiseInjection then
 * FusedLeakyReLU): y = lrelu_alpha(x + noise_w * noise[hw] + bias[c]) * scale.
 * x,y [B, C, HW] f32; noise [HW] f32 (one map broadcast over B and C) or NULL;
 * noise_w is a DEVICE pointer to 1 float. */
int g2s_noise_bias_act(const float *x, const float *noise, const float *noise_w,
                       const float *bias, float *y, int B, int C, int HW, float alpha,
                       float scale, g2s_stream_t stream);
/* The same tail with ONE MAP PER SAMPLE (csrc/synth_batch.hip; the batched projector and sampler, synthesis.py):
 *     y[b,c,i] = scale * lrelu_alpha(x[b,c,i] + noise_w[0] * noise[b,i] + bias[c])
 * x, y [B, C, HW] f32 (the same buffer is allowed); noise [B, HW], not NULL; bias [C] or NULL.  16-byte loads and stores
 * when HW % 4 == 0 and x, y, noise are 16-byte aligned, a scalar path otherwise.  The additions and their order are
 * those of g2s_noise_bias_act: B equal maps give its bits. */
int g2s_noise_bias_act_ps(const float *x, const float *noise, const float *noise_w, const float *bias, float *y, int B,
                          int C, int HW, float alpha, float scale, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * upfirdn2d.
 * Replaces upfirdn2d_op.upfirdn2d(input[M,H,W,1], kernel[kh,kw], up_x, up_y, down_x, down_y,
 * pad_x0, pad_x1, pad_y0, pad_y1) (op/upfirdn2d.cpp:12-22, op/upfirdn2d_kernel.cu:209-369).
 * x [major, in_h, in_w] (minor == 1), k [kh, kw] f32 on device, y [major, out_h, out_w] with
 * out = (in*up + pad0 + pad1 - k + down) / down.  Negative pads crop.
 * ---------------------------------------------------------------------------------------- */
int g2s_upfirdn2d(const void *x, const float *k, void *y, int major, int in_h, int in_w, int kh,
                  int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                  int pad_y0, int pad_y1, int dtype, g2s_stream_t stream);
/* upfirdn2d (f32, one up / down factor for both axes) with the StyledConv tail of an UP-SAMPLING layer in its store
 * (stylegan2-pytorch/model.py:264-275: conv_transpose2d, then Blur; :349-355: noise, bias, leaky ReLU):
 *     y[m, oy, ox] = gain * leaky_relu(upfirdn2d(x)[m, oy, ox] + noise_w[0] * noise[oy, ox] + bias[m % channels], alpha)
 * x [major = B * channels, in_h, in_w]; noise [out_h, out_w]; noise_w a DEVICE pointer to 1 float. */
int g2s_upfirdn2d_nba(const float *x, const float *k, float *y, int major, int channels, int in_h, int in_w, int kh,
                      int kw, int up, int down, int pad_x0, int pad_x1, int pad_y0, int pad_y1, const float *bias,
                      const float *noise, const float *noise_w, float alpha, float gain, g2s_stream_t stream);
/* g2s_upfirdn2d_nba with ONE MAP PER SAMPLE: noise [B = major / channels, out_h, out_w]; plane m reads the map of
 * b = m / channels.  The same kernel body and arithmetic: B equal maps give g2s_upfirdn2d_nba's bits. */
int g2s_upfirdn2d_nba_ps(const float *x, const float *k, float *y, int major, int channels, int in_h, int in_w, int kh,
                         int kw, int up, int down, int pad_x0, int pad_x1, int pad_y0, int pad_y1, const float *bias,
                         const float *noise, const float *noise_w, float alpha, float gain, g2s_stream_t stream);



/* ------------------------------------------------------------------------------------------
 * Modulated convolution (StyleGAN2 generator) as an fp32-MFMA implicit GEMM.
 * Replaces the grouped F.conv2d / F.conv_transpose2d inside ModulatedConv2d.forward
 * (stylegan2-pytorch/model.py:250-291) and their autograd data-gradients, using the
 * input-scaling formulation
 *     y[b,o] = out_scale[b,o] * sum_{i,ky,kx} w[o,i,ky,kx] * (in_scale[b,i] * x[b,i, ...])
 * (in_scale = modulated style, out_scale = demodulation factor), which equals the reference's
 * per-sample-weight formulation up to fp32 rounding.
 *
 * w is always the forward layout [Cout, Cin, k, k] (already multiplied by 1/sqrt(fan_in)).
 * transpose = 0: x has Cin channels, y has Cout channels, reduction over (i, ky, kx):
 *   G2S_CONV_PLAIN : y[b,o,Y,X]            = sum x[b,i,Y+ky-k/2,X+kx-k/2] w[o,i,ky,kx]  (model.py:286-289)
 *   G2S_CONV_UP2   : y[b,o,2y+ky,2x+kx]   += x[b,i,y,x] w[o,i,ky,kx]   out (H-1)*2+k    (model.py:264-274;
 *                    the Blur that follows is g2s_upfirdn2d)
 *   G2S_CONV_DOWN2 : y[b,o,Y,X]            = sum x[b,i,2Y+ky,2X+kx] w[o,i,ky,kx]  out (H-k)/2+1 (model.py:277-283)
 * transpose = 1: the ADJOINT of the same mode's transpose=0 map w.r.t. x — x has Cout channels,
 *   y has Cin channels, reduction over (o, ky, kx), no weight repacking:
 *   G2S_CONV_PLAIN : y[b,i,Y,X]            = sum x[b,o,Y-ky+k/2,X-kx+k/2] w[o,i,ky,kx]
 *   G2S_CONV_DOWN2 : y[b,i,2Y+ky,2X+kx]   += x[b,o,Y,X] w[o,i,ky,kx]            (adjoint of DOWN2)
 *   G2S_CONV_UP2   : y[b,i,Y,X]            = sum x[b,o,2Y+ky,2X+kx] w[o,i,ky,kx] (adjoint of UP2;
 *                    here H, W are the sizes of x and must be odd: out (H-k)/2+1)
 * x [B, C_in_of_this_call, H, W] f32; in_scale [B, C_in_of_this_call] or NULL;
 * out_scale [B, C_out_of_this_call] or NULL; y fully overwritten.  k in {1, 3}.
 *
 * Epilogue, on the convolution's output c = out_scale[b,o] * conv(in_scale * x)[b,o,h,w]:
 *   y = c + bias[o]                                                          act = 0
 *   y = gain * leaky_relu(c + noise_w[0] * noise[h,w] + bias[o], alpha)     act = 1 (alpha = 0, gain = 1: ReLU)
 * bias [C_out_of_this_call] or NULL.  noise [OH, OW] f32 (one map for all samples and channels) or NULL, noise_w a
 * DEVICE pointer to 1 float: with a noise, the epilogue is the WHOLE StyledConv tail (stylegan2-pytorch/model.py:
 * 321-355: ModulatedConv2d, NoiseInjection, FusedLeakyReLU — the reference runs conv, `image + weight * noise` and
 * fused_bias_act as three ops), and bias, noise_w and act = 1 are required.  The frozen VGG16 of the LPIPS loss
 * (conv3x3 + bias + ReLU, lpips/pretrained_networks.py:97-135) and the discriminator's ConvLayer take bias + act
 * without scales.  A split-K launch finishes with g2s_fused_bias_act / g2s_noise_bias_act in place.
 * y_is_zero != 0: the caller's promise that y is already all zeros — e.g. a slice of a pool cleared ONCE per
 * training step (gan-2d-to-3d_amd/zeropool.py).  Launches that add partial sums into y (split-K slices of small
 * layers; polyphase classes that leave holes) then skip their own clear: one graph node less each (36 of step 1's
 * 319 nodes were such clears).
 * g2s_modconv_needs_zero answers, without launching anything, whether that signature adds into a cleared output (1)
 * or overwrites y (0) under the calling thread's current tuning state, so that only those outputs are taken from the
 * pool.  has_scales = in_scale or out_scale is given; fused = a bias / activation epilogue is present.
 * ---------------------------------------------------------------------------------------- */
#define G2S_CONV_PLAIN 0
#define G2S_CONV_UP2 1
#define G2S_CONV_DOWN2 2

int g2s_modconv(const float *x, const float *w, const float *in_scale, const float *out_scale, const float *bias,
                const float *noise, const float *noise_w, float *y, int B, int Cin, int Cout, int H, int W, int k,
                int mode, int transpose, int act, float alpha, float gain, int y_is_zero, g2s_stream_t stream);
int g2s_modconv_needs_zero(int B, int Cin, int Cout, int H, int W, int k, int mode, int transpose,
                           int has_scales, int fused);

/* General 2-D convolution on the same fp32-MFMA implicit-GEMM kernel: the trained nets of the step
 * (depth / albedo / viewpoint / lighting / offset-encoder nets, GAN2Shape/networks.py:23-244:
 * nn.Conv2d k in {1,3,4,5} stride 1/2, nn.ConvTranspose2d k4 stride 1/2), forward and data-gradient.
 *   adjoint = 0: y[b,m,oy,ox]               = sum_{c,ky,kx} x[b,c,oy*s+ky-p,ox*s+kx-p] W(m,c,ky,kx),
 *                out ((H+2p-k)/s+1) x ((W+2p-k)/s+1)                    (Conv2d forward; ConvTranspose2d dgrad)
 *   adjoint = 1: y[b,m,iy*s+ky-p,ix*s+kx-p] += x[b,c,iy,ix] W(m,c,ky,kx), out out_h x out_w, 0 = (H-1)s-2p+k
 *                (up to s-1 more, as a strided Conv2d's input can be)    (ConvTranspose2d forward; Conv2d dgrad)
 *   W(m,c,ky,kx) = w[(m*Cr + c)*k*k + ky*k + kx] if w_m_major (w is [M,Cr,k,k]) else w[(c*M + m)*k*k + ...]
 * x [B,Cr,H,W], y [B,M,...] f32, fully overwritten; bias [M] or NULL; act 0: none, 1: leaky-ReLU(alpha) * gain.
 * k 1..5, stride 1 or 2, 0 <= pad < k.
 * g2s_conv2d_wgrad: dw[a,g,ky,kx] = sum_{b,py,px} A[b,a,py,px] * G[b,g,py*s+ky-p,px*s+kx-p]
 *   (zero outside G), A [B,Ca,PH,PW], G [B,Cg,GH,GW], dw [Ca,Cg,k,k] fully overwritten.
 *   Conv2d weight gradient: A = grad_out, G = input; ConvTranspose2d: A = input, G = grad_out.
 *   Summation over pixels is split over workgroups and added with float atomics.
 * y_is_zero / dw_is_zero != 0: the caller hands over zero-filled outputs (e.g. slices of one cleared
 *   arena per network pass), so the split-K paths skip their own clear of the output.
 * groups (1..8): that many independent convolutions in one launch — two structurally identical trained nets
 *   (depth + albedo, viewpoint + lighting: GAN2Shape/networks.py:53-167 differ only in their last layer) run with
 *   their channels side by side: x [B, groups*Cr, H, W], y [B, groups*M, ...], w and bias hold the groups back to
 *   back ([groups][M][Cr][k][k], or [groups][Cr][M][k][k] when w_m_major = 0); for the weight gradient
 *   A [B, groups*Ca, ...], G [B, groups*Cg, ...], dw [groups][Ca][Cg][k][k].  Per group the arithmetic is that of
 *   groups = 1, the shapes above. */
int g2s_conv2d(const float *x, const float *w, const float *bias, float *y, int B, int Cr, int M, int H,
               int W, int k, int stride, int pad, int adjoint, int w_m_major, int out_h, int out_w,
               int act, float alpha, float gain, int y_is_zero, int groups, g2s_stream_t stream);
int g2s_conv2d_wgrad(const float *A, const float *G, float *dw, int B, int Ca, int Cg, int PH, int PW,
                     int GH, int GW, int k, int stride, int pad, int dw_is_zero, int groups, g2s_stream_t stream);

/* Backward of one convolution layer of the trained nets as ONE launch: the data-gradient
 *   g2s_conv2d(gy, w, NULL, gx, B, Cr, M, H, W, k, stride, pad, adjoint, w_m_major, out_h, out_w,
 *              0, 0, 1, gx_is_zero, groups, stream)
 * and the weight-gradient
 *   g2s_conv2d_wgrad(A, G, dw, B, Ca, Cg, PH, PW, GH, GW, k, stride, pad, dw_is_zero, groups, stream)
 * of the same layer (k, stride, pad, B, groups shared) in one grid — the two are independent and
 * latency-bound at these sizes, so the layer costs the longer of the two.  Results are those of
 * the two separate calls.  (torch's ConvolutionBackward of nn.Conv2d / nn.ConvTranspose2d,
 * GAN2Shape/networks.py:23-244.) */
int g2s_conv2d_bwd(const float *gy, const float *w, float *gx, int B, int Cr, int M, int H, int W, int k,
                   int stride, int pad, int adjoint, int w_m_major, int out_h, int out_w, int gx_is_zero,
                   const float *A, const float *G, float *dw, int Ca, int Cg, int PH, int PW, int GH, int GW,
                   int dw_is_zero, int groups, g2s_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Adam step of a list of parameter tensors in ONE launch (torch.optim.Adam(params, lr, betas,
 * weight_decay) of GAN2Shape/trainer.py:163-171: classic L2 weight decay, amsgrad off):
 *   g' = g + wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  t = *step + 1;
 *   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);  then *step = t.
 * tensors  DEVICE array [n_tensors] of {p, m, v, n, step, ticket} — everything that persists from
 *          step to step: p, m, v f32 with n elements each; step a DEVICE f32 scalar per tensor
 *          (steps taken so far, as torch counts them per parameter; advanced by the launch, so a
 *          captured graph replays the right bias correction); ticket a DEVICE int per tensor, zero
 *          before and after every launch;
 * chunk0   DEVICE array [n_tensors + 1]: prefix sums of ceil(n / g2s_adam_chunk()) — tensor i owns
 *          the chunks chunk0[i] .. chunk0[i + 1] - 1; n_chunks = chunk0[n_tensors];
 * grads    HOST array [n_tensors] of device pointers to the gradients (they move from step to step;
 *          passed to the kernel by value).  n_tensors <= G2S_ADAM_MAX_TENSORS per call. */
#define G2S_ADAM_MAX_TENSORS 128
typedef struct g2s_adam_tensor {
    float *p, *m, *v;
    int64_t n;
    float *step;
    int *ticket;
} g2s_adam_tensor;
int64_t g2s_adam_chunk(void);
int g2s_adam_step(const g2s_adam_tensor *tensors, const int *chunk0, const float *const *grads, int n_tensors,
                  int n_chunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                  g2s_stream_t stream);

/* fp16-OPERAND form of g2s_modconv (BASELINE config 5, "fp16 MFMA path"): the same geometry and arguments without
 * noise / noise_w / y_is_zero; x, w, y stay fp32 in memory, both GEMM operands are rounded to fp16 on
 * their way into LDS and multiplied by v_mfma_f32_32x32x8_f16 with fp32 accumulation.  bias (NULL ok)
 * and act (0 none / 1 leaky-ReLU(alpha) * gain) form the epilogue.  1x1 and 3x3 kernels only.
 * Results differ from the fp32 kernels at the 1e-3 level (fp16 rounding of the operands). */
int g2s_modconv_f16(const float *x, const float *w, const float *in_scale, const float *out_scale,
                    const float *bias, float *y, int B, int Cin, int Cout, int H, int W, int k, int mode,
                    int transpose, int act, float alpha, float gain, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 3x3 stride-1 convolution (padding 1) as Winograd F(2x2, 3x3) on the fp32 matrix cores
 * (csrc/winograd.hip): the same map as g2s_modconv(mode = G2S_CONV_PLAIN, k = 3) — the generator's
 * plain StyledConvs (stylegan2-pytorch/model.py:285-289), the discriminator's ResBlock conv1
 * (model.py:679-697), the VGG16 trunk of LPIPS (lpips/pretrained_networks.py:97-135) and their
 * data-gradients — with 2.25x fewer multiplications; results equal up to fp32 rounding.
 *
 * g2s_wino_weights: U = G g G^T for every (output, reduction) channel pair of w [Cout, Cin, 3, 3],
 *   written to U (g2s_wino_weights_floats(M, Cr) floats, tiled layout private to the library).
 *   transpose = 0: M = Cout, Cr = Cin (forward).  transpose = 1: M = Cin, Cr = Cout, taps flipped
 *   (the data-gradient of the forward map).  Done once per weight tensor by the caller.
 * g2s_conv3x3_wino: y[b,m] = act(out_scale[b,m] * sum_c conv3x3(in_scale[b,c] * x[b,c], w(m,c)) + noise_w[0] *
 *   noise[h,w] + bias[m]); x [B, Cr, H, W], y [B, M, H, W]; in_scale [B, Cr], out_scale [B, M], bias [M], noise
 *   [H, W] may be NULL; act 0: none, 1: leaky-ReLU(alpha) * gain.  A noise is the StyledConv tail (see g2s_modconv):
 *   it requires bias, noise_w and act = 1, and the reduce passes below add it with the bias.
 *   splitk = 0: partition chosen by the library — whole
 *   tiles, or "stream-K": equal runs of (tile, K tile) units over 256 workgroups when whole tiles
 *   would fill the last round of CUs badly; splitk > 0: that K split of every tile; splitk < 0:
 *   stream-K over -splitk workgroups.  Partial sums meet by float atomics in a cleared y and the
 *   bias / activation then runs as one deferred elementwise launch — or, for split-K with a
 *   workspace `ws` (device scratch of ws_floats >= slices x B*M*H*W floats, <= 8 slices; NULL = none;
 *   contents undefined afterwards; one per stream), the slices store their partial sums side by
 *   side in ws and one elementwise pass adds them with the bias / activation: no clear, no atomics
 *   (this kernel's workgroups reach their epilogue together, so their atomics cannot hide behind
 *   matrix work: 35 of 72 us on 8 x 512 x 16 x 16 in 4 slices), deterministic sums.
 * ---------------------------------------------------------------------------------------- */
size_t g2s_wino_weights_floats(int M, int Cr);
int g2s_wino_weights(const float *w, float *U, int Cout, int Cin, int transpose, g2s_stream_t stream);
int g2s_conv3x3_wino(const float *x, const float *U, const float *in_scale, const float *out_scale,
                     const float *bias, const float *noise, const float *noise_w, float *y, int B, int Cr, int M,
                     int H, int W, int act, float alpha, float gain, int splitk, float *ws, int64_t ws_floats,
                     g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same map as Winograd F(4x4, 3x3) (csrc/winograd4.hip): 36 multiplications per 16 outputs — 1.78x fewer than
 * g2s_conv3x3_wino, 4x fewer than the direct form — for the large maps of the frozen networks.  Interpolation points
 * 0, +-1, +-2, inf; U in double arithmetic, one rounding; fp32 everywhere else (error bound and measurements: DESIGN §4.3b).
 * g2s_wino4_supported: 1 when the kernel takes the shape (H, W multiples of 4, W / 4 divides 32, M a multiple of 64,
 *   Cr a multiple of 4); the caller falls back to g2s_conv3x3_wino otherwise.
 * g2s_wino4_weights / _floats: as g2s_wino_weights, in this kernel's own tiled layout.
 * g2s_conv3x3_wino4: y[b,m] = act(out_scale[b,m] * sum_c conv3x3(in_scale[b,c] * x[b,c], w(m,c)) + noise_w[0] *
 *   noise[h,w] + bias[m]); in_scale, out_scale, bias, noise (+ noise_w) may be NULL.  splitk = 0: whole tiles, or K
 *   slices through the workspace `ws` (as above) when whole tiles would leave CUs idle; splitk > 0: that split (needs
 *   ws; falls back to whole tiles without one).  No atomics on any path: sums have a fixed order.
 * ---------------------------------------------------------------------------------------- */
size_t g2s_wino4_weights_floats(int M, int Cr);
int g2s_wino4_weights(const float *w, float *U, int Cout, int Cin, int transpose, g2s_stream_t stream);
int g2s_wino4_supported(int B, int Cr, int M, int H, int W);
int g2s_conv3x3_wino4(const float *x, const float *U, const float *in_scale, const float *out_scale,
                      const float *bias, const float *noise, const float *noise_w, float *y, int B, int Cr, int M,
                      int H, int W, int act, float alpha, float gain, int splitk, float *ws, int64_t ws_floats,
                      g2s_stream_t stream);

/* Measurement aid (csrc/probe.hip, tools/bench_mfma_peak.py), not part of the training path: `blocks` workgroups of
 * `waves` wavefronts (1..8), each issuing iters x 8 independent v_mfma_f32_32x32x2_f32 from registers — what the fp32
 * matrix pipe sustains against the nominal 157.3 TFLOP/s the rooflines use.  FLOP = blocks * waves * iters * 8 * 4096. */
int g2s_mfma_probe(float *out, int blocks, int waves, int iters, g2s_stream_t stream);
/* The same with the Winograd inner loop's operand traffic: 8 x 16-byte LDS reads per lane per 16 MFMAs; acc_agpr = 1
 * forces the accumulators into AccVGPRs.  FLOP = blocks * waves * iters * 16 * 4096. */
int g2s_mfma_lds_probe(float *out, int blocks, int waves, int iters, int acc_agpr, g2s_stream_t stream);

/* Tuning hook (tools/tune_modconv.py): force the tile configuration (0: 128x128, 1: 128x64,
 * 2: 64x64, 3: 32x128, 4: 64x128 output channels x pixels) and/or the split-K factor of the calling thread's following
 * g2s_modconv / g2s_conv2d launches (slices of the deepest polyphase class of a
 * strided scatter; shallower classes get proportionally fewer); -1 restores the built-in choice
 * (measured tables csrc/modconv_tuned.inc / conv2d_tuned.inc, else a heuristic), tile = -2 selects
 * the heuristic alone.  Results do not depend on the choice beyond the fp32 summation order. */
int g2s_modconv_tune(int tile, int splitk);

/* ------------------------------------------------------------------------------------------
 * Row-wise fused reductions around the modulated convolution (csrc/rowops.hip).
 * g2s_rows_dot_scale: a, b, out are [rows, n] f32; s, inv, dot are [rows].
 *   dot[r]   = (sum_i a[r,i] * b[r,i]) * (inv ? 1 / inv[r] : 1)      (dot may be NULL; needs a)
 *   out[r,i] = b[r,i] * s[r]                                          (out may be NULL or alias b)
 * g2s_demod_fwd: demod[b,o] = rsqrt(sum_i wsq[o,i] * s[b,i]^2 + eps)  (model.py:254-258)
 * g2s_demod_bwd: gs[b,i] = -s[b,i] * sum_o gd[b,o] * demod[b,o]^3 * wsq[o,i]
 * ---------------------------------------------------------------------------------------- */
int g2s_rows_dot_scale(const float *a, const float *b, const float *s, const float *inv, float *out,
                       float *dot, int rows, int n, g2s_stream_t stream);
int g2s_demod_fwd(const float *wsq, const float *s, float *demod, int B, int Cin, int Cout,
                  float eps, g2s_stream_t stream);
int g2s_demod_bwd(const float *wsq, const float *s, const float *demod, const float *gd, float *gs,
                  int B, int Cin, int Cout, g2s_stream_t stream);
/* The same plus a gradient that reaches s from elsewhere (the convolution's own in_scale path):
 * gs = gs_add + (the above); gs_add [B, Cin] may be NULL, may alias gs.  Saves autograd's accumulation launch. */
int g2s_demod_bwd_add(const float *wsq, const float *s, const float *demod, const float *gd, const float *gs_add,
                      float *gs, int B, int Cin, int Cout, g2s_stream_t stream);
/* out[c] = sum over b and i of g[b, c, i] — the bias gradient of nn.Conv2d(bias=True) (the offset encoder's residual
 * blocks, GAN2Shape/networks.py:170-244; autograd's sum over dims (0, 2, 3)).  g [B, C, n], out [C] f32; fixed order. */
int g2s_channel_sum(const float *g, float *out, int B, int C, int n, g2s_stream_t stream);
/* g2s_demod_fwd / g2s_demod_bwd_add of up to G2S_DEMOD_MAX_LAYERS layers in ONE launch each (the styled layers of
 * the frozen generator, synthesis.py): HOST arrays of `layers` device pointers / sizes; layer l has wsq [Cout_l,
 * Cin_l], s [B, Cin_l], demod [B, Cout_l], gd [B, Cout_l]; the backward ADDS its result to gs [B, Cin_l] in place. */
#define G2S_DEMOD_MAX_LAYERS 24
int g2s_demod_fwd_multi(const void *const *wsq, const void *const *s, const void *const *demod, const int *Cin,
                        const int *Cout, int layers, int B, float eps, g2s_stream_t stream);
int g2s_demod_bwd_multi(const void *const *wsq, const void *const *s, const void *const *demod, const void *const *gd,
                        const void *const *gs, const int *Cin, const int *Cout, int layers, int B, g2s_stream_t stream);
/* Backward of the frozen generator, one pass per activation x = gain * leaky_relu(yconv + noise_w * noise + bias)
 * between two layers (stylegan2-pytorch/model.py:321-355,545-627; gan-2d-to-3d_amd/synthesis.py).  x is the output
 * of the producer's StyledConv tail and the input of its consumers: the next modulated convolution (g1 = gradient
 * w.r.t. s1 * x from its data-gradient GEMM) and, where present, ToRGB (g2, s2; all three NULL otherwise).
 * Rows r = (b, c) of n = H * W:
 *     dot1[r] = sum_i x g1,  dot2[r] = sum_i x g2                               (style gradients of the consumers)
 *     out[r,i] = (g1 s1[r] + g2 s2[r]) * gain * (x > 0 ? 1 : slope)             (op/fused_act.py:33-38 with ref = x;
 *                                                                                out may be NULL)
 *     gdot[r]  = sum_i out * yconv / demod[r],  yconv = (x > 0 ? x : x / slope) / gain - noise_w[0] noise[i] - bias[c]
 *                (d loss / d demodulation of the producer; gdot NULL: skipped, noise / bias / demod unused)
 * x, g1, g2, out [rows, n] f32; s1, s2, demod, dot1, dot2, gdot [rows]; bias [channels], c = r % channels; noise [n]. */
int g2s_synth_bwd_rows(const float *x, const float *g1, const float *s1, const float *g2, const float *s2,
                       const float *noise, const float *noise_w, const float *bias, const float *demod, float *out,
                       float *dot1, float *dot2, float *gdot, int rows, int channels, int n, float slope, float gain,
                       g2s_stream_t stream);
/* g2s_synth_bwd_rows with ONE MAP PER SAMPLE: noise [B = rows / channels, n] (rows a multiple of channels); row r reads
 * the map of b = r / channels, in gdot only.  The same kernel with a noise stride of n instead of 0: every sum keeps its
 * order, no atomics, the same bits in either mode of g2s_set_deterministic, and B equal maps give g2s_synth_bwd_rows'
 * bits. */
int g2s_synth_bwd_rows_ps(const float *x, const float *g1, const float *s1, const float *g2, const float *s2,
                          const float *noise, const float *noise_w, const float *bias, const float *demod, float *out,
                          float *dot1, float *dot2, float *gdot, int rows, int channels, int n, float slope, float gain,
                          g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The latent projector's additions to the frozen generator (csrc/projector.hip; stylegan2-pytorch/projector.py:16-44,
 * gan-2d-to-3d_amd/projector.py).  No float atomics anywhere: every sum has one fixed order, and none depends on
 * g2s_set_deterministic.
 *
 * g2s_noise_grad: the gradient of a StyledConv's noise map from the gradient of its pre-activation (the `out` of
 *   g2s_synth_bwd_rows):  gnoise[b,i] = noise_w[0] * sum_c gpre[b,c,i].  gpre [B, C, n], gnoise [B, n] f32, noise_w a
 *   device scalar.  16-byte loads when n % 4 == 0 and both pointers are 16-byte aligned, a scalar path otherwise.
 *
 * The two entries below take ALL noise maps of a generator in one call: HOST arrays of `maps` device pointers and
 * sides (maps <= G2S_NOISE_MAX_MAPS; map m is [B, 1, side_m, side_m] f32, contiguous; every side a power of two,
 * 4 .. 512; 1 <= B <= 64), scratch in a caller-provided workspace of at least *_workspace_bytes (0 for invalid
 * arguments; contents undefined afterwards), no host synchronisation.  A NULL / short workspace is G2S_ERR_WORKSPACE;
 * every check precedes the first launch.
 *
 * g2s_noise_regularize: value and gradient of the reference's noise_regularize.  Per map n_0, levels l = 0, 1, ...
 *   of side S_l = S / 2^l; each adds mean(n_l * roll(n_l, 1, x))^2 + mean(n_l * roll(n_l, 1, y))^2, the means over all
 *   B * S_l^2 elements and the rolls wrapping at S_l; the first level with S_l <= 8 is the last, otherwise n_{l+1} is
 *   the 2x2 mean of n_l.  loss [1] (device) receives the sum over maps; grad (NULL: value only) is a HOST array of
 *   device pointers, grad[m] shaped like map m and 16-byte aligned, and receives d loss / d n_0.  At most three
 *   launches whatever the number of maps (two when no map has a side above 8).
 * g2s_noise_normalize: n <- (n - mean) / std in place, mean and the unbiased (N - 1) standard deviation over all
 *   elements of a map, batch included.  Two launches.
 * ---------------------------------------------------------------------------------------- */
#define G2S_NOISE_MAX_MAPS 32
int g2s_noise_grad(const float *gpre, const float *noise_w, float *gnoise, int B, int C, int n, g2s_stream_t stream);
size_t g2s_noise_regularize_workspace_bytes(const int *sides, int maps, int B);
int g2s_noise_regularize(const void *const *noise, const void *const *grad, const int *sides, int maps, int B,
                         float *loss, void *workspace, size_t workspace_bytes, g2s_stream_t stream);
size_t g2s_noise_normalize_workspace_bytes(const int *sides, int maps, int B);
int g2s_noise_normalize(const void *const *noise, const int *sides, int maps, int B, void *workspace,
                        size_t workspace_bytes, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LPIPS per-layer tail (csrc/lpips.hip): unit-normalise both feature maps over channels, weighted
 * squared difference, spatial mean — lpips/networks_basic.py:64-92 + lpips/__init__.py:40-42.
 * f0, f1 [N, C, HW] f32; w [C] (the 1x1 `lin` weights); out [N] is ACCUMULATED into
 * (out[n] += mean_hw sum_c w_c (f0n - f1n)^2): zero it before the first layer.
 * _bwd: g0 [N, C, HW] = d(sum_n gout[n] * out[n]) / d f0   (f1 is the target branch).
 * ---------------------------------------------------------------------------------------- */
int g2s_lpips_layer_fwd(const float *f0, const float *f1, const float *w, float *out, int N, int C,
                        int HW, g2s_stream_t stream);
int g2s_lpips_layer_bwd(const float *f0, const float *f1, const float *w, const float *gout,
                        float *g0, int N, int C, int HW, g2s_stream_t stream);
/* The same inside the VGG trunk's hand-written backward (gan2shape_amd/lpips.py): f0 is the ReLU output
 * of the slice's last convolution (pretrained_networks.py:97-135), so the gradient that reaches it is
 * g_in (from the next slice through its max pool; NULL for the last slice) + this layer's tail, passed
 * only where f0 > 0 when relu_gate = 1 — one launch instead of tail + add + ReLU backward. */
int g2s_lpips_layer_bwd_ex(const float *f0, const float *f1, const float *w, const float *gout,
                           const float *g_in, int relu_gate, float *g0, int N, int C, int HW,
                           g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Masked L1 (csrc/losses.hip): the numerator of PhotometricLoss and of every DiscriminatorLoss level
 * (GAN2Shape/losses.py:6-51: (|a - b| * mask.expand_as(loss)).sum() / mask.expand_as(loss).sum()).
 * x, y [B, C, HW] f32; w [B, HW] (the mask at this resolution) or NULL (weight 1); HW % 4 == 0.
 * _fwd: *num += sum |x - y| * w   (num: a ZEROED device float).  The denominator C * sum(w) only
 *       needs the small mask and is left to the caller.
 * _bwd: gx = sign(x - y) * w * coef[0]   (coef: device float = incoming gradient / denominator).
 * ---------------------------------------------------------------------------------------- */
int g2s_weighted_l1_fwd(const float *x, const float *y, const float *w, float *num, int B, int C, int HW,
                        g2s_stream_t stream);
int g2s_weighted_l1_bwd(const float *x, const float *y, const float *w, const float *coef, float *gx, int B,
                        int C, int HW, g2s_stream_t stream);
/* The loss one division away, in the same two passes:
 * _fwd2: numden[0] += sum |x - y| * w,  numden[1] += sum over (b, c, p) of w — the reference's
 *        mask.expand_as(loss).sum(); w == NULL: the element count.  numden: two ZEROED device floats.
 * _bwd2: gx = gadd + sign(x - y) * w * g[0] / den[0]   (g: incoming gradient, den: numden + 1, both device
 *        floats; gadd [B, C, HW] another gradient reaching x, or NULL). */
int g2s_weighted_l1_fwd2(const float *x, const float *y, const float *w, float *numden, int B, int C, int HW,
                         g2s_stream_t stream);
int g2s_weighted_l1_bwd2(const float *x, const float *y, const float *w, const float *g, const float *den,
                         const float *gadd, float *gx, int B, int C, int HW, g2s_stream_t stream);
/* One launch per level of the discriminator-feature loss's backward (losses._DFeatureL1; GAN2Shape/losses.py:11-36 on
 * stylegan2-pytorch/model.py:679-697):  gx = (gadd + gadd2) * add_scale + [x != NULL] sign(x - y) w g[0] / den[0] — the
 * residual join of the block above with this level's masked-L1 gradient — and, optionally, gx_gate = gx * gain *
 * (gate_ref > 0 ? 1 : slope), the gradient behind the block's activated conv2.  Any of gadd2, gx, gx_gate may be NULL.
 * _bwd and _bwd2 are launches of the same kernel (den = NULL; gadd2 = NULL, add_scale = 1, no gate): where their
 * arguments describe the same sum, the three entries give the same bits. */
int g2s_weighted_l1_bwd3(const float *x, const float *y, const float *w, const float *g, const float *den,
                         const float *gadd, const float *gadd2, float add_scale, float *gx, const float *gate_ref,
                         float slope, float gain, float *gx_gate, int B, int C, int HW, g2s_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Fused renderer geometry / loss glue (csrc/geometry.hip).  All f32, device pointers; K is a HOST
 * pointer to 9 floats.  rays [H*W, 3] = K^-1 (u, v, 1)^T per pixel (renderer.py:74-80); R [B,3,3],
 * t [B,3]; rot_center_depth = z of the rotation centre (renderer.py:64-69).
 *   g2s_view_transform_*  view [B,6] -> R = Rz Ry Rx, t  (model.py:330-335 + renderer/utils.py:33-73)
 *   g2s_warp_verts_*      verts [B,H*W,3] = R (d ray - c) + c + t          (renderer.py:90-95)
 *   g2s_inv_warp_grid_*   grid [B,H,W,2] = normalise(K (R^T (d ray - t - c) + c))  (renderer.py:97-114)
 *   g2s_smooth_loss_*     mean|dx2| + mean|dxdy| + mean|dydx| + mean|dy2| of p [N,H,W]  (losses.py:54-79)
 * Backward entry points write gdepth / gview / gp fully; gRt [B,12] (9 of R, 3 of t; may be NULL)
 * is zero-filled by the callee (unless acc_is_zero = 1: already zero) then accumulated with one float atomic per
 * workgroup; so is the smoothness loss (one device float).
 * ---------------------------------------------------------------------------------------- */
int g2s_view_transform_fwd(const float *view, float rot_scale, float txy_scale, float tz_scale,
                           float *R, float *t, int B, g2s_stream_t stream);
int g2s_view_transform_bwd(const float *view, float rot_scale, float txy_scale, float tz_scale,
                           const float *gR, const float *gt, float *gview, int B, g2s_stream_t stream);
int g2s_warp_verts_fwd(const float *depth, const float *rays, const float *R, const float *t,
                       float rot_center_depth, float *verts, int B, int P, g2s_stream_t stream);
int g2s_warp_verts_bwd(const float *depth, const float *rays, const float *R, const float *gverts,
                       float rot_center_depth, float *gdepth, float *gRt, int B, int P, int acc_is_zero,
                       g2s_stream_t stream);
int g2s_inv_warp_grid_fwd(const float *depth, const float *rays, const float *R, const float *t,
                          const float *K, float rot_center_depth, float *grid, int B, int H, int W,
                          g2s_stream_t stream);
int g2s_inv_warp_grid_bwd(const float *depth, const float *rays, const float *R, const float *t,
                          const float *K, float rot_center_depth, const float *ggrid, float *gdepth,
                          float *gRt, int B, int H, int W, int acc_is_zero, g2s_stream_t stream);
/*   g2s_normal_*      normal [B,H,W,3] from depth (renderer.py:127-139), gradient to depth
 *   g2s_shading_*     light [B,4] (a, b, dx, dy raw), normal [Bn,H,W,3], albedo [Ba,3,H,W] (Bn, Ba in
 *                     {1, B}) -> diffuse [B,1,H,W], texture [B,3,H,W] (model.py:347-360); backward
 *                     writes per-sample gnormal [B,H,W,3], galbedo [B,3,H,W] and adds into glight [B,4],
 *                     which it clears first unless acc_is_zero = 1. */
int g2s_normal_fwd(const float *depth, const float *rays, float *normal, int B, int H, int W,
                   g2s_stream_t stream);
int g2s_normal_bwd(const float *depth, const float *rays, const float *gnormal, float *gdepth, int B,
                   int H, int W, g2s_stream_t stream);
int g2s_shading_fwd(const float *normal, const float *light, const float *albedo, float *diffuse,
                    float *texture, int B, int Bn, int Ba, int P, g2s_stream_t stream);
int g2s_shading_bwd(const float *normal, const float *light, const float *albedo,
                    const float *gdiffuse, const float *gtexture, float *gnormal, float *galbedo,
                    float *glight, int B, int Bn, int Ba, int P, int acc_is_zero, g2s_stream_t stream);
int g2s_smooth_loss_fwd(const float *p, float *loss, int N, int H, int W, int acc_is_zero, g2s_stream_t stream);
int g2s_smooth_loss_bwd(const float *p, const float *gloss, float *gp, int N, int H, int W,
                        g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm + (leaky-)ReLU of the depth / albedo nets (csrc/groupnorm.hip), replacing the
 * nn.GroupNorm -> nn.ReLU / nn.LeakyReLU(0.2) pairs of GAN2Shape/networks.py:88-127.
 *   y = act((x - mean_g) * rstd_g * gamma[c] + beta[c]),  rstd_g = 1 / sqrt(var_g + eps) (biased var)
 * x, y, gy, dx [B, C, HW] f32 (HW % 4 == 0); gamma, beta, dgamma, dbeta [C]; mean, rstd [B, G]
 * (written by fwd, read by bwd); act 0: none, 1: leaky-ReLU(alpha) (alpha = 0: ReLU), the
 * backward taking the activation's slope from the sign of y.  workspace: at least
 * g2s_groupnorm_workspace_floats(B, C, HW, G) floats, scratch of one call.  No atomics.
 * ---------------------------------------------------------------------------------------- */
size_t g2s_groupnorm_workspace_floats(int B, int C, int HW, int G);
int g2s_groupnorm_act_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean,
                          float *rstd, float *workspace, int B, int C, int HW, int G, float eps,
                          int act, float alpha, g2s_stream_t stream);
int g2s_groupnorm_act_bwd(const float *gy, const float *y, const float *x, const float *gamma,
                          const float *mean, const float *rstd, float *dx, float *dgamma, float *dbeta,
                          float *workspace, int B, int C, int HW, int G, int act, float alpha,
                          g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Depth priors of the depth-net pre-training (csrc/priors.hip), replacing the host-side
 * PriorGenerator of GAN2Shape/priors.py:7-107 (a CPU mask, three F.conv2d passes with a global
 * min / max between them, torch.nonzero for the bounding box, a copy back to the device).
 * mask, x, out [B, S, S] f32; every image is independent (each min / max / bounding box is per image);
 * 1 <= S <= 2048, B <= 65535, B = 0 is a no-op that returns G2S_OK.  The scalars are the doubles the
 * reference's Python holds; each is rounded to fp32 where torch rounds it, so that the maps restate the
 * torch expressions operation by operation.  Nothing synchronises: all calls can be recorded in a HIP
 * graph.  Results are bit-reproducible from run to run, whatever g2s_set_deterministic says (fixed
 * summation order; min / max through integer atomics).  In-place use (out == mask, out == x) is safe.
 *
 *   g2s_prior_map   kind 0 box:        1 inside the centred 0.8 S x 0.5 S box, else 0 (mask unused, may be NULL)
 *                   kind 1 masked_box: far - far * ((m' - t) / (1 - t)), m' = m < t ? 0 : m  (below the
 *                                      threshold that is far * (1 + t / (1 - t)), as in the reference)
 *                   kind 2 confidence: far - far * m
 *   g2s_prior_smooth  `passes` x { valid taps x taps box filter, every tap 1 / taps; per-image min lo and
 *                   max hi; near + (v - lo) * (far - near) / (hi - lo); border of width taps / 2 = far }.
 *                   Each output is summed directly (taps row taps, then taps column taps): no running
 *                   window, the rounding error does not grow with S.  taps odd and <= S, passes >= 0
 *                   (0: out = x), near < far.  A constant filtered map (hi == lo, where the host
 *                   expression is 0 / 0 = NaN) rescales to `near`.
 *                   workspace: >= g2s_prior_smooth_workspace_bytes(B, S, taps, passes) bytes, scratch of one call.
 *   g2s_prior_ellipsoid  spherical cap of `radius` over the bounding box (max_y, min_y, max_x, min_x) of
 *                   mask >= threshold, reduced on the device: depth near at the centre, far at the rim and
 *                   outside.  The host path raises on an empty mask; this one cannot without a
 *                   synchronisation: an image with no pixel at or above the threshold, or whose box has
 *                   zero width or zero height, gets `far` everywhere.  radius > 0, near < far <= near + 2 radius.
 *                   workspace: >= g2s_prior_ellipsoid_workspace_bytes(B) bytes.
 * A NULL / short workspace is G2S_ERR_WORKSPACE; every check precedes the first launch.
 * ---------------------------------------------------------------------------------------- */
int g2s_prior_map(const float *mask, int B, int S, int kind, double threshold, double far, float *out,
                  g2s_stream_t stream);
size_t g2s_prior_smooth_workspace_bytes(int B, int S, int taps, int passes);
int g2s_prior_smooth(const float *x, int B, int S, int taps, int passes, double near, double far, float *out,
                     void *workspace, size_t workspace_bytes, g2s_stream_t stream);
size_t g2s_prior_ellipsoid_workspace_bytes(int B);
int g2s_prior_ellipsoid(const float *mask, int B, int S, double threshold, double radius, double near,
                        double far, float *out, void *workspace, size_t workspace_bytes, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Parsing networks behind the object masks (csrc/parsing.hip): what BiSeNet / PSPNet (GAN2Shape/networks.py:247-586,
 * resnet.py) and MaskingModel (GAN2Shape/model.py:473-551) need beside g2s_conv2d.  All tensors f32, contiguous
 * NCHW; `planes` = B * C.  No float atomics: results are bit-reproducible from run to run.  Nothing
 * synchronises; every check precedes the first launch; an empty batch (B or planes = 0) returns G2S_OK.
 * The ABI version stays 1, as for every earlier addition: symbols are only added.
 *
 *   g2s_conv_stem7        y = act(conv(x, w) + bias), w [M, 3, 7, 7], stride 2, padding 3, x [B, 3, H, W],
 *                         y [B, M, (H-1)/2+1, (W-1)/2+1]; bias [M] or NULL; relu != 0: ReLU.  (g2s_conv2d stops at k = 5.)
 *   g2s_maxpool3x3s2      3x3 window, stride 2, padding 1 that behaves as -inf; y [planes, (H-1)/2+1, (W-1)/2+1].
 *   g2s_adaptive_avgpool  y[i, j] = mean of x[floor(i H / out_h) .. ceil((i+1) H / out_h), same in W): PyTorch's
 *                         adaptive_avg_pool2d, also its 'area' interpolation; out_h > H is allowed.
 *   g2s_resize_bilinear   PyTorch's bilinear interpolation with or without align_corners.
 *   g2s_gate_add_act      y = act(x * s' + t + r): x, r, y [planes, HW]; s, t [planes]; each of s, t, r may be NULL.
 *                         s' = s, through a logistic sigmoid if sigmoid != 0, plus 1 if plus_one != 0 (both need s);
 *                         act = ReLU if relu != 0.  y must not overlap x or r.
 *   g2s_parse_head        logits [B, C, h, w], C <= 32.  For every pixel of the size x size grid the C logits are
 *                         interpolated bilinearly (align_corners = 1) and reduced by a rule given as data:
 *                           mode 0 (hard mask):  v = 1 if the argmax over the channels other than `drop` (-1: none;
 *                                                ties to the lowest channel) is a member of class_set (bit c = channel
 *                                                c of the logits), else 0;
 *                           mode 1 (confidence): v = sum of the channels in class_set (drop must be -1).
 *                         out [B, 1, S, S], S <= size, receives the area average of v over the adaptive bins
 *                         (g2s_adaptive_avgpool's); the full-resolution logits are never stored.  Then, per sample:
 *                         mode 0: a sample without a single member pixel gets out = 1 everywhere (and full_mask = 1);
 *                         fallback[b] = 1 for such a sample, else 0.  mode 1: out = (out - min v) / (max v - min v)
 *                         with the full-resolution min and max (the affine map commutes with the average);
 *                         fallback[b] = 0.  full_mask (mode 0 only, may be NULL): uint8 [B, 1, size, size], v per
 *                         pixel.  fallback may be NULL.  workspace: >= g2s_parse_head_workspace_bytes(B) bytes,
 *                         scratch of one call (cleared by the call); NULL / short is G2S_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
int g2s_conv_stem7(const float *x, const float *w, const float *bias, float *y, int B, int M, int H, int W, int relu,
                   g2s_stream_t stream);
int g2s_maxpool3x3s2(const float *x, float *y, int planes, int H, int W, g2s_stream_t stream);
int g2s_adaptive_avgpool(const float *x, float *y, int planes, int H, int W, int out_h, int out_w,
                         g2s_stream_t stream);
int g2s_resize_bilinear(const float *x, float *y, int planes, int H, int W, int out_h, int out_w, int align_corners,
                        g2s_stream_t stream);
int g2s_gate_add_act(const float *x, const float *s, const float *t, const float *r, float *y, int planes, int HW,
                     int sigmoid, int plus_one, int relu, g2s_stream_t stream);
size_t g2s_parse_head_workspace_bytes(int B);
int g2s_parse_head(const float *logits, int B, int C, int h, int w, int size, int S, int mode, int drop,
                   uint32_t class_set, float *out, uint8_t *full_mask, int *fallback, void *workspace,
                   size_t workspace_bytes, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Depth and normal accuracy of a recovered depth against a ground-truth depth (csrc/metrics.hip): the
 * figures of the BFM table of the GAN2Shape / Unsup3D papers, per image, in two launches.
 * depth_pred, depth_gt, mask_pred, mask_gt [B, H, W] f32 (either mask may be NULL: all ones); rays [H * W, 3],
 * K^-1 (u, v, 1) per pixel; out [B, 5] = {count, mae, mse, side, mad_deg} of image b.
 *   raw validity   mask_pred > 0.5 (or NULL), mask_gt > 0.5 (or NULL), both depths finite and > 0.  A NaN
 *                  depth is "outside the object", not an error.
 *   erode != 0     a pixel counts if it and its eight neighbours are raw-valid; outside the image is invalid, so
 *                  the border row and column drop out (avg_pool2d(mask, 3, 1, 1) > 0.99 of the papers' evaluation).
 *   erode == 0     raw validity decides.  A pixel on the border, or one of whose four stencil neighbours has a
 *                  non-finite depth (in either map), counts for count, mae, mse, side but not for mad_deg;
 *                  mad_deg divides by its own count.
 *   count          number n of counted pixels (exact to 2^24);  mae = sum |p - g| / n;  mse = sum (p - g)^2 / n
 *   side           delta = log p - log g;  sqrt(max(0, sum (delta - mean delta)^2 / n)), moments held in double
 *   mad_deg        mean angle, in degrees, between the normals n_p and n_g of the two depths, each computed as
 *                  g2s_normal_fwd does for interior pixels (P = rays * depth; cross(P(y, x+1) - P(y, x-1),
 *                  P(y+1, x) - P(y-1, x)) / (norm + 1e-7)).  The angle is atan2(|n_p x n_g|, n_p . n_g): it
 *                  equals acos(n_p . n_g) for unit vectors and does not depend on the 1e-7 that leaves them
 *                  slightly shorter than 1.
 *   n == 0         count 0, the four metrics NaN; no pixel with a stencil: mad_deg NaN.
 * 3 <= H, W <= 32768, 1 <= B <= 65535.  workspace: >= g2s_depth_metrics_workspace_bytes(B, H, W) bytes, 8-byte
 * aligned, scratch of one call; NULL / short is G2S_ERR_WORKSPACE.  Every check precedes the first launch;
 * nothing allocates or synchronises; no atomics: every sum has one fixed order, the output is bit-identical
 * from run to run.
 * ---------------------------------------------------------------------------------------- */
size_t g2s_depth_metrics_workspace_bytes(int B, int H, int W);
int g2s_depth_metrics(const float *depth_pred, const float *depth_gt, const float *mask_pred, const float *mask_gt,
                      const float *rays, int B, int H, int W, int erode, float *out, void *workspace,
                      size_t workspace_bytes, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * How well an image a reproduces an image b (csrc/image_metrics.hip): masked MAE, MSE, PSNR and the mean structural
 * similarity (SSIM; Wang, Bovik, Sheikh, Simoncelli 2004), per image, in two launches.
 * a, b [B, C, H, W] f32, finite; mask [B, H, W] f32 or NULL (all ones); out [B, 6] = {count, mae, mse, psnr,
 * ssim_count, ssim} of image b.  L = data_range > 0, the width of the images' value range.
 *   count          number n of pixels with mask > 0.5 (pixels, not pixels x channels; exact to 2^24)
 *   mae, mse       d = a - b;  mae = sum |d| / (n C),  mse = sum d^2 / (n C), over the counted pixels and all channels
 *   psnr           10 log10(L^2 / mse); +inf when mse == 0
 *   window         w[j] = exp(-(j - 5)^2 / (2 1.5^2)) / sum_j of the same, j = 0 .. 10: 11 taps, sigma 1.5, sum 1.
 *                  F(u)(y, x) = sum_i sum_j w[i] w[j] u(y - 5 + i, x - 5 + j), defined only where the whole 11 x 11
 *                  window lies inside the image: centres (y, x) in [5, H - 6] x [5, W - 6].  No padding.
 *   SSIM map       per channel:  mu_a = F(a), mu_b = F(b);  var_a = F(a a) - mu_a mu_a,  var_b = F(b b) - mu_b mu_b,
 *                  cov = F(a b) - mu_a mu_b  (weighted, biased moments);  C1 = (0.01 L)^2,  C2 = (0.03 L)^2;
 *                  S = ((2 mu_a mu_b + C1) (2 cov + C2)) / ((mu_a mu_a + mu_b mu_b + C1) (var_a + var_b + C2))
 *   ssim_count     number n_w of window centres with mask > 0.5 at the centre
 *   ssim           sum of S over the counted centres and all channels / (n_w C).  For a == b it is exactly 1.
 *   empty          n == 0: count 0 and mae, mse, psnr NaN.  H < 11, W < 11 or n_w == 0: ssim_count 0, ssim NaN.
 * Without a mask this is skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5,
 * use_sample_covariance=False, data_range=L) averaged over the channels.  The filter and all sums run in double.
 * 1 <= C <= 4, 1 <= H, W <= 32768, 1 <= B <= 65535.  workspace: >= g2s_image_metrics_workspace_bytes(B, C, H, W)
 * bytes, 8-byte aligned, scratch of one call; NULL / short is G2S_ERR_WORKSPACE.  Every check precedes the first
 * launch; nothing allocates or synchronises; no atomics: every sum has one fixed order, the output is bit-identical
 * from run to run and in either mode of g2s_set_deterministic; the two launches can be captured in a graph.
 * ---------------------------------------------------------------------------------------- */
size_t g2s_image_metrics_workspace_bytes(int B, int C, int H, int W);
int g2s_image_metrics(const float *a, const float *b, const float *mask, int B, int C, int H, int W, float data_range,
                      float *out, void *workspace, size_t workspace_bytes, g2s_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * ADA augmentation (csrc/ada.hip): random_apply_affine and random_apply_color of stylegan2-pytorch/non_leaking.py
 * with the SYM6 filter k (12 taps), f32, NCHW, two launches forward and two backward.
 *
 * g2s_ada_up2: x [B, C, H, W] -> x2 [B, C, 2 (H + py0 + py1), 2 (W + px0 + px1)].  Reflect padding by the four pads
 *   (each 0 .. size - 1, as F.pad(mode='reflect') requires) and the separable 2x upsampling upfirdn(k, up 2,
 *   pad (6, 5)) per axis, in one pass; no padded copy exists.
 * g2s_ada_warp_down: x2 [B, C, H2, W2], Ginv [B, 2, 3], Cmat [B, 3, 4] or NULL -> y [B, C, H, W].
 *   A = F.grid_sample(x2, F.affine_grid(Ginv, [B, C, 2 (H + 6), 2 (W + 6)], align_corners=False), 'bilinear',
 *   'zeros', align_corners=False);  y = upfirdn(A, flipped k, down 2, pad (-1, -1)) on both axes;  with Cmat,
 *   y[:, c] <- sum_c' Cmat[:, c, c'] y[:, c'] + Cmat[:, c, 3] (C must be 3).  A is never written to memory.
 * g2s_ada_warp_down_bwd: gy [B, C, H, W] -> gx2 [B, C, H2, W2], the adjoint of the above in x2 (Cmat transposed).
 *   Float atomics into gx2, which the call clears first unless acc_is_zero = 1 says it is zero already.  There is
 *   no fixed-point variant: in deterministic mode (g2s_set_deterministic) the call returns G2S_ERR_INVALID.
 * g2s_ada_warp_down_bwd_gather: the same adjoint as a gather, in two launches.  ga [B, C, 2 (H + 6), 2 (W + 6)] is a
 *   caller-provided workspace that receives the gradient of A (every element written once); then every gx2[b, c, sy, sx]
 *   sums, in one fixed order (A's rows outer, columns inner), weight * ga over the positions of A whose bilinear
 *   footprint holds (sy, sx) — the weights are those of the forward's own sample routine.  No atomics, every element
 *   of gx2 is written (no clear needed), and the bits do not depend on g2s_set_deterministic: it runs in either mode.
 *   It differs from g2s_ada_warp_down_bwd in summation order only.
 * g2s_ada_up2_bwd: gx2 -> gx [B, C, H, W], the adjoint of g2s_ada_up2 (mirror images gathered, no atomics; every
 *   element of gx is written).
 * Ginv and Cmat get no gradient.  B * C <= 65535, H, W <= 16384.  Every check precedes the first launch; nothing
 * allocates or synchronises.  All but g2s_ada_warp_down_bwd are bit-identical from run to run.
 * ---------------------------------------------------------------------------------------- */
int g2s_ada_up2(const float *x, float *x2, int B, int C, int H, int W, int px0, int px1, int py0, int py1,
                g2s_stream_t stream);
int g2s_ada_up2_bwd(const float *gx2, float *gx, int B, int C, int H, int W, int px0, int px1, int py0, int py1,
                    g2s_stream_t stream);
int g2s_ada_warp_down(const float *x2, const float *Ginv, const float *Cmat, float *y, int B, int C, int H, int W,
                      int H2, int W2, g2s_stream_t stream);
int g2s_ada_warp_down_bwd(const float *gy, const float *Ginv, const float *Cmat, float *gx2, int B, int C, int H,
                          int W, int H2, int W2, int acc_is_zero, g2s_stream_t stream);
int g2s_ada_warp_down_bwd_gather(const float *gy, const float *Ginv, const float *Cmat, float *gx2, float *ga, int B,
                                 int C, int H, int W, int H2, int W2, g2s_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * Discriminator training (csrc/dtrain.hip): minibatch stddev, logistic loss, R1 penalty.  f32, fixed summation
 * order, no atomics: bit-identical from run to run in either mode of g2s_set_deterministic.  Every check precedes
 * the first launch; nothing allocates or synchronises.
 *
 * Minibatch stddev (stylegan2-pytorch/model.py:756-765).  x [B, C, H, W]; G = min(B, 4) members per group (B a
 * multiple of G), member g of group n is sample g * (B / G) + n; F feature blocks of C / F channels.
 *   d = x - mean_g x,  s = sqrt(mean_g d^2 + 1e-8),  f[n, j] = mean of s over block j's E = (C / F) H W elements.
 * g2s_mbstd_fwd: out [B, C + F, H, W] = x followed by the F constant maps f[n(b), j] — one launch, no cat.
 * g2s_mbstd_bwd: gout [B, C + F, H, W], x -> gx [B, C, H, W] = gout[:, :C] + a d / s with
 *   a[n, j] = (sum_{g,h,w} gout[b, C + j, h, w]) / (E G).
 * g2s_mbstd_bwd2: the backward of g2s_mbstd_bwd for a cotangent ggx [B, C, H, W] on gx:
 *   ggout [B, C + F, H, W]: ggx, then on each appended map sum_{g,e} ggx_g d_g / (s E G);
 *   xg [B, C, H, W] = a [ (ggx_h - mean_g ggx) / s - d_h (sum_g ggx_g d_g) / (G s^3) ], the gradient on x.
 *
 * g2s_d_logistic (train.py:64-68): real [Br], fake [Bf] -> out[4] = { mean softplus(-real) + mean softplus(fake),
 *   mean real, mean fake, sum sign(real) }; g_real [Br] = -sigmoid(-real) / Br and g_fake [Bf] = sigmoid(fake) / Bf,
 *   the gradients of out[0], where the pointers are not NULL.  softplus(x) = max(x, 0) + log1p(exp(-|x|)).
 * g2s_r1_penalty (train.py:71-78): grad [B, n] -> per_sample [B] = sum_i grad[b, i]^2 and, where mean is not NULL,
 *   mean[0] = their mean.  Two stages: partial [B * g2s_r1_penalty_chunks(n)] floats of scratch hold the sums of
 *   fixed chunks, a second launch adds them in index order.  B <= 65535.
 * ---------------------------------------------------------------------------------------- */
int g2s_mbstd_fwd(const float *x, float *out, int B, int C, int H, int W, int F, g2s_stream_t stream);
int g2s_mbstd_bwd(const float *gout, const float *x, float *gx, int B, int C, int H, int W, int F, g2s_stream_t stream);
int g2s_mbstd_bwd2(const float *ggx, const float *gout, const float *x, float *ggout, float *xg, int B, int C, int H,
                   int W, int F, g2s_stream_t stream);
int g2s_d_logistic(const float *real, const float *fake, float *out, float *g_real, float *g_fake, int Br, int Bf,
                   g2s_stream_t stream);
int64_t g2s_r1_penalty_chunks(int64_t n);
int g2s_r1_penalty(const float *grad, float *per_sample, float *mean, float *partial, int B, int64_t n,
                   g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Generator training (csrc/gtrain.hip; gan2shape_amd/gtrain.py, op/conv2d_gradfix.py).  float32.
 *
 * g2s_modconv_wgrad: the weight gradient of the modulated convolution y = demod * conv(s * x, w),
 *   dw[a,g,ky,kx] = sum_{b,py,px} sa[b,a] A[b,a,py,px] * sg[b,g] G[b,g,py*s+ky-p,px*s+kx-p]      (zero outside G)
 *   A [B,Ca,PH,PW], G [B,Cg,GH,GW], sa [B,Ca] or NULL, sg [B,Cg] or NULL, dw [Ca,Cg,k,k] fully overwritten.  The
 *   scales multiply the operands as they are loaded: neither product is written to memory.  Geometry, the split of
 *   the pixel sum and dw_is_zero as g2s_conv2d_wgrad (groups = 1); with both scales NULL and
 *   g2s_set_deterministic(1) the result is that of g2s_conv2d_wgrad bit for bit.
 *
 * g2s_path_penalty (train.py:94-100): grad [B, L, D], mean_path a DEVICE scalar (the running mean) ->
 *   lengths [B] = sqrt(mean_l sum_d grad^2);  pm = mean_path + decay * (mean lengths - mean_path);
 *   stats [3] = { mean_b (lengths - pm)^2, pm, mean lengths };  dgrad [B, L, D] (or NULL) = d stats[0] / d grad, with
 *   pm a function of grad as in the reference.  One workgroup, fixed summation order.  B <= 1024.
 * g2s_g_nonsaturating (train.py:81-84): fake [B] -> out[0] = mean softplus(-fake); g_fake [B] (or NULL) =
 *   -sigmoid(-fake) / B.  One workgroup.
 * g2s_ema_accumulate (train.py:50-55): dst = dst * decay + src * one_minus_decay for every tensor of a DEVICE table
 *   in one launch.  chunk0 DEVICE [n_tensors + 1]: prefix sums of ceil(n / g2s_ema_chunk()); n_chunks =
 *   chunk0[n_tensors].  16-byte accesses where both pointers of a tensor are 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
typedef struct g2s_ema_tensor {
    float *dst;
    const float *src;
    int64_t n;
} g2s_ema_tensor;
int g2s_modconv_wgrad(const float *A, const float *sa, const float *G, const float *sg, float *dw, int B, int Ca,
                      int Cg, int PH, int PW, int GH, int GW, int k, int stride, int pad, int dw_is_zero,
                      g2s_stream_t stream);
int g2s_path_penalty(const float *grad, const float *mean_path, float decay, float *lengths, float *stats,
                     float *dgrad, int B, int L, int D, g2s_stream_t stream);
int g2s_g_nonsaturating(const float *fake, float *out, float *g_fake, int B, g2s_stream_t stream);
int64_t g2s_ema_chunk(void);
int g2s_ema_accumulate(const g2s_ema_tensor *tensors, const int *chunk0, int n_tensors, int n_chunks, float decay,
                       float one_minus_decay, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Data path of the trainer (csrc/dataprep.hip; prepare_data.py, dataset.DeviceBatches).
 *
 * g2s_u8_batch: out[b, c, y, x] = t[data[idx[b], c, y, flip[b] ? S - 1 - x : x]], t[v] = float(v) / 255 rounded to
 *   f32, then * 2 - 1 (dataset.ImageDataset's arithmetic, bit for bit).  data u8 [N, 3, S, S] planar; idx DEVICE
 *   int64 [B] (what torch.randperm yields); flip DEVICE u8 [B]; out f32 [B, 3, S, S].  One launch, no host read-back.
 *   16-byte loads and stores when S % 16 == 0 and data, out are 16-byte aligned, a scalar path otherwise.  An index
 *   outside [0, N) reads nothing and fills its sample with NaN.
 *
 * g2s_resize_u8: Pillow's ImagingResample for 8-bit images with a crop window.  src u8 [N, H, W, 3] interleaved;
 *   dst u8 [N, 3, oh_c, ow_c] planar = the window (left, top, ow_c, oh_c) of the image resized to [oh, ow].
 *   kx int32 [ow, ksx], bx int32 [ow, 2] (first tap, tap count) and ky [oh, ksy], by [oh, 2]: DEVICE tables of 22-bit
 *   fixed-point coefficients (prepare_data.resample_coeffs).  The horizontal pass runs first and is skipped when
 *   ow == W (kx, bx may be NULL), the vertical pass second, skipped when oh == H (ky, by may be NULL); each
 *   accumulates in int32 from 1 << 21, shifts right by 22 and clips to 0..255; the intermediate is u8.
 *   tmp u8 [N, 3, rows, ow_c]: the intermediate, needed when both passes run; it holds the source rows
 *   row0 .. row0 + rows, which must cover every vertical window of the crop (ignored when oh == H).
 *   Windows are clamped to the source, so no table makes the kernels read outside their buffers.
 * ---------------------------------------------------------------------------------------- */
int g2s_u8_batch(const uint8_t *data, int64_t N, const int64_t *idx, const uint8_t *flip, float *out, int B, int S,
                 g2s_stream_t stream);
int g2s_resize_u8(const uint8_t *src, uint8_t *dst, uint8_t *tmp, int N, int H, int W, int oh, int ow,
                  const int32_t *kx, const int32_t *bx, int ksx, const int32_t *ky, const int32_t *by, int ksy,
                  int left, int top, int ow_c, int oh_c, int row0, int rows, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Symmetry pair of a flipped step (csrc/mirror.hip; model.py forward_step1 / forward_step3 with flip1 / flip3).
 *
 * g2s_mirror_pair_fwd: x [N, C, H, W], repeat >= 1 -> y [2 N repeat, C, H, W]: row n * repeat + r is x[n], row
 *   N * repeat + n * repeat + r is x[n] mirrored along W (y[.., w] = x[.., W - 1 - w]).  Two tensors that share
 *   N, H, W and repeat (the depth, C0 = 1, and the albedo, C1 = 3) go through ONE launch; the second is optional
 *   (x1 = y1 = NULL, C1 = 0).
 * g2s_mirror_pair_bwd: gy [2 N repeat, C, H, W] -> gx [N, C, H, W], fully overwritten: gx[n] = sum_r gy[n * repeat + r]
 *   + sum_r mirror(gy[N * repeat + n * repeat + r]), added in that order, r ascending.  A gather without atomics:
 *   bit-reproducible in every mode (g2s_set_deterministic changes nothing); repeat = 1 is one f32 addition.
 *   16-byte accesses for a tensor whose two pointers are 16-byte aligned when W % 4 == 0 (the mirror of the float4
 *   at column quad q is the reversed float4 at quad W / 4 - 1 - q), a scalar path otherwise, chosen per tensor.
 * ---------------------------------------------------------------------------------------- */
int g2s_mirror_pair_fwd(const float *x0, float *y0, int C0, const float *x1, float *y1, int C1, int N, int H, int W,
                        int repeat, g2s_stream_t stream);
int g2s_mirror_pair_bwd(const float *gy0, float *gx0, int C0, const float *gy1, float *gx1, int C1, int N, int H,
                        int W, int repeat, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Canonical object mask (csrc/canon_mask.hip; Renderer.canon_mask, model.py forward_step1 with object_mask on).
 *
 * g2s_canon_mask: out [B, 1, H, W] = grid_sample(mask, get_warped_2d_grid(depth), bilinear, zeros padding,
 *   align_corners=True) in ONE launch: per canonical pixel p of sample b
 *     Y = R_b (d ray_p - c) + c + t_b,   (u, v) = K (Y / Y.z),   g = (u / (W - 1), v / (H - 1)) * 2 - 1
 *   and the four-tap bilinear read of the mask at g, taps outside the image counting as 0.
 *   depth [B, H, W], rays [H*W, 3], R [B,3,3], t [B,3], K a HOST pointer to 9 floats, rot_center_depth = c.z as for
 *   g2s_warp_verts_fwd; mask [Bm, 1, H, W] with Bm = B, or Bm = 1 (one mask shared by the batch).  All f32.
 *   No gradient, no workspace, no atomics: every element is written once from the inputs alone, bit-identical from run
 *   to run in every mode.  A pixel whose position is not finite reads nothing and gives 0.
 * ---------------------------------------------------------------------------------------- */
int g2s_canon_mask(const float *depth, const float *rays, const float *R, const float *t, const float *K,
                   float rot_center_depth, const float *mask, float *out, int B, int Bm, int H, int W,
                   g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Separable banded resampler (csrc/resample.hip; op/resample.py crop_resize: the centre crop of step 2,
 * resize -> crop -> resize, and its transpose, each as ONE launch).
 *
 * g2s_resample_sep: x [planes, Hin, Win] -> y [planes, Hout, Wout],
 *     y[p,i,j] = sum_{a < ylen[i]} yw[i*Ky + a] * ( sum_{b < xlen[j]} xw[j*Kx + b] * x[p, ylo[i] + a, xlo[j] + b] ).
 *   The horizontal sum runs first, then the vertical one, each an ascending fmaf chain from 0; no atomics, no
 *   workspace: two calls are bit-identical in every mode.  EVERY element of y is written; where ylen[i] == 0 or
 *   xlen[j] == 0 it is 0.  Only rows and columns inside the bands are read.
 *   ylo, ylen [Hout] and yw [Hout, Ky], xlo, xlen [Wout] and xw [Wout, Kx] are DEVICE memory (int32 / f32), so the
 *   launcher cannot look into them: it refuses NULL pointers, sizes < 1, Ky or Kx outside 1..g2s_resample_max_taps()
 *   (8), and shapes whose one-row tile does not fit 64 KB of LDS (g2s_resample_tile_rows(...) == 0).  The bands
 *   themselves are checked once, on the host copy, by g2s_resample_bands_check below; the kernel skips a tap outside
 *   the input, so an unchecked table gives wrong values, never an out-of-bounds access.
 * g2s_resample_bands_check: HOST tables lo, len [n_out] of K-tap bands over an input of n_in positions.  Refuses
 *   K outside 1..8, len outside 0..K, a band that leaves [0, n_in), and bands that do not ascend or that leave a gap
 *   between consecutive non-empty ones (the LDS budget of a tile rests on that: tr output rows touch <= tr*K rows).
 * g2s_resample_tile_rows: output rows per workgroup the launcher picks for a shape (0: does not fit).
 * ---------------------------------------------------------------------------------------- */
int g2s_resample_max_taps(void);
int g2s_resample_tile_rows(int Hin, int Win, int Hout, int Wout, int Ky, int Kx);
int g2s_resample_bands_check(const int *lo, const int *len, int n_out, int K, int n_in);
int g2s_resample_sep(const float *x, float *y, int planes, int Hin, int Win, int Hout, int Wout,
                     const int *ylo, const int *ylen, const float *yw, int Ky,
                     const int *xlo, const int *xlen, const float *xw, int Kx, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gather of the projected-sample bank (csrc/bank.hip; bank.py SampleBank.gather: the step-3 hand-off of the
 * trainers with config `collect_iters` on).
 *
 * g2s_bank_gather: bank_img [rows, 3, S, S], bank_mask [rows, 1, S, S], idx [b] in DEVICE memory (int64 when idx64,
 *   else int32), head [h, 3, S, S] (h >= 0; NULL exactly when h == 0)  ->
 *     out_img  [h + b, 3, S, S]: rows 0 .. h are head, row h + j is bank_img[idx[j]]
 *     out_mask [b, 1, S, S]:     row j is bank_mask[idx[j]]
 *   in ONE launch; repeats in idx are allowed.  The launcher cannot look into idx: an entry outside 0 .. rows - 1 is
 *   clamped into the range by the kernel (nothing is read out of bounds, every output element is still written) and
 *   j + 1, the 1-based position of one such entry, is stored to *err (DEVICE int32; the caller clears it and reads
 *   it when it wants the report).  Because idx is read on the device, the launch can be captured, or run in front
 *   of a replayed graph, with a static index buffer.
 *   16-byte accesses for a copy whose row length is a multiple of 4 floats and whose base addresses are all 16-byte
 *   aligned (chosen separately for the image rows with the head and for the mask rows), dword accesses otherwise.
 *   Exact copies: no arithmetic, no atomics, no workspace.  The outputs must not overlap the inputs.
 * ---------------------------------------------------------------------------------------- */
int g2s_bank_gather(const float *bank_img, const float *bank_mask, long rows, const void *idx, int idx64, int b,
                    const float *head, int h, float *out_img, float *out_mask, int S, int *err, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mean, covariance and block Cholesky factor of a set of rows (csrc/mvn.hip; view_light.py mvn_fit: the fit of the
 * view and light priors, view_mvn.pth / light_mvn.pth, from a trained model's estimates).
 *
 * g2s_mvn_fit: rows [N, D] fp32 with row stride ld >= D (in floats; columns D .. ld - 1 are never read),
 *   1 <= D <= G2S_MVN_MAX_D, 2 <= N < 2^31; blocks [nblk] HOST ints, 1 <= nblk <= G2S_MVN_MAX_BLOCKS, each >= 1,
 *   summing to D  ->
 *     mean [D]       fp32
 *     cov  [D, D]    fp32, the full joint covariance with divisor N - 1 (numpy.cov / torch.cov) plus ridge on the
 *                    diagonal; exactly symmetric (the upper triangle is computed and mirrored)
 *     tril [D, D]    fp32, block diagonal: diagonal block k holds the lower Cholesky factor of that block of cov;
 *                    every other entry, the upper triangles included, is 0.0
 *     status         DEVICE int32: 0 fine; 1 + j: the pivot of global column j was not positive (tril is then
 *                    unspecified, mean and cov are valid); -1: some input was not finite (mean, cov, tril unspecified)
 *   in ONE launch of ONE workgroup of 256 threads.  Two passes: the mean is accumulated in double, then the centred
 *   products in double; the Cholesky runs in double on the double covariance; each output is rounded to fp32 once.
 *   Thread t takes rows t, t + 256, ... in ascending order and the partials meet in a fixed tree in LDS: no atomics,
 *   no workspace, bit-identical from run to run whatever g2s_set_deterministic says.  The outputs must not overlap
 *   rows.  Every check precedes the launch.
 * ---------------------------------------------------------------------------------------- */
#define G2S_MVN_MAX_D 16
#define G2S_MVN_MAX_BLOCKS 4
int g2s_mvn_fit(const float *rows, long N, int D, long ld, const int *blocks, int nblk, double ridge,
                float *mean, float *cov, float *tril, int *status, g2s_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training monitor (csrc/monitor.hip; monitor.py: sample grids and the perceptual path length).
 *
 * g2s_image_grid_u8: x [N, C, H, W] f32, C in {1, 3}  ->  out [Hg, Wg, 3] uint8, the grid that torchvision's
 *   save_image(x, nrow=, padding=, normalize=True, range=(lo, hi), pad_value=) writes, in ONE launch:
 *     xmaps = min(nrow, N), ymaps = ceil(N / xmaps), Hg = ymaps (H + padding) + padding, Wg = xmaps (W + padding) + padding;
 *     image k has its top-left pixel at ((k / xmaps) (H + padding) + padding, (k % xmaps) (W + padding) + padding);
 *     a value v becomes  u = (clamp(v, lo, hi) - lo) / max(hi - lo, 1e-5);  uint8(clamp(u * 255 + 0.5, 0, 255)),
 *     every step rounded to f32, truncated; C = 1 fills the three channels with the one value;
 *     every other pixel, the cells after the last image included, is uint8(clamp(pad_value * 255 + 0.5, 0, 255)).
 *   N == 1 gives the bare image: Hg = H, Wg = W, no border (make_grid returns early).
 *   Every byte of out is written exactly once: no memset is needed.  No atomics, no workspace; capturable.
 *   Hg * Wg < 2^31.  lo, hi, pad_value must not be NaN; a NaN in x gives an unspecified byte.
 *
 * g2s_ppl_latents: pairs [2B, D] f32 (rows 2i, 2i + 1 = the ends a, b of pair i), t [B] f32  ->  out [2B, D]:
 *   row 2i is the point at t[i], row 2i + 1 the point at t1 = t[i] + eps, that sum rounded to f32.
 *     mode 0 (w):  a + (b - a) * t
 *     mode 1 (z):  n(x) = x / sqrt(sum x^2);  a = n(a), b = n(b), d = sum(a b), p = t acos(d), c = n(b - d a),
 *                  n(a cos p + c sin p)
 *   ONE launch, one 64-lane wave per pair, both rows from one read of the pair (D <= 512; longer rows are read again
 *   by each pass).  The arithmetic is double, the sums fixed-order butterflies: no atomics, bit-identical from run to
 *   run in every mode.  Any D >= 1; 16-byte accesses when D % 4 == 0 and pairs and out are 16-byte aligned.
 *   out must not overlap pairs.  Parallel ends (a = +-b up to scale) give NaN in mode 1, as the formula does.
 * ---------------------------------------------------------------------------------------- */
int g2s_image_grid_u8(const float *x, uint8_t *out, int N, int C, int H, int W, int nrow, int padding,
                      float lo, float hi, float pad_value, g2s_stream_t stream);
int g2s_ppl_latents(const float *pairs, const float *t, float eps, int mode, float *out, int B, int D,
                    g2s_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* G2S_H */
