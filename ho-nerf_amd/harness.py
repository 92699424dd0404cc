"""The image-rendering caller of the renderers: `Runner.test` of exp_runner.py:308-374 restated over the C ABI.

What the reference does per test view: build the full NDC pixel grid (exp_runner.py:338-350), turn it into
rays (`_xy_to_ray_bundle`, utils/utils.py:31-115), split the rays into `batch_size` chunks, call
`renderer.render` per chunk, concatenate `color_fine`, and form the image as `(rgb * 255).clip(0, 255)`
reshaped `[H, W, 3]` (exp_runner.py:356-372).  Here the ray bundle comes from `hn_ray_gen` and one `render`
call covers all H*W rays (chunking stays available for memory-bound hosts through `batch_size`).

`render_views` is the two-field counterpart, `get_res.py --render True` (get_res.py:246-287): the fitted hand and object from a set
of held-out cameras, quantised on the device; `write_image` / `read_image` store such images without an image library.
"""
import os
import pickle

import numpy as np
import torch

from . import lib as L
from . import synth


def image_rays(camera, H, W, device):
    """rays_o, rays_d [H*W, 3] of the full pixel grid for one camera dict {'R','T','focal','principal'}
    (arrays shaped like PerspectiveCameras' arguments: [1,3,3], [1,3], [1,2], [1,2])."""
    lib = L.load()
    xy = torch.from_numpy(synth.ndc_grid(H, W)).to(device).contiguous()
    t = {k: torch.as_tensor(np.asarray(camera[k], dtype=np.float32)).to(device).contiguous() for k in ('R', 'T', 'focal', 'principal')}
    B = H * W
    rays_o = torch.empty(B, 3, device=device)
    rays_d = torch.empty(B, 3, device=device)
    L.check(lib.hn_ray_gen(L.ptr(xy), L.ptr(t['R']), L.ptr(t['T']), L.ptr(t['focal']), L.ptr(t['principal']), 1, B,
                           L.ptr(rays_o), L.ptr(rays_d), L.stream_ptr()), 'hn_ray_gen')
    return rays_o, rays_d


def to_image(color_fine, H, W):
    """exp_runner.py:370: `(rgb.reshape(H, W, 3) * 255).clip(0, 255)`, as uint8 like the cv2.imwrite that follows."""
    img = (color_fine.detach().float().cpu().numpy().reshape(H, W, 3) * 255.0).clip(0, 255)
    return img.astype(np.uint8)


def render_image(renderer, camera, H, W, near, far, bt_inv, T_pose_21, Ro=None, To=None, batch_size=None, t_rand=None,
                 index=0):
    """One test view -> uint8 image [H, W, 3] (+ the raw render outputs of the last chunk's keys, concatenated).

    `Ro`/`To` default to the identity pose; as in the reference the renderer receives `Ro.T` (exp_runner.py:365)."""
    device = torch.device('cuda')
    rays_o, rays_d = image_rays(camera, H, W, device)
    Ro = torch.eye(3, device=device) if Ro is None else torch.as_tensor(Ro, dtype=torch.float32, device=device)
    To = torch.zeros(3, device=device) if To is None else torch.as_tensor(To, dtype=torch.float32, device=device)
    B = H * W
    step = B if not batch_size else int(batch_size)
    outs = []
    for s in range(0, B, step):
        kw = {} if t_rand is None else {'t_rand': t_rand[s:s + step]}
        outs.append(renderer.render(rays_o[s:s + step], rays_d[s:s + step], near, far, bt_inv, T_pose_21, None,
                                    Ro.T.contiguous(), To, index, **kw))
    merged = {k: torch.cat([o[k] for o in outs], 0) for k in ('color_fine', 'weight_sum', 'weight_max')}
    return to_image(merged['color_fine'], H, W), merged


def render_views(renderer, cameras, H, W, near, far, bt_inv, T_pose_21, Ro, To, batch_size=16384, t_rand=None):
    """get_res.py:246-287 for a NeuSRenderer_fitting: every camera of `cameras` (a dict of R [V,3,3], T [V,3], focal [V,2], principal
    [V,2], as synth.ring_cameras returns) -> uint8 [V, H, W, 3] on the device.

    Per camera the full NDC grid goes through `image_rays` and then through `renderer.render(.., None, Ro.T, To)` in chunks of
    `batch_size` rays under torch.no_grad() (:263-281; the chunks keep the per-sample outputs of a full image, about 1 GB at
    512 x 334 x 192 samples, out of memory).  `color_fine` is quantised on the device exactly as `to_image` does on the host: fp32
    * 255, clamp to [0, 255], truncate.  `t_rand` is [V, H*W, 1] (the stratified jitter, fixed for a reproducible render) or None.

    There is no argument for the arithmetic: the renderer's `precision` selects it.  These renders keep no tape, so `'f16'` runs BOTH
    fields' single-pass evaluation kernels (k_field2_hand_f16 / k_field2_obj_f16; DESIGN.md 3.17 has the speed and the PSNR / SSIM cost
    against the default `'f16x3'` views)."""
    device = torch.device('cuda')
    cams = {k: np.asarray(cameras[k], dtype=np.float32) for k in ('R', 'T', 'focal', 'principal')}
    V = cams['R'].shape[0]
    if cams['R'].shape != (V, 3, 3) or cams['T'].shape != (V, 3) or cams['focal'].shape != (V, 2) or cams['principal'].shape != (V, 2):
        raise ValueError('render_views: cameras must hold R [V,3,3], T [V,3], focal [V,2], principal [V,2]')
    B, step = H * W, int(batch_size)
    if step < 1:
        raise ValueError('render_views: batch_size = %d' % step)
    if t_rand is not None and tuple(t_rand.shape) != (V, B, 1):
        raise ValueError('render_views: t_rand is %s, expected [%d, %d, 1]' % (tuple(t_rand.shape), V, B))
    Ro_t = torch.as_tensor(Ro, dtype=torch.float32, device=device).T.contiguous()
    To = torch.as_tensor(To, dtype=torch.float32, device=device)
    out = torch.empty(V, H, W, 3, dtype=torch.uint8, device=device)
    with torch.no_grad():
        for v in range(V):
            rays_o, rays_d = image_rays({k: a[v:v + 1] for k, a in cams.items()}, H, W, device)
            flat = out[v].view(B, 3)
            for s in range(0, B, step):
                kw = {} if t_rand is None else {'t_rand': t_rand[v, s:s + step]}
                color = renderer.render(rays_o[s:s + step], rays_d[s:s + step], near, far, bt_inv, T_pose_21, None, Ro_t, To, **kw)['color_fine']
                flat[s:s + step] = (color.detach().float().reshape(-1, 3) * 255.0).clamp(0, 255).to(torch.uint8)
    return out


def render_view_buffers(renderer, cameras, H, W, near, far, bt_inv, T_pose_21, Ro, To, batch_size=16384, t_rand=None, opacity_threshold=0.5):
    """`render_views` with the geometry buffers next to the colour: the same cameras, rays, chunks and `t_rand`, through
    `renderer.render_buffers` under torch.no_grad().  Returns device tensors, with opacity = opacity_hand + opacity_obj per pixel:
      color  uint8 [V, H, W, 3]    `render_views`' bits
      depth  float32 [V, H, W]     depth / opacity where opacity >= opacity_threshold, else 0
      normal uint8 [V, H, W, 3]    the composited normal in the CAMERA frame (row vectors, SURVEY 8c: n_view = n_world @ R), normalised,
                                   (n * 0.5 + 0.5) * 255 clamped and truncated; 0 where opacity < opacity_threshold
      label  uint8 [V, H, W]       0 where opacity < opacity_threshold, else 1 (hand) if opacity_hand >= opacity_obj, else 2 (object)"""
    device = torch.device('cuda')
    cams = {k: np.asarray(cameras[k], dtype=np.float32) for k in ('R', 'T', 'focal', 'principal')}
    V = cams['R'].shape[0]
    if cams['R'].shape != (V, 3, 3) or cams['T'].shape != (V, 3) or cams['focal'].shape != (V, 2) or cams['principal'].shape != (V, 2):
        raise ValueError('render_view_buffers: cameras must hold R [V,3,3], T [V,3], focal [V,2], principal [V,2]')
    B, step = H * W, int(batch_size)
    if step < 1:
        raise ValueError('render_view_buffers: batch_size = %d' % step)
    if t_rand is not None and tuple(t_rand.shape) != (V, B, 1):
        raise ValueError('render_view_buffers: t_rand is %s, expected [%d, %d, 1]' % (tuple(t_rand.shape), V, B))
    Ro_t = torch.as_tensor(Ro, dtype=torch.float32, device=device).T.contiguous()
    To = torch.as_tensor(To, dtype=torch.float32, device=device)
    out = {'color': torch.empty(V, H, W, 3, dtype=torch.uint8, device=device), 'depth': torch.empty(V, H, W, device=device),
           'normal': torch.empty(V, H, W, 3, dtype=torch.uint8, device=device), 'label': torch.empty(V, H, W, dtype=torch.uint8, device=device)}
    with torch.no_grad():
        for v in range(V):
            rays_o, rays_d = image_rays({k: a[v:v + 1] for k, a in cams.items()}, H, W, device)
            R = torch.from_numpy(cams['R'][v]).to(device)
            color, depth, normal, label = out['color'][v].view(B, 3), out['depth'][v].view(B), out['normal'][v].view(B, 3), out['label'][v].view(B)
            for s in range(0, B, step):
                kw = {} if t_rand is None else {'t_rand': t_rand[v, s:s + step]}
                o = renderer.render_buffers(rays_o[s:s + step], rays_d[s:s + step], near, far, bt_inv, T_pose_21, None, Ro_t, To, **kw)
                color[s:s + step] = (o['color_fine'].detach().float().reshape(-1, 3) * 255.0).clamp(0, 255).to(torch.uint8)
                oh, oo = o['opacity_hand'].reshape(-1), o['opacity_obj'].reshape(-1)
                opacity = oh + oo
                seen = opacity >= opacity_threshold
                depth[s:s + step] = torch.where(seen, o['depth'].reshape(-1) / opacity, torch.zeros_like(opacity))
                n = torch.nn.functional.normalize(o['normal'].reshape(-1, 3) @ R, dim=-1)
                normal[s:s + step] = ((n * 0.5 + 0.5) * 255.0).clamp(0, 255).to(torch.uint8) * seen[:, None]
                label[s:s + step] = torch.where(seen, torch.where(oh >= oo, 1, 2), 0).to(torch.uint8)
    return out


def render_mesh_buffers(meshes, cameras, H, W, near, far):
    """`render_view_buffers` for triangle meshes: the same cameras and the same rays (`image_rays`), cast at the meshes by
    `meshcast.MeshCaster`.  `meshes`: one (vertices, triangles) pair, a list of them, or a MeshCaster (prepared once,
    for several calls).  Returns device tensors:
      depth  float32 [V, H, W]     t along the ray of the nearest triangle with near <= t <= far; 0 where there is none
      normal uint8 [V, H, W, 3]    that triangle's own unit normal in the CAMERA frame, render_view_buffers' encoding exactly: n_world @ R,
                                   normalised, (n * 0.5 + 0.5) * 255 clamped and truncated; 0 where nothing is hit
      label  uint8 [V, H, W]       0 where nothing is hit, else 1 + the mesh's index in the list: hand, then object gives
                                   render_view_buffers' labels
      face   int32 [V, H, W]       the triangle's index in the concatenation of the meshes (MeshCaster.face_offsets); -1"""
    from .meshcast import MeshCaster
    device = torch.device('cuda')
    caster = meshes if isinstance(meshes, MeshCaster) else MeshCaster(meshes)
    if caster.n_meshes > 254:
        raise ValueError('render_mesh_buffers: %d meshes, a uint8 label holds 254' % caster.n_meshes)
    cams = {k: np.asarray(cameras[k], dtype=np.float32) for k in ('R', 'T', 'focal', 'principal')}
    V = cams['R'].shape[0]
    if cams['R'].shape != (V, 3, 3) or cams['T'].shape != (V, 3) or cams['focal'].shape != (V, 2) or cams['principal'].shape != (V, 2):
        raise ValueError('render_mesh_buffers: cameras must hold R [V,3,3], T [V,3], focal [V,2], principal [V,2]')
    out = {'depth': torch.empty(V, H, W, device=device), 'normal': torch.empty(V, H, W, 3, dtype=torch.uint8, device=device),
           'label': torch.empty(V, H, W, dtype=torch.uint8, device=device), 'face': torch.empty(V, H, W, dtype=torch.int32, device=device)}
    with torch.no_grad():
        for v in range(V):
            rays_o, rays_d = image_rays({k: a[v:v + 1] for k, a in cams.items()}, H, W, device)
            R = torch.from_numpy(cams['R'][v]).to(device)
            c = caster.cast(rays_o, rays_d, near, far)
            out['depth'][v] = c['t'].view(H, W)
            n = torch.nn.functional.normalize(c['normal'] @ R, dim=-1)
            out['normal'][v] = (((n * 0.5 + 0.5) * 255.0).clamp(0, 255).to(torch.uint8) * c['hit'][:, None]).view(H, W, 3)
            out['label'][v] = (c['mesh'] + 1).to(torch.uint8).view(H, W)
            out['face'][v] = c['face'].view(H, W)
    return out


def label_iou(a, b, label):
    """Intersection over union of the pixels `a == label` and `b == label`, per view: a, b [V, H, W] (or [H, W], one view) label images
    (arrays or tensors; computed where `a` lives, on the device for the outputs of render_view_buffers / render_mesh_buffers) ->
    float64 [V].  A view in which neither image has the label (an empty union) gives 1.0."""
    a = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    b = (b if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b))).to(a.device)
    if a.shape != b.shape or a.dim() not in (2, 3):
        raise ValueError('label_iou: label images of %s and %s, expected two of one shape [V, H, W] or [H, W]' % (tuple(a.shape), tuple(b.shape)))
    ma, mb = (a == label).reshape(a.shape[0] if a.dim() == 3 else 1, -1), (b == label).reshape(a.shape[0] if a.dim() == 3 else 1, -1)
    inter = (ma & mb).sum(1).to(torch.float64)
    union = (ma | mb).sum(1).to(torch.float64)
    return torch.where(union > 0, inter / union.clamp_min(1.0), torch.ones_like(union))


# ---- image files: binary PPM by our own code (always there), anything else through PIL when it imports ---------------------------
def write_image(path, img):
    """uint8 [H, W, 3] (array or tensor) -> a file.  `.ppm`: binary PPM (P6, maxval 255), the channels stored as they are in the array.
    Any other extension is handed to PIL; without PIL that is a RuntimeError."""
    a = _host(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
        raise ValueError('write_image: expected a non-empty uint8 [H, W, 3] image, got %s %s' % (a.dtype, a.shape))
    a = np.ascontiguousarray(a)
    if os.path.splitext(str(path))[1].lower() == '.ppm':
        with open(path, 'wb') as f:
            f.write(b'P6\n%d %d\n255\n' % (a.shape[1], a.shape[0]))
            f.write(a.tobytes())
        return
    _pil(path).fromarray(a).save(path)


def read_image(path):
    """A file -> uint8 [H, W, 3] numpy.  `.ppm`: the binary PPM `write_image` writes (P6, maxval 255; comments in the header are
    allowed); any other extension through PIL (converted to RGB)."""
    if os.path.splitext(str(path))[1].lower() != '.ppm':
        with _pil(path).open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8))
    with open(path, 'rb') as f:
        data = f.read()
    w, h, maxval, pos = _pnm_header(path, data, b'P6', 'PPM')
    if maxval != 255:
        raise ValueError('%s: maxval %d, only 8-bit PPM (maxval 255) is read' % (path, maxval))
    if w < 1 or h < 1:
        raise ValueError('%s: a %d x %d image' % (path, w, h))
    if len(data) - pos < 3 * w * h:
        raise ValueError('%s: truncated: %d bytes of pixels, %d x %d x 3 = %d expected' % (path, len(data) - pos, w, h, 3 * w * h))
    return np.frombuffer(data, dtype=np.uint8, count=3 * w * h, offset=pos).reshape(h, w, 3).copy()


def _pnm_header(path, data, magic, kind):
    """The header of a binary PPM / PGM file's bytes -> (width, height, maxval, offset of the raster)."""
    if data[:2] != magic:
        raise ValueError('%s: not a binary %s (magic %r)' % (path, kind, data[:2]))
    pos, fields = 2, []
    while len(fields) < 3:                                      # width, height, maxval: decimal, separated by whitespace / comments
        while pos < len(data) and (data[pos:pos + 1].isspace() or data[pos:pos + 1] == b'#'):
            if data[pos:pos + 1] == b'#':
                while pos < len(data) and data[pos:pos + 1] not in (b'\n', b'\r'):
                    pos += 1
            else:
                pos += 1
        end = pos
        while end < len(data) and data[end:end + 1].isdigit():
            end += 1
        if end == pos:
            raise ValueError('%s: truncated or malformed %s header' % (path, kind))
        fields.append(int(data[pos:end]))
        pos = end
    if not data[pos:pos + 1].isspace():
        raise ValueError('%s: truncated or malformed %s header' % (path, kind))
    return fields[0], fields[1], fields[2], pos + 1             # (the single whitespace byte before the raster)


# ---- single-channel images: binary PGM (P5), 8 bit for the label maps, 16 bit for depth in millimetres --------------------------------
def write_gray(path, img):
    """uint8 or uint16 [H, W] (array or tensor) -> a binary PGM (P5; maxval 255, or 65535 with the samples big-endian, as the format
    says)."""
    a = _host(img)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim != 2 or a.size == 0:
        raise ValueError('write_gray: expected a non-empty uint8 or uint16 [H, W] image, got %s %s' % (a.dtype, a.shape))
    with open(path, 'wb') as f:
        f.write(b'P5\n%d %d\n%d\n' % (a.shape[1], a.shape[0], 255 if a.dtype == np.uint8 else 65535))
        f.write(np.ascontiguousarray(a).astype('>u2' if a.dtype == np.uint16 else np.uint8).tobytes())


def read_gray(path):
    """The binary PGM `write_gray` writes -> uint8 (maxval 255) or uint16 (maxval 65535) [H, W] numpy; comments in the header are
    allowed."""
    with open(path, 'rb') as f:
        data = f.read()
    w, h, maxval, pos = _pnm_header(path, data, b'P5', 'PGM')
    if maxval not in (255, 65535):
        raise ValueError('%s: maxval %d, only 8-bit (255) and 16-bit (65535) PGM is read' % (path, maxval))
    if w < 1 or h < 1:
        raise ValueError('%s: a %d x %d image' % (path, w, h))
    size = 1 if maxval == 255 else 2
    if len(data) - pos < size * w * h:
        raise ValueError('%s: truncated: %d bytes of pixels, %d x %d x %d = %d expected' % (path, len(data) - pos, w, h, size, size * w * h))
    a = np.frombuffer(data, dtype=np.uint8 if size == 1 else '>u2', count=w * h, offset=pos).reshape(h, w)
    return a.astype(np.uint8 if size == 1 else np.uint16)


def write_depth(path, depth_m):
    """float [H, W] depth in metres (array or tensor) -> a 16-bit PGM in millimetres, rounded to nearest and clamped to 65535; 0 stays
    0, "no surface" (render_view_buffers)."""
    a = np.asarray(_host(depth_m), dtype=np.float64)
    if a.ndim != 2 or a.size == 0 or not np.isfinite(a).all() or (a < 0).any():
        raise ValueError('write_depth: expected a non-empty [H, W] image of finite depths >= 0, got %s' % (a.shape,))
    write_gray(path, np.minimum(np.rint(a * 1000.0), 65535.0).astype(np.uint16))


def read_depth(path):
    """The file `write_depth` writes -> float32 [H, W] metres (0: no surface)."""
    a = read_gray(path)
    if a.dtype != np.uint16:
        raise ValueError('%s: a depth file is a 16-bit PGM' % path)
    return a.astype(np.float32) / np.float32(1000.0)


def _pil(path):
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError('%s: only .ppm is read and written without PIL, and the module PIL does not import' % path)
    return Image


# ---- mesh export: the `mesh_*/{cid}_hand.ply` / `_obj.ply` files of get_res.py, without a mesh library --------------------------
_PLY_HEADER = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
               'element face %d\nproperty list uchar int vertex_indices\nend_header\n')
_PLY_FACE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: float32 vertex x / y / z, faces as uchar-count int32 lists (what open3d and trimesh read).
    vertices [V,3], triangles [T,3] (numpy or tensors)."""
    v = np.ascontiguousarray(_host(vertices), dtype='<f4').reshape(-1, 3)
    t = _host(triangles).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError('write_ply: triangle indices outside [0, %d)' % len(v))
    faces = np.empty(len(t), dtype=_PLY_FACE)
    faces['n'] = 3
    faces['v'] = t
    with open(path, 'wb') as f:
        f.write((_PLY_HEADER % (len(v), len(t))).encode('ascii'))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """The files write_ply writes -> (vertices float32 [V,3], triangles int64 [T,3])."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError('%s: not a PLY file' % path)
    counts = {}
    for line in data[:end].decode('ascii').splitlines():
        w = line.split()
        if w[:1] == ['format'] and w[1] != 'binary_little_endian':
            raise ValueError('%s: only binary_little_endian PLY is read' % path)
        if w[:1] == ['element']:
            counts[w[1]] = int(w[2])
    nv, nf = counts.get('vertex', 0), counts.get('face', 0)
    body = end + len(b'end_header\n')
    v = np.frombuffer(data, dtype='<f4', count=3 * nv, offset=body).reshape(nv, 3).copy()
    faces = np.frombuffer(data, dtype=_PLY_FACE, count=nf, offset=body + 12 * nv)
    if nf and (faces['n'] != 3).any():
        raise ValueError('%s: only triangle faces are read' % path)
    return v, faces['v'].astype(np.int64).reshape(nf, 3)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


# ---- pose files: the `pose_<fit_type>/<cid>.pickle` of fitting_single.py:164-166, 297-315, what analys_results/ reads ---------------
_POSE_SHAPES = {'joint3d': (21, 3), 'Ro': (3, 3), 'To': (3,)}


def write_pose(path, pred_joint3d, pred_Ro, pred_To, gt_joint3d=None, gt_Ro=None, gt_To=None):
    """The reference's pose pickle: a dict of float32 numpy arrays pred_joint3d [21,3], pred_Ro [3,3], pred_To [3] and, when given
    (all three or none), gt_joint3d, gt_Ro, gt_To.  Arrays or tensors; a leading frame axis of 1 is dropped."""
    gts = (gt_joint3d, gt_Ro, gt_To)
    if any(g is None for g in gts) and not all(g is None for g in gts):
        raise ValueError('write_pose: gt_joint3d, gt_Ro and gt_To go together')
    param = {}
    for prefix, vals in (('pred', (pred_joint3d, pred_Ro, pred_To)), ('gt', gts)):
        for (name, shape), a in zip(_POSE_SHAPES.items(), vals):
            if a is None:
                continue
            a = np.array(_host(a), dtype=np.float32)
            if a.shape == (1,) + shape:
                a = a[0]
            if a.shape != shape:
                raise ValueError('write_pose: %s_%s has shape %s, expected %s' % (prefix, name, a.shape, shape))
            param['%s_%s' % (prefix, name)] = np.ascontiguousarray(a)
    with open(path, 'wb') as f:
        pickle.dump(param, f)


def read_pose(path):
    """A pose pickle -> its dict of numpy arrays.  A file without pred_joint3d, pred_Ro and pred_To is refused."""
    with open(path, 'rb') as f:
        param = pickle.load(f)
    need = ['pred_' + k for k in _POSE_SHAPES]
    if not isinstance(param, dict) or any(k not in param for k in need):
        have = sorted(param) if isinstance(param, dict) else type(param).__name__
        raise ValueError('%s: not a pose file: %s missing (it holds %s)' % (path, ', '.join(k for k in need if not isinstance(param, dict)
                                                                                                or k not in param), have))
    return {k: np.asarray(v) for k, v in param.items()}
