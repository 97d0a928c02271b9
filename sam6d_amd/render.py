"""Template views of a CAD mesh rendered on the device, and the rest of the road from a mesh file to ``FramePipeline``.

The reference renders its templates off the machine that runs the models: BlenderProc (``Render/render_custom_templates.py``) for
the custom flow, pyrender over EGL / OpenGL (``Instance_Segmentation_Model/utils/poses/pyrender.py``) for the BOP flow.  An
Instinct accelerator has no raster pipeline, so here the views come from a compute rasteriser (csrc/s6d_raster.hip):

    mesh = load_textured_ply(path)          # (vertices, faces, colors, uv, texture); load_ply for vertex colours alone
    onboarded = onboard_from_mesh(descriptor_model, pem_net, [mesh], poses, K, (H, W), surface_uniforms=u, keys=k)
    FramePipeline(..., scorer=onboarded.scorer, pem_templates=onboarded.pem_templates, object_radius=onboarded.object_radius)

What is exact and what is defined.  Which pixels a view covers, which face is visible there, the model coordinate of the surface
point (the reference's ``xyz_i.npy`` / NOCS map) and the depth follow a fixed arithmetic stated in the kernel source.  The COLOUR of
a path-traced or OpenGL render cannot be reproduced; the shading is a small defined model -- albedo (vertex colour, or the mesh's
texture map sampled from a mip pyramid: data, hence part of the definition) times
``ambient + diffuse * |n . d|`` with the light at the camera, as in both reference renderers (render_custom_templates.py:67-73,
pyrender.py:37-43) -- in the way this project defines its samplers instead of imitating a generator.

The template pose table stays an argument (object -> camera, OpenCV axes: x right, y down, z forward; translation in model units).
The reference's ``cam_poses_level*.npy`` are its data and are not shipped.  They hold camera -> object poses ``C = [Rc | tc]`` in
OpenCV axes with ``tc`` in millimetres; converting them:

  * pyrender flow: the object pose it renders with is ``inv(C)`` (the ``obj_poses_level*.npy`` files), with the camera fixed at
    ``diag(1, -1, -1)``, i.e. the OpenCV camera seen from OpenGL (pyrender.py:25-29), and the translation scaled to the mesh's
    unit (pyrender.py:75-80: ``/ 1000`` for a mesh in metres).  For a mesh in millimetres pass ``inv(C)`` as it is.
  * BlenderProc flow: render_custom_templates.py:62-65 flips the y and z columns of ``C`` (OpenCV -> Blender camera axes) and
    places the camera at ``tc * 0.001 * 2`` in front of an object scaled by ``1 / (2 r)``, r the radius get_norm_info measures.
    A projection does not see a common scale, so the same views come from the unscaled mesh with ``R = Rc^T`` and
    ``t = -Rc^T tc * 0.004 r`` (model units).
"""
import collections
import os

import numpy as np
import torch

from . import onboarding, ops

GREY = 102          # 0.4 * 255: pyrender.py:99-103 paints untextured (T-LESS) meshes a uniform 0.4; render_custom_templates.py:56-60 a uniform base colour


def _device_tensor(a, dtype, name):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a)).cuda()
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    return t.contiguous()


@torch.no_grad()
def render_templates(vertices, faces, poses, K, size, colors=None, ambient=0.3, diffuse=0.7, znear=1.0, *, uv=None, texture=None):
    """T views of one mesh.  vertices (V,3) f32 in model units (millimetres for the reference's meshes), faces (F,3) int32,
    poses (T,4,4) f32 object -> camera (OpenCV axes, translation in model units), K the 3 x 3 camera matrix (fx, fy, cx, cy are
    read from it; pixel (u, v) is sampled at its integer coordinate, as K projects), size = (H, W); colors (V,3) uint8 vertex
    colours, None = a uniform grey (``GREY``).  Tensors on the device; numpy arrays are copied there.
    uv (F,3,2) f32 per face corner and texture (Ht,Wt,3) uint8 RGB, both or neither: the albedo is then the texture, sampled
    bilinearly from its box-filtered mip pyramid at a per-pixel level (csrc/s6d_raster.hip states it), and ``colors`` plays no
    part; the geometry outputs are the same bits either way.  The textured render runs on the device kernels only: with them
    switched off (``policy.disable_fused``) or on host tensors it is refused, never rendered grey.
    ambient / diffuse: the defined shading ``colour * (ambient + diffuse * |n . d|)``; znear in model units (pyrender.py:48 uses
    0.05 m): a triangle with a vertex at Z <= znear is not clipped but refused.
    -> dict: ``rgb`` (T,H,W,3) uint8, ``mask`` (T,H,W) uint8 255 / 0, ``xyz_mm`` (T,H,W,3) f32 model coordinates (0 on background)
    -- the three as ``pem_template_inputs``, ``ism_template_inputs`` and ``onboard`` take them -- ``depth`` (T,H,W) f32 camera Z
    (0 on background) and ``face`` (T,H,W) int32 (-1 on background).
    Raises ValueError when a view has skipped triangles: templates have the object wholly in front of the camera."""
    v = _device_tensor(vertices, torch.float32, "vertices")
    f = _device_tensor(faces, torch.int32, "faces")
    p = _device_tensor(poses, torch.float32, "poses")
    if (uv is None) != (texture is None):
        raise ValueError("render_templates: uv and texture must be given together (got " + ("uv" if texture is None else "texture") + " alone)")
    Km = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    if Km.shape != (3, 3):
        raise ValueError(f"K must be 3 x 3, got {Km.shape}")
    H, W = (int(s) for s in size)
    if uv is None:
        c = torch.full((v.shape[0], 3), GREY, dtype=torch.uint8, device=v.device) if colors is None else _device_tensor(colors, torch.uint8, "colors")
        out = ops.render_views(v, f, c, p, Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2], H, W, ambient, diffuse, znear)
    else:
        if not ops.have("render_views_textured"):
            raise RuntimeError("render_templates: the textured render has no library statement: it needs the device kernel "
                               "(render_views_textured is switched off by policy.disable_fused or missing from the library)")
        image = _device_tensor(texture, torch.uint8, "texture")
        out = ops.render_views_textured(v, f, _device_tensor(uv, torch.float32, "uv"), ops.texture_pyramid(image), p, Km[0, 0], Km[1, 1],
                                        Km[0, 2], Km[1, 2], H, W, ambient, diffuse, znear, tex_size=image.shape[:2])
    skipped = out["skipped"].cpu()
    if bool(skipped.any()):
        bad = torch.nonzero(skipped).squeeze(1).tolist()
        raise ValueError("render_templates: triangles behind znear or far outside the image (they are not clipped) in view(s) " +
                         ", ".join(f"{i} ({int(skipped[i])})" for i in bad))
    return dict(rgb=out["rgb"], mask=out["mask"], xyz_mm=out["xyz"], depth=out["depth"], face=out["face"])


@torch.no_grad()
def sample_surface(vertices, faces, n, uniforms):
    """``trimesh.sample.sample_surface`` in a defined form: the caller's uniforms instead of numpy's generator.

    vertices (V,3), faces (F,3), uniforms (n,3) in [0, 1).  Face: areas and their cumulative sums in float64, accumulated in face
    order on the host (the result does not depend on the device); the face of sample i is the first whose cumulative area exceeds
    ``u[i,0] * total`` (a binary search; a zero-area face is never picked).  Point: ``(a, b) = (u[i,1], u[i,2])``, reflected to
    ``(1 - a, 1 - b)`` when ``a + b > 1`` (trimesh's ``abs(r - 1)``), ``p = v0 + a (v1 - v0) + b (v2 - v0)`` in float64, rounded
    to float32.  Runs once per object: torch ops.
    -> (points (n,3) f32 on vertices' device, face (n,) int64, barycentrics (n,3) f64 = (1 - a - b, a, b))."""
    dev = vertices.device if torch.is_tensor(vertices) else torch.device("cpu")
    v = torch.as_tensor(vertices).detach().cpu().double()
    f = torch.as_tensor(faces).detach().cpu().long()
    u = torch.as_tensor(uniforms).detach().cpu().double()
    if tuple(u.shape) != (int(n), 3) or bool(((u < 0) | (u >= 1)).any()):
        raise ValueError(f"uniforms must be ({int(n)}, 3) in [0, 1), got {tuple(u.shape)}")
    tri = v[f]                                                             # (F,3,3)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = torch.linalg.cross(e1, e2).norm(dim=1) / 2
    cum = torch.cumsum(area, 0)
    if not bool(cum[-1] > 0):
        raise ValueError("sample_surface: the mesh has no area")
    pick = torch.searchsorted(cum, u[:, 0] * cum[-1], right=True).clamp(max=len(f) - 1)
    a, b = u[:, 1], u[:, 2]
    over = a + b > 1
    a, b = torch.where(over, 1 - a, a), torch.where(over, 1 - b, b)
    pts = tri[pick, 0] + a[:, None] * e1[pick] + b[:, None] * e2[pick]
    return pts.float().to(dev), pick.to(dev), torch.stack([1 - a - b, a, b], 1).to(dev)


_PLY_FLOAT = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}
_PLY_INT = {"char": "<i1", "int8": "<i1", "uchar": "<u1", "uint8": "<u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
            "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


_PLY_UV = {"texture_u": 0, "texture_v": 1, "s": 0, "t": 1, "u": 0, "v": 1}          # vertex properties that hold a texture coordinate
_PLY_VERTEX_LISTS = ("vertex_indices", "vertex_index")


def load_ply(path):
    """A triangle mesh from a PLY file -> (vertices (V,3) float32, faces (F,3) int32, colors (V,3) uint8 or None), numpy arrays.
    Formats ``ascii`` and ``binary_little_endian``.  Vertex properties ``x y z``, optionally ``nx ny nz`` (read over) and
    ``red green blue [alpha]``; one face property, the list ``vertex_indices`` (or ``vertex_index``), every face a triangle.
    Anything else -- another element, property or format, a face that is no triangle -- raises ValueError naming it
    (texture coordinates too: ``load_textured_ply`` reads those)."""
    return _read_ply(path, False)[:3]


TexturedMesh = collections.namedtuple("TexturedMesh", "vertices faces colors uv texture")


def load_textured_ply(path, texture=None):
    """``load_ply`` for a mesh whose appearance is a texture map -> TexturedMesh(vertices, faces, colors, uv, texture): uv
    (F,3,2) float32 per face corner and texture (Ht,Wt,3) uint8 RGB (row 0 at the top), both None for a file without texture
    coordinates.  On top of ``load_ply``'s properties it reads

      * vertex properties ``texture_u texture_v`` (or ``s t``, or ``u v``), expanded to per-corner values through the faces;
      * the face list ``texcoord`` of six floats (u, v per corner: MeshLab's wedge coordinates), which wins when both are
        present, and an optional face property ``texnumber``, 0 throughout;
      * the image: ``texture`` (a path, or an (Ht,Wt,3) uint8 array) or, without it, the file the single
        ``comment TextureFile NAME`` names, beside the PLY.  Read with Pillow, ``.convert("RGB")``: no alpha, no gamma.

    ValueError naming the cause: two TextureFile comments, a texcoord list whose length is not 6, a texnumber other than 0,
    texture coordinates with no image (or an image with no coordinates), a 16-bit image."""
    vertices, faces, colors, uv, names = _read_ply(path, True)
    if len(names) > 1:
        raise ValueError(f"{path}: {len(names)} TextureFile comments ({', '.join(names)}): one texture per mesh is supported")
    if texture is None and uv is not None and names:
        texture = os.path.join(os.path.dirname(os.path.abspath(path)), names[0])
    if uv is None:
        if texture is not None:
            raise ValueError(f"{path}: a texture was given but the file has no texture coordinates")
        return TexturedMesh(vertices, faces, colors, None, None)
    if texture is None:
        raise ValueError(f"{path}: texture coordinates but no image (no 'comment TextureFile NAME' in the header and no texture argument)")
    return TexturedMesh(vertices, faces, colors, uv, _texture_image(texture))


def _texture_image(texture):
    """A path or an array -> (Ht,Wt,3) uint8."""
    if isinstance(texture, (str, os.PathLike)):
        from PIL import Image
        with Image.open(texture) as im:
            if im.mode.startswith("I") or im.mode == "F":                  # I;16, I;16B, I (what Pillow makes of 16-bit files), F
                raise ValueError(f"{texture}: image mode '{im.mode}' (16-bit or float) is not supported: 8 bits per channel are read")
            return np.array(im.convert("RGB"))
    a = np.asarray(texture.detach().cpu() if torch.is_tensor(texture) else texture)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"texture must be a path or an (Ht,Wt,3) uint8 array, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _read_ply(path, textured):
    """-> (vertices, faces, colors or None, uv (F,3,2) float32 or None, the names of the TextureFile comments); ``textured``
    admits the texture properties, which are refused otherwise."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data[data.index(b"\n", end) + 1:]
    fmt, elements, tex_names = None, [], []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            if len(w) > 2 and w[0] == "comment" and w[1] == "TextureFile":
                tex_names.append(line.split(None, 2)[2].strip())
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            elements[-1][2].append(w[1:])
        else:
            raise ValueError(f"{path}: unsupported header line '{line}'")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unsupported format '{fmt}' (ascii and binary_little_endian are read)")
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise ValueError(f"{path}: unsupported elements {[e[0] for e in elements]} (vertex, then face)")
    (_, V, vprops), (_, F, fprops) = elements
    names, fields = [p[-1] for p in vprops], []
    for p in vprops:
        kind = _PLY_FLOAT if p[-1] in ("x", "y", "z", "nx", "ny", "nz") or (textured and p[-1] in _PLY_UV) else \
            _PLY_INT if p[-1] in ("red", "green", "blue", "alpha") else None
        if len(p) != 2 or kind is None or p[0] not in kind:
            raise ValueError(f"{path}: unsupported vertex property '{' '.join(p)}'")
        fields.append((p[-1], kind[p[0]]))
    if not all(k in names for k in "xyz"):
        raise ValueError(f"{path}: vertex properties x, y, z are required (got {names})")
    has_rgb = all(k in names for k in ("red", "green", "blue"))
    if has_rgb and any(dict(fields)[k] != "<u1" for k in ("red", "green", "blue")):
        raise ValueError(f"{path}: unsupported vertex property 'red green blue' of a type other than uchar")
    # the face element as a fixed record: (name, dtype of the list's count or None for a scalar, dtype of an item, items)
    layout = []
    for p in fprops:
        if len(p) == 4 and p[0] == "list" and p[3] in _PLY_VERTEX_LISTS and p[1] in _PLY_INT and p[2] in _PLY_INT:
            layout.append(("faces", _PLY_INT[p[1]], _PLY_INT[p[2]], 3))
        elif textured and len(p) == 4 and p[0] == "list" and p[3] == "texcoord" and p[1] in _PLY_INT and p[2] in _PLY_FLOAT:
            layout.append(("texcoord", _PLY_INT[p[1]], _PLY_FLOAT[p[2]], 6))
        elif textured and len(p) == 2 and p[1] == "texnumber" and p[0] in _PLY_INT:
            layout.append(("texnumber", None, _PLY_INT[p[0]], 1))
        else:
            raise ValueError(f"{path}: unsupported face property '{' '.join(p)}'")
    if sorted(e[0] for e in layout) != sorted({e[0] for e in layout} | {"faces"}):
        raise ValueError(f"{path}: unsupported face property '{' '.join(fprops[-1]) if fprops else '(none)'}' (one vertex_indices list, "
                         "no property twice)")
    fdt = np.dtype([(n + k, t, s) for n, ct, it, items in layout for k, t, s in ((("#", ct, ()),) if ct else ()) + (("", it, (items,)),)])
    if fmt == "ascii":
        tok = body.split()
        nv = V * len(fields)
        vt = np.array(tok[:nv], dtype=np.float64).reshape(V, len(fields))
        cols = {name: vt[:, i] for i, (name, _) in enumerate(fields)}
        ft = np.array(tok[nv:], dtype=np.float64)
        width = sum(items + (ct is not None) for _, ct, _, items in layout)
        rows = ft[:len(ft) // width * width].reshape(-1, width)
        rec, at = {}, 0
        for n, ct, _, items in layout:
            if ct:
                rec[n + "#"], at = rows[:, at], at + 1
            rec[n], at = rows[:, at:at + items], at + items
        short = len(ft) != width * F
    else:
        vdt = np.dtype(fields)
        vt = np.frombuffer(body, dtype=vdt, count=V)
        cols = {name: vt[name] for name, _ in fields}
        rest = body[V * vdt.itemsize:]
        rec = np.frombuffer(rest, dtype=fdt, count=min(F, len(rest) // fdt.itemsize))
        rec = {n: rec[n] for n in fdt.names}
        short = len(rest) < F * fdt.itemsize
    # the first record that is not of the fixed form: everything in front of it was read at the right place
    bad = [(int(np.argmax(rec[n + "#"] != items)), n, items) for n, ct, _, items in layout if ct and bool((rec[n + "#"] != items).any())]
    if bad:
        row, n, items = min(bad)
        size = int(rec[n + "#"][row])
        raise ValueError(f"{path}: face size {size} is not supported (triangles only)" if n == "faces" else
                         f"{path}: texcoord list of length {size} is not supported (6 values: u, v per corner)")
    if short:
        raise ValueError(f"{path}: truncated face list" if fmt != "ascii" else f"{path}: face size (truncated list) is not supported (triangles only)")
    if "texnumber" in rec and bool((rec["texnumber"] != 0).any()):
        raise ValueError(f"{path}: texnumber {int(rec['texnumber'][rec['texnumber'] != 0][0])}: one texture per mesh is supported (texnumber 0)")
    vertices = np.stack([cols[k] for k in "xyz"], 1).astype(np.float32)
    colors = np.stack([cols[k] for k in ("red", "green", "blue")], 1).astype(np.uint8) if has_rgb else None
    faces = np.ascontiguousarray(rec["faces"]).astype(np.int32).reshape(F, 3)
    uv = None
    if "texcoord" in rec:
        uv = np.ascontiguousarray(rec["texcoord"]).astype(np.float32).reshape(F, 3, 2)
    else:
        pair = [next((k for k in names if _PLY_UV.get(k) == axis), None) for axis in (0, 1)] if textured else [None, None]
        if (pair[0] is None) != (pair[1] is None):
            raise ValueError(f"{path}: vertex property '{pair[0] or pair[1]}' without its partner")
        if pair[0] is not None:
            if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
                raise ValueError(f"{path}: face indices must lie in [0, {V})")
            uv = np.stack([cols[pair[0]], cols[pair[1]]], 1).astype(np.float32)[faces.reshape(-1)].reshape(F, 3, 2)
    return vertices, faces, colors, uv, tex_names


@torch.no_grad()
def onboard_from_mesh(descriptor_model, pem_net, meshes, poses, K, size, *, surface_uniforms, keys=None, rng=None, n_model_points=1024,
                      n_ism_points=2048, unit_scale=1000.0, ambient=0.3, diffuse=0.7, znear=1.0, **onboard_kw):
    """Mesh -> views -> ``onboarding.onboard`` in one process.

    meshes: a list of (vertices (V,3) f32 model units, faces (F,3) int32, colors (V,3) uint8 or None) -- what ``load_ply`` returns
    -- or of five-element entries (vertices, faces, colors, uv, texture) -- what ``load_textured_ply`` returns: with uv and texture
    the views carry the texture (``render_templates``), with both None the entry is the three-element one;
    poses (T,4,4) object -> camera, one table for every object (module docstring: converting the reference's tables); K, size,
    ambient, diffuse, znear: ``render_templates``.
    surface_uniforms (O, n_model_points + n_ism_points, 3) in [0, 1): the uniforms of ``sample_surface``, the first n_model_points
    rows of an object for the PEM's model cloud, the rest for the cloud the ISM projects.  The defaults are the reference's:
    ``mesh.sample(cfg.n_sample_model_point)`` with 1024 in the test configuration (Pose_Estimation_Model/run_inference_custom.py:
    183-184, config/base.yaml:86) and ``mesh.sample(2048)`` (Instance_Segmentation_Model/run_inference_custom.py:189-190); both
    scripts divide the samples by 1000.0, millimetres to metres, which ``unit_scale`` does here (float32 division).
    keys / rng and the remaining keywords (n_view, n_sample, img_size, normalize, ...) go to ``onboarding.onboard``.
    -> Onboarded, exactly what ``onboard`` returns for the rendered views and these samples."""
    n_m, n_i = int(n_model_points), int(n_ism_points)
    su = torch.as_tensor(surface_uniforms)
    if tuple(su.shape) != (len(meshes), n_m + n_i, 3):
        raise ValueError(f"surface_uniforms must be ({len(meshes)}, {n_m + n_i}, 3), got {tuple(su.shape)}")
    pose_t = _device_tensor(poses, torch.float32, "poses")
    objects = []
    for o, mesh in enumerate(meshes):
        if len(mesh) not in (3, 5):
            raise ValueError(f"meshes[{o}] must have 3 (vertices, faces, colors) or 5 (..., uv, texture) elements, got {len(mesh)}")
        vertices, faces, colors, uv, texture = tuple(mesh) + (None, None) * (len(mesh) == 3)
        v = _device_tensor(vertices, torch.float32, "vertices")
        f = _device_tensor(faces, torch.int32, "faces")
        views = render_templates(v, f, pose_t, K, size, colors=colors, ambient=ambient, diffuse=diffuse, znear=znear, uv=uv, texture=texture)
        pts = sample_surface(v, f, n_m + n_i, su[o])[0] / torch.full((1,), float(unit_scale), device=v.device)
        objects.append(dict(rgb=views["rgb"], mask=views["mask"], xyz_mm=views["xyz_mm"], model_points=pts[:n_m].contiguous(),
                            ism_points=pts[n_m:].contiguous(), poses=pose_t))
    return onboarding.onboard(descriptor_model, pem_net, objects, keys=keys, rng=rng, **onboard_kw)
