"""The host side of the textured meshes (no GPU): ``render.load_textured_ply`` -- per-vertex and per-wedge texture coordinates,
ascii and binary, the image beside the file or passed in, every refusal -- ``load_ply``'s unchanged refusals, and the argument
rules of ``render_templates`` / ``onboard_from_mesh`` that need no device."""
import numpy as np
import pytest
import torch

from sam6d_amd import render
from tests import render_ref as R
from tests import texture_ref as X


def write_textured_ply(path, v, f, binary=False, vertex_uv=None, names=("texture_u", "texture_v"), wedge=None, wedge_len=6, texnumber=None,
                       texture_files=("tex.png",), colors=None):
    """The layouts MeshLab and the BOP models use: ``comment TextureFile``, per-vertex ``texture_u texture_v`` (or an alias) and / or
    the face list ``texcoord`` (+ ``texnumber``)."""
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment written by the tests"]
    head += [f"comment TextureFile {n}" for n in texture_files]
    head += [f"element vertex {len(v)}"] + [f"property float {k}" for k in "xyz"]
    if colors is not None:
        head += [f"property uchar {k}" for k in ("red", "green", "blue")]
    if vertex_uv is not None:
        head += [f"property float {k}" for k in names]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices"]
    if wedge is not None:
        head.append("property list uchar float texcoord")
    if texnumber is not None:
        head.append("property int texnumber")
    head.append("end_header")
    rows = []
    for i in range(len(v)):
        row = [("f", x) for x in v[i]]
        if colors is not None:
            row += [("B", int(x)) for x in colors[i]]
        if vertex_uv is not None:
            row += [("f", x) for x in vertex_uv[i]]
        rows.append(row)
    for j in range(len(f)):
        row = [("B", 3)] + [("i", int(x)) for x in f[j]]
        if wedge is not None:
            n = wedge_len if j == 1 else 6
            row += [("B", n)] + [("f", x) for x in (list(wedge[j].reshape(-1)) + [0.0] * 6)[:n]]
        if texnumber is not None:
            row.append(("i", int(texnumber[j])))
        rows.append(row)
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for row in rows:
            if binary:
                fh.write(b"".join(np.array([x], dtype={"f": "<f4", "B": "<u1", "i": "<i4"}[k]).tobytes() for k, x in row))
            else:
                fh.write((" ".join(repr(float(np.float32(x))) if k == "f" else str(x) for k, x in row) + " \n").encode())


def _png(path, img):
    from PIL import Image
    Image.fromarray(img).save(path)


@pytest.fixture
def cube(tmp_path):
    v, f, c = R.cube()
    img = X.texture(8, 16, 3)
    _png(tmp_path / "tex.png", img)
    return v, f, c, img, str(tmp_path / "m.ply")


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
@pytest.mark.parametrize("names", [("texture_u", "texture_v"), ("s", "t"), ("u", "v")], ids=lambda n: n[0])
def test_per_vertex_coordinates_are_expanded_through_the_faces(cube, binary, names):
    v, f, c, img, path = cube
    vuv = np.random.RandomState(1).rand(len(v), 2).astype(np.float32) * 3 - 1
    write_textured_ply(path, v, f, binary=binary, vertex_uv=vuv, names=names, colors=c)
    m = render.load_textured_ply(path)
    assert isinstance(m, tuple) and m._fields == ("vertices", "faces", "colors", "uv", "texture") and len(m) == 5
    assert np.array_equal(m.vertices, v) and np.array_equal(m.faces, f) and np.array_equal(m.colors, c)
    assert m.uv.dtype == np.float32 and m.uv.shape == (12, 3, 2) and np.array_equal(m.uv, vuv[f])
    assert m.texture.dtype == np.uint8 and np.array_equal(m.texture, img)          # the file the comment names, beside the PLY


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
@pytest.mark.parametrize("with_vertex_uv", [False, True], ids=["wedge", "wedge-and-vertex"])
def test_per_wedge_coordinates_win(cube, binary, with_vertex_uv):
    v, f, _, img, path = cube
    wedge = X.cube_uv()
    vuv = np.zeros((len(v), 2), np.float32) if with_vertex_uv else None
    write_textured_ply(path, v, f, binary=binary, vertex_uv=vuv, wedge=wedge, texnumber=np.zeros(12, int))
    m = render.load_textured_ply(path)
    assert np.array_equal(m.uv, wedge) and m.uv.dtype == np.float32 and m.colors is None
    assert np.array_equal(m.faces, f) and m.faces.dtype == np.int32 and np.array_equal(m.texture, img)


def test_explicit_texture_argument(cube, tmp_path):
    v, f, _, img, path = cube
    other = X.texture(4, 4, 9)
    _png(tmp_path / "other.png", other)
    write_textured_ply(path, v, f, wedge=X.cube_uv(), texture_files=())                 # no comment at all
    assert np.array_equal(render.load_textured_ply(path, texture=str(tmp_path / "other.png")).texture, other)
    assert np.array_equal(render.load_textured_ply(path, texture=other).texture, other)
    write_textured_ply(path, v, f, wedge=X.cube_uv())                                    # the argument wins over the comment
    assert np.array_equal(render.load_textured_ply(path, texture=other).texture, other)
    from PIL import Image
    Image.fromarray(np.dstack([img, np.full(img.shape[:2], 128, np.uint8)]), "RGBA").save(tmp_path / "tex.png")
    assert np.array_equal(render.load_textured_ply(path).texture, img)                  # .convert("RGB"): the alpha is dropped
    with pytest.raises(ValueError, match="uint8"):
        render.load_textured_ply(path, texture=other.astype(np.float32))


def test_a_mesh_without_coordinates_loads_as_load_ply_does(cube):
    v, f, c, _, path = cube
    write_textured_ply(path, v, f, colors=c, texture_files=())
    m = render.load_textured_ply(path)
    assert m.uv is None and m.texture is None and np.array_equal(m.colors, c) and np.array_equal(m.vertices, v)
    got = render.load_ply(path)
    assert len(got) == 3 and np.array_equal(got[0], v) and np.array_equal(got[1], f) and np.array_equal(got[2], c)


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
def test_refusals_name_the_cause(cube, tmp_path, binary):
    v, f, _, img, path = cube
    wedge = X.cube_uv()
    write_textured_ply(path, v, f, binary=binary, wedge=wedge, texture_files=("tex.png", "tex2.png"))
    with pytest.raises(ValueError, match="2 TextureFile comments"):
        render.load_textured_ply(path)
    write_textured_ply(path, v, f, binary=binary, wedge=wedge, wedge_len=4)
    with pytest.raises(ValueError, match="texcoord list of length 4"):
        render.load_textured_ply(path)
    tn = np.zeros(12, int)
    tn[5] = 1
    write_textured_ply(path, v, f, binary=binary, wedge=wedge, texnumber=tn)
    with pytest.raises(ValueError, match="texnumber 1"):
        render.load_textured_ply(path)
    write_textured_ply(path, v, f, binary=binary, wedge=wedge, texture_files=())
    with pytest.raises(ValueError, match="texture coordinates but no image"):
        render.load_textured_ply(path)
    write_textured_ply(path, v, f, binary=binary, texture_files=())
    with pytest.raises(ValueError, match="no texture coordinates"):
        render.load_textured_ply(path, texture=img)
    from PIL import Image
    Image.fromarray((np.arange(64, dtype=np.uint16) * 900).reshape(8, 8)).save(tmp_path / "deep.png")
    write_textured_ply(path, v, f, binary=binary, wedge=wedge, texture_files=("deep.png",))
    with pytest.raises(ValueError, match="16-bit"):
        render.load_textured_ply(path)


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
def test_load_ply_still_refuses_the_texture_properties(cube, binary):
    v, f, _, _, path = cube
    write_textured_ply(path, v, f, binary=binary, vertex_uv=np.zeros((len(v), 2), np.float32))
    with pytest.raises(ValueError, match="vertex property 'float texture_u'"):
        render.load_ply(path)
    write_textured_ply(path, v, f, binary=binary, wedge=X.cube_uv())
    with pytest.raises(ValueError, match="face property 'list uchar float texcoord'"):
        render.load_ply(path)
    write_textured_ply(path, v, f, binary=binary, texnumber=np.zeros(12, int))
    with pytest.raises(ValueError, match="face property 'int texnumber'"):
        render.load_ply(path)


def test_uv_and_texture_go_together():
    """Checked before anything reaches a device."""
    v, f, _ = R.cube()
    P, KM = R.poses(1, 0), np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="uv and texture must be given together"):
        render.render_templates(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(P), KM, (48, 64), uv=X.cube_uv())
    with pytest.raises(ValueError, match="uv and texture must be given together"):
        render.render_templates(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(P), KM, (48, 64), texture=X.texture(4, 4, 0))
    with pytest.raises(ValueError, match="3 .* or 5"):
        render.onboard_from_mesh(None, None, [(v, f, None, X.cube_uv())], torch.from_numpy(P), KM, (48, 64),
                                 surface_uniforms=torch.zeros(1, 3, 3), n_model_points=2, n_ism_points=1)


def test_textured_ops_refuse_host_tensors():
    from sam6d_amd import ops
    assert ops.have("render_views_textured")
    v, f, _ = R.cube()
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.texture_pyramid(torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.render_views_textured(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(X.cube_uv()), torch.zeros(21, 4, dtype=torch.uint8),
                                  torch.from_numpy(R.poses(1, 0)), 60.0, 60.0, 32.0, 24.0, 48, 64, 0.3, 0.7, 1.0, tex_size=(4, 4))
