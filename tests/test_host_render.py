"""The host side of sam6d_amd/render.py (no GPU): the PLY reader and the defined surface sampler."""
import os

import numpy as np
import pytest
import torch

from sam6d_amd import render
from tests import render_ref as R

REF_MESH = os.path.join(os.environ.get("S6D_REFERENCE_ROOT", "/root/reference"), "SAM-6D", "Data", "Example", "obj_000005.ply")


def write_ply(path, v, f, c=None, binary=False, normals=False, alpha=False, extra_vertex=None, face_sizes=None, face_extra=None,
              fmt=None):
    """A small PLY writer for the tests (the layouts MeshLab / trimesh / Open3D write)."""
    fmt = fmt or ("binary_little_endian" if binary else "ascii")
    head = ["ply", f"format {fmt} 1.0", "comment written by the tests", f"element vertex {len(v)}"]
    head += [f"property float {k}" for k in "xyz"]
    if normals:
        head += [f"property float {k}" for k in ("nx", "ny", "nz")]
    if c is not None:
        head += [f"property uchar {k}" for k in ("red", "green", "blue")] + (["property uchar alpha"] if alpha else [])
    if extra_vertex:
        head.append(f"property float {extra_vertex}")
    head += [f"element face {len(f)}", "property list uchar int vertex_indices"]
    if face_extra:
        head.append(f"property uchar {face_extra}")
    head.append("end_header")
    rows_v, rows_f = [], []
    for i in range(len(v)):
        row = [("f", x) for x in v[i]] + ([("f", 0.0), ("f", 0.0), ("f", 1.0)] if normals else [])
        if c is not None:
            row += [("B", int(x)) for x in c[i]] + ([("B", 255)] if alpha else [])
        if extra_vertex:
            row.append(("f", 0.5))
        rows_v.append(row)
    for j in range(len(f)):
        idx = list(f[j]) if face_sizes is None else list(range(face_sizes[j]))
        rows_f.append([("B", len(idx))] + [("i", int(x)) for x in idx] + ([("B", 1)] if face_extra else []))
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        for row in rows_v + rows_f:
            if binary:
                fh.write(b"".join(np.array([x], dtype={"f": "<f4", "B": "<u1", "i": "<i4"}[k]).tobytes() for k, x in row))
            else:
                fh.write((" ".join(repr(float(np.float32(x))) if k == "f" else str(x) for k, x in row) + " \n").encode())


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("coloured", [False, True])
def test_load_ply_round_trip(tmp_path, binary, coloured):
    v, f, c = R.cube()
    v = v + np.float32(0.123)
    path = tmp_path / "m.ply"
    write_ply(path, v, f, c if coloured else None, binary=binary, normals=coloured, alpha=coloured)
    gv, gf, gc = render.load_ply(str(path))
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and np.array_equal(gv, v) and np.array_equal(gf, f)
    assert (gc is None) if not coloured else (gc.dtype == np.uint8 and np.array_equal(gc, c))


def test_load_ply_names_what_it_refuses(tmp_path):
    v, f, c = R.cube()
    path = str(tmp_path / "m.ply")
    write_ply(path, v, f, extra_vertex="quality")
    with pytest.raises(ValueError, match="vertex property 'float quality'"):
        render.load_ply(path)
    write_ply(path, v, f, face_extra="flags")
    with pytest.raises(ValueError, match="face property 'uchar flags'"):
        render.load_ply(path)
    for binary in (False, True):
        write_ply(path, v, f, binary=binary, face_sizes=[3, 3, 4] + [3] * 9)
        with pytest.raises(ValueError, match="face size 4"):
            render.load_ply(path)
    write_ply(path, v, f, fmt="binary_big_endian")
    with pytest.raises(ValueError, match="format 'binary_big_endian'"):
        render.load_ply(path)
    with open(path, "wb") as fh:
        fh.write(b"solid cube\n")
    with pytest.raises(ValueError, match="not a PLY file"):
        render.load_ply(path)


def test_load_ply_reads_the_reference_example_mesh():
    if not os.path.exists(REF_MESH):
        pytest.skip("the reference's example mesh is not present")
    v, f, c = render.load_ply(REF_MESH)
    assert v.shape == (22831, 3) and f.shape == (45666, 3) and c.shape == (22831, 3)
    assert f.min() == 0 and f.max() == 22830 and np.isfinite(v).all()


def _lattice(n):
    """A fixed lattice of uniforms in [0, 1): a Kronecker sequence, no generator involved."""
    i = np.arange(n, dtype=np.float64)[:, None]
    return torch.from_numpy(np.mod((i + 0.5) * np.array([0.5545497, 0.3080614, 0.7548776]), 1.0).astype(np.float32))


def test_sample_surface():
    v, f, _ = R.torus()
    n = 4000
    u = _lattice(n)
    pts, face, bary = render.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, u)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (n, 3) and face.dtype == torch.int64
    # barycentrics: non-negative, summing to one, and the point they give on the chosen face
    assert (bary >= 0).all() and (bary.sum(1) - 1).abs().max() < 1e-15
    tri = torch.from_numpy(v).double()[torch.from_numpy(f).long()][face]
    want = (bary[:, :, None] * tri).sum(1)
    assert (pts.double() - want).abs().max() <= 2.0 ** -24 * 85 * 1.01 + 1e-12          # one float32 rounding of a coordinate <= 85
    # per-face counts against a float64 cumulative-area search written with numpy
    t64 = v.astype(np.float64)[f]
    area = np.linalg.norm(np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0]), axis=1) / 2
    cum = np.cumsum(area)
    want_face = np.searchsorted(cum, u[:, 0].double().numpy() * cum[-1], side="right")
    assert np.array_equal(np.bincount(face.numpy(), minlength=len(f)), np.bincount(want_face, minlength=len(f)))
    assert np.array_equal(face.numpy(), want_face)
    # area-weighted: the outer half of the torus (larger triangles) gets more than the inner half
    assert len(np.unique(face.numpy())) > 500
    again = render.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, u)
    assert all(torch.equal(a, b) for a, b in zip((pts, face, bary), again))
    with pytest.raises(ValueError, match="uniforms"):
        render.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, u[:-1])
    with pytest.raises(ValueError, match="uniforms"):
        render.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, u + 1)


def test_sample_surface_reflects_the_upper_triangle():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    u = torch.tensor([[0.3, 0.25, 0.5], [0.3, 0.75, 0.5]])
    pts, face, bary = render.sample_surface(v, f, 2, u)
    assert torch.equal(pts, torch.tensor([[0.25, 0.5, 0.0], [0.25, 0.5, 0.0]])) and face.tolist() == [0, 0]


def test_ops_render_views_refuses_host_tensors():
    from sam6d_amd import ops
    assert ops.have("render_views")
    v, f, c = R.cube()
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.render_views(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c), torch.from_numpy(R.poses(1, 0)), 60.0, 60.0, 32.0,
                         24.0, 48, 64, 0.3, 0.7, 1.0)
