"""Vertex colours in the mesh files (ngp_hip/mesh.py: write_ply, write_obj, read_ply, read_obj): the round trips, the uchar rounding,
and that nothing changes for a caller who passes no colours.  Host code: no GPU."""
import numpy as np
import pytest
import torch

F32 = np.float32


def _mesh(normals):
    from ngp_hip import mesh
    rng = np.random.default_rng(11)
    v = rng.random((7, 3)).astype(F32)
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], np.int32)
    n = rng.standard_normal((7, 3)).astype(F32) if normals else None
    return mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n))


def _colors():
    c = np.random.default_rng(12).random((7, 3)).astype(F32)
    c[0] = (0.0, 1.0, 0.5)
    c[1] = (-0.25, 1.5, np.nan)                                               # clamped in a PLY, kept as they are in an OBJ
    return c


def _same_mesh(a, b):
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
    assert (a.normals is None) == (b.normals is None) and (a.normals is None or torch.equal(a.normals, b.normals))


def test_uchar_rounding():
    """round(clamp(c, 0, 1) 255): the ends, the clamp, halves to even (numpy's rint), a NaN to 0."""
    from ngp_hip.mesh import color_bytes
    c = np.array([0.0, 1.0, -3.0, 7.0, 0.5, 0.4 / 255, 0.6 / 255, 1.25 / 255, 2.75 / 255, 254.4 / 255, np.nan, 1e-9], F32)
    assert color_bytes(c).tolist() == [0, 255, 0, 255, 128, 0, 1, 1, 3, 254, 0, 0]         # 0.5 x 255 = 127.5 exactly: to the even 128
    assert color_bytes(c).dtype == np.uint8 and color_bytes(np.zeros((0, 3), F32)).shape == (0, 3)
    every = np.arange(256, dtype=F32) / F32(255.0)
    assert color_bytes(every).tolist() == list(range(256))                      # what read_ply hands back is written as the same bytes


@pytest.mark.parametrize("normals", [False, True])
def test_ply_round_trip(tmp_path, normals):
    from ngp_hip import mesh
    m, c = _mesh(normals), _colors()
    path = str(tmp_path / "c.ply")
    mesh.write_ply(path, m, colors=torch.from_numpy(c))
    header = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    props = [line for line in header if line.startswith("property")]
    assert props[-4:] == ["property uchar red", "property uchar green", "property uchar blue", "property list uchar int vertex_indices"]
    assert props[-5] == ("property float nz" if normals else "property float z")
    back, col = mesh.read_ply(path, return_colors=True)
    _same_mesh(m, back)
    assert col.dtype == torch.float32 and np.array_equal(col.numpy(), mesh.color_bytes(c).astype(F32) / F32(255.0))
    again = str(tmp_path / "again.ply")
    mesh.write_ply(again, back, colors=col)                                     # a second generation is stable
    assert open(again, "rb").read() == open(path, "rb").read()
    with pytest.raises(ValueError, match="not the PLY layout"):                 # a coloured file still raises for a caller who asks for none
        mesh.read_ply(path)
    with pytest.raises(ValueError, match="colors must be"):
        mesh.write_ply(path, m, colors=c[:5])
    plain = str(tmp_path / "plain.ply")
    mesh.write_ply(plain, m)
    back, col = mesh.read_ply(plain, return_colors=True)
    _same_mesh(m, back)
    assert col is None
    _same_mesh(m, mesh.read_ply(plain))
    truncated = str(tmp_path / "short.ply")
    open(truncated, "wb").write(open(path, "rb").read()[:-1])
    with pytest.raises(ValueError, match="bytes"):
        mesh.read_ply(truncated, return_colors=True)


@pytest.mark.parametrize("normals", [False, True])
def test_obj_round_trip(tmp_path, normals):
    from ngp_hip import mesh
    m, c = _mesh(normals), _colors()
    c[1, 2] = 0.125                                                            # text: a NaN is not a round trip worth promising
    path = str(tmp_path / "c.obj")
    mesh.write_obj(path, m, colors=c)
    lines = [line for line in open(path).read().split("\n") if line.startswith("v ")]
    assert len(lines) == 7 and all(len(line.split()) == 7 for line in lines)
    back, col = mesh.read_obj(path, return_colors=True)
    _same_mesh(m, back)
    assert col.dtype == torch.float32 and np.array_equal(col.numpy(), c)         # nine digits: the f32 itself, unclamped
    with pytest.raises(ValueError, match="not what write_obj produces"):
        mesh.read_obj(path)
    plain = str(tmp_path / "plain.obj")
    mesh.write_obj(plain, m)
    back, col = mesh.read_obj(plain, return_colors=True)
    _same_mesh(m, back)
    assert col is None
    mixed = str(tmp_path / "mixed.obj")
    open(mixed, "w").write(open(path).read().replace(lines[3], " ".join(lines[3].split()[:4])))
    with pytest.raises(ValueError, match="coloured vertices"):
        mesh.read_obj(mixed, return_colors=True)


@pytest.mark.parametrize("normals", [False, True])
def test_default_paths_write_the_same_bytes(tmp_path, normals):
    """colors=None is the writer of before: the same bytes as the positional call, byte for byte the known layout."""
    from ngp_hip import mesh
    m = _mesh(normals)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    mesh.write_ply(a, m)
    mesh.write_ply(b, m, colors=None)
    data = open(a, "rb").read()
    assert data == open(b, "rb").read()
    cols = 6 if normals else 3
    props = "".join("property float %s\n" % p for p in ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []))
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 7\n%selement face 4\nproperty list uchar int vertex_indices\nend_header\n" % props
    rows = b"".join(b"\x03" + np.asarray(r, "<i4").tobytes() for r in m.faces.numpy())
    body = (m.vertices.numpy() if not normals else np.concatenate([m.vertices.numpy(), m.normals.numpy()], 1)).astype("<f4").tobytes()
    assert data == header.encode("ascii") + body + rows and len(body) == 4 * cols * 7
    a, b = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
    mesh.write_obj(a, m)
    mesh.write_obj(b, m, colors=None)
    text = open(a).read()
    assert text == open(b).read() and text.startswith("# 7 vertices, 4 faces\nv ")
    assert all(len(line.split()) == 4 for line in text.split("\n") if line.startswith(("v ", "vn ", "f ")))
    assert ("vn " in text) == normals and ("//" in text) == normals
