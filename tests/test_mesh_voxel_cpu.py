"""The mesh voxeliser's rules and its host side, without a GPU: the NumPy twin (tests/mesh_voxel_ref.py) against closed forms,
an independent half-space test and invariants that a wrong tie rule cannot satisfy; then rendernet_amd.mesh (load_mesh, fit,
prepare) and the mesh_to_binvox tool.  Everything at S = 32."""
import itertools
import os
import struct

import numpy as np
import pytest

import mesh_voxel_ref as R

S = 32


def _grids(q, tris):
    return R.solid(q, tris, S), R.surface(q, tris, S)


@pytest.fixture(scope="module")
def octa():
    q, t = R.octahedron(4224, 2560)
    return q, t, _grids(q, t)


def _ico(rot):
    v, t = R.icosahedron()
    return R.to_lattice(v @ R.rotation(*rot).T, S, 11.3), t


MESHES = {"octahedron": lambda: R.octahedron(4224, 2560), "cube": lambda: R.cube(1344, 5320),
          "icosahedron": lambda: _ico((0.3, 0.5)), "torus": lambda: R.torus(S, 9, 3.5), "plate": lambda: R.plate(S)}


@pytest.fixture(scope="module", params=sorted(MESHES))
def mesh(request):
    q, t = MESHES[request.param]()
    return request.param, q, t, _grids(q, t)


def test_cube_closed_form():
    q, t = R.cube(1344, 5320)
    solid, surf = _grids(q, t)
    want = np.zeros((S, S, S), bool)
    want[5:21, 5:21, 5:21] = True
    assert solid.sum() == 4096 and np.array_equal(solid, want)
    shell = want.copy()
    shell[6:20, 6:20, 6:20] = False
    assert surf.sum() == 16 ** 3 - 14 ** 3 == 1352 and np.array_equal(surf, shell)
    assert np.array_equal(R.voxelize(q, t, S)[0, ..., 0].astype(bool), want)


def test_octahedron_closed_form_and_its_ties(octa):
    q, t, (solid, surf) = octa
    assert solid.sum() == 1340 and surf.sum() == 1208
    assert not solid[:, :, -1].any() and not surf[:, :, -1].any()
    # the hostile part: after two subdivisions voxel centres lie exactly on projected edges hundreds of times
    q2, t2 = R.subdivide(*R.subdivide(q, t))
    p = q2.astype(np.int64)[t2]
    c = R.U * np.arange(S, dtype=np.int64) + 128
    cu, cv = np.meshgrid(c, c, indexing="ij")
    ties = 0
    for tri in p:
        u, v = tri[:, 0], tri[:, 1]
        E = [(u[(k + 1) % 3] - u[k]) * (cv - v[k]) - (v[(k + 1) % 3] - v[k]) * (cu - u[k]) for k in range(3)]
        A = E[0] + E[1] + E[2]
        if A[0, 0] == 0:
            continue
        sgn = 1 if A[0, 0] > 0 else -1
        closed = (sgn * E[0] >= 0) & (sgn * E[1] >= 0) & (sgn * E[2] >= 0)
        ties += sum(int((closed & (e == 0)).sum()) for e in E)
    print("(centre, edge) pairs with the centre on the edge of a projected triangle: %d" % ties)
    assert ties == 576


@pytest.mark.parametrize("rot", [(0.3, 0.5), (1.1, 2.0), (0.0, 0.0)])
def test_icosahedron_against_the_half_space_test(rot):
    q, t = _ico(rot)
    assert (q % 4 == 0).all()
    inside, on = R.inside_convex(q, t, S)
    assert not on.any()                                       # so the exclusion below hides nothing here
    solid = R.solid(q, t, S)
    assert inside.sum() > 3000 and np.array_equal(solid, inside)


def test_octahedron_against_the_half_space_test(octa):
    q, t, (solid, _) = octa
    inside, on = R.inside_convex(q, t, S)
    assert on.sum() > 0 and np.array_equal(solid[~on], inside[~on])


def test_subdivision_changes_no_voxel(mesh):
    name, q, t, (solid, surf) = mesh
    assert (q % 4 == 0).all()
    q2, t2 = R.subdivide(*R.subdivide(q, t))
    assert len(t2) == 16 * len(t)
    assert np.array_equal(R.solid(q2, t2, S), solid), name
    assert np.array_equal(R.surface(q2, t2, S), surf), name


def test_order_rotation_and_orientation_change_no_voxel(mesh):
    name, q, t, (solid, surf) = mesh
    rng = np.random.default_rng(5)
    shuffled = t[rng.permutation(len(t))]
    assert np.array_equal(R.solid(q, shuffled, S), solid) and np.array_equal(R.surface(q, shuffled, S), surf)
    for r in (1, 2):
        rolled = np.roll(t, r, axis=1)
        assert np.array_equal(R.solid(q, rolled, S), solid) and np.array_equal(R.surface(q, rolled, S), surf)
    mixed = t.copy()
    flip = rng.random(len(t)) < 0.5
    mixed[flip] = mixed[flip][:, [0, 2, 1]]
    assert np.array_equal(R.solid(q, mixed, S), solid)        # parity does not read the orientation
    assert np.array_equal(R.surface(q, t[:, [0, 2, 1]], S), surf)


def test_torus_and_plate():
    q, t = R.torus(S, 9, 3.5)
    solid, surf = _grids(q, t)
    c = S // 2
    assert solid.sum() > 1500 and not solid[c, c, c] and not solid[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1].any()   # the hole
    assert (surf & ~solid).any() and (solid & ~surf).any()
    q, t = R.plate(S)
    solid, surf = _grids(q, t)
    assert not solid.any() and surf.sum() > 100               # two sheets cancel; a thin part lives in the surface rule alone


def test_a_mesh_reaching_outside_is_clipped():
    q, t = R.cube(1344, 5320)
    big = (q.astype(np.int64) - 3332) * 3 + 3332 + 1700       # from below 0 to past 256 S on every axis
    assert big.min() < 0 and big.max() > R.U * S
    solid, surf = _grids(big, t)
    clamped = np.clip(big, 0, R.U * S)
    assert np.array_equal(solid, R.solid(clamped, t, S)) and np.array_equal(surf, R.surface(clamped, t, S))
    assert solid.any() and surf.any() and surf[-1].any()      # the far face sits on the grid's last layer
    huge = np.array([[-2 ** 31, 5, 2 ** 31 - 1], [2 ** 31 - 1, -2 ** 31, 0], [77, 2 ** 31 - 1, -2 ** 31]], np.int64)
    R.voxelize(huge, np.array([[0, 1, 2]]), S)                # any int32 is a legal coordinate


# ---- rendernet_amd.mesh ------------------------------------------------------------------------------------------------------

def test_prepare_drops_and_counts_degenerates_and_splits_by_size():
    from rendernet_amd import mesh
    q, t = R.cube(1344, 5320)
    extra = np.array([[0, 0, 1], [2, 2, 2], [0, 7, 0]], np.int32)             # repeated vertices: zero area
    qq = np.concatenate([q, (q[:1] + q[7:8]) // 2])                            # vertex 8 = the midpoint of the diagonal 0-7
    tt = np.concatenate([t[:5], extra, [[0, 8, 7]], t[5:]]).astype(np.int32)  # collinear: zero area
    d = mesh.prepare(qq, tt, S)
    assert d["dropped"] == 4 and np.array_equal(d["tris"], t) and d["q"].dtype == np.int32 and d["S"] == S
    for a, b in (("small_solid", "large_solid"), ("small_surf", "large_surf")):
        assert d[a].dtype == d[b].dtype == np.int32 and not set(d[a]) & set(d[b])
    assert sorted(set(d["small_surf"]) | set(d["large_surf"])) == list(range(12))
    # the four faces across axes 0 and 1 project to segments: they cross no ray
    assert len(d["small_solid"]) + len(d["large_solid"]) == 4 and len(d["large_solid"]) == 4 and len(d["large_surf"]) == 12
    tiny = mesh.prepare(*R.cube(1344, 1344 + 300), S)
    assert len(tiny["large_solid"]) == 0 and len(tiny["large_surf"]) == 0 and len(tiny["small_surf"]) == 12
    assert len(mesh.prepare(q, t, S, threshold=10 ** 6)["large_surf"]) == 0
    for bad_q, bad_t in ((q.astype(np.float32), t), (q, t + 1), (q[:, :2], t), (q, t[:, :2])):
        with pytest.raises(ValueError):
            mesh.prepare(bad_q, bad_t, S)
    with pytest.raises(ValueError):
        mesh.prepare(q, t, 48)
    empty = mesh.prepare(q, np.zeros((0, 3), np.int32), S)
    assert empty["dropped"] == 0 and all(len(empty[k]) == 0 for k in ("tris", "small_solid", "large_solid", "small_surf", "large_surf"))


def test_fit_centres_keeps_the_margin_and_permutes():
    from rendernet_amd import mesh
    rng = np.random.default_rng(3)
    verts = rng.uniform(-1, 1, (50, 3)) * (3.0, 1.0, 0.5) + (10, -4, 2)
    for margin in (0, 1, 3):
        q = mesh.fit(verts, S, margin)
        assert q.dtype == np.int32 and q.shape == (50, 3)
        lo, hi = q.min(0), q.max(0)
        assert lo[0] == 256 * margin and hi[0] == 256 * (S - margin)          # the longest axis fills the grid less the margin
        assert (np.abs(lo + hi - 256 * S) <= 1).all()                         # centred on every axis, to the rounding
    base = mesh.fit(verts, S, 1, "x,y,z")
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            axes = ",".join(("-" if s < 0 else "") + "xyz"[p] for p, s in zip(perm, signs))
            want = mesh.fit(verts[:, perm] * signs, S, 1)
            got = mesh.fit(verts, S, 1, axes)
            assert np.array_equal(got, want), axes
            # against the default: column j is mesh axis perm[j], mirrored about the grid centre where the sign is negative
            ref = np.where(np.asarray(signs) > 0, base[:, perm], 256 * S - base[:, perm])
            assert (np.abs(got - ref) <= 1).all(), axes
    for bad in ("x,y", "x,x,z", "x,y,w", "xyz", ""):
        with pytest.raises(ValueError):
            mesh.fit(verts, S, 1, bad)
    for v, kw in ((np.zeros((4, 3)), {}), (verts, {"margin": 16}), (verts, {"margin": -1}), (verts[:, :2], {}), (verts * np.nan, {})):
        with pytest.raises(ValueError):
            mesh.fit(v, S, **kw)
    with pytest.raises(ValueError):
        mesh.fit(verts, 48)


def test_fit_rounds_half_to_even():
    from rendernet_amd import mesh
    # L = 32 and margin 0: g = p + 16 for a box centred on the origin, so 256 g = 256 p + 4096; p = k / 512 lands on halves
    p = np.array([-16.0, 16.0, 1 / 512, 3 / 512, 5 / 512, -1 / 512, -3 / 512])
    verts = np.stack([p, p, p], 1)
    q = mesh.fit(verts, S, 0)[:, 0]
    assert np.array_equal(q, [0, 8192, 4096, 4098, 4098, 4096, 4094])         # 4096.5 -> 4096, 4097.5 -> 4098, 4098.5 -> 4098


OBJ = """# every face form, a negative index and a quad
mtllib none.mtl
v 0 0 0
v 1 0 0 1.0
v 1 1 0
v 0 1 0
vt 0 0
vn 0 0 1
f 1 2 3
f 1/1 3/1 4/1
f 1//1 2//1 3//1
f 1/1/1 2/1/1 4/1/1
v 0 0 1
f -1 -5 -4
f 1 2 3 4
g tail
"""


def test_load_obj(tmp_path):
    from rendernet_amd import mesh
    p = tmp_path / "m.obj"
    p.write_text(OBJ)
    v, t = mesh.load_mesh(str(p))
    assert v.dtype == np.float64 and v.shape == (5, 3) and t.dtype == np.int32
    assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 3], [4, 0, 1], [0, 1, 2], [0, 2, 3]]
    assert np.array_equal(v[4], [0, 0, 1]) and np.array_equal(v[1], [1, 0, 0])
    for text, line in (("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4), ("v 0 0 0\nf 1 2\n", 2), ("v 0 0\n", 1), ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", 4),
                       ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n", 4), ("v a b c\n", 1), ("v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n", 3)):
        p.write_text(text)
        with pytest.raises(ValueError, match=r"m\.obj line %d" % line):
            mesh.load_mesh(str(p))
    with pytest.raises(ValueError):
        mesh.load_mesh(str(tmp_path / "m.stl"))


def _ply_header(fmt, vprops, fline, nv=4, nf=2):
    return ("ply\nformat %s 1.0\ncomment made by hand\nelement vertex %d\n%selement face %d\n%send_header\n"
            % (fmt, nv, "".join("property %s\n" % p for p in vprops), nf, fline)).encode()


def test_load_ply(tmp_path):
    from rendernet_amd import mesh
    p = tmp_path / "m.ply"
    pts = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.5), (1.0, 1.0, 0.0), (0.0, 1.0, 0.25)]
    want_t = [[0, 1, 2], [0, 2, 3], [0, 1, 3]]
    # ascii: an extra vertex property in the middle, a quad and a triangle
    p.write_bytes(_ply_header("ascii", ["float x", "uchar red", "float y", "float z"], "property list uchar int vertex_indices\n")
                  + "".join("%g 7 %g %g\n" % (x, y, z) for x, y, z in pts).encode() + b"4 0 1 2 3\n3 0 1 3\n")
    v, t = mesh.load_mesh(str(p))
    assert np.array_equal(v, pts) and t.tolist() == want_t and v.dtype == np.float64 and t.dtype == np.int32
    # binary: double coordinates, a short in front, uchar counts with int indices, and a face property before the list
    body = b"".join(struct.pack("<hddd", 9, x, y, z) for x, y, z in pts)
    body += struct.pack("<BB4i", 5, 4, 0, 1, 2, 3) + struct.pack("<BB3i", 6, 3, 0, 1, 3)
    p.write_bytes(_ply_header("binary_little_endian", ["short s", "double x", "double y", "double z"],
                              "property uchar flag\nproperty list uchar int vertex_index\n") + body)
    v, t = mesh.load_mesh(str(p))
    assert np.array_equal(v, pts) and t.tolist() == want_t
    # int counts with uchar indices, float coordinates
    body = b"".join(struct.pack("<fff", x, y, z) for x, y, z in pts) + struct.pack("<i4B", 4, 0, 1, 2, 3) + struct.pack("<i3B", 3, 0, 1, 3)
    p.write_bytes(_ply_header("binary_little_endian", ["float x", "float y", "float z"], "property list int uchar vertex_indices\n") + body)
    v, t = mesh.load_mesh(str(p))
    assert np.array_equal(v, pts) and t.tolist() == want_t
    vline = ["float x", "float y", "float z"]
    flist = "property list uchar int vertex_indices\n"
    rows = "".join("%g %g %g\n" % pt for pt in pts).encode()
    bad = {"big endian": (_ply_header("binary_big_endian", vline, flist) + body, "header"),
           "list on vertex": (_ply_header("ascii", vline + ["list uchar int n"], flist) + rows, "element vertex"),
           "no z": (_ply_header("ascii", ["float x", "float y"], flist) + rows, "element vertex"),
           "integer x": (_ply_header("ascii", ["int x", "float y", "float z"], flist) + rows, "element vertex"),
           "index out of range": (_ply_header("ascii", vline, flist) + rows + b"3 0 1 4\n3 0 1 2\n", "element face"),
           "negative index": (_ply_header("ascii", vline, flist) + rows + b"3 0 1 -1\n3 0 1 2\n", "element face"),
           "no list": (_ply_header("ascii", vline, "property int n\n") + rows + b"1\n2\n", "element face"),
           "short file": (_ply_header("ascii", vline, flist) + rows + b"3 0 1 2\n", "element face"),
           "short binary": (_ply_header("binary_little_endian", vline, flist) + body[:20], "element vertex"),
           "not ply": (b"solid\n", "header")}
    for what, (blob, where) in bad.items():
        p.write_bytes(blob)
        with pytest.raises(ValueError, match=r"m\.ply %s" % where):
            mesh.load_mesh(str(p))
        print("%s: refused" % what)


def test_mesh_to_binvox_round_trip(tmp_path, monkeypatch, capsys):
    """The tool end to end with the twin in the device's place: file -> fit -> prepare -> grid -> binvox -> binvox_rw."""
    import torch
    from rendernet_amd import mesh, ops
    from rendernet_amd.tools import binvox_rw, mesh_to_binvox
    src, dst = tmp_path / "cube.obj", tmp_path / "cube.binvox"
    q, t = R.cube(0, 1)
    src.write_text("".join("v %d %d %d\n" % (x, 2 * y, 3 * z) for x, y, z in q) + "".join("f %d %d %d\n" % tuple(i + 1) for i in t))
    calls = []

    def twin(prepared, S=64, mode="both", return_bits=False, device=None, **kw):
        calls.append((S, mode))
        return torch.as_tensor(R.voxelize(prepared["q"], prepared["tris"], S, mesh.MODES[mode]))
    monkeypatch.setattr(ops, "voxelize_mesh", twin)
    mesh_to_binvox.main([str(src), str(dst), "--size", "32", "--mode", "solid", "--margin", "2", "--axes", "z,y,x"])
    assert calls == [(32, "solid")]
    with open(dst, "rb") as f:
        back = binvox_rw.read_as_3d_array(f)
    want = np.zeros((32, 32, 32), bool)                                        # mesh extents 1, 2, 3: z is the longest, on array axis 0
    want[2:30, 16 - 9:16 + 9, 16 - 5:16 + 5] = True                            # 28 voxels; 28 * 2 / 3 = 18.67, 28 / 3 = 9.33
    assert back.dims == [32, 32, 32] and np.array_equal(back.data, want)
    assert str(dst) in capsys.readouterr().out
    for argv in ([str(src), str(dst), "--size", "48"], [str(src), str(dst), "--mode", "thick"], [str(src)]):
        with pytest.raises(SystemExit):
            mesh_to_binvox.main(argv)
    with pytest.raises(SystemExit, match="axes"):
        mesh_to_binvox.main([str(src), str(dst), "--axes", "x,y"])
