"""The surface-net mesh extractor without a device: the NumPy twin (tests/mesh_extract_ref.py) against closed forms and against the
voxeliser's twin (the round trip: the mesh, voxelised in solid mode, is the thresholded grid voxel for voxel), save_mesh ->
load_mesh, the header / binding / build entries, and the argument checks of ops.extract_mesh that need no device."""
import os
import re

import numpy as np
import pytest

import mesh_extract_ref as E
import mesh_voxel_ref as R
from header_version import states_version

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32


@pytest.fixture(scope="module")
def cases():
    """name -> (vol, threshold, inside bool, {smooth: (q, faces)}), computed once."""
    out = {}
    for name, (vol, thr) in E.cases32().items():
        inside = vol.astype(np.float32) > np.float32(thr)
        out[name] = (vol, thr, inside, {sm: E.extract(vol, thr, sm) for sm in (True, False)})
    return out


def _signed_volume6(q, tris):
    """Sum of det(p0, p1, p2) over the triangles = 6 x the enclosed volume, in Python integers."""
    p = q.astype(np.int64)[tris]
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    det = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0]) +
           a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]))                  # |coordinate| <= 2^13 at 32^3: below 2^41
    return int(det.sum())


def test_a_lone_voxel_is_its_eight_corners_and_six_outward_quads():
    vol = np.zeros((S, S, S), np.float32)
    vol[5, 9, 20] = 1.0
    q, faces = E.extract(vol, 0.5, smooth=False)
    lo = 256 * np.array([5, 9, 20])
    want = np.array([lo + 256 * np.array([i, j, k]) for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.int32)
    assert q.dtype == np.int32 and faces.dtype == np.int32
    assert np.array_equal(q, want)                                             # cell flat-index order
    assert faces.shape == (6, 4)
    centre = lo + 128
    for ring in faces:
        p = q[ring].astype(np.int64)
        n = np.cross(p[1] - p[0], p[2] - p[1])
        assert np.count_nonzero(n) == 1 and n @ (p.mean(0) - centre) > 0       # axis-aligned and outward
        assert np.array_equal(np.cross(p[2] - p[0], p[3] - p[2]), n)           # a planar square
    # quads by (owning cell, axis): cell (4, 8, 19), vertex 0, owns the three edges INTO the voxel; cells (5, 8, 19), (4, 9, 19)
    # and (4, 8, 20), vertices 4, 2 and 1, each own one edge OUT of it
    assert faces[:, 0].tolist() == [0, 0, 0, 1, 2, 4]
    q2, f2 = E.extract(vol, 0.5, smooth=True)
    assert np.array_equal(f2, faces) and ((q2 > want - 128) & (q2 < want + 128)).all()          # strictly inside its cell


def test_blocky_volume_edge_pairing_and_no_zero_area(cases):
    for name, (vol, thr, inside, meshes) in cases.items():
        for smooth, (q, faces) in meshes.items():
            tris = E.fan(faces)
            if not smooth:                                                     # exactly the exposed faces: the voxels' volume
                assert _signed_volume6(q, tris) == 6 * 256 ** 3 * int(inside.sum()), name
            # every directed edge as often as its reverse (closed, also across diagonal voxel contacts)
            e = np.concatenate([faces[:, [k, (k + 1) % 4]] for k in range(4)]).astype(np.int64)
            key, rev = e[:, 0] * len(q) + e[:, 1], e[:, 1] * len(q) + e[:, 0]
            ku, kc = np.unique(key, return_counts=True)
            ru, rc = np.unique(rev, return_counts=True)
            assert np.array_equal(ku, ru) and np.array_equal(kc, rc), name
            p = q.astype(np.int64)[tris]
            n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1])
            assert (n != 0).any(1).all(), (name, smooth)
            assert int(faces.min()) >= 0 and int(faces.max()) < len(q)
            assert len(np.unique(faces)) == len(q)                             # every vertex is used
    q, faces = cases["edge_contact"][3][False]
    assert len(q) == 14 and len(faces) == 12                                   # the shared edge: two vertices, four quads meet


@pytest.mark.parametrize("smooth", [True, False], ids=["smooth", "blocky"])
def test_round_trip_through_the_solid_rule(cases, smooth):
    """The voxeliser's twin, fed the mesh, returns the inside set: no voxel differs."""
    for name, (vol, thr, inside, meshes) in cases.items():
        q, faces = meshes[smooth]
        back = R.solid(q, E.fan(faces), S)
        diff = int((back != inside).sum())
        print("%s %s: %d vertices, %d quads, %d of %d inside, %d voxels differ" % (name, "smooth" if smooth else "blocky", len(q),
                                                                                   len(faces), int(inside.sum()), S ** 3, diff))
        assert diff == 0, name
    assert cases["full"][2].all() and len(cases["full"][3][smooth][0]) == 33 ** 3 - 31 ** 3     # only boundary cells are active
    assert int(cases["threshold_ties"][2].sum()) < int((cases["threshold_ties"][0] >= 0.5).sum())   # the ties are outside


def test_smooth_vertices_follow_the_field(cases):
    """Not only legal but sensible: on the sphere field the smooth vertices lie within half a voxel of the sphere."""
    q, _ = cases["sphere"][3][True]
    r = np.sqrt((((q / 256.0 - 0.5) - np.array([15.7, 16.15, 15.55])) ** 2).sum(1))
    assert np.abs(r - 0.37 * S).max() < 0.5
    qb, _ = cases["sphere"][3][False]
    rb = np.sqrt((((qb / 256.0 - 0.5) - np.array([15.7, 16.15, 15.55])) ** 2).sum(1))
    assert np.abs(r - 0.37 * S).mean() < 0.25 * np.abs(rb - 0.37 * S).mean()


def test_batch_twin_offsets():
    vols = np.stack([E.cases32()["sphere"][0], np.zeros((S, S, S), np.float32), E.cases32()["edge_contact"][0]])
    q, f, vo, fo = E.extract_batch(vols[..., None], 0.5, True, triangles=True)
    assert vo.tolist() == [0, 2646, 2646, 2660] and fo.tolist() == [0, 2 * 2644, 2 * 2644, 2 * 2644 + 24]
    assert f.shape == (fo[-1], 3) and int(f[fo[2]:].max()) == 13


@pytest.mark.parametrize("ext", ["obj", "ply"])
def test_save_mesh_reads_back_exactly(tmp_path, cases, ext):
    from rendernet_amd import mesh
    q, faces = cases["sphere"][3][True]
    path = str(tmp_path / ("m." + ext))
    mesh.save_mesh(path, q, faces)
    v, t = mesh.load_mesh(path)
    assert np.array_equal(v, q / 256.0) and np.array_equal(t, E.fan(faces))
    mesh.save_mesh(path, q, E.fan(faces))                                      # triangles as given
    v, t = mesh.load_mesh(path)
    assert np.array_equal(v, q / 256.0) and np.array_equal(t, E.fan(faces))
    # axes: written backwards, so the same string brings the vertices back onto the grid's axes; a mirroring one turns the faces
    for axes, mirrored in (("z,y,x", True), ("y,z,x", False), ("-y,z,x", True), ("-x,-y,z", False)):
        mesh.save_mesh(path, q, faces, axes=axes)
        v, t = mesh.load_mesh(path)
        perm, sign = mesh.parse_axes(axes)
        assert np.array_equal(v[:, perm] * np.asarray(sign), q / 256.0), axes
        assert np.array_equal(t, E.fan(faces[:, [0, 3, 2, 1]] if mirrored else faces)), axes
        vol6 = _signed_volume6(np.rint(v * 256).astype(np.int32), t)
        assert vol6 > 0, axes                                                  # still outward in the mesh's own frame
    # fit with margin 0 on a mesh that spans the grid is the identity: the file voxelises to the grid it came from
    full_q, full_f = cases["full"][3][False]
    mesh.save_mesh(path, full_q, full_f)
    v, t = mesh.load_mesh(path)
    assert np.array_equal(mesh.fit(v, S, margin=0), full_q)
    mesh.save_mesh(path, np.zeros((0, 3), np.int32), np.zeros((0, 4), np.int32))       # an empty grid's mesh
    v, t = mesh.load_mesh(path)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    for bad in ((q.astype(np.float32), faces), (q, faces[:, :2]), (q, faces + len(q)), (q[:, :2], faces)):
        with pytest.raises(ValueError):
            mesh.save_mesh(path, *bad)
    with pytest.raises(ValueError):
        mesh.save_mesh(str(tmp_path / "m.stl"), q, faces)


def test_header_declares_and_lib_binds_the_entries():
    from rendernet_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    src = open(os.path.join(ROOT, "rendernet_amd", "csrc", "mesh_extract.hip")).read()
    want = {"rn_mesh_extract_workspace_bytes": ("size_t", ["int B", "int S"]),
            "rn_mesh_extract_count": ("int", ["const void* vol", "int vol_is_u8", "float threshold", "int B", "int S", "void* workspace",
                                              "size_t workspace_bytes", "int* totals", "void* stream"]),
            "rn_mesh_extract_emit": ("int", ["const void* vol", "int vol_is_u8", "float threshold", "int B", "int S", "int mode",
                                             "int triangles", "const void* workspace", "size_t workspace_bytes",
                                             "const long long* vert_offsets", "const long long* quad_offsets", "long long n_verts",
                                             "long long n_quads", "int* cellvert", "int* q", "int* faces", "void* stream"])}
    ctype = {"int": _lib._c_int, "float": _lib._c_f, "size_t": _lib.ctypes.c_size_t, "long long": _lib.ctypes.c_longlong}
    for name, (ret, params) in want.items():
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
        assert m, name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[ret]
        assert list(args) == [_lib._c_vp if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in params], name
        assert 'extern "C" %s %s(' % (ret, name) in src
    for kernel in ("extract_count_kernel", "extract_scan_kernel", "extract_verts_kernel", "extract_quads_kernel"):
        assert re.search(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, src), kernel
    assert "mesh_extract.hip" in build.SOURCES and build.EXTRA_FLAGS["mesh_extract.hip"] == ["-ffp-contract=off"]
    assert re.search(r"#define\s+RN_EXTRACT_BLOCKY\s+0\b", text) and _lib.RN_EXTRACT_BLOCKY == 0
    assert re.search(r"#define\s+RN_EXTRACT_SMOOTH\s+1\b", text) and _lib.RN_EXTRACT_SMOOTH == 1
    assert states_version(text)
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "hipcub" not in code and "rocprim" not in code and "asm" not in code


def test_the_host_checks_of_the_c_abi_need_no_device():
    """Arguments that are refused before any HIP call: the library is loaded, nothing is launched."""
    from rendernet_amd import _lib
    L = _lib.lib()
    assert L.rn_mesh_extract_workspace_bytes(1, 32) == (33 ** 3 + 255) // 256 * 8 + 8          # 141 totals, rounded up to 16
    assert L.rn_mesh_extract_workspace_bytes(24, 64) == 24 * ((65 ** 3 + 255) // 256) * 8
    assert L.rn_mesh_extract_workspace_bytes(3, 128) % 16 == 0
    for B, s in ((1, 48), (-1, 32), (65536, 32), (1, 256)):
        assert L.rn_mesh_extract_workspace_bytes(B, s) == 0 and b"rn_mesh_extract_workspace_bytes" in L.rn_last_error()
    assert L.rn_mesh_extract_count(None, 0, 0.5, 1, 48, None, 0, None, None) != 0 and b"rn_mesh_extract_count: S=48" in L.rn_last_error()
    assert L.rn_mesh_extract_count(None, 0, float("nan"), 1, 32, None, 0, None, None) != 0 and b"NaN" in L.rn_last_error()
    assert L.rn_mesh_extract_count(None, 0, 0.5, 1, 32, None, 0, None, None) != 0 and b"null pointer" in L.rn_last_error()
    assert L.rn_mesh_extract_emit(None, 0, 0.5, -1, 32, 1, 0, None, 0, None, None, 0, 0, None, None, None, None) != 0
    assert b"rn_mesh_extract_emit: B=-1" in L.rn_last_error()
    assert L.rn_mesh_extract_count(None, 0, 0.5, 0, 32, None, 0, None, None) == 0              # B == 0: a no-op


def test_ops_extract_mesh_checks_before_any_launch():
    import torch
    from rendernet_amd import mesh, ops
    from rendernet_amd._lib import RenderNetHipError
    ok = torch.zeros((1, 32, 32, 32, 1))
    bad = [(np.zeros((1, 32, 32, 32, 1), np.float32), {}),                     # not a tensor
           (ok, {}),                                                           # not on the device
           (ok.double(), {}), (ok.int(), {}),                                  # dtype
           (torch.zeros((1, 48, 48, 48, 1)), {}), (torch.zeros((1, 32, 32, 16)), {}), (torch.zeros((32, 32, 32)), {}),
           (torch.zeros((1, 32, 32, 32, 2)), {}),
           (ok, {"threshold": float("nan")}), (ok, {"threshold": float("inf")}), (ok, {"threshold": "0.5"}),
           (ok, {"smooth": 1}), (ok, {"triangles": None})]
    for vol, kw in bad:
        with pytest.raises(RenderNetHipError):
            ops.extract_mesh(vol, **kw)
    with pytest.raises(ValueError):
        mesh.extract(np.zeros((2, 32, 32, 32), np.float32))                    # one grid at a time


def test_the_scripts_know_the_mesh_flags():
    import RenderNet_demo
    from rendernet_amd.tools import binvox_to_mesh
    args = RenderNet_demo.build_parser().parse_args(["--save_mesh", "x.ply", "--mesh_blocky", "True"])
    assert args.save_mesh == "x.ply" and args.mesh_blocky is True
    none = RenderNet_demo.build_parser().parse_args([])
    assert none.save_mesh is None and none.mesh_blocky is False
    with pytest.raises(SystemExit, match="expected an .obj or .ply"):
        RenderNet_demo.main(["--save_mesh", "x.stl"])
    a = binvox_to_mesh.build_parser().parse_args(["in.npz", "out.obj", "--threshold", "0.1", "--blocky", "--axes", "z,y,x"])
    assert (a.grid, a.mesh, a.threshold, a.blocky, a.axes) == ("in.npz", "out.obj", 0.1, True, "z,y,x")
    for argv, what in ((["in.binvox", "out.stl"], "expected an .obj or .ply"), (["in.txt", "out.obj"], "expected a .binvox or .npz"),
                       (["in.binvox", "out.obj", "--axes", "x,x,y"], "signed permutation")):
        with pytest.raises(SystemExit, match=what):
            binvox_to_mesh.main(argv)
