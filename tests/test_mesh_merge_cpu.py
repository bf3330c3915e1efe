"""The merged blocky mesh without a device: the NumPy twin (tests/mesh_merge_ref.py) against closed forms, the blocky extractor's
twin and the voxeliser's twin (the round trip: the merged mesh, voxelised in solid mode, is the thresholded grid voxel for
voxel), counts for this rule that were obtained independently, the header / binding / build entries, and the argument checks
of the C ABI, of ops.extract_mesh_merged and of the tools that need no device."""
import os
import re

import numpy as np
import pytest

import mesh_extract_ref as E
import mesh_merge_ref as M
import mesh_voxel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32
PINNED = {"sphere": (1189, 1511), "full": (6, 8), "binary_u8": (32989, 30957), "uniform_noise": (33702, 31584),
          "threshold_ties": (31333, 30012), "edge_contact": (12, 14), "grid_corners": (12, 16)}


@pytest.fixture(scope="module")
def cases():
    """name -> (vol, threshold, inside bool, the twin's five arrays), computed once: cases32() and the geometry edges."""
    out = {}
    for name, (vol, thr) in list(M.cases32().items()) + list(M.edge_cases().items()):
        out[name] = (vol, thr, vol.astype(np.float32) > np.float32(thr), M.merge(vol, thr))
    return out


def _signed_volume6(q, tris):
    """Sum of det(p0, p1, p2) over the triangles = 6 x the enclosed volume."""
    p = q.astype(np.int64)[tris]
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    det = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0]) +
           a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]))                  # |coordinate| <= 2^13 at 32^3: below 2^41
    return int(det.sum())


def _plane_areas(q, faces):
    """{(axis, lattice coordinate, sign of the normal): area in lattice units^2} of an axis-aligned quad mesh."""
    p = q.astype(np.int64)[faces]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1])                         # the rectangle's area along its axis
    assert (np.count_nonzero(n, axis=1) == 1).all()                            # axis-aligned, no zero area
    assert np.array_equal(np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 2]), n)   # planar, both fan triangles the same way
    axis = np.argmax(n != 0, axis=1)
    out = {}
    for a, k, v in zip(axis.tolist(), p[np.arange(len(p)), 0, axis].tolist(), n[np.arange(len(p)), axis].tolist()):
        key = (a, k, v > 0)
        out[key] = out.get(key, 0) + abs(v)
    return out


def test_a_lone_voxel_and_a_plate():
    vol = np.zeros((S, S, S), np.float32)
    vol[5, 9, 20] = 1.0
    q, faces, voxel, direction, size = M.merge(vol)
    bq, _ = E.extract(vol, 0.5, smooth=False)
    assert np.array_equal(q, bq) and faces.shape == (6, 4) and q.dtype == faces.dtype == voxel.dtype == np.int32
    assert direction.tolist() == [1, 0, 3, 2, 5, 4]                            # (a, k, side): the lower plane has side 1
    assert (voxel == (5 * S + 9) * S + 20).all() and (size == 1).all()
    centre = 256 * np.array([5, 9, 20]) + 128
    for ring in faces:
        p = q[ring].astype(np.int64)
        assert np.cross(p[1] - p[0], p[2] - p[1]) @ (p.mean(0) - centre) > 0   # outward
    vol[5, 9:12, 20:27] = 1.0                                                  # a 1 x 3 x 7 plate: six rectangles, eight corners
    q, faces, voxel, direction, size = M.merge(vol)
    assert len(q) == 8 and direction.tolist() == [1, 0, 3, 2, 5, 4]
    assert size.tolist() == [[3, 7], [3, 7], [7, 1], [7, 1], [1, 3], [1, 3]]   # (u, v) = (a + 1, a + 2) mod 3
    first = (5 * S + 9) * S + 20                                               # the inside voxel at (u0, v0): on side 0 below plane k
    assert voxel.tolist() == [first, first, first, first + 2 * S, first, first + 6]


def test_areas_volume_and_planes_against_the_blocky_mesh(cases):
    for name, (vol, thr, inside, (q, faces, voxel, direction, size)) in cases.items():
        bq, bf = E.extract(vol, thr, smooth=False)
        assert int(size.astype(np.int64).prod(1).sum()) == len(bf) == M.blocky_count(vol, thr), name
        assert _signed_volume6(q, E.fan(faces)) == 6 * 256 ** 3 * int(inside.sum()), name
        assert _plane_areas(q, faces) == _plane_areas(bq, bf), name            # the same surface, plane by plane and side by side
        lattice = ((bq[:, 0].astype(np.int64) // 256) * (S + 1) + bq[:, 1] // 256) * (S + 1) + bq[:, 2] // 256
        mine = ((q[:, 0].astype(np.int64) // 256) * (S + 1) + q[:, 1] // 256) * (S + 1) + q[:, 2] // 256
        assert (np.diff(mine) > 0).all() and np.isin(mine, lattice).all(), name   # a subsequence of the blocky vertices
        assert len(np.unique(faces)) == len(q), name                           # every vertex is used


def test_round_trip_through_the_solid_rule(cases):
    for name, (vol, thr, inside, (q, faces, *_)) in cases.items():
        assert np.array_equal(R.solid(q, E.fan(faces), S), inside), name
        uq, uf = M.unshared(q, faces)
        assert len(uq) == 4 * len(faces) and np.array_equal(uq[uf], q[faces])
        assert np.array_equal(R.solid(uq, E.fan(uf), S), inside), name


def test_pinned_counts(cases, fixtures_vox):
    for name, want in PINNED.items():
        q, faces = cases[name][3][:2]
        assert (len(faces), len(q)) == want, name
    q, faces, _, _, size = M.merge(fixtures_vox[0, ..., 0])                    # the chair at 64^3
    assert (len(faces), len(q)) == (831, 1180) and int(size.prod(1).sum()) == 6780
    assert np.array_equal(R.solid(q, E.fan(faces), 64), fixtures_vox[0, ..., 0] > 0.5)
    q, faces = M.merge(fixtures_vox[1, ..., 0])[:2]                            # the bunny
    assert (len(faces), len(q)) == (6434, 8422)


def test_face_fields_follow_the_rule(cases):
    rng = np.random.RandomState(3)
    labels = rng.randint(-2, 2, (S, S, S)).astype(np.int32)
    labels[labels == 1] = np.iinfo(np.int32).max
    for name, (vol, thr, inside, plain) in cases.items():
        for lab, (q, faces, voxel, direction, size) in ((None, plain), (labels, M.merge(vol, thr, labels))):
            pad = np.pad(inside, 1)
            s = np.stack(np.unravel_index(voxel, (S, S, S)), 1)
            a, side = direction // 2, direction % 2
            assert inside[s[:, 0], s[:, 1], s[:, 2]].all(), name
            out = s.copy()
            out[np.arange(len(s)), a] += np.where(side == 0, 1, -1)            # the neighbour across the face
            assert not pad[out[:, 0] + 1, out[:, 1] + 1, out[:, 2] + 1].any(), name
            covered = 0
            for i in range(len(s)) if len(s) < 300 else rng.choice(len(s), 300, replace=False):
                u, v = (a[i] + 1) % 3, (a[i] + 2) % 3
                box = [slice(s[i, j], s[i, j] + 1) for j in range(3)]
                box[u] = slice(s[i, u], s[i, u] + size[i, 0])
                box[v] = slice(s[i, v], s[i, v] + size[i, 1])
                assert inside[tuple(box)].all(), name
                if lab is not None:
                    assert (lab[tuple(box)] == lab[tuple(s[i])]).all(), name   # one label under a rectangle
                covered += 1
            assert covered == min(len(s), 300)
            if lab is not None:
                assert len(faces) >= len(plain[1]) and int(size.astype(np.int64).prod(1).sum()) == M.blocky_count(vol, thr)
                assert np.array_equal(R.solid(q, E.fan(faces), S), inside), name


def test_a_checkerboard_merges_nothing_and_order_is_the_stated_one(cases):
    vol = M.checkerboard(S)
    q, faces, voxel, direction, size = M.merge(vol)
    assert len(faces) == M.blocky_count(vol) == 3 * S ** 3 and (size == 1).all()    # half of each border plane short of 3 S^2 (S + 1)
    for name, (_, _, _, (q, faces, voxel, direction, size)) in cases.items():
        a, side = direction // 2, direction % 2
        p = q[faces[:, 0]].astype(np.int64) // 256                             # the ring starts at (u0, v0) on both sides
        rows = np.arange(len(p))
        key = np.stack([a, p[rows, a], side, p[rows, (a + 1) % 3], p[rows, (a + 2) % 3]], 1)
        order = np.lexsort(key.T[::-1])
        assert np.array_equal(order, rows), name


def test_batch_twin_offsets_and_triangles():
    c = M.cases32()
    vol = np.stack([c["sphere"][0], np.zeros((S, S, S), np.float32), c["edge_contact"][0]])
    q, f, vo, fo, voxel, direction, size = M.merge_batch(vol[..., None], triangles=True)
    q0, f0 = M.merge(vol[0])[:2]
    assert vo.tolist() == [0, len(q0), len(q0), len(q0) + 14] and fo.tolist() == [0, 2 * len(f0), 2 * len(f0), 2 * len(f0) + 24]
    assert np.array_equal(f[:fo[1]], E.fan(f0)) and len(voxel) == len(direction) == len(size) == len(f0) + 12


def test_a_sparse_128_grid_takes_seconds():
    import time
    vol, side = M.word_cases()["word128"]
    t = time.time()
    q, faces, _, _, size = M.merge(vol)
    assert time.time() - t < 20.0 and int(size.max()) == side == 128
    assert int(size.astype(np.int64).prod(1).sum()) == M.blocky_count(vol)


def test_header_declares_and_lib_binds_the_entries():
    from rendernet_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    src = open(os.path.join(ROOT, "rendernet_amd", "csrc", "mesh_merge.hip")).read()
    want = {"rn_mesh_merge_workspace_bytes": ("size_t", ["int B", "int S"]),
            "rn_mesh_merge_count": ("int", ["const void* vol", "int vol_is_u8", "const int* labels", "float threshold", "int B", "int S",
                                            "void* workspace", "size_t workspace_bytes", "int* totals", "void* stream"]),
            "rn_mesh_merge_emit": ("int", ["const int* labels", "int B", "int S", "int triangles", "void* workspace",
                                           "size_t workspace_bytes", "const long long* vert_offsets", "const long long* quad_offsets",
                                           "long long n_verts", "long long n_quads", "int* q", "int* faces", "int* face_voxel",
                                           "int* face_dir", "int* face_size", "void* stream"])}
    ctype = {"int": _lib._c_int, "float": _lib._c_f, "size_t": _lib.ctypes.c_size_t, "long long": _lib.ctypes.c_longlong}
    for name, (ret, params) in want.items():
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
        assert m, name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[ret]
        assert list(args) == [_lib._c_vp if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in params], name
        assert 'extern "C" %s %s(' % (ret, name) in src
        assert getattr(_lib.lib(), name).argtypes == list(args)
    for kernel in ("merge_pack_kernel", "merge_count_kernel", "merge_marks_kernel", "merge_scan_kernel", "merge_verts_kernel",
                   "merge_quads_kernel"):
        assert re.search(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, src), kernel
    assert "mesh_merge.hip" in build.SOURCES
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "hipcub" not in code and "rocprim" not in code and "asm" not in code


def test_the_host_checks_of_the_c_abi_need_no_device():
    """Arguments that are refused before any HIP call: the library is loaded, nothing is launched."""
    from rendernet_amd import _lib
    L = _lib.lib()

    def up16(n):
        return (n + 15) // 16 * 16
    for B, s in ((1, 32), (24, 64), (3, 128)):
        rows, corners = B * 3 * s * s * (16 if s == 128 else 8), B * (s + 1) ** 3
        want = (2 * up16(rows) + up16(corners) + up16(4 * corners) + up16(4 * B * ((3 * (s + 1) * 2 * s + 255) // 256)) +
                up16(4 * B * (((s + 1) ** 3 + 255) // 256)))
        assert L.rn_mesh_merge_workspace_bytes(B, s) == want
    for B, s in ((1, 48), (-1, 32), (65536, 32), (1, 256)):
        assert L.rn_mesh_merge_workspace_bytes(B, s) == 0 and b"rn_mesh_merge_workspace_bytes" in L.rn_last_error()
    assert L.rn_mesh_merge_count(None, 0, None, 0.5, 1, 48, None, 0, None, None) != 0 and b"rn_mesh_merge_count: S=48" in L.rn_last_error()
    assert L.rn_mesh_merge_count(None, 0, None, float("nan"), 1, 32, None, 0, None, None) != 0 and b"NaN" in L.rn_last_error()
    assert L.rn_mesh_merge_count(None, 2, None, 0.5, 1, 32, None, 0, None, None) != 0 and b"vol_is_u8=2" in L.rn_last_error()
    assert L.rn_mesh_merge_count(None, 0, None, 0.5, 1, 32, None, 0, None, None) != 0 and b"null pointer" in L.rn_last_error()
    assert L.rn_mesh_merge_count(None, 0, None, 0.5, 65536, 32, None, 0, None, None) != 0 and b"B=65536" in L.rn_last_error()
    host = (_lib.ctypes.c_int * 64)()                              # host memory stands in for the pointers: refused before any use
    at = _lib.ctypes.addressof(host)
    at += -at % 16
    assert L.rn_mesh_merge_count(at, 0, None, 0.5, 1, 32, at, 16, at, None) != 0 and b"workspace of 16 bytes" in L.rn_last_error()
    assert L.rn_mesh_merge_count(at, 0, None, 0.5, 1, 32, at + 4, 1 << 30, at, None) != 0 and b"16-byte aligned" in L.rn_last_error()
    assert L.rn_mesh_merge_count(at, 0, at + 2, 0.5, 1, 32, at, 1 << 30, at, None) != 0 and b"labels must be 4-byte" in L.rn_last_error()
    assert L.rn_mesh_merge_emit(None, -1, 32, 0, None, 0, None, None, 0, 0, None, None, None, None, None, None) != 0
    assert b"rn_mesh_merge_emit: B=-1" in L.rn_last_error()
    assert L.rn_mesh_merge_emit(None, 1, 32, 2, at, 1 << 30, at, at, 0, 0, None, None, None, None, None, None) != 0
    assert b"triangles=2" in L.rn_last_error()
    assert L.rn_mesh_merge_emit(None, 1, 32, 0, at, 1 << 30, at, at, -1, 0, None, None, None, None, None, None) != 0
    assert b"n_verts=-1" in L.rn_last_error()
    assert L.rn_mesh_merge_emit(None, 1, 32, 0, at, 1 << 30, at, at, 4, 1, at, None, at, at, at, None) != 0 and b"null pointer" in L.rn_last_error()
    assert L.rn_mesh_merge_emit(None, 1, 32, 0, at, 1 << 30, at, at, 4, 1, at, at, at, at, at + 4, None) != 0
    assert b"face_size must be 8-byte" in L.rn_last_error()
    assert L.rn_mesh_merge_count(None, 0, None, 0.5, 0, 32, None, 0, None, None) == 0                # B == 0: a no-op
    assert L.rn_mesh_merge_emit(None, 0, 64, 1, None, 0, None, None, 0, 0, None, None, None, None, None, None) == 0


def test_ops_extract_mesh_merged_checks_before_any_launch():
    import torch
    from rendernet_amd import mesh, ops
    from rendernet_amd._lib import RenderNetHipError
    ok = torch.zeros((1, 32, 32, 32, 1))
    good = torch.zeros((1, 32, 32, 32), dtype=torch.int32)
    bad = [(np.zeros((1, 32, 32, 32, 1), np.float32), {}), (ok, {}), (ok.double(), {}), (ok.int(), {}),
           (torch.zeros((1, 48, 48, 48, 1)), {}), (torch.zeros((32, 32, 32)), {}), (torch.zeros((1, 32, 32, 32, 2)), {}),
           (ok, {"threshold": float("nan")}), (ok, {"threshold": "0.5"}), (ok, {"triangles": None}), (ok, {"triangles": 1})]
    for vol, kw in bad:
        with pytest.raises(RenderNetHipError):
            ops.extract_mesh_merged(vol, **kw)
    for labels in (good.long(), good.float(), np.zeros((1, 32, 32, 32), np.int32), torch.zeros((2, 32, 32, 32), dtype=torch.int32),
                   torch.zeros((1, 32, 32, 16), dtype=torch.int32), torch.zeros((1, 64, 64, 64), dtype=torch.int32)):
        with pytest.raises(RenderNetHipError, match="labels"):
            ops.extract_mesh_merged(ok, labels=labels)
    with pytest.raises(RenderNetHipError, match="CPU|device|cuda"):
        ops.extract_mesh_merged(ok, labels=good)                               # good labels: the grid itself is refused next
    with pytest.raises(RenderNetHipError, match="MergedMesh"):
        ops.merged_face_colours(ops.ExtractedMesh(None, None, None, None), torch.zeros((1, 32, 32, 32, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="merge needs the blocky mesh"):
        mesh.extract(np.zeros((32, 32, 32), np.float32), merge=True)
    with pytest.raises(ValueError, match="merge needs the blocky mesh"):
        mesh.extract(np.zeros((32, 32, 32), np.float32), smooth=False, relax=2, merge=True)
    assert issubclass(ops.MergedMesh, ops.ExtractedMesh)
    doc = ops.extract_mesh_merged.__doc__
    assert "T-junctions" in doc and "export" in doc and "unit-quad form is the one to draw" in doc


def test_the_tools_know_the_merge_flags(capsys):
    import RenderNet_demo
    from rendernet_amd.tools import binvox_to_mesh, colour_voxels
    args = RenderNet_demo.build_parser().parse_args(["--save_mesh", "x.ply", "--mesh_blocky", "True", "--mesh_merge", "True"])
    assert args.mesh_blocky is True and args.mesh_merge is True
    assert RenderNet_demo.build_parser().parse_args([]).mesh_merge is False
    for argv in (["--save_mesh", "x.ply", "--mesh_merge", "True"],
                 ["--save_mesh", "x.ply", "--mesh_blocky", "True", "--mesh_merge", "True", "--mesh_relax", "2"]):
        with pytest.raises(SystemExit, match="--mesh_merge goes with --mesh_blocky"):
            RenderNet_demo.main(argv)
    a = binvox_to_mesh.build_parser().parse_args(["in.npz", "out.obj", "--blocky", "--merge"])
    assert a.blocky and a.merge and not binvox_to_mesh.build_parser().parse_args(["in.npz", "out.obj", "--blocky"]).merge
    for argv in (["in.binvox", "out.obj", "--merge"], ["in.binvox", "out.obj", "--blocky", "--merge", "--relax", "4"]):
        with pytest.raises(SystemExit, match="--merge goes with --blocky and without --relax"):
            binvox_to_mesh.main(argv)
    a = colour_voxels.parse_args(["--from-voxels", "chair.binvox", "out.ply", "--blocky", "--merge"])
    assert a.blocky and a.merge and not colour_voxels.parse_args(["--from-voxels", "chair.binvox", "out.ply", "--blocky"]).merge
    for argv in (["--from-voxels", "chair.binvox", "out.ply", "--merge"],
                 ["--from-voxels", "chair.binvox", "out.ply", "--blocky", "--merge", "--relax", "4"]):
        with pytest.raises(SystemExit):
            colour_voxels.parse_args(argv)
        assert "--merge goes with --blocky and without --relax" in capsys.readouterr().err
