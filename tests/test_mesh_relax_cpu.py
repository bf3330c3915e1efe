"""Surface-net relaxation without a device: the NumPy twin (tests/mesh_relax_ref.py) against hand-worked cases, the corner
rule of the links against the quad rings, the invariants the header promises (cells, bounds, faces, the solid round trip
through the voxeliser's twin), the quality table of DESIGN.md 5c, the header / binding / build entries and the argument checks
of ops.extract_mesh and of the C entry that need no device."""
import os
import re

import numpy as np
import pytest

import mesh_extract_ref as E
import mesh_relax_ref as X
import mesh_voxel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32
PASSES = (1, 4, 5, 64)
WEIGHTS = (256, 128, 1)
ROUND_TRIP = ("chair32", "full", "touching", "sphere_binary")    # through the voxeliser's twin, which takes its time; the rest keep to the bounds


def _chair32():
    """The chair at 32^3: each 2x2x2 block of the 64^3 model reduced by max."""
    from rendernet_amd.tools import binvox_rw
    with open(os.path.join(ROOT, "binvox", "chair.binvox"), "rb") as f:
        g = np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
    return g.reshape(32, 2, 32, 2, 32, 2).max((1, 3, 5))


def _touching():
    """Five voxels that touch only at edges and corners, the grid corners (0,0,0) and (31,31,31) among them."""
    v = np.zeros((S, S, S), np.uint8)
    v[0, 0, 0] = v[1, 1, 1] = v[1, 2, 2] = v[S - 1, S - 1, S - 1] = v[S - 2, S - 2, S - 1] = 1
    return v


@pytest.fixture(scope="module")
def grids():
    """name -> (vol, threshold, inside, (q, faces) smooth): the binary grids and cases32(), extracted once."""
    out = {"sphere_binary": ((E.sphere_field(S, radius=11.3) > 0.5).astype(np.uint8), 0.5), "chair32": (_chair32(), 0.5),
           "touching": (_touching(), 0.5)}
    out.update(E.cases32())
    return {name: (vol, thr, vol.astype(np.float32) > np.float32(thr), E.extract(vol, thr, True)) for name, (vol, thr) in out.items()}


def test_a_lone_voxel_by_hand():
    """Eight vertices of degree 3.  Blocky, they are the voxel's corners, and one pass at weight 256 puts each at the rounded
    mean of its three neighbours: per axis (2 own + 1 other) / 3, a third of the way across, which the cell bound then stops."""
    vol = np.zeros((S, S, S), np.float32)
    vol[5, 9, 20] = 1.0
    q, faces = E.extract(vol, 0.5, smooth=False)
    lo = 256 * np.array([5, 9, 20])
    links = X.ring_links(faces, len(q))
    assert len(links) == 12 and np.bincount(links.ravel()).tolist() == [3] * 8
    got = X.relax(q, faces, S, 1, 256)
    # a low corner (coordinate x): neighbours x, x, x + 256 -> (3 x + 256 + 1.5) // 3 = x + 85; the bound x + 127 does not bind
    # a high corner (x + 256): neighbours x + 256 twice and x -> floor(x + 512 / 3 + 1 / 2) = x + 171
    bits = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    assert np.array_equal(got, np.where(bits == 0, lo + 85, lo + 171).astype(np.int32))
    # weight 128 goes half of the way, rounded half up: 85.33 / 2 = 42.67 -> 43, and 256 - 42.67 = 213.33 -> 213
    assert np.array_equal(X.relax(q, faces, S, 1, 128), np.where(bits == 0, lo + 43, lo + 213).astype(np.int32))
    # by symmetry low = x + a, high = x + 256 - a, and a pass is a -> round((a + 256) / 3): 85, 114, 123, 126, 127, and then
    # 127.67 -> 128 would reach the sample plane: the bounds x + 127 and x + 129 stop it for good
    for passes, a in ((2, 114), (3, 123), (4, 126), (5, 127), (6, 127), (64, 127)):
        assert np.array_equal(X.relax(q, faces, S, passes, 256), np.where(bits == 0, lo + a, lo + 256 - a).astype(np.int32)), passes
    # the smooth vertices of a lone voxel: every crossing is o = 128, so the mean of the three crossing edges of a corner cell
    # is (128 + 256 + 256) / 3 = 213 from the cell's low planes on the low side of the voxel and 43 on the high side
    qs, fs = E.extract(vol, 0.5, smooth=True)
    assert np.array_equal(fs, faces) and np.array_equal(qs, np.where(bits == 0, lo - 128 + 213, lo + 128 + 43).astype(np.int32))


def test_a_bar_of_two_voxels_by_hand():
    """2x1x1 along axis 0: twelve vertices, the four in the middle of degree 4 (two along the bar, two around it)."""
    vol = np.zeros((S, S, S), np.float32)
    vol[5, 9, 20] = vol[6, 9, 20] = 1.0
    q, faces = E.extract(vol, 0.5, smooth=False)
    assert len(q) == 12 and len(faces) == 10
    x, y, z = 256 * 5, 256 * 9, 256 * 20
    assert q.tolist() == [[x + 256 * i, y + 256 * j, z + 256 * k] for i in (0, 1, 2) for j in (0, 1) for k in (0, 1)]
    links = X.ring_links(faces, 12)
    assert np.bincount(links.ravel()).tolist() == [3] * 4 + [4] * 4 + [3] * 4
    got = X.relax(q, faces, S, 1, 256)
    # ends as for the lone voxel; the middle ring: along the bar the two neighbours cancel, (4 m + 2) // 4 = m; across it
    # the neighbours are own, own, own, other: (4 y + 256 + 2) // 4 = y + 64 from the low side, y + 192 from the high side
    want = [[x + a, y + b, z + c] for a in (85, 256, 512 - 85) for b in ((85, 171) if a != 256 else (64, 192))
            for c in ((85, 171) if a != 256 else (64, 192))]
    assert got.tolist() == want


def test_links_from_the_corner_bits_are_the_ring_links(grids):
    for name, (vol, thr, inside, (q, faces)) in grids.items():
        ring, corner = X.ring_links(faces, len(q)), X.corner_links(vol, thr)
        assert np.array_equal(ring, corner), (name, len(ring), len(corner))
        if len(q):
            deg = np.bincount(ring.ravel(), minlength=len(q))
            assert 3 <= deg.min() and deg.max() <= 6, (name, deg.min(), deg.max())


@pytest.mark.parametrize("weight", WEIGHTS)
def test_cells_bounds_faces_and_the_solid_round_trip(grids, weight):
    for name in sorted(grids):
        vol, thr, inside, (q, faces) = grids[name]
        if len(q) == 0:
            continue
        keep = faces.copy()
        lo, hi = X.bounds(q, S)
        assert np.array_equal(X.relax(q, faces, S, 0, weight), q)
        for passes in PASSES:
            r = X.relax(q, faces, S, passes, weight)
            assert r.dtype == np.int32 and r.shape == q.shape
            assert np.array_equal(X.cells(r), X.cells(q)) and (lo <= r).all() and (r <= hi).all(), (name, passes)
            if name in ROUND_TRIP:
                assert int((R.solid(r, E.fan(faces), S) != inside).sum()) == 0, (name, passes, weight)
        assert np.array_equal(faces, keep)
    q, faces = grids["full"][3]
    r = X.relax(q, faces, S, 4, weight)
    assert int(r.min()) == 0 and int(r.max()) == 256 * S         # the clipped boundary cells: the clamps at 0 and 256 S hold


def test_blocky_start_and_jacobi_order(grids):
    """smooth=False starts from the cell centres and ends in the same cells; a pass reads only the pass before it, so two
    passes are one pass of one pass."""
    vol, thr, inside, _ = grids["chair32"]
    q, faces = E.extract(vol, thr, False)
    r = X.relax(q, faces, S, 4)
    assert np.array_equal(X.cells(r), X.cells(q)) and int((R.solid(r, E.fan(faces), S) != inside).sum()) == 0
    assert np.array_equal(X.relax(X.relax(q, faces, S, 1), faces, S, 1), X.relax(q, faces, S, 2))
    assert not np.array_equal(r, q)


def test_no_zero_area_quad_at_full_weight(grids):
    for name in ("sphere_binary", "chair32", "full"):
        vol, thr, inside, (q, faces) = grids[name]
        for passes in (0,) + PASSES:
            assert X.zero_area_quads(X.relax(q, faces, S, passes, 256), faces) == 0, (name, passes)


def test_quality_on_the_binary_sphere(grids):
    """The table of DESIGN.md 5c: the angle between a normal and the direction from the middle of the grid (lattice point
    128 S on every axis, sample coordinate 15.5), mean / max in degrees, quad normals and vertex normals, to two decimals."""
    vol, thr, inside, (q, faces) = grids["sphere_binary"]
    assert len(q) == 2404 and len(faces) == 2402
    table = {0: (12.14, 36.82, 8.24, 31.29), 2: (4.60, 14.52, 4.17, 13.14), 4: (4.18, 14.51, 3.64, 9.90),
             8: (6.02, 21.08, 4.13, 12.81), 64: (10.48, 31.38, 6.22, 20.67)}
    got = {p: X.sphere_normal_errors(X.relax(q, faces, S, p, 256), faces, [15.5] * 3) for p in table}
    for p, row in table.items():
        print("passes %2d: quad %.2f / %.2f, vertex %.2f / %.2f" % ((p,) + got[p]))
    for p, row in table.items():
        assert [round(v, 2) for v in got[p]] == list(row), (p, got[p])
    assert got[4][0] < 0.5 * got[0][0] and got[4][2] < 0.5 * got[0][2]
    half = X.sphere_normal_errors(X.relax(q, faces, S, 8, 128), faces, [15.5] * 3)
    assert [round(v, 2) for v in half] == [4.30, 14.94, 3.72, 10.25]


def test_header_declares_and_lib_binds_the_entries():
    from rendernet_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    src = open(os.path.join(ROOT, "rendernet_amd", "csrc", "mesh_relax.hip")).read()
    vp, i, ll, f, sz = _lib._c_vp, _lib._c_int, _lib.ctypes.c_longlong, _lib._c_f, _lib.ctypes.c_size_t
    assert _lib.SIGNATURES["rn_mesh_relax_workspace_bytes"] == (sz, [ll])
    assert _lib.SIGNATURES["rn_mesh_relax"] == (i, [vp, i, f, i, i, vp, vp, ll, i, i, vp, sz, vp, vp])
    for name in ("rn_mesh_relax_workspace_bytes", "rn_mesh_relax"):
        assert re.search(r'extern "C" \w+ %s\(' % name, src) and re.search(r"\b%s\(" % name, text), name
    for kernel in ("relax_links_kernel", "relax_pass_kernel"):
        assert re.search(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, src), kernel
    assert "mesh_relax.hip" in build.SOURCES and "mesh_cells.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "mesh_cells.h"))
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("atomic", "cooperative", "hipcub", "rocprim", "asm"):
        assert word not in code, word


def test_the_host_checks_of_the_c_abi_need_no_device():
    """Arguments that are refused before any HIP call: the library is loaded, nothing is launched."""
    from rendernet_amd import _lib
    L = _lib.lib()
    assert L.rn_mesh_relax_workspace_bytes(0) == 0 and L.rn_mesh_relax_workspace_bytes(1) == 48
    assert L.rn_mesh_relax_workspace_bytes(2404) == (2404 * 36 + 15) // 16 * 16
    assert L.rn_mesh_relax_workspace_bytes(-1) == 0 and b"rn_mesh_relax_workspace_bytes" in L.rn_last_error()
    assert L.rn_mesh_relax_workspace_bytes(1 << 31) == 0

    def call(B=1, s=32, nv=8, passes=4, weight=256, thr=0.5, u8=0):
        return L.rn_mesh_relax(None, u8, thr, B, s, None, None, nv, passes, weight, None, 0, None, None)
    for kw, text in ((dict(s=48), b"S=48"), (dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(nv=-1), b"n_verts=-1"),
                     (dict(nv=1 << 31), b"n_verts="), (dict(passes=-1), b"passes=-1"), (dict(passes=65), b"passes=65"),
                     (dict(weight=0), b"weight=0"), (dict(weight=257), b"weight=257"), (dict(thr=float("nan")), b"NaN"),
                     (dict(u8=2), b"vol_is_u8=2"), (dict(B=0), b"of no grid"), (dict(), b"null pointer")):
        assert call(**kw) == _lib.RN_E_INVALID, kw
        assert b"rn_mesh_relax:" in L.rn_last_error() and text in L.rn_last_error(), (kw, L.rn_last_error())
    assert call(B=0, nv=0) == _lib.RN_OK and call(nv=0) == _lib.RN_OK                          # no-ops


def test_ops_extract_mesh_checks_relax_before_any_launch():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    vol = torch.zeros((1, 32, 32, 32, 1))                        # a host tensor: refused LAST, after the relax arguments
    for kw in (dict(relax=True), dict(relax=4.0), dict(relax=-1), dict(relax=65), dict(relax="4"), dict(relax=None),
               dict(relax=4, relax_weight=0), dict(relax=4, relax_weight=257), dict(relax=4, relax_weight=True),
               dict(relax=4, relax_weight=128.0), dict(relax=0, relax_weight=0)):
        with pytest.raises(RenderNetHipError, match="extract_mesh: relax"):
            ops.extract_mesh(vol, **kw)
    with pytest.raises(RenderNetHipError) as e:                  # good relax arguments: the next check speaks
        ops.extract_mesh(vol, relax=64, relax_weight=1)
    assert "relax" not in str(e.value)


def test_the_scripts_know_the_relax_flags():
    import RenderNet_demo
    from rendernet_amd.tools import align_voxels, binvox_to_mesh, carve_voxels, clean_voxels, colour_voxels
    args = RenderNet_demo.build_parser().parse_args(["--save_mesh", "x.ply", "--mesh_relax", "4", "--mesh_relax_weight", "128"])
    assert (args.mesh_relax, args.mesh_relax_weight) == (4, 128)
    none = RenderNet_demo.build_parser().parse_args([])
    assert (none.mesh_relax, none.mesh_relax_weight) == (0, 256)
    a = binvox_to_mesh.build_parser().parse_args(["in.npz", "out.obj", "--relax", "4", "--relax-weight", "77"])
    assert (a.relax, a.relax_weight) == (4, 77)
    a = binvox_to_mesh.build_parser().parse_args(["in.npz", "out.obj"])
    assert (a.relax, a.relax_weight) == (0, 256)
    for tool, argv in ((clean_voxels, ["in.binvox", "out.ply"]), (align_voxels, ["a.binvox", "b.binvox", "out.ply"]),
                       (carve_voxels, ["shots", "out.ply"]), (colour_voxels, ["m.binvox", "shots", "out.ply"])):
        assert tool.build_parser().parse_args(argv).relax == 0, tool.__name__
        assert tool.build_parser().parse_args(argv + ["--relax", "4"]).relax == 4, tool.__name__
