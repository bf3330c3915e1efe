"""The voxel colouring without a device: the NumPy twin (tests/voxel_colour_ref.py) against cases worked by hand, the exact
recovery of a colour field from unsmoothed albedo views on the twins alone, coloured .obj / .ply files there and back, the cell
of a surface-net vertex, and the tool's argument parsing."""
import numpy as np
import pytest

import mesh_extract_ref as XR
import raycast_albedo_ref as AR
import raycast_ref as RR
import voxel_carve_ref as VC
import voxel_colour_ref as CR
from rendernet_amd import mesh, synth

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the twin against hand-computed cases ---------------------------------------------------------------------------------------

def test_accumulate_by_hand():
    S = 32
    hits = np.array([[[[5, 5, 7], [-1, S ** 3, 5]],
                      [[7, INT_MIN, INT_MAX], [5, 5, 5]]]], np.int64)                 # B = 1, K = 2, 2 x 3 pixels
    img = (np.arange(2 * 2 * 3 * 3).reshape(1, 2, 2, 3, 3) * 7 % 256).astype(np.uint8)
    mask = np.ones((1, 2, 2, 3), np.uint8)
    mask[0, 1, 1, 2] = 0                                                               # the last 5 is masked out
    sums = CR.accumulate(img, hits, S, mask).reshape(S ** 3, 4)
    px = img.reshape(-1, 3).astype(np.int64)
    want5 = px[0] + px[1] + px[5] + px[9] + px[10]
    want7 = px[2] + px[6]
    assert sums[5].tolist() == want5.tolist() + [5] and sums[7].tolist() == want7.tolist() + [2]
    rest = np.ones(S ** 3, bool)
    rest[[5, 7]] = False
    assert not sums[rest].any()
    # without the mask the sixth pixel of voxel 5 joins; adding into given sums is plain addition
    more = CR.accumulate(img, hits, S).reshape(S ** 3, 4)
    assert more[5].tolist() == (want5 + px[11]).tolist() + [6]
    twice = CR.accumulate(img, hits, S, mask, sums=sums.reshape(1, S, S, S, 4)).reshape(S ** 3, 4)
    assert np.array_equal(twice, 2 * sums)


def test_resolve_rounds_half_up_and_marks_unseen():
    sums = np.zeros((1, 32, 32, 32, 4), np.int32)
    sums[0, 0, 0, 0] = (1, 2, 3, 2)                     # 0.5 -> 1, 1 -> 1, 1.5 -> 2
    sums[0, 0, 0, 1] = (255 * 3, 0, 254 * 3 + 1, 3)     # 255, 0, 254.33 -> 254
    sums[0, 0, 0, 2] = (10, 10, 10, 0)                  # n = 0: unseen whatever the sums hold
    sums[0, 0, 0, 3] = (7, 8, 10, 4)                    # 1.75 -> 2, 2 -> 2, 2.5 -> 3
    col, known = CR.resolve(sums, unseen=(9, 8, 7))
    assert col[0, 0, 0, 0].tolist() == [1, 1, 2] and col[0, 0, 0, 1].tolist() == [255, 0, 254]
    assert col[0, 0, 0, 2].tolist() == [9, 8, 7] and col[0, 0, 0, 3].tolist() == [2, 2, 3]
    assert known[0, 0, 0, :4].tolist() == [1, 1, 0, 1] and known.sum() == 3
    assert (col.reshape(-1, 3)[4:] == (9, 8, 7)).all()


def test_fill_is_jacobi_and_stops_at_the_grid():
    S = 32
    occ = np.zeros((S, S, S), bool)
    occ[0, 0, 0:4] = True                               # a row in the grid's corner: neighbours outside do not exist
    occ[5, 5, 5] = True                                 # occupied, but no neighbour is ever known
    col = np.full((S, S, S, 3), 128, np.uint8)
    known = np.zeros((S, S, S), np.uint8)
    col[0, 0, 0], known[0, 0, 0] = (10, 20, 31), 1
    col[1, 1, 1], known[1, 1, 1] = (11, 21, 30), 1      # known but not occupied: a neighbour all the same, of (0, 0, 0..2)
    c1, k1 = CR.fill_pass(col, known, occ)
    # (0,0,1) sees both: the means 10.5, 20.5, 30.5 round half up
    assert c1[0, 0, 1].tolist() == [11, 21, 31] and k1[0, 0, 1] == 2
    # (0,0,2) sees (1,1,1) only; (0,0,3) sees nothing yet: a pass reads the state before it
    assert c1[0, 0, 2].tolist() == [11, 21, 30] and k1[0, 0, 2] == 2
    assert k1[0, 0, 3] == 0 and c1[0, 0, 3].tolist() == [128, 128, 128]
    assert k1[0, 0, 0] == 1 and k1[1, 1, 1] == 1 and c1[0, 0, 0].tolist() == [10, 20, 31]
    assert k1[5, 5, 5] == 0 and k1.astype(bool).sum() == 4
    c2, k2 = CR.fill_pass(c1, k1, occ)
    assert k2[0, 0, 3] == 2 and c2[0, 0, 3].tolist() == [11, 21, 30]                  # from (0,0,2) alone: 2 counts like 1
    assert np.array_equal(c2[0, 0, :3], c1[0, 0, :3]) and k2[5, 5, 5] == 0
    both, kb = CR.colours_of(np.zeros((1, S, S, S, 4), np.int32), occ[None], fill=3)
    assert not kb.any() and (both == 128).all()                                        # nothing known: nothing spreads


def test_from_hits_by_hand():
    S = 32
    col = np.zeros((2, S, S, S, 3), np.uint8)
    col[0].reshape(-1, 3)[5] = (1, 2, 3)
    col[1].reshape(-1, 3)[5] = (4, 5, 6)
    hit = np.array([[[5, -1, S ** 3, INT_MIN]], [[INT_MAX, 5, 5, 0]]], np.int64)
    out = CR.from_hits(hit, col, S, background=(9, 9, 9))
    assert out[0, 0].tolist() == [[1, 2, 3], [9, 9, 9], [9, 9, 9], [9, 9, 9]]
    assert out[1, 0].tolist() == [[9, 9, 9], [4, 5, 6], [4, 5, 6], [0, 0, 0]]
    soft = CR.from_hits(hit, col, S, smooth=1, background=(9, 9, 9))
    # item 1: hits at columns 1..3 with reds 4, 4, 0: column 2 averages all three, (2 * 8 + 3) // 6 = 3; misses keep the background
    assert soft[1, 0, 2].tolist() == [3, 3, 4] and soft[1, 0, 0].tolist() == [9, 9, 9] and soft[0, 0, 0].tolist() == [1, 2, 3]


def test_vertex_colours_by_hand():
    S = 32
    col = np.zeros((2, S, S, S, 3), np.uint8)
    known = np.zeros((2, S, S, S), np.uint8)
    col[1, 3, 4, 5], known[1, 3, 4, 5] = (100, 0, 255), 1
    col[1, 4, 4, 5], known[1, 4, 4, 5] = (101, 1, 254), 2
    col[1, 4, 5, 6] = (77, 77, 77)                                 # not known: does not count
    q = np.array([[0, 0, 0],                                       # grid 0, cell (0,0,0): one corner sample inside the grid, unknown
                  [4 * 256, 5 * 256, 6 * 256],                     # grid 1, blocky, cell (4,5,6): samples 3..4, 4..5, 5..6
                  [4 * 256 - 127, 5 * 256 + 127, 6 * 256 - 1],     # grid 1, smooth, the same cell
                  [S * 256, S * 256, S * 256]], np.int32)          # grid 1, cell (S,S,S): sample (31,31,31) only
    vo = np.array([0, 1, 4], np.int64)
    assert CR.vertex_cells(q).tolist() == [[0, 0, 0], [4, 5, 6], [4, 5, 6], [S, S, S]]
    out = CR.vertex_colours(q, vo, col, known, unseen=(1, 2, 3))
    assert out[0].tolist() == [1, 2, 3] and out[3].tolist() == [1, 2, 3]
    assert out[1].tolist() == [101, 1, 255] and out[2].tolist() == [101, 1, 255]     # 100.5 -> 101, 0.5 -> 1, 254.5 -> 255


# ---- the exact-recovery identity, on the twins alone ------------------------------------------------------------------------------

S32, N64, F2, K6 = 32, 64, 2, 6


def scan_twin(occ):
    """(hits int32 [K,ph,pw], pictures uint8 [K,ph,pw,3], waves, code_q, base) of the K6 scan poses, by the twin casters."""
    poses, low = synth.scan_poses(K6)
    _, M = VC.cameras(poses, low, S32, N64, F2)
    hits = np.stack([RR.cast(occ, M[k], N64, F2, view_from_low_x=low[k])[0] for k in range(K6)])
    cm = synth.ColourModel(3, 8)
    code_q = cm.quantise(np.random.default_rng(3).standard_normal((1, 8)))
    pictures = AR.albedo(hits, cm.waves, np.repeat(code_q, K6, 0), S32, cm.base)
    return hits, pictures, cm.waves, code_q, cm.base


def test_unsmoothed_albedo_views_give_the_field_back():
    occ = XR.sphere_field(S32) > np.float32(0.5)
    hits, pictures, waves, code_q, base = scan_twin(occ)
    sums = CR.accumulate(pictures[None], hits[None], S32)
    col, known = CR.resolve(sums)
    field = AR.albedo(np.arange(S32 ** 3).reshape(1, S32, S32 * S32), waves, code_q, S32, base).reshape(S32, S32, S32, 3)
    seen = known[0] == 1
    print("the twin sees %d voxels of the sphere (%d surface voxels)" % (seen.sum(), CR.surface_voxels(occ).sum()))
    assert seen.sum() > 1000 and not (seen & ~CR.surface_voxels(occ)).any()           # a ray stops at a surface voxel
    assert np.array_equal(col[0][seen], field[seen])
    assert (col[0][~seen] == 128).all()
    # and the coloured grid re-rendered on the same hits is the input, pixel for pixel
    again = CR.from_hits(hits, np.repeat(col, K6, 0), S32)
    assert np.array_equal(again, pictures)
    # the fill reaches what the six views missed, and leaves what they saw
    fc, fk = CR.colours_of(sums, occ[None], fill=3)
    assert np.array_equal(fc[0][seen], col[0][seen]) and (fk[0][seen] == 1).all()
    assert ((fk[0] == 2) & occ).sum() > 0 and not (fk[0].astype(bool) & ~occ).any()


# ---- coloured mesh files ---------------------------------------------------------------------------------------------------------

def coloured_mesh():
    q, faces = XR.extract(XR.sphere_field(32), 0.5, smooth=True)
    rng = np.random.default_rng(8)
    colours = rng.integers(0, 256, (len(q), 3)).astype(np.uint8)
    colours[:4] = [(0, 0, 0), (255, 255, 255), (1, 127, 128), (254, 2, 129)]
    return q, faces, colours


@pytest.mark.parametrize("ext", [".ply", ".obj"])
@pytest.mark.parametrize("axes", ["x,y,z", "z,-y,x"])
def test_coloured_files_there_and_back(tmp_path, ext, axes):
    q, faces, colours = coloured_mesh()
    plain, tinted = str(tmp_path / ("plain" + ext)), str(tmp_path / ("tinted" + ext))
    mesh.save_mesh(plain, q, faces, axes=axes)
    mesh.save_mesh(tinted, q, faces, axes=axes, colours=colours)
    assert mesh.load_mesh_colours(plain) is None
    back = mesh.load_mesh_colours(tinted)
    assert back.dtype == np.uint8 and np.array_equal(back, colours)
    v0, t0 = mesh.load_mesh(plain)
    v1, t1 = mesh.load_mesh(tinted)
    assert np.array_equal(v0, v1) and np.array_equal(t0, t1) and len(v1) == len(q) and len(t1) == 2 * len(faces)
    # colours=None is the call of old
    again = str(tmp_path / ("again" + ext))
    mesh.save_mesh(again, q, faces, axes, None)
    assert open(again, "rb").read() == open(plain, "rb").read()


def test_uncoloured_files_keep_their_bytes(tmp_path):
    q = np.array([[0, 256, 384], [256, 256, 1], [256, 0, 8191], [0, 0, 640]], np.int32)
    faces = np.array([[0, 1, 2, 3]], np.int32)
    obj, ply = str(tmp_path / "a.obj"), str(tmp_path / "a.ply")
    mesh.save_mesh(obj, q, faces)
    mesh.save_mesh(ply, q, faces)
    assert open(obj).read() == ("# 4 vertices, 1 faces, voxel units\nv 0 1 1.5\nv 1 1 0.00390625\nv 1 0 31.99609375\nv 0 0 2.5\n"
                                "f 1 2 3 4\n")
    assert open(ply).read() == ("ply\nformat ascii 1.0\ncomment voxel units\nelement vertex 4\nproperty float x\nproperty float y\n"
                                "property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                                "0 1 1.5\n1 1 0.00390625\n1 0 31.99609375\n0 0 2.5\n4 0 1 2 3\n")
    cols = np.array([[0, 128, 255], [1, 2, 3], [255, 255, 255], [51, 102, 204]], np.uint8)
    mesh.save_mesh(obj, q, faces, colours=cols)
    mesh.save_mesh(ply, q, faces, colours=cols)
    assert open(obj).read().splitlines()[1] == "v 0 1 1.5 0.000000 0.501961 1.000000"
    assert open(obj).read().splitlines()[4] == "v 0 0 2.5 0.200000 0.400000 0.800000"
    lines = open(ply).read().splitlines()
    assert lines[7:10] == ["property uchar red", "property uchar green", "property uchar blue"] and lines[13] == "0 1 1.5 0 128 255"
    with pytest.raises(ValueError, match="colours"):
        mesh.save_mesh(obj, q, faces, colours=cols[:3])
    with pytest.raises(ValueError, match="colours"):
        mesh.save_mesh(obj, q, faces, colours=cols.astype(np.float32))


def test_binary_ply_colours(tmp_path):
    import struct
    path = str(tmp_path / "b.ply")
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\n"
            "property list uchar int vertex_indices\nend_header\n")
    body = b"".join(struct.pack("<fffBBB", *v) for v in ((0, 0, 0, 1, 2, 3), (1, 0, 0, 4, 5, 6), (0, 1, 0, 255, 0, 7)))
    with open(path, "wb") as f:
        f.write(head.encode() + body + struct.pack("<Biii", 3, 0, 1, 2))
    v, t = mesh.load_mesh(path)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and t.tolist() == [[0, 1, 2]]
    assert mesh.load_mesh_colours(path).tolist() == [[1, 2, 3], [4, 5, 6], [255, 0, 7]]


# ---- the cell of a vertex -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("case", ["sphere", "binary_u8", "grid_corners", "full"])
def test_vertex_cell_formula(case, smooth):
    """(q + 128) >> 8 names each vertex's own cell: the cells found are distinct, in cell order, and exactly those whose 2^3
    corner samples cell - 1 + {0, 1} hold both an inside and an outside sample, the outside of the grid being outside."""
    vol, thr = XR.cases32()[case]
    S = 32
    q, _ = XR.extract(vol, thr, smooth=smooth)
    cell = CR.vertex_cells(q)
    assert cell.min() >= 0 and cell.max() <= S
    inside = np.zeros((S + 2,) * 3, bool)
    inside[1:-1, 1:-1, 1:-1] = np.asarray(vol).astype(np.float32) > np.float32(thr)
    count = sum(inside[i:i + S + 1, j:j + S + 1, k:k + S + 1].astype(int) for i in (0, 1) for j in (0, 1) for k in (0, 1))
    active = np.argwhere((count > 0) & (count < 8))                # cell m has corner samples m - 1, m: padded index m, m + 1
    assert np.array_equal(cell, active)
    if not smooth:
        assert np.array_equal(q, 256 * cell)
    else:
        inner = ((q > 0) & (q < 256 * S)).all(1)                   # the others were clamped to the grid's faces
        off = q - (256 * cell - 128)
        assert ((off[inner] >= 1) & (off[inner] <= 255)).all()


# ---- the tool's arguments ---------------------------------------------------------------------------------------------------------

def test_tool_arguments():
    from rendernet_amd.tools import colour_voxels as CT
    a = CT.parse_args(["chair.binvox", "shots", "out.ply"])
    assert (a.model, a.images_dir, a.output) == ("chair.binvox", "shots", "out.ply")
    assert (a.size, a.background, a.threshold, a.fill, a.blocky, a.axes, a.save_colours) == (64, "black", 8.0, 0, False, "x,y,z", None)
    a = CT.parse_args(["m.obj", "shots", "out.obj", "--size", "32", "--background", "white", "--threshold", "3", "--fill", "4",
                       "--blocky", "--axes", "z,y,x", "--save-colours", "c.npz"])
    assert (a.size, a.background, a.threshold, a.fill, a.blocky, a.axes, a.save_colours) == (32, "white", 3.0, 4, True, "z,y,x", "c.npz")
    a = CT.parse_args(["--from-voxels", "chair.binvox", "--views", "6", "--seed", "9", "--size", "32", "back.ply"])
    assert (a.model, a.images_dir, a.output, a.views, a.seed) == ("chair.binvox", None, "back.ply", 6, 9)
    for bad in (["chair.binvox", "out.ply"], ["--from-voxels", "a.binvox", "shots", "out.ply"], ["a.binvox", "shots", "out.binvox"],
                ["a.txt", "shots", "out.ply"], ["a.binvox", "shots", "out.ply", "--size", "48"],
                ["a.binvox", "shots", "out.ply", "--fill", "65"], ["a.binvox", "shots", "out.ply", "--fill", "-1"],
                ["--from-voxels", "a.binvox", "--views", "0", "out.ply"], ["--from-voxels", "a.binvox", "--views", "256", "out.ply"],
                ["a.binvox", "shots", "out.ply", "--save-colours", "c.npy"], ["a.binvox", "shots", "out.ply", "--background", "red"]):
        with pytest.raises(SystemExit):
            CT.parse_args(bad)


def test_surface_voxels():
    from rendernet_amd.tools import colour_voxels as CT
    occ = np.zeros((32,) * 3, bool)
    occ[0:3, 0:3, 0:3] = True                                      # in the corner: only (1,1,1) has six occupied neighbours
    occ[10:15, 10:15, 10:15] = True
    for fn in (CT.surface_voxels, CR.surface_voxels):
        s = fn(occ)
        assert s.sum() == 26 + (125 - 27) and not s[1, 1, 1] and s[0, 0, 0] and not s[12, 12, 12] and not (s & ~occ).any()
