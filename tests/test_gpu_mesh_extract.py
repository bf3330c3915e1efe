"""rn_mesh_extract_count / _emit on the device against the NumPy twin (tests/mesh_extract_ref.py): vertices, faces and both
offset arrays exactly, order included; batches, the scan over many workgroup totals, the round trip through the device
voxeliser at 32, 64 and 128 and through a .ply file, determinism, the argument checks, the two command lines and the
reconstruction script's "save_mesh" key.  -m gpu."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_extract_ref as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES32 = E.cases32()


def _as_u8(vol, thr):
    """The same field in bytes: 200 steps per unit, so the values on the threshold 0.5 stay exactly on the threshold 100."""
    if vol.dtype == np.uint8:
        return vol.astype(np.float32), thr                       # the binary case: the other dtype is float32
    return np.clip(np.rint(vol.astype(np.float64) * 200.0), 0, 255).astype(np.uint8), 200.0 * thr


def _device(vol):
    import torch
    return torch.as_tensor(np.ascontiguousarray(vol)).cuda()


def _same(m, want, what):
    q, f, vo, fo = want
    got = (m.q.cpu().numpy(), m.faces.cpu().numpy(), m.vert_offsets.cpu().numpy(), m.face_offsets.cpu().numpy())
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int64 and got[3].dtype == np.int64
    assert got[0].shape == q.shape and got[1].shape == f.shape, (what, got[0].shape, q.shape, got[1].shape, f.shape)
    for g, w, name in zip(got, (q, f, vo, fo), ("q", "faces", "vert_offsets", "face_offsets")):
        assert np.array_equal(g, w), (what, name, int((g != w).sum()))


@pytest.fixture(scope="module")
def sphere128():
    vol = E.sphere_field(128)
    return vol, E.extract_batch(vol[None], 0.5, True)


@pytest.fixture(scope="module")
def csg64():
    """One 64^3 procedural CSG grid (uint8 [1,64,64,64,1] on the device) and its twin mesh."""
    import torch
    from rendernet_amd import ops, synth
    vox = ops.voxel_shapes(torch.as_tensor(synth.shape_prims(1234, [0x1a2b3c4d], 64)).cuda(), 64)
    return vox, E.extract_batch(vox.cpu().numpy(), 0.5, True)


@pytest.mark.parametrize("name", sorted(CASES32))
def test_device_equals_twin_at_32(name):
    """33^3 cells are no multiple of 256: the last workgroup of every grid is ragged."""
    from rendernet_amd import ops
    vol, thr = CASES32[name]
    for v, t in ((vol, thr), _as_u8(vol, thr)):
        for smooth in (True, False):
            want = E.extract_batch(v[None], t, smooth)
            _same(ops.extract_mesh(_device(v[None, ..., None]), threshold=t, smooth=smooth), want, (name, v.dtype, smooth))
    want = E.extract_batch(vol[None], thr, True, triangles=True)
    _same(ops.extract_mesh(_device(vol[None]), threshold=thr, triangles=True), want, (name, "triangles"))


def test_device_equals_twin_on_a_csg_grid_at_64(csg64):
    from rendernet_amd import ops
    vox, want = csg64
    assert len(want[0]) > 1000
    _same(ops.extract_mesh(vox), want, "csg64")
    _same(ops.extract_mesh(vox, smooth=False), E.extract_batch(vox.cpu().numpy(), 0.5, False), "csg64 blocky")


def test_device_equals_twin_on_a_sphere_at_128(sphere128):
    """129^3 > 2^21 cells and a scan over 8386 workgroup totals, 33 rounds of the scan loop."""
    from rendernet_amd import ops
    vol, want = sphere128
    _same(ops.extract_mesh(_device(vol[None])), want, "sphere128")


def test_batch_with_an_empty_grid_in_the_middle():
    from rendernet_amd import ops
    vols = np.stack([CASES32["sphere"][0], np.zeros((32, 32, 32), np.float32), CASES32["uniform_noise"][0]])
    for triangles in (False, True):
        m = ops.extract_mesh(_device(vols), triangles=triangles)
        _same(m, E.extract_batch(vols, 0.5, True, triangles), ("batch", triangles))
        vo, fo = m.vert_offsets.tolist(), m.face_offsets.tolist()
        assert vo[1] == vo[2] and fo[1] == fo[2] and vo[0] == fo[0] == 0
        for b in range(3):                                       # offsets and local indices: three single calls
            one = ops.extract_mesh(_device(vols[b:b + 1]), triangles=triangles)
            q, f = m.grid(b)
            assert np.array_equal(q.cpu().numpy(), one.q.cpu().numpy()) and np.array_equal(f.cpu().numpy(), one.faces.cpu().numpy())
    empty = ops.extract_mesh(_device(vols[1:2]))
    assert tuple(empty.q.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 4) and empty.vert_offsets.tolist() == [0, 0]
    none = ops.extract_mesh(_device(vols[:0]), triangles=True)
    assert tuple(none.q.shape) == (0, 3) and tuple(none.faces.shape) == (0, 3) and none.face_offsets.tolist() == [0]


@pytest.mark.parametrize("S", [64, 128])
def test_scan_over_empty_workgroups(S):
    """Active cells only at the two ends of the cell order, around voxels [0,0,0] and [S-1,S-1,S-1].  (The eight cells of one voxel
    lie up to N^2 + N + 1 cells apart, so they cannot all fall into one workgroup of 256: the first and the last few workgroups
    hold them, with more than a thousand empty ones and, at 128, 32 empty scan rounds between.)"""
    from rendernet_amd import ops
    vol = np.zeros((S, S, S), np.float32)
    vol[0, 0, 0] = vol[S - 1, S - 1, S - 1] = 0.9
    want = E.extract_batch(vol[None], 0.5, True)
    assert len(want[0]) == 16 and len(want[1]) == 12
    _same(ops.extract_mesh(_device(vol[None])), want, S)


def _round_trip(vol, thr, S, smooth):
    import torch
    from rendernet_amd import ops
    dev = _device(vol.reshape(1, S, S, S, 1))
    m = ops.extract_mesh(dev, threshold=thr, smooth=smooth, triangles=True)
    _, bits = ops.voxelize_mesh(m.q, m.faces, S=S, mode="solid", return_bits=True)
    want, _ = ops.voxel_pack(dev, thr)
    assert int(want.ne(0).sum()) > 0
    assert torch.equal(bits, want), int((bits != want).sum())


@pytest.mark.parametrize("smooth", [True, False], ids=["smooth", "blocky"])
def test_device_round_trip_at_32_64_128(smooth, sphere128, csg64):
    """extract -> voxelise (solid) returns the bits voxel_pack gives, all on the device (the voxeliser is pinned to its own twin
    by tests/test_gpu_mesh_voxel.py)."""
    for name in ("uniform_noise", "threshold_ties", "full", "edge_contact", "grid_corners"):
        _round_trip(CASES32[name][0], CASES32[name][1], 32, smooth)
    _round_trip(csg64[0].cpu().numpy(), 0.5, 64, smooth)
    _round_trip(sphere128[0], 0.5, 128, smooth)


def test_chair_binvox_round_trip_through_a_ply_file(tmp_path):
    """.binvox -> .ply -> voxelise (solid): the input grid bit for bit."""
    import torch
    from rendernet_amd import mesh, ops
    from rendernet_amd.tools import binvox_rw
    with open(os.path.join(ROOT, "binvox", "chair.binvox"), "rb") as f:
        grid = np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
    path = str(tmp_path / "chair.ply")
    mesh.save_mesh(path, *mesh.extract(grid))
    v, t = mesh.load_mesh(path)
    q = np.rint(v * 256).astype(np.int32)
    assert np.array_equal(q / 256.0, v)
    back = ops.voxelize_mesh(_device(q), _device(t), S=64, mode="solid")
    assert torch.equal(back, _device(grid.reshape(1, 64, 64, 64, 1)))


def test_save_meshes_writes_one_file_per_grid(tmp_path):
    """What the reconstruction script does with its hypotheses: soft volumes at the config's threshold, one .ply each."""
    from rendernet_amd import mesh
    soft = np.stack([E.sphere_field(32) * np.float32(0.2), np.zeros((32, 32, 32), np.float32), CASES32["uniform_noise"][0] * np.float32(0.2)])
    paths = [str(tmp_path / ("h%d.ply" % b)) for b in range(3)]
    mesh.save_meshes(paths, _device(soft[..., None]), threshold=0.1)
    for b, path in enumerate(paths):
        q, faces = E.extract(soft[b], 0.1, True)
        v, t = mesh.load_mesh(path)
        assert np.array_equal(v, q / 256.0) and np.array_equal(t, E.fan(faces)), b
    assert len(mesh.load_mesh(paths[1])[0]) == 0 and len(mesh.load_mesh(paths[2])[0]) > 10000
    with pytest.raises(ValueError):
        mesh.save_meshes(paths[:2], _device(soft))


def test_reconstruct_script_writes_a_ply_beside_each_binvox(tmp_path, capsys):
    """Config key "save_mesh": one step of the five hypotheses; every .ply, voxelised in solid mode, is its .binvox grid."""
    import json
    import torch
    from PIL import Image
    import Reconstruct_RenderNet_Face
    from rendernet_amd import mesh, ops
    from rendernet_amd.tools import binvox_rw
    rng = np.random.default_rng(0)
    for name in ("albedo.png", "normal.png"):
        Image.fromarray((rng.random((512, 512, 3)) * 255).astype(np.uint8)).save(str(tmp_path / name))
    cfg = {"target_albedo": str(tmp_path / "albedo.png"), "target_normal": str(tmp_path / "normal.png"),
           "target_azimuth_light": 294, "target_elevation_light": 105, "weight_dir": str(tmp_path / "nope"),
           "weight_dir_decoder": str(tmp_path / "nope2"), "gpu": 0, "batch_size": 5, "z_dim": 200, "inner_step": 1,
           "max_epochs": 1, "threshold": 0.1, "shape_eta": 0.8, "pose_eta": 0.01, "tex_eta": 0.8, "light_eta": 0.4,
           "sample_save": str(tmp_path / "out"), "save_mesh": True}
    cfgp = str(tmp_path / "config.json")
    json.dump(cfg, open(cfgp, "w"))
    Reconstruct_RenderNet_Face.main([cfgp, "--max-steps", "1"])
    capsys.readouterr()
    files = sorted(os.listdir(cfg["sample_save"]))
    plys = [f for f in files if f.endswith(".ply")]
    assert len(plys) == 5 and [f[:-4] + ".binvox" for f in plys] == [f for f in files if f.endswith(".binvox")]
    for f in plys[:2]:
        v, t = mesh.load_mesh(os.path.join(cfg["sample_save"], f))
        with open(os.path.join(cfg["sample_save"], f[:-4] + ".binvox"), "rb") as fh:
            grid = np.ascontiguousarray(binvox_rw.read_as_3d_array(fh).data)
        assert grid.any() and len(t) > 0
        back = ops.voxelize_mesh(_device(np.rint(v * 256).astype(np.int32)), _device(t), S=64, mode="solid")
        assert torch.equal(back, _device(grid.astype(np.uint8).reshape(1, 64, 64, 64, 1)))


def test_two_calls_give_identical_tensors():
    import torch
    from rendernet_amd import ops
    dev = _device(np.stack([CASES32["uniform_noise"][0], CASES32["threshold_ties"][0]]))
    a, b = ops.extract_mesh(dev), ops.extract_mesh(dev)
    assert a.q.data_ptr() != b.q.data_ptr()
    for name in ("q", "faces", "vert_offsets", "face_offsets"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_argument_checks_through_the_c_abi():
    """Every invalid argument is refused by the validation, with the entry's name in the error; nothing is launched, so the
    outputs keep the pattern they were filled with."""
    import torch
    from rendernet_amd import _lib as L
    lib, vp = L.lib(), ctypes.c_void_p
    S, B = 32, 1
    vol = torch.zeros((B, S, S, S), device="cuda")
    vol[0, 3, 4, 5] = 1.0
    nws = int(lib.rn_mesh_extract_workspace_bytes(B, S))
    ws = torch.full((nws // 4 + 4,), -7, dtype=torch.int32, device="cuda")
    totals = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    off = torch.zeros((B + 1,), dtype=torch.int64, device="cuda")
    cellvert = torch.full((B, (S + 1) ** 3), -7, dtype=torch.int32, device="cuda")
    q = torch.full((8, 3), -7, dtype=torch.int32, device="cuda")
    faces = torch.full((6 + 1, 4), -7, dtype=torch.int32, device="cuda")
    st = L.stream_ptr()
    P = lambda t, byte=0: vp(t.data_ptr() + byte)
    nan = float("nan")

    def count(vol_p=P(vol), u8=0, thr=0.5, b=B, s=S, ws_p=P(ws), n=nws, tot=P(totals)):
        return lib.rn_mesh_extract_count(vol_p, u8, thr, b, s, ws_p, n, tot, st)

    def emit(vol_p=P(vol), u8=0, thr=0.5, b=B, s=S, mode=1, tri=0, ws_p=P(ws), n=nws, vo=P(off), qo=P(off), nv=8, nq=6,
             cv=P(cellvert), q_p=P(q), f_p=P(faces)):
        return lib.rn_mesh_extract_emit(vol_p, u8, thr, b, s, mode, tri, ws_p, n, vo, qo, nv, nq, cv, q_p, f_p, st)
    bad_count = [dict(vol_p=None), dict(ws_p=None), dict(tot=None), dict(s=48), dict(s=0), dict(b=-1), dict(b=65536), dict(thr=nan),
                 dict(u8=2), dict(vol_p=P(vol, 2)), dict(ws_p=P(ws, 8)), dict(tot=P(totals, 2)), dict(n=nws - 16)]
    for kw in bad_count:
        assert count(**kw) != 0, kw
        assert b"rn_mesh_extract_count:" in lib.rn_last_error(), (kw, lib.rn_last_error())
    bad_emit = [dict(vol_p=None), dict(ws_p=None), dict(vo=None), dict(qo=None), dict(cv=None), dict(q_p=None), dict(f_p=None),
                dict(s=96), dict(b=-1), dict(b=65536), dict(thr=nan), dict(u8=-1), dict(mode=2), dict(mode=-1), dict(tri=2),
                dict(nv=-1), dict(nq=-1), dict(vol_p=P(vol, 1)), dict(ws_p=P(ws, 4)), dict(vo=P(off, 4)), dict(qo=P(off, 4)),
                dict(cv=P(cellvert, 2)), dict(q_p=P(q, 2)), dict(f_p=P(faces, 8)), dict(n=0)]
    for kw in bad_emit:
        assert emit(**kw) != 0, kw
        assert b"rn_mesh_extract_emit:" in lib.rn_last_error(), (kw, lib.rn_last_error())
    torch.cuda.synchronize()
    for t in (ws, totals, cellvert, q, faces):
        assert bool((t == -7).all())
    # and the same buffers with valid arguments: the lone voxel
    assert count() == 0 and emit() == 0
    torch.cuda.synchronize()
    assert totals.tolist() == [[8, 6]] and int(q.min()) >= 256 * 3 and int(faces[:6].max()) == 7 and bool((faces[6] == -7).all())


def _child(args):
    return subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_command_lines_write_the_twins_mesh(tmp_path):
    from rendernet_amd import mesh
    from rendernet_amd.tools import binvox_rw
    chair = os.path.join(ROOT, "binvox", "chair.binvox")
    with open(chair, "rb") as f:
        grid = np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
    q, faces = E.extract(grid, 0.5, True)
    out = str(tmp_path / "chair.ply")
    r = _child([os.path.join(ROOT, "RenderNet_demo.py"), "--voxel_path", chair, "--save_mesh", out, "--render_dir", str(tmp_path / "render")])
    assert r.returncode == 0 and out in r.stdout, r.stderr[-2000:]
    v, t = mesh.load_mesh(out)
    assert np.array_equal(v, q / 256.0) and np.array_equal(t, E.fan(faces))
    # the tool: the blocky mesh as OBJ, and the raw .npz volume of the reconstruction script at its own threshold
    obj = str(tmp_path / "chair.obj")
    r = _child(["-m", "rendernet_amd.tools.binvox_to_mesh", chair, obj, "--blocky"])
    assert r.returncode == 0 and obj in r.stdout, r.stderr[-2000:]
    qb, fb = E.extract(grid, 0.5, False)
    v, t = mesh.load_mesh(obj)
    assert np.array_equal(v, qb / 256.0) and np.array_equal(t, E.fan(fb))
    soft = E.sphere_field(32) * np.float32(0.2)
    np.savez(str(tmp_path / "soft_Param.txt"), soft)
    ply = str(tmp_path / "soft.ply")
    r = _child(["-m", "rendernet_amd.tools.binvox_to_mesh", str(tmp_path / "soft_Param.txt.npz"), ply, "--threshold", "0.1", "--axes", "z,y,x"])
    assert r.returncode == 0, r.stderr[-2000:]
    qs, fs = E.extract(soft, 0.1, True)
    v, t = mesh.load_mesh(ply)
    assert len(qs) > 1000 and np.array_equal(v[:, ::-1], qs / 256.0) and np.array_equal(t, E.fan(fs[:, [0, 3, 2, 1]]))
