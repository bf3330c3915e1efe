"""rn_mesh_voxelize on the device against its NumPy twin (tests/mesh_voxel_ref.py): every voxel and every mask word, exactly, in
the three modes; the small and the large path, forced either way; determinism; the argument checks.  -m gpu."""
import ctypes

import numpy as np
import pytest

import mesh_voxel_ref as R

pytestmark = pytest.mark.gpu
MODES = (("solid", R.SOLID), ("surface", R.SURFACE), ("both", R.BOTH))


def _icosphere(n, S, radius):
    v, t = R.icosphere(n)
    return R.to_lattice(v @ R.rotation(0.3, 0.5).T, S, radius), t


def _outside(S):
    q, t = R.cube(1344, 5320)
    return ((q.astype(np.int64) - 3332) * 3 + 3332 + 1700).astype(np.int32), t


CASES = {"cube32": (32, lambda: R.cube(1344, 5320)),
         "cube64": (64, lambda: R.cube(300, 256 * 64 - 300)),
         "cube128": (128, lambda: R.cube(300, 256 * 128 - 300)),
         "octahedron": (32, lambda: R.octahedron(4224, 2560)),
         "icosphere2": (32, lambda: _icosphere(2, 32, 11.3)),
         "icosphere3": (64, lambda: _icosphere(3, 64, 25.0)),
         "torus": (32, lambda: R.torus(32, 9, 3.5)),
         "plate": (32, lambda: R.plate(32)),
         "outside": (32, lambda: _outside(32)),
         "empty": (32, lambda: (np.zeros((3, 3), np.int32), np.zeros((0, 3), np.int32)))}


@pytest.fixture(scope="module")
def meshes():
    """name -> (S, q, tris, {mode: twin grid uint8 [1,S,S,S,1]}), computed once."""
    out = {}
    for name, (S, make) in CASES.items():
        q, t = make()
        solid, surf = R.solid(q, t, S), R.surface(q, t, S)
        grids = {"solid": solid, "surface": surf, "both": solid | surf}
        out[name] = (S, q, t, {m: g.astype(np.uint8)[None, ..., None] for m, g in grids.items()})
    return out


def _device(q, t, S, mode, **kw):
    import torch
    from rendernet_amd import ops
    vox, bits = ops.voxelize_mesh(torch.as_tensor(np.ascontiguousarray(q, np.int32)).cuda(),
                                  torch.as_tensor(np.ascontiguousarray(t, np.int32)).cuda(), S=S, mode=mode, return_bits=True, **kw)
    assert vox.dtype is torch.uint8 and tuple(vox.shape) == (1, S, S, S, 1) and vox.is_cuda
    assert bits.dtype is torch.int32 and tuple(bits.shape) == (1, S ** 3 // 32)
    return vox, bits


def _same(got_vox, got_bits, want, what):
    vox, bits = got_vox.cpu().numpy(), got_bits.cpu().numpy()
    diff = int((vox != want).sum())
    print("%s: %d of %d voxels differ, %d set" % (what, diff, want.size, int(want.sum())))
    assert diff == 0
    assert np.array_equal(bits, R.pack(want)), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_twin_in_every_mode(meshes, name):
    from rendernet_amd import mesh
    S, q, t, want = meshes[name]
    d = mesh.prepare(q, t, S)
    print("%s: T %d, solid small/large %d/%d, surface small/large %d/%d" % (name, len(t), len(d["small_solid"]), len(d["large_solid"]),
                                                                         len(d["small_surf"]), len(d["large_surf"])))
    if name.startswith("cube"):
        assert len(d["large_solid"]) == 4 and len(d["large_surf"]) == 12 and not len(d["small_surf"])      # the large path
    if name == "icosphere3":
        assert len(d["small_surf"]) > 1000 and len(d["small_solid"]) > 1000 and len(d["large_solid"]) == 0  # the small path
    for mode, _ in MODES:
        _same(*_device(q, t, S, mode), want[mode], "%s %s" % (name, mode))
    if name == "plate":
        assert not want["solid"].any() and want["surface"].any()
    if name == "empty":
        assert not want["both"].any()


@pytest.mark.parametrize("name", ["icosphere2", "torus", "octahedron"])
def test_any_split_of_the_lists_gives_the_same_grid(meshes, name):
    S, q, t, want = meshes[name]
    every, none = np.arange(len(t), dtype=np.int32), np.zeros(0, np.int32)
    small = {"small_solid": every, "large_solid": none, "small_surf": every, "large_surf": none}
    large = {"small_solid": none, "large_solid": every, "small_surf": none, "large_surf": every}
    mixed = {"small_solid": every[::2], "large_solid": every[1::2], "small_surf": every[1::2], "large_surf": every[::2]}
    for what, lists in (("all small", small), ("all large", large), ("alternating", mixed)):
        _same(*_device(q, t, S, "both", lists=lists), want["both"], "%s %s" % (name, what))


def test_prepared_dict_two_calls_and_the_packer(meshes):
    import torch
    from rendernet_amd import mesh, ops
    S, q, t, want = meshes["icosphere3"]
    d = mesh.prepare(q, t, S)
    a_vox, a_bits = ops.voxelize_mesh(d, S=S, return_bits=True)
    b_vox, b_bits = ops.voxelize_mesh(d, S=S, return_bits=True)
    assert torch.equal(a_vox, b_vox) and torch.equal(a_bits, b_bits)
    _same(a_vox, a_bits, want["both"], "prepared dict")
    assert torch.equal(a_bits, ops.voxel_pack(a_vox)[0])
    only = ops.voxelize_mesh(d, S=S)
    assert torch.is_tensor(only) and torch.equal(only, a_vox)
    S, q, t, want = meshes["cube128"]
    vox, bits = _device(q, t, S, "both")
    assert torch.equal(bits, ops.voxel_pack(vox)[0])


def test_ops_refuses_bad_arguments(meshes):
    import torch
    from rendernet_amd import mesh, ops
    from rendernet_amd._lib import RenderNetHipError
    S, q, t, _ = meshes["cube32"]
    q, t = torch.as_tensor(q).cuda(), torch.as_tensor(t).cuda()
    bad_t = t.clone()
    bad_t[3, 1] = 8
    neg_t = t.clone()
    neg_t[0, 0] = -1
    every = np.arange(12, dtype=np.int32)
    for args, kw in (((q.long(), t), {}), ((q, t.long()), {}), ((q.float(), t), {}), ((q[:, :2], t), {}), ((q, t[:, :2]), {}),
                     ((q.reshape(-1), t), {}), ((q, bad_t), {}), ((q, neg_t), {}), ((q.cpu(), t.cpu()), {}),
                     ((q.cpu().numpy(), t), {}), ((q, t), {"S": 48}), ((q, t), {"S": 16}), ((q, t), {"S": 64.0}),
                     ((q, t), {"mode": "thick"}), ((q, t), {"mode": 3}),
                     ((q, t), {"lists": {"small_solid": every + 1}}), ((mesh.prepare(q.cpu().numpy(), t.cpu().numpy(), 32),), {"S": 64})):
        with pytest.raises(RenderNetHipError):
            ops.voxelize_mesh(*args, **kw)


def test_the_c_entry_refuses_before_it_launches(meshes):
    """RN_E_INVALID, and output buffers filled with 0xAA keep every byte, for each bad argument."""
    import torch
    from rendernet_amd import _lib
    L = _lib.lib()
    S, q, t, want = meshes["cube32"]
    q, t = torch.as_tensor(q).cuda(), torch.as_tensor(t).cuda()
    lst = torch.arange(16, dtype=torch.int32, device="cuda")
    words = S ** 3 // 32
    ws = torch.full((2 * words + 4,), 0x55, dtype=torch.int32, device="cuda")
    bits = torch.full((words + 4,), 0x55, dtype=torch.int32, device="cuda")
    vox = torch.full((S ** 3 + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    vp, st = ctypes.c_void_p, _lib.stream_ptr()
    P = lambda x, off=0: vp(x.data_ptr() + off)
    assert all(x.data_ptr() % 16 == 0 for x in (ws, bits, vox, lst))

    def call(verts=P(q), V=8, tris=P(t), T=12, ss=P(lst), n_ss=12, ls=P(lst), n_ls=12, sf=P(lst), n_sf=12, lf=P(lst), n_lf=12,
             w=P(ws), b=P(bits), v=P(vox), size=S, mode=3):
        return L.rn_mesh_voxelize(verts, V, tris, T, ss, n_ss, ls, n_ls, sf, n_sf, lf, n_lf, w, b, v, size, mode, st)
    cases = {"S = 48": dict(size=48), "S = 256": dict(size=256), "mode 0": dict(mode=0), "mode 4": dict(mode=4), "V = -1": dict(V=-1),
             "T = -1": dict(T=-1), "T without V": dict(V=0), "negative list": dict(n_sf=-1), "lists without T": dict(T=0),
             "null verts": dict(verts=None), "null tris": dict(tris=None), "null list": dict(ls=None), "null ws": dict(w=None),
             "null bits": dict(b=None), "null vox": dict(v=None), "misaligned ws": dict(w=P(ws, 4)),
             "misaligned bits": dict(b=P(bits, 4)), "misaligned vox": dict(v=P(vox, 4))}
    for what, kw in cases.items():
        assert call(**kw) == -1, what                                            # RN_E_INVALID
        assert b"rn_mesh_voxelize" in L.rn_last_error(), what
    torch.cuda.synchronize()
    assert bool((vox == 0xAA).all()) and bool((bits == 0x55).all()) and bool((ws == 0x55).all())
    assert call() == 0                                                           # every triangle in all four lists: small and large
    torch.cuda.synchronize()                                                     # twice over is the empty solid and the same surface
    assert np.array_equal(vox[:S ** 3].cpu().numpy().reshape(want["surface"].shape), want["surface"])
    assert bool((vox[S ** 3:] == 0xAA).all()) and bool((bits[words:] == 0x55).all()) and bool((ws[2 * words:] == 0x55).all())
    assert call(verts=None, V=0, tris=None, T=0, ss=None, n_ss=0, ls=None, n_ls=0, sf=None, n_sf=0, lf=None, n_lf=0) == 0
    torch.cuda.synchronize()
    assert not bool(vox[:S ** 3].any()) and not bool(bits[:words].any())
