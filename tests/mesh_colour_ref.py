"""NumPy twin of rn_mesh_colour_from_ids / rn_mesh_face_voxels (include/rendernet_hip.h states the two rules): the colour picture
of ONE triangle mesh on given triangle ids, and the voxel behind every face of ONE grid's surface net.  TEST INFRASTRUCTURE
ONLY.  int64 throughout; built on tests/mesh_raster_ref.py (the projection, the lattice normals) and tests/mesh_extract_ref.py
(the nets the tests feed it)."""
import numpy as np

import mesh_raster_ref as MR

U = MR.U


def colour_from_ids(q, tris, cam, tri_id, S, window, vertex_colours=None, face_colours=None, background=(0, 0, 0)):
    """One mesh, one item.  q int [V,3], tris int [T,3], cam int64 [3,4], tri_id int [ph,pw], window (row0, col0, ph, pw) and
    exactly one of vertex_colours uint8 [V,3], face_colours uint8 [T,3] -> uint8 [ph,pw,3]."""
    assert (vertex_colours is None) != (face_colours is None)
    row0, col0, ph, pw = (int(v) for v in window)
    tri_id = np.asarray(tri_id, np.int64).reshape(ph, pw)
    out = np.empty((ph, pw, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    qc = np.clip(np.asarray(q, np.int64).reshape(-1, 3), 0, U * S)
    tc = np.asarray(tris, np.int64).reshape(-1, 3)
    V, T = len(qc), len(tc)
    ok = (tri_id >= 0) & (tri_id < T) & (V > 0)
    if not ok.any():
        return out
    tc = np.clip(tc, 0, V - 1)                                   # a stray index stays inside its mesh
    pr, pc = np.nonzero(ok)
    t = tri_id[pr, pc]
    if face_colours is not None:
        out[pr, pc] = np.asarray(face_colours, np.uint8).reshape(T, 3)[t]
        return out
    P = MR.project(cam, qc, S)[tc[t]]                            # [n,3 vertices,(X, Y, Z)]
    A = (P[:, 1, 0] - P[:, 0, 0]) * (P[:, 2, 1] - P[:, 0, 1]) - (P[:, 1, 1] - P[:, 0, 1]) * (P[:, 2, 0] - P[:, 0, 0])
    p = qc[tc[t]]
    no_normal = (np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1]) == 0).all(1)
    mean_rule = (A == 0) | no_normal
    order = np.where((A < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))          # wound to A > 0
    W = np.take_along_axis(P, order[:, :, None], 1)
    vid = np.take_along_axis(tc[t], order, 1)                    # the vertex at wound position k
    X, Y = W[..., 0], W[..., 1]
    cu, cv = U * (pc + col0) + 128, U * (pr + row0) + 128
    E = []
    for k in range(3):
        n = (k + 1) % 3
        E.append((X[:, n] - X[:, k]) * (cv - Y[:, k]) - (Y[:, n] - Y[:, k]) * (cu - X[:, k]))
    w = np.stack([E[1], E[2], E[0]], 1)                          # position k carries E_(k+1)
    col = np.asarray(vertex_colours, np.uint8).reshape(V, 3)[vid].astype(np.int64)       # [n,3 positions,3 channels]
    num = (w[:, :, None] * col).sum(1)
    Aw = np.where(mean_rule, 1, np.abs(A))[:, None]
    byte = np.clip((2 * num + Aw) // (2 * Aw), 0, 255)           # floor division
    mean = (2 * col.sum(1) + 3) // 6
    out[pr, pc] = np.where(mean_rule[:, None], mean, byte).astype(np.uint8)
    return out


def face_voxels(q, faces, vol, threshold=0.5):
    """One grid.  q int [V,3], faces int [F,3] or [F,4] (indices into q), vol [S,S,S] float32 or uint8 -> int32 [F]: the flat id
    of the solid voxel each face bounds, or -1."""
    vol = np.asarray(vol)
    S = vol.shape[0]
    assert vol.shape == (S, S, S)
    inside = vol.astype(np.float32) > np.float32(threshold)
    q = np.asarray(q, np.int64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64)
    F, V = len(faces), len(q)
    if F == 0 or V == 0:
        return np.full((F,), -1, np.int32)
    c = ((q[np.clip(faces[:, :3], 0, V - 1)] + 128) >> 8) - 1    # [F,3 vertices,3 axes]
    d1, d2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    ring = (((d1 == 0) | (d1 == 1)) & ((d2 == 0) | (d2 == 1))).all(1)
    both = (d1 == 0) & (d2 == 0)
    ok = ring & (both.sum(1) == 1)
    a = np.argmax(both, 1)
    rows = np.arange(F)
    s = c[:, 0] + 1
    s[rows, a] -= 1                                              # (c_a, c_u + 1, c_v + 1)
    for k in (1, 2):
        x = s[rows, (a + k) % 3]
        ok &= (x >= 0) & (x <= S - 1)
    e = s.copy()
    e[rows, a] += 1

    def sample(x):                                               # a sample outside the grid is outside
        real = ((x >= 0) & (x < S)).all(1)
        xc = np.clip(x, 0, S - 1)
        return real & inside[xc[:, 0], xc[:, 1], xc[:, 2]]
    lo, hi = sample(s), sample(e)
    end = np.where(hi[:, None], e, s)
    flat = (end[:, 0] * S + end[:, 1]) * S + end[:, 2]
    return np.where(ok & (lo != hi), flat, -1).astype(np.int32)


def face_voxels_batch(q, faces, vert_offsets, face_offsets, vol, threshold=0.5):
    """The batch form, what ops.mesh_face_voxels returns: vol [B,S,S,S] or [B,S,S,S,1]."""
    vol = np.asarray(vol)
    if vol.ndim == 5:
        vol = vol[..., 0]
    out = [np.zeros((0,), np.int32)]
    for b, g in enumerate(vol):
        out.append(face_voxels(q[vert_offsets[b]:vert_offsets[b + 1]], faces[face_offsets[b]:face_offsets[b + 1]], g, threshold))
    return np.concatenate(out)
