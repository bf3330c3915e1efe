"""Triangle meshes as occupancy grids: OBJ / PLY reader, the quantisation onto the voxeliser's integer lattice and the work
lists of rn_mesh_voxelize (rendernet_amd/csrc/mesh_voxel.hip; the rules are stated in include/rendernet_hip.h and DESIGN.md
5c "Mesh input").  Everything here is host code on NumPy; `voxelize`, `extract`, `save_meshes` and `MeshSet` reach the device, through `ops`.

    load_mesh(path)                     -> verts float64 [V,3], tris int32 [T,3]
    fit(verts, S, margin, axes)         -> q int32 [V,3], lattice coordinates, 256 units per voxel, column j = array axis j
    prepare(q, tris, S)                 -> dict: the kept triangles and the small / large lists of the two rules
    voxelize(path, S, mode, ...)        -> uint8 [1,S,S,S,1] on the device
    extract(vox, threshold, smooth)     -> q int32 [V,3], faces int32 [F,4] of one grid (ops.extract_mesh), as NumPy arrays;
                                           relax=N relaxes the vertices inside their cells for N passes (rn_mesh_relax)
    save_mesh(path, q, faces, axes)     -> writes .obj or ASCII .ply in voxel units, q / 256; colours=uint8 [V,3] colours the vertices
    load_mesh_colours(path)             -> uint8 [V,3], the vertex colours of such a file, or None
    save_meshes(paths, vol, threshold)  -> one file per grid of a batch on the device, from one ops.extract_mesh call
    axes_sign(axes)                     -> +1 or -1: whether `fit` with these axes keeps or mirrors the mesh's handedness
    MeshSet(meshes, names, S)           -> the fitted meshes of a folder, concatenated on the device with their vertex normals,
                                           ready for ops.rasterize_mesh (MeshSet.from_files reads and fits the files)

Array axes.  The grid is [a0][a1][a2] = [zs][ys][xs] of the resampler and the ray caster (flat index (a0*S + a1)*S + a2), and in
the shipped models array axis 1 is UP, towards higher indices (the chair's legs are at low a1).  `axes` is a signed permutation
of the mesh axes: entry j names the mesh axis that becomes array axis j.  The default "x,y,z" is what `binvox` followed by
`binvox_rw.read_as_3d_array` gives for the same mesh; it stands a y-up mesh upright but mirrors it (mesh x and z change
places).  "z,y,x" stands a y-up OBJ upright without the mirror; "-y,z,x" does the same for a z-up mesh.
"""
import os
import struct

import numpy as np

LATTICE = 256                 # lattice units per voxel
SIZES = (32, 64, 128)
MODES = {"solid": 1, "surface": 2, "both": 3}       # RN_MESH_SOLID, RN_MESH_SURFACE, RN_MESH_BOTH
THRESHOLD = 64                # a triangle with more candidates than this gets a wave to itself (measured)


def _fan(idx):
    return [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]


def _load_obj(path, cols=None):
    """`cols`, a list, receives one (r, g, b) of floats per vertex, or None for a vertex without colours."""
    verts, tris = [], []
    name = os.path.basename(path)
    with open(path, "r", errors="replace") as f:
        for ln, line in enumerate(f, 1):
            rec = line.split()
            if not rec or rec[0] not in ("v", "f"):
                continue
            try:
                if rec[0] == "v":
                    if len(rec) < 4:
                        raise ValueError("a vertex needs x y z")
                    verts.append((float(rec[1]), float(rec[2]), float(rec[3])))
                    if cols is not None:
                        cols.append((float(rec[4]), float(rec[5]), float(rec[6])) if len(rec) >= 7 else None)
                    continue
                if len(rec) < 4:
                    raise ValueError("a face needs at least three vertices")
                idx = []
                for ref in rec[1:]:
                    i = int(ref.split("/")[0])                  # i, i/t, i//n, i/t/n
                    i = i - 1 if i > 0 else len(verts) + i      # negative: relative to the vertices read so far
                    if i < 0 or i >= len(verts):                # also the index 0, which OBJ does not have
                        raise ValueError("vertex index %s outside the %d vertices read so far" % (ref, len(verts)))
                    idx.append(i)
                tris += _fan(idx)
            except ValueError as e:
                raise ValueError("%s line %d: %s" % (name, ln, e))
    return verts, tris


_PLY_TYPES = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h", "ushort": "H", "uint16": "H",
              "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f", "double": "d", "float64": "d"}
_PLY_INTS = "bBhHiI"
_PLY_COLOURS = ("red", "green", "blue")


def _load_ply(path, cols=None):
    """`cols`, a list, receives the vertex properties red, green, blue as an array [V,3] (and whether they are integers), if the
    file has all three."""
    name = os.path.basename(path)
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s header: not a PLY file" % name)
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError("%s header: no line end after end_header" % name)
    fmt, elements = None, []                                     # elements: [name, count, [(prop, type) | (prop, count_t, item_t)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        rec = line.split()
        if not rec or rec[0] in ("comment", "obj_info"):
            continue
        try:
            if rec[0] == "format":
                fmt = rec[1]
                if fmt not in ("ascii", "binary_little_endian") or rec[2] != "1.0":
                    raise ValueError("format %s (ascii and binary_little_endian 1.0 are read)" % " ".join(rec[1:]))
            elif rec[0] == "element":
                elements.append([rec[1], int(rec[2]), []])
            elif rec[0] == "property":
                if not elements:
                    raise ValueError("property before any element")
                if rec[1] == "list":
                    ct, it = _PLY_TYPES[rec[2]], _PLY_TYPES[rec[3]]
                    elements[-1][2].append((rec[4], ct, it))
                else:
                    elements[-1][2].append((rec[2], _PLY_TYPES[rec[1]]))
            else:
                raise ValueError("record %r" % rec[0])
        except (IndexError, KeyError) as e:
            raise ValueError("%s header: cannot read %r (%s)" % (name, line, e))
        except ValueError as e:
            raise ValueError("%s header: %s" % (name, e))
    if fmt is None:
        raise ValueError("%s header: no format line" % name)
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError("%s header: no vertex element" % name)
    vprops = elements[names.index("vertex")][2]
    if any(len(p) == 3 for p in vprops):
        raise ValueError("%s element vertex: list properties are not read" % name)
    for c in "xyz":
        t = dict(vprops).get(c)
        if t is None:
            raise ValueError("%s element vertex: no property %s" % (name, c))
        if t not in "fd":
            raise ValueError("%s element vertex: property %s is neither float nor double" % (name, c))
    if "face" in names:
        fprops = elements[names.index("face")][2]
        lists = [p for p in fprops if len(p) == 3 and p[0] in ("vertex_indices", "vertex_index")]
        if len(lists) != 1:
            raise ValueError("%s element face: no list vertex_indices / vertex_index" % name)
        if lists[0][1] not in _PLY_INTS or lists[0][2] not in _PLY_INTS:
            raise ValueError("%s element face: the vertex list needs integer count and index types" % name)

    verts, tris, ascii_cols = [], [], []
    if fmt == "ascii":
        tokens = data[nl + 1:].split()
        pos = [0]

        def scalar(t, what):
            if pos[0] >= len(tokens):
                raise ValueError("%s element %s: the file ends early" % (name, what))
            tok = tokens[pos[0]]
            pos[0] += 1
            try:
                return int(tok) if t in _PLY_INTS else float(tok)
            except ValueError:
                raise ValueError("%s element %s: cannot read %r" % (name, what, tok.decode("ascii", "replace")))
    else:
        pos = [nl + 1]

        def scalar(t, what):
            n = struct.calcsize("<" + t)
            if pos[0] + n > len(data):
                raise ValueError("%s element %s: the file ends early" % (name, what))
            v = struct.unpack_from("<" + t, data, pos[0])[0]
            pos[0] += n
            return v
    for ename, count, props in elements:
        if ename == "vertex" and fmt != "ascii":                 # fixed-size records: one structured read
            dt = np.dtype([(p[0] + "_%d" % k, "<" + np.dtype(p[1]).str[1:]) for k, p in enumerate(props)])
            if pos[0] + count * dt.itemsize > len(data):
                raise ValueError("%s element vertex: the file ends early" % name)
            rec = np.frombuffer(data, dt, count, pos[0])
            pos[0] += count * dt.itemsize
            col = {p[0]: p[0] + "_%d" % k for k, p in enumerate(props)}
            verts = np.stack([rec[col[c]].astype(np.float64) for c in "xyz"], 1) if count else []
            if cols is not None and all(c in col for c in _PLY_COLOURS):
                cols.append((np.stack([rec[col[c]].astype(np.float64) for c in _PLY_COLOURS], 1).reshape(-1, 3),
                             all(dict(vprops)[c] in _PLY_INTS for c in _PLY_COLOURS)))
            continue
        for _ in range(count):
            row = {}
            for p in props:
                if len(p) == 3:
                    n = scalar(p[1], ename)
                    if n < 0:
                        raise ValueError("%s element %s: list of %d entries" % (name, ename, n))
                    row[p[0]] = [scalar(p[2], ename) for _ in range(n)]
                else:
                    row[p[0]] = scalar(p[1], ename)
            if ename == "vertex":
                verts.append((row["x"], row["y"], row["z"]))
                if cols is not None and all(c in row for c in _PLY_COLOURS):
                    ascii_cols.append(tuple(row[c] for c in _PLY_COLOURS))
            elif ename == "face":
                idx = row.get("vertex_indices", row.get("vertex_index"))
                if len(idx) < 3:
                    raise ValueError("%s element face: a face of %d vertices" % (name, len(idx)))
                tris += _fan(idx)
    nv = len(verts)
    for t in tris:
        if min(t) < 0 or max(t) >= nv:
            raise ValueError("%s element face: vertex index %d outside the %d vertices" % (name, min(t) if min(t) < 0 else max(t), nv))
    if cols is not None and fmt == "ascii" and all(c in dict(vprops) for c in _PLY_COLOURS):
        cols.append((np.asarray(ascii_cols, np.float64).reshape(-1, 3), all(dict(vprops)[c] in _PLY_INTS for c in _PLY_COLOURS)))
    return verts, tris


def load_mesh(path):
    """(verts float64 [V,3], tris int32 [T,3]) of an .obj or .ply file; polygons are split as fans around their first vertex.
    Every index lies in [0, V).  Malformed files raise ValueError with the file name and the line (OBJ) or element (PLY)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        verts, tris = _load_obj(path)
    elif ext == ".ply":
        verts, tris = _load_ply(path)
    else:
        raise ValueError("%s: expected an .obj or .ply file" % os.path.basename(path))
    return (np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(tris, np.int64).reshape(-1, 3).astype(np.int32))


def load_mesh_colours(path):
    """The vertex colours of an .obj or .ply file as uint8 [V,3], in `load_mesh`'s vertex order, or None when the file has none.
    An .obj carries them as `v x y z r g b` with r, g, b in 0..1, read as round(255 r); a .ply as the vertex properties red,
    green, blue -- integers are taken as bytes, floats as 0..1.  An .obj in which only some vertices have colours has none."""
    ext = os.path.splitext(path)[1].lower()
    cols = []
    if ext == ".obj":
        _load_obj(path, cols)
        if not cols or any(c is None for c in cols):
            return None
        c = np.rint(255.0 * np.asarray(cols, np.float64))
    elif ext == ".ply":
        _load_ply(path, cols)
        if not cols:
            return None
        c, ints = cols[0]
        c = c if ints else np.rint(255.0 * c)
    else:
        raise ValueError("%s: expected an .obj or .ply file" % os.path.basename(path))
    return np.clip(c, 0, 255).astype(np.uint8).reshape(-1, 3)


def parse_axes(axes):
    """"z,x,-y" -> ((2, 0, 1), (1.0, 1.0, -1.0)): per array axis the mesh axis it takes and its sign."""
    parts = [p.strip() for p in str(axes).split(",")]
    perm, sign = [], []
    for p in parts:
        s = -1.0 if p.startswith("-") else 1.0
        p = p.lstrip("+-").lower()
        if p not in ("x", "y", "z"):
            break
        perm.append("xyz".index(p))
        sign.append(s)
    if len(parts) != 3 or sorted(perm) != [0, 1, 2]:
        raise ValueError("axes=%r: expected a signed permutation of x, y, z such as \"z,x,-y\"" % (axes,))
    return tuple(perm), tuple(sign)


def axes_sign(axes):
    """+1 when `fit` with this axis string keeps the handedness of the mesh in array-axis order, -1 when it mirrors it (the
    determinant of the signed permutation): a mirrored mesh has every triangle wound the other way round."""
    perm, sign = parse_axes(axes)
    return 1 if np.linalg.det(np.eye(3)[list(perm)] * np.asarray(sign)[:, None]) > 0 else -1


def _check_size(S):
    if isinstance(S, (bool, float)) or int(S) not in SIZES:
        raise ValueError("S=%r (32, 64 or 128)" % (S,))
    return int(S)


def fit(verts, S, margin=1, axes="x,y,z"):
    """verts float64 [V,3] -> lattice coordinates int32 [V,3], column j = array axis j of the grid [S,S,S], 256 units per voxel.
    float64 throughout: with p the permuted, signed vertex, lo and hi its bounding box and L = max(hi - lo),
        g = (p - (lo + hi) / 2) * (S - 2 margin) / L + S / 2,      q = clip(rint(256 g), 0, 256 S)        (rint: half to even)
    so the model is centred on every axis and `margin` voxels stay empty on each side."""
    S = _check_size(S)
    perm, sign = parse_axes(axes)
    if isinstance(margin, (bool, float)) or not 0 <= int(margin) < S // 2:
        raise ValueError("margin=%r: expected an integer in 0..%d" % (margin, S // 2 - 1))
    verts = np.asarray(verts, np.float64)
    if verts.ndim != 2 or verts.shape[1] != 3 or len(verts) == 0 or not np.isfinite(verts).all():
        raise ValueError("fit: expected finite vertices [V,3] with V >= 1, got %s" % (verts.shape,))
    p = verts[:, perm] * np.asarray(sign, np.float64)
    lo, hi = p.min(0), p.max(0)
    L = (hi - lo).max()
    if L == 0:
        raise ValueError("fit: the mesh has no extent")
    g = (p - (lo + hi) / 2) * (S - 2 * int(margin)) / L + S / 2
    return np.clip(np.rint(LATTICE * g), 0, LATTICE * S).astype(np.int32)


def _centre_range(lo, hi, S):
    """Voxels whose centre 256 k + 128 lies in [lo, hi], clipped to the grid: (first, count)."""
    a = np.clip(-((128 - lo) // LATTICE), 0, S)                  # ceil((lo - 128) / 256)
    b = np.clip((hi - 128) // LATTICE, -1, S - 1)
    return a, np.maximum(b - a + 1, 0)


def _cell_range(lo, hi, S):
    """Voxels whose closed cell [256 k, 256 (k + 1)] meets [lo, hi], clipped to the grid: (first, count)."""
    a = np.clip(-((-lo) // LATTICE) - 1, 0, S)                   # ceil(lo / 256) - 1
    b = np.clip(hi // LATTICE, -1, S - 1)
    return a, np.maximum(b - a + 1, 0)


def prepare(q, tris, S, threshold=None):
    """The work of one rn_mesh_voxelize call.  q int [V,3] lattice coordinates (clamped to [0, 256 S] as the kernel clamps them),
    tris int [T,3] with every index in [0, V).  Triangles whose lattice normal (p1 - p0) x (p2 - p1) is zero are dropped and
    counted.  A triangle's size is its candidate count -- columns whose centre lies in its projected bounding box for the solid
    rule, voxels whose cell meets its bounding box for the surface rule; at most `threshold` (default THRESHOLD) is small.
    Returns {"q", "tris" (the kept ones), "S", "dropped", "small_solid", "large_solid", "small_surf", "large_surf"} with int32
    lists of indices into "tris"; the solid lists leave out triangles with no candidate column or a zero projected area."""
    S = _check_size(S)
    threshold = THRESHOLD if threshold is None else int(threshold)
    q = np.ascontiguousarray(q)
    tris = np.ascontiguousarray(tris)
    if q.ndim != 2 or q.shape[1] != 3 or q.dtype.kind not in "iu":
        raise ValueError("prepare: q must be integers [V,3], got %s %s" % (q.dtype, q.shape))
    if tris.ndim != 2 or tris.shape[1] != 3 or tris.dtype.kind not in "iu":
        raise ValueError("prepare: tris must be integers [T,3], got %s %s" % (tris.dtype, tris.shape))
    if len(tris) and (int(tris.min()) < 0 or int(tris.max()) >= len(q)):
        raise ValueError("prepare: a triangle index outside [0, %d)" % len(q))
    q = q.astype(np.int32)
    qc = np.clip(q.astype(np.int64), 0, LATTICE * S)
    p = qc[tris.astype(np.int64)]                                # [T,3 vertices,3 axes]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1]) if len(tris) else np.zeros((0, 3), np.int64)
    keep = (n != 0).any(1)
    tris, p, n = tris[keep].astype(np.int32), p[keep], n[keep]
    lo, hi = p.min(1), p.max(1)
    cols = _centre_range(lo[:, 0], hi[:, 0], S)[1] * _centre_range(lo[:, 1], hi[:, 1], S)[1]
    cols = np.where(n[:, 2] != 0, cols, 0)                       # A = n_2: no projected area, no crossings
    cells = np.prod([_cell_range(lo[:, k], hi[:, k], S)[1] for k in range(3)], 0) if len(tris) else np.zeros(0, np.int64)
    idx = np.arange(len(tris), dtype=np.int32)
    return {"q": q, "tris": tris, "S": S, "dropped": int((~keep).sum()),
            "small_solid": idx[(cols > 0) & (cols <= threshold)], "large_solid": idx[cols > threshold],
            "small_surf": idx[(cells > 0) & (cells <= threshold)], "large_surf": idx[cells > threshold]}


def voxelize(path, S=64, mode="both", margin=1, axes="x,y,z", device="cuda", return_bits=False):
    """The occupancy grid of the mesh file `path`: uint8 [1,S,S,S,1] on `device` (load_mesh, fit, prepare, ops.voxelize_mesh)."""
    from . import ops
    verts, tris = load_mesh(path)
    if len(verts) == 0:
        raise ValueError("%s: no vertices" % os.path.basename(path))
    return ops.voxelize_mesh(prepare(fit(verts, S, margin, axes), tris, S), S=S, mode=mode, return_bits=return_bits, device=device)


def extract(vox, threshold=0.5, smooth=True, triangles=False, device="cuda", relax=0, relax_weight=256, merge=False):
    """The surface-net mesh of ONE grid -- [S,S,S], [S,S,S,1], [1,S,S,S] or [1,S,S,S,1], float32 or uint8, a NumPy array or a
    tensor -- as NumPy arrays (q int32 [V,3] on the lattice, faces int32 [F,4] or [2F,3]); `ops.extract_mesh` does the work on
    `device` (a tensor stays where it is).  `relax` passes of surface-net relaxation at `relax_weight` / 256 smooth the vertices
    inside their cells (4 at 256 is the recommended setting).  `merge` (with smooth=False and relax=0 only) merges the coplanar
    voxel faces into rectangles (`ops.extract_mesh_merged`): the same surface in far fewer quads, for export."""
    import torch
    from . import ops
    if merge and (smooth or relax):
        raise ValueError("extract: merge needs the blocky mesh (smooth=False) and no relaxation")
    t = vox if torch.is_tensor(vox) else torch.as_tensor(np.ascontiguousarray(vox))
    if t.dtype not in (torch.float32, torch.uint8):
        t = t.float()
    if t.dim() == 5 and t.shape[0] == 1 and t.shape[4] == 1:
        t = t[0, ..., 0]
    elif t.dim() == 4 and t.shape[3] == 1:
        t = t[..., 0]
    elif t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3:
        raise ValueError("extract: expected one grid [S,S,S], got %s" % (tuple(vox.shape),))
    if not t.is_cuda:
        t = t.to(device)
    if merge:
        m = ops.extract_mesh_merged(t[None], threshold=threshold, triangles=triangles)
    else:
        m = ops.extract_mesh(t[None], threshold=threshold, smooth=smooth, triangles=triangles, relax=relax, relax_weight=relax_weight)
    return m.q.cpu().numpy(), m.faces.cpu().numpy()


class MeshSet(object):
    """Fitted triangle meshes concatenated on the device, in the layout `ops.rasterize_mesh` takes and `ops.ExtractedMesh` has:
    `q` int32 [V,3] lattice vertices, `tris` int32 [T,3] with indices local to their mesh, `vert_offsets` and `tri_offsets`
    int64 [M+1], `vertex_normals` int64 [V,3] (`ops.mesh_vertex_normals`, computed once here), `names` and the grid side `S` the
    vertices were fitted to.  `meshes` is a list of (q, tris) host arrays, as `fit` and `load_mesh` give them, wound outwards in
    array-axis order.  `colours` is None, or a uint8 [V,3] tensor, a row per row of `q`: given to the constructor as one uint8
    [V_m,3] host array per mesh (the set keeps every mesh's vertex order, so `load_mesh_colours` of a file aligns with its `q`),
    and what `rasterize_colour` draws with."""

    def __init__(self, meshes, names, S=64, device="cuda", colours=None):
        import torch
        from . import ops
        self.S = _check_size(S)
        self.names = [str(n) for n in names]
        if len(self.names) != len(meshes) or not meshes:
            raise ValueError("MeshSet: %d names for %d meshes (at least one)" % (len(self.names), len(meshes)))
        qs, ts = [], []
        for name, (q, tris) in zip(self.names, meshes):
            q, tris = np.ascontiguousarray(q), np.ascontiguousarray(tris)
            if q.ndim != 2 or q.shape[1] != 3 or q.dtype.kind not in "iu" or tris.ndim != 2 or tris.shape[1] != 3 or tris.dtype.kind not in "iu":
                raise ValueError("MeshSet: %s: expected integers q [V,3] and tris [T,3], got %s %s and %s %s"
                                 % (name, q.dtype, q.shape, tris.dtype, tris.shape))
            if len(q) == 0 or len(tris) == 0 or int(tris.min()) < 0 or int(tris.max()) >= len(q):
                raise ValueError("MeshSet: %s: no triangles, or a triangle index outside [0, %d)" % (name, len(q)))
            qs.append(q.astype(np.int32))
            ts.append(tris.astype(np.int32))
        self.device = torch.device(device)
        self.q = torch.as_tensor(np.concatenate(qs)).to(self.device)
        self.tris = torch.as_tensor(np.concatenate(ts)).to(self.device)
        self.vert_offsets = torch.as_tensor(np.cumsum([0] + [len(a) for a in qs]).astype(np.int64)).to(self.device)
        self.tri_offsets = torch.as_tensor(np.cumsum([0] + [len(a) for a in ts]).astype(np.int64)).to(self.device)
        self.vertex_normals = ops.mesh_vertex_normals(self.q, self.tris, self.S, self.vert_offsets, self.tri_offsets)
        self.colours = None
        if colours is not None:
            cs = [np.asarray(c) for c in colours]
            if len(cs) != len(qs) or any(c.dtype != np.uint8 or c.shape != (len(q), 3) for c, q in zip(cs, qs)):
                raise ValueError("MeshSet: colours must be one uint8 [V,3] array per mesh, a row per vertex")
            self.colours = torch.as_tensor(np.ascontiguousarray(np.concatenate(cs))).to(self.device)

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_files(cls, paths, S=64, margin=1, axes="x,y,z", device="cuda", names=None):
        """load_mesh + fit per file, the way `voxelize` reads it, so the set overlays the files' grids; axes that mirror the mesh
        (`axes_sign` < 0) get triangle columns 1 and 2 swapped, which winds them outwards again.  When EVERY file carries vertex
        colours (`load_mesh_colours`) the set has `colours`; otherwise it has none."""
        meshes, colours = [], []
        for p in paths:
            verts, tris = load_mesh(p)
            if len(verts) == 0:
                raise ValueError("%s: no vertices" % os.path.basename(p))
            if axes_sign(axes) < 0:
                tris = np.ascontiguousarray(tris[:, [0, 2, 1]])
            meshes.append((fit(verts, S, margin, axes), tris))
            c = load_mesh_colours(p)
            colours.append(c if c is not None and len(c) == len(verts) else None)
        return cls(meshes, names if names is not None else [os.path.splitext(os.path.basename(p))[0] for p in paths], S, device,
                   colours if all(c is not None for c in colours) else None)

    def rasterize(self, mesh_ids, pose_or_m_inv, new_size=128, pixels_per_cell=4, **options):
        """`ops.rasterize_mesh` of meshes `mesh_ids` (a sequence of B indices into the set, or an int32 tensor [B]) at the B poses;
        `options` are its window, affine, smooth, cull, view_from_low_x and return_ids."""
        import torch
        from . import ops
        ids = mesh_ids if torch.is_tensor(mesh_ids) else torch.as_tensor(np.asarray(mesh_ids, np.int32).reshape(-1))
        return ops.rasterize_mesh(self.q, self.tris, pose_or_m_inv, self.S, new_size=new_size, pixels_per_cell=pixels_per_cell,
                                  vert_offsets=self.vert_offsets, tri_offsets=self.tri_offsets,
                                  mesh_of_item=ids.to(self.device, torch.int32), vertex_normals=self.vertex_normals, **options)

    def rasterize_colour(self, mesh_ids, pose_or_m_inv, new_size=128, pixels_per_cell=4, **options):
        """`ops.rasterize_mesh_colour` of meshes `mesh_ids` at the B poses with the set's vertex `colours`; `options` are its
        window, affine, smooth, cull, view_from_low_x, background, return_normals and return_ids -- or `face_colours` uint8 [T,3]
        (or other `vertex_colours`), which then take the place of the set's own.  A set without colours needs one of them."""
        import torch
        from . import ops
        if "face_colours" not in options and "vertex_colours" not in options:
            if self.colours is None:
                raise ValueError("MeshSet.rasterize_colour: the set has no colours; pass vertex_colours or face_colours")
            options["vertex_colours"] = self.colours
        ids = mesh_ids if torch.is_tensor(mesh_ids) else torch.as_tensor(np.asarray(mesh_ids, np.int32).reshape(-1))
        return ops.rasterize_mesh_colour(self.q, self.tris, pose_or_m_inv, self.S, new_size=new_size, pixels_per_cell=pixels_per_cell,
                                         vert_offsets=self.vert_offsets, tri_offsets=self.tri_offsets,
                                         mesh_of_item=ids.to(self.device, torch.int32), vertex_normals=self.vertex_normals, **options)


def save_meshes(paths, vol, threshold=0.5, smooth=True, axes="x,y,z", relax=0, relax_weight=256):
    """vol [B,S,S,S] (or [B,S,S,S,1]) on the device, float32 or uint8 -> one mesh file per grid, paths[b] for grid b, from a single
    `ops.extract_mesh` call; what Reconstruct_RenderNet_Face.py does with its hypotheses.  An empty grid gives a file without
    vertices.  `relax` and `relax_weight` are `ops.extract_mesh`'s."""
    import torch
    from . import ops
    if len(paths) != int(vol.shape[0]):
        raise ValueError("save_meshes: %d paths for %d grids" % (len(paths), int(vol.shape[0])))
    if vol.dtype not in (torch.float32, torch.uint8):
        vol = vol.float()
    m = ops.extract_mesh(vol, threshold=threshold, smooth=smooth, relax=relax, relax_weight=relax_weight)
    q, faces = m.q.cpu().numpy(), m.faces.cpu().numpy()
    vo, fo = m.vert_offsets.tolist(), m.face_offsets.tolist()
    for b, path in enumerate(paths):
        save_mesh(path, q[vo[b]:vo[b + 1]], faces[fo[b]:fo[b + 1]], axes=axes)


def save_mesh(path, q, faces, axes="x,y,z", colours=None):
    """Writes lattice vertices q int [V,3] and faces int [F,3] or [F,4] (indices into q) as .obj or ASCII .ply, by extension.
    `colours` uint8 [V,3] (`ops.mesh_vertex_colours`) adds a colour to every vertex: the properties uchar red, green, blue of a
    .ply, and the common `v x y z r g b` extension of an .obj with byte / 255 at 6 decimals, which `load_mesh_colours` reads back
    to the byte; without it the file is what it always was.
    Coordinates are in voxel units, q / 256, printed with every digit they have (a multiple of 1/256 below 2^15 has at most 12),
    so `load_mesh` reads back q / 256 exactly and its fan of a quad is (0,1,2),(0,2,3).  `axes` is the signed permutation `fit`
    takes, applied backwards: array axis j is written to the mesh axis that entry j names, so that
    fit(load_mesh(path), axes=axes) stands the mesh where the grid was.  A mirroring `axes` reverses every face, (0,3,2,1), so
    the normals keep pointing outwards."""
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".obj", ".ply"):
        raise ValueError("%s: expected an .obj or .ply file" % os.path.basename(path))
    perm, sign = parse_axes(axes)
    q, faces = np.asarray(q), np.asarray(faces)
    if q.ndim != 2 or q.shape[1] != 3 or q.dtype.kind not in "iu":
        raise ValueError("save_mesh: q must be integers [V,3], got %s %s" % (q.dtype, q.shape))
    if faces.ndim != 2 or faces.shape[1] not in (3, 4) or faces.dtype.kind not in "iu":
        raise ValueError("save_mesh: faces must be integers [F,3] or [F,4], got %s %s" % (faces.dtype, faces.shape))
    if len(faces) and (int(faces.min()) < 0 or int(faces.max()) >= len(q)):
        raise ValueError("save_mesh: a face index outside [0, %d)" % len(q))
    if len(q) and int(np.abs(q).max()) > 1 << 23:
        raise ValueError("save_mesh: lattice coordinates beyond 2^23 do not print exactly")
    if colours is not None:
        colours = np.asarray(colours)
        if colours.dtype != np.uint8 or colours.shape != (len(q), 3):
            raise ValueError("save_mesh: colours must be uint8 [%d,3], got %s %s" % (len(q), colours.dtype, colours.shape))
    xyz = np.empty(q.shape, np.float64)
    for j in range(3):
        xyz[:, perm[j]] = sign[j] * (q[:, j].astype(np.float64) / LATTICE)
    mirrored = np.linalg.det(np.eye(3)[list(perm)] * np.asarray(sign)[:, None]) < 0
    if mirrored:
        faces = faces[:, [0] + list(range(faces.shape[1] - 1, 0, -1))]
    k = faces.shape[1]
    with open(path, "w") as f:
        if ext == ".obj":
            f.write("# %d vertices, %d faces, voxel units\n" % (len(xyz), len(faces)))
            if colours is None:
                f.write("".join("v %.12g %.12g %.12g\n" % tuple(p) for p in xyz.tolist()))
            else:
                f.write("".join("v %.12g %.12g %.12g %.6f %.6f %.6f\n" % (tuple(p) + tuple(c))
                                for p, c in zip(xyz.tolist(), (colours.astype(np.float64) / 255.0).tolist())))
            f.write("".join(("f" + " %d" * k + "\n") % tuple(r) for r in (faces.astype(np.int64) + 1).tolist()))
        else:
            f.write("ply\nformat ascii 1.0\ncomment voxel units\nelement vertex %d\nproperty float x\nproperty float y\n"
                    "property float z\n%selement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                    % (len(xyz), "" if colours is None else "".join("property uchar %s\n" % c for c in _PLY_COLOURS), len(faces)))
            if colours is None:
                f.write("".join("%.12g %.12g %.12g\n" % tuple(p) for p in xyz.tolist()))
            else:
                f.write("".join("%.12g %.12g %.12g %d %d %d\n" % (tuple(p) + tuple(c)) for p, c in zip(xyz.tolist(), colours.tolist())))
            f.write("".join(("%d" % k + " %d" * k + "\n") % tuple(r) for r in faces.tolist()))
