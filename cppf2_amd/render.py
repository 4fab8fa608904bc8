"""Training items from meshes: the front of the reference's "Training with your own data" workflow (README; train_custom.ipynb
cell 4; dataset.py:177-319 ShapeNetDirectDataset, :371-413 dump_data) without OpenGL.

    python -m cppf2_amd.render --mesh obj_000015.ply --mesh-scale 0.001 --count 1000 --out data/demo_data [--full-rot]

renders each item's random pose with cppf_render_depth (a depth-only rasterizer, include/cppf_hip.h), then runs the rest of the
reference's recipe on the library: back-projection (ops.backproject), voxel down-sample (ops.downsample), SHOT descriptors and
normals (shot.compute_device, radii res*10), NaN -> 0.  Items are the reference's ShapeNetDirectDataset dicts without `rgb`;
the exported files hold (pc, pc_canon, bound, shot, normal) of a 100-point subsample, which ExportedItems /
ShapeNetExportDataset read for train_shot.py.  There is no RGB shading and no DINO descriptor (`desc`): the items serve
train_shot.py, not train_dino.py.

Every random draw of an item comes from numpy Generator([seed, item, attempt]), and the kernels' results do not depend on the
batch, so an item is the same whatever batch it is generated in.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import pickle
import struct
import sys

import numpy as np
import torch

from . import _lib, hostargs, ops, shot
from ._lib import CppfError
from .geometry import map_sym

_L = _lib.load()

INTRINSICS = np.array([[591.0125, 0, 320], [0, 590.16775, 240], [0, 0, 1]])      # dataset.py:193, notebook cell 2
HEIGHT, WIDTH = 480, 640                                                          # OffscreenRenderer(640, 480)
ZNEAR, ZFAR = 0.05, 100.0                                                         # pyrender's IntrinsicsCamera defaults
GL2CV = np.diag([1.0, -1.0, -1.0])                                                # OpenGL camera -> OpenCV camera
FLIP2NOCS = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], dtype=np.float64)        # dataset.py:213
MIN_POINTS = 100                                                                  # dataset.py:263: fewer -> draw again
MAX_ATTEMPTS = 16
SUBSAMPLE_STREAM = 1 << 30       # third seed word of the exported 100-point subsample's draw (attempts stay far below it)


# ----------------------------------------------------------------------------------------------
# mesh loaders
# ----------------------------------------------------------------------------------------------
class Mesh:
    """verts float64 [V,3] (already multiplied by the load scale), faces int32 [F,3]; device copies made on first use.  scale:
    the factor that took the file's units to these vertices' (load_mesh's `scale`)."""

    def __init__(self, verts, faces, scale=1.0):
        self.verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        self.scale = float(scale)
        if self.faces.size and (self.faces.min() < 0 or self.faces.max() >= len(self.verts)):
            raise ValueError("mesh face indices outside [0, %d)" % len(self.verts))
        self._dev = {}

    @property
    def bounds(self):
        return np.stack([self.verts.min(0), self.verts.max(0)])

    def device(self, dev):
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = (torch.as_tensor(self.verts.astype(np.float32)).to(dev),
                              torch.as_tensor(self.faces).to(dev))
        return self._dev[key]


_PLY_TYPES = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h", "ushort": "H", "uint16": "H",
              "int": "i", "int32": "i", "uint": "I", "uint32": "I", "float": "f", "float32": "f", "double": "d", "float64": "d"}


def _fan(polys):
    """Fan triangulation of a list of index lists: (a, b, c), (a, c, d), ..."""
    out = [(p[0], p[k], p[k + 1]) for p in polys for k in range(1, len(p) - 1)]
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def load_ply(path):
    """(verts float64 [V,3], faces int32 [F,3]) of an ascii or binary_little_endian PLY; faces from the `vertex_indices` /
    `vertex_index` list of the face element, polygons fan-triangulated.  Other elements and properties are skipped."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elements = None, []          # elements: (name, count, [(property, list count type or None, value type)])
        for line in iter(f.readline, b""):
            t = line.decode("ascii", "replace").split()
            if not t or t[0] in ("comment", "obj_info"):
                continue
            if t[0] == "end_header":
                break
            if t[0] == "format":
                fmt = t[1]
            elif t[0] == "element":
                elements.append((t[1], int(t[2]), []))
            elif t[0] == "property":
                elements[-1][2].append((t[4], _PLY_TYPES[t[2]], _PLY_TYPES[t[3]]) if t[1] == "list" else (t[2], None, _PLY_TYPES[t[1]]))
        else:
            raise ValueError("%s: PLY header without end_header" % path)
        body = f.read()
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("%s: PLY format %r is not supported (ascii, binary_little_endian)" % (path, fmt))
    binary = fmt != "ascii"
    toks = None if binary else body.split()
    pos, data = 0, {}
    for name, count, props in elements:
        if all(p[1] is None for p in props):          # rows of scalars: one block
            if binary:
                arr = np.frombuffer(body, np.dtype([(p[0], "<" + p[2]) for p in props]), count, pos)
                pos += arr.nbytes
                data[name] = {p[0]: arr[p[0]] for p in props}
            else:
                arr = np.asarray(toks[pos:pos + len(props) * count], dtype=np.float64).reshape(count, len(props))
                pos += arr.size
                data[name] = {p[0]: arr[:, i] for i, p in enumerate(props)}
            continue
        cols = {p[0]: [] for p in props}              # rows with lists: row by row
        for _ in range(count):
            for pname, ct, vt in props:
                if binary:
                    n = 1
                    if ct is not None:
                        n = struct.unpack_from("<" + ct, body, pos)[0]
                        pos += struct.calcsize(ct)
                    val = struct.unpack_from("<%d%s" % (n, vt), body, pos)
                    pos += n * struct.calcsize(vt)
                else:
                    n = 1 if ct is None else int(toks[pos])
                    pos += ct is not None
                    val = [float(x) for x in toks[pos:pos + n]]
                    pos += n
                cols[pname].append([int(x) for x in val] if ct is not None else val[0])
        data[name] = cols
    v = data.get("vertex")
    if v is None or not all(k in v for k in "xyz"):
        raise ValueError("%s: PLY without vertex x, y, z" % path)
    face = data.get("face", {})
    key = "vertex_indices" if "vertex_indices" in face else "vertex_index" if "vertex_index" in face else None
    if key is None:
        raise ValueError("%s: PLY without a face vertex_indices / vertex_index list" % path)
    verts = np.stack([np.asarray(v[k], dtype=np.float64) for k in "xyz"], -1)
    return verts, _fan(face[key]).astype(np.int32)


def load_obj(path):
    """(verts float64 [V,3], faces int32 [F,3]) of a Wavefront OBJ: `v` lines and polygon `f` lines (v, v/vt, v//vn, v/vt/vn;
    negative indices count back from the last vertex read), fan-triangulated; groups, objects, materials, texture
    coordinates, normals and comments are skipped.  Enough for ShapeNetCore's model_normalized.obj."""
    verts, polys = [], []
    with open(path, "r", errors="replace") as f:
        for line in f:
            if line.startswith("v "):
                p = line.split()
                verts.append((float(p[1]), float(p[2]), float(p[3])))
            elif line.startswith("f "):
                idx = []
                for t in line.split()[1:]:
                    i = int(t.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                polys.append(idx)
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    return verts, _fan(polys).astype(np.int32)


_MESHES = {}


def load_mesh(path, scale=1.0):
    """A Mesh from a .ply or .obj file with its vertices multiplied by `scale` (e.g. 0.001: mm -> m, the notebook's
    mesh.apply_scale).  Parsed once per process (keyed by path, size, modification time and scale)."""
    path = os.path.abspath(path)
    st = os.stat(path)
    key = (path, st.st_size, st.st_mtime_ns, float(scale))
    m = _MESHES.get(key)
    if m is None:
        ext = os.path.splitext(path)[1].lower()
        if ext == ".ply":
            v, f = load_ply(path)
        elif ext == ".obj":
            v, f = load_obj(path)
        else:
            raise ValueError("%s: only .ply and .obj meshes are read" % path)
        m = _MESHES[key] = Mesh(v * float(scale), f, scale)
    return m


# ----------------------------------------------------------------------------------------------
# depth rendering
# ----------------------------------------------------------------------------------------------
_CAP = {}                # (device index, stream) -> the tile lists' capacity of that stream's workspace


class _Workspaces(hostargs.ScratchCache):
    def __getitem__(self, key):                # the entry as one: (workspace, list capacity)
        return self.buffers[key], _CAP[key]


_WS = _Workspaces("cppf_render_depth_workspace_bytes", CppfError, on_drop=lambda key: _CAP.pop(key, None))
INITIAL_CAPACITY = 1 << 16


def _workspace(B, T, H, W, dev, capacity=None):
    """(workspace tensor, list capacity) for the current stream: the capacity given, else the one remembered, else the initial."""
    key = hostargs.stream_key(dev)
    cap = max(int(capacity if capacity is not None else _CAP.get(key, INITIAL_CAPACITY)), 1)
    ws = _WS.get(key, _L.cppf_render_depth_workspace_bytes(B, T, H, W, cap), dev)
    _CAP[key] = cap
    return ws, cap


def render_depth(verts, tris, tri_off, poses, intrinsics=INTRINSICS, height=HEIGHT, width=WIDTH, cull=True, znear=ZNEAR,
                 zfar=ZFAR, with_ids=False):
    """Depth maps of B views (cppf_render_depth): verts float32 [V,3], tris int32 [T,3], tri_off int32 [B+1] (view b draws
    tris[tri_off[b]:tri_off[b+1]], tri_off[B] = T), poses float32 [B,3,4] or [B,12] model -> OpenCV camera; all on the
    device.  Returns depth float32 [B,H,W] (0 = nothing drawn)[, tri_id int32 [B,H,W] (-1 = nothing)].  cull=True drops
    back faces (pyrender draws single-sided materials with GL_CULL_FACE).  The tile lists' workspace is cached per (device,
    stream) and grown (the call issued again) when a batch needs more entries.  Raises CppfError if a triangle had to be
    rejected (a vertex nearer than znear: there is no near-plane clipping; or off the +-2^22 px guard band)."""
    dev = verts.device
    B = tri_off.numel() - 1
    T = tris.shape[0]
    verts = verts.to(torch.float32).contiguous()
    tris = tris.to(torch.int32).contiguous()
    tri_off = tri_off.to(torch.int32).contiguous()
    poses = poses.to(device=dev, dtype=torch.float32).reshape(B, 12).contiguous()
    hK = hostargs.camera4(intrinsics)
    depth = torch.empty((B, height, width), dtype=torch.float32, device=dev)
    ids = torch.empty((B, height, width), dtype=torch.int32, device=dev) if with_ids else None
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    ent = _workspace(B, T, height, width, dev)
    for _ in range(2):
        ws, cap = ent
        _lib.check(_L.cppf_render_depth(B, ops._p(verts), verts.shape[0], ops._p(tris), ops._p(tri_off), T, ops._p(poses), hK,
                                        height, width, C.c_float(znear), C.c_float(zfar), int(bool(cull)), ops._p(depth),
                                        ops._p(ids), ops._p(status), ops._p(ws), ws.numel(), cap, ops._stream()),
                   "cppf_render_depth")
        rejected, needed = (int(x) for x in status.cpu().tolist())
        if rejected:
            raise CppfError("cppf_render_depth: %d triangles rejected (a vertex nearer than znear=%g, or outside the +-2^22 px "
                            "guard band); the renderer does not clip" % (rejected, znear))
        if needed <= cap:
            break
        ent = _workspace(B, T, height, width, dev, capacity=needed + needed // 4 + 1024)
    else:
        raise CppfError("cppf_render_depth: tile lists still overflow after growing the workspace")
    return (depth, ids) if with_ids else depth


# ----------------------------------------------------------------------------------------------
# poses
# ----------------------------------------------------------------------------------------------
def rotx(a):
    """3x3 block of dataset.py:97-101 rotx."""
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])


def roty(a):
    """3x3 block of dataset.py:91-95 roty."""
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, -s], [0, 1.0, 0], [s, 0, c]])


def item_rng(seed, item, attempt=0):
    """The generator of every random draw of one item: numpy Generator seeded with the words (seed, item, attempt)."""
    return np.random.default_rng([int(seed), int(item), int(attempt)])


def sample_pose(rng, full_rot=False):
    """(R [3,3], tr [3]) of one mesh pose in the OpenGL camera frame, dataset.py:215-225: uniform SO(3) if full_rot,
    else roty(yy) rotx(x) roty(y) with y in [0, 2pi), x in [10, 80] deg, yy in [-20, 20] deg; tr = (U(-.3,.3), U(-.3,.3),
    -U(.6, 2))."""
    if full_rot:
        q = rng.standard_normal(4)
        w, x, y, z = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    else:
        y_angle = rng.uniform(0, 2 * np.pi)
        x_angle = rng.uniform(10 / 180 * np.pi, 80 / 180 * np.pi)
        yy_angle = rng.uniform(-20 / 180 * np.pi, 20 / 180 * np.pi)
        R = roty(yy_angle) @ rotx(x_angle) @ roty(y_angle)
    tr = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -rng.uniform(0.6, 2.0)])
    return R, tr


def camera_pose(R, tr, scale, centre):
    """float32 [12]: diag(1,-1,-1) . mesh_pose . scale . centre, the model -> OpenCV camera transform of the rasterizer."""
    M = np.eye(4)
    M[:3, :3] = GL2CV @ (R * float(scale))
    M[:3, 3] = GL2CV @ tr
    T = np.eye(4)
    T[:3, 3] = -np.asarray(centre, dtype=np.float64)
    return (M @ T)[:3].astype(np.float32).reshape(12)


def _quat_wxyz(R):
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(R).as_quat()[[3, 0, 1, 2]]


# ----------------------------------------------------------------------------------------------
# items
# ----------------------------------------------------------------------------------------------
def make_items(meshes, items, seed=0, full_rot=False, res=2e-3, num_more=3, scale_ranges=None, nocs=False, sym_axis=None,
               intrinsics=INTRINSICS, height=HEIGHT, width=WIDTH, max_attempts=MAX_ATTEMPTS):
    """One batch of the reference's ShapeNetDirectDataset items (dataset.py:277-305 without `rgb`), one per id of `items`.

    meshes: a Mesh for all items or one per item.  scale_ranges: None (scale 1: the notebook's custom object, mesh already in
    metres) or one (lo, hi) per item (dataset.py:165-172, the ShapeNet synsets).  nocs: ShapeNet's flip2nocs and bound swap.
    sym_axis: the up axis of a rotationally symmetric category (map_sym; categories 1, 2, 4), else None.
    A view with fewer than 100 points after the down-sample is drawn again with the next attempt number (at most
    max_attempts, then CppfError).  Returns a list of dicts."""
    items = [int(i) for i in items]
    meshes = list(meshes) if isinstance(meshes, (list, tuple)) else [meshes] * len(items)
    if len(meshes) != len(items):
        raise ValueError("make_items: one mesh for all items or one per item")
    dev = ops._dev()
    K = np.asarray(intrinsics, dtype=np.float64).reshape(3, 3)
    out = [None] * len(items)
    attempt = [0] * len(items)
    todo = list(range(len(items)))
    while todo:
        # per-item draws: pose, then scale (dataset.py:215-235 order)
        rngs, params, poses = {}, {}, []
        for j in todo:
            rng = rngs[j] = item_rng(seed, items[j], attempt[j])
            R, tr = sample_pose(rng, full_rot)
            s = rng.uniform(*scale_ranges[j]) if scale_ranges is not None else 1.0
            b = meshes[j].bounds
            params[j] = (R, tr, s, b)
            poses.append(camera_pose(R, tr, s, (b[0] + b[1]) / 2))
        depth = _render_views([meshes[j] for j in todo], np.stack(poses), K, height, width, dev)
        kept, pcs, rcs = [], [], []
        for v, j in enumerate(todo):
            pc, (rows, cols) = ops.backproject(depth[v], K, depth[v] > 0, return_device=True)
            sel = ops.downsample(pc, res, seed=items[j], return_device=True) if pc.shape[0] else pc.new_zeros((0,), dtype=torch.long)
            if sel.numel() < MIN_POINTS:
                attempt[j] += 1
                if attempt[j] >= max_attempts:
                    raise CppfError("make_items: item %d has fewer than %d points in %d poses" % (items[j], MIN_POINTS, max_attempts))
                continue
            kept.append((v, j))
            pcs.append(pc[sel].contiguous())
            rcs.append(torch.stack([rows[sel], cols[sel]], -1))
        done = {j for _, j in kept}
        todo = [j for j in todo if j not in done]
        if not kept:
            continue
        pts = torch.cat(pcs, 0)
        pt_off = ops._offsets([p.shape[0] for p in pcs], dev)
        sfeat, nrm = shot.compute_device(pts, pt_off, res * 10, res * 10)
        ops.nan_to_zero_(sfeat)
        ops.nan_to_zero_(nrm)
        off = pt_off.cpu().numpy()
        sfeat, nrm, pts = sfeat.cpu().numpy(), nrm.cpu().numpy(), pts.cpu().numpy()
        for n, (v, j) in enumerate(kept):
            a, e = off[n], off[n + 1]
            out[j] = _item(pts[a:e], sfeat[a:e], nrm[a:e], rcs[n].cpu().numpy().astype(np.int64), depth[v].cpu().numpy(),
                           params[j], rngs[j], nocs, sym_axis, num_more)
    return out


def _render_views(meshes, poses, K, height, width, dev):
    uniq, first = [], {}
    for m in meshes:
        if id(m) not in first:
            first[id(m)] = len(uniq)
            uniq.append(m)
    if len(uniq) == 1:
        verts, tris = uniq[0].device(dev)
        tris = tris.repeat(len(meshes), 1)
        counts = [uniq[0].faces.shape[0]] * len(meshes)
    else:
        vbase = np.cumsum([0] + [m.verts.shape[0] for m in uniq])
        verts = torch.cat([m.device(dev)[0] for m in uniq], 0)
        tris = torch.cat([m.device(dev)[1] + int(vbase[first[id(m)]]) for m in meshes], 0)
        counts = [m.faces.shape[0] for m in meshes]
    tri_off = ops._offsets(counts, dev)
    return render_depth(verts, tris, tri_off, torch.as_tensor(poses).to(dev), K, height, width, cull=True)


def _item(pc, shot_feat, normal, idxs, depth, params, rng, nocs, sym_axis, num_more):
    R, tr, s, b = params
    rot = GL2CV @ R @ (np.linalg.inv(FLIP2NOCS) if nocs else np.eye(3))      # dataset.py:258, notebook: back to OpenCV
    if sym_axis is not None:
        rot = map_sym(rot.T, sym_axis).T                                      # dataset.py:259-260
    trans = GL2CV @ tr
    bound = b[1] - b[0]
    if nocs:
        bound[[0, 2]] = bound[[2, 0]]                                         # dataset.py:264: flip2nocs swaps the size too
    bound = bound * s
    scale = bound.max()
    point_idxs_all = rng.integers(0, pc.shape[0], (10000, 2 + num_more))
    pc_canon = (pc - trans) @ rot / scale
    return {
        "pc": pc.astype(np.float32),
        "pc_canon": pc_canon.astype(np.float32),
        "trans": trans.astype(np.float32),
        "quat": _quat_wxyz(rot).astype(np.float32),
        "bound": bound.astype(np.float32),
        "scale": np.float32(scale),
        "point_idxs_all": point_idxs_all.astype(int),
        "depth": depth.astype(np.float32),
        "idxs": idxs,
        "shot": shot_feat.astype(np.float32),
        "normal": normal.astype(np.float32),
    }


def export_item(item, item_id, seed=0, n=100):
    """The exported form of an item (dataset.py:388-412 without `desc`): a 100-point subsample drawn with replacement
    (Generator(seed, item_id, SUBSAMPLE_STREAM)) of pc, pc_canon, shot, normal, plus bound."""
    sub = item_rng(seed, item_id, SUBSAMPLE_STREAM).choice(item["pc"].shape[0], n)
    return {"pc": item["pc"][sub], "pc_canon": item["pc_canon"][sub], "bound": item["bound"], "shot": item["shot"][sub],
            "normal": item["normal"][sub]}


def write_items(out_dir, items, item_ids, seed=0):
    """Writes `<out_dir>/{:06d}.pkl` per item id: the layout ExportedItems and ShapeNetExportDataset read."""
    os.makedirs(out_dir, exist_ok=True)
    for it, i in zip(items, item_ids):
        with open(os.path.join(out_dir, "{:06d}.pkl".format(int(i))), "wb") as f:
            pickle.dump(export_item(it, i, seed), f)


def generate(mesh, out_dir, count, mesh_scale=1.0, full_rot=False, res=2e-3, num_more=3, seed=0, batch=64, log=None):
    """train_custom.ipynb cell 4: `count` items of one mesh (centred on its bounding box, scale 1 after mesh_scale) written
    to out_dir in batches of `batch` views.  Returns the number of files written."""
    m = load_mesh(mesh, mesh_scale) if isinstance(mesh, str) else mesh
    for a in range(0, int(count), int(batch)):
        ids = list(range(a, min(a + int(batch), int(count))))
        write_items(out_dir, make_items(m, ids, seed=seed, full_rot=full_rot, res=res, num_more=num_more), ids, seed)
        if log:
            log("%d / %d items" % (ids[-1] + 1, count))
    return int(count)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cppf2_amd.render", description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True, help=".ply or .obj mesh of the object")
    ap.add_argument("--mesh-scale", type=float, default=1.0, help="vertex scale to metres (0.001 for a mesh in mm)")
    ap.add_argument("--count", type=int, required=True, help="number of items")
    ap.add_argument("--out", required=True, help="output directory of the {:06d}.pkl items")
    ap.add_argument("--full-rot", action="store_true", help="uniform SO(3) poses (else the NOCS-limited range)")
    ap.add_argument("--res", type=float, default=2e-3, help="voxel size of the down-sample (SHOT radii are res*10)")
    ap.add_argument("--num-more", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=64, help="views rendered per call")
    a = ap.parse_args(argv)
    n = generate(a.mesh, a.out, a.count, a.mesh_scale, a.full_rot, a.res, a.num_more, a.seed, a.batch,
                 log=lambda s: print(s, file=sys.stderr, flush=True))
    print("wrote %d items to %s" % (n, a.out))


if __name__ == "__main__":
    main()
