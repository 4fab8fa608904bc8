"""BOP-format datasets (Hodan et al., the BOP challenge's layout): reading a dataset folder, writing one from rendered scenes,
the results CSV, and the BOP'19 average recall of a results file over a dataset.  The reference has none of this.

    ds = Dataset("data/ycbv", "test")                       # models/, test/000048/{scene_camera,scene_gt}.json, depth/, ...
    res = read_results("cppf_ycbv-test.csv")
    report = score(ds, res, targets="data/ycbv/test_targets_bop19.json")
    report["AR"], report["per_object"][15]["AR_VSD"]

Layout read (and written by write_dataset): models/models_info.json and models/obj_{id:06d}.ply (model units, `mesh_scale` to
metres); {split}/{scene:06d}/scene_camera.json (cam_K, depth_scale per image), scene_gt.json (cam_R_m2c, cam_t_m2c, obj_id per
instance), depth/{im:06d}.png (16 bit; metres = value * depth_scale / 1000), and optionally scene_gt_info.json and
mask_visib/{im:06d}_{gt:06d}.png, which are computed with bop.gt_visibility when absent; read_detections / write_detections
handle a detections file (COCO-style JSON, run-length encoded masks: masks.py).  Poses are handed out in the record
convention of bop.py (centred model, metres).  No BOP dataset and no bop_toolkit were available to compare against: the formats
and rules are written from the BOP'19 definitions and parity with bop_toolkit's numbers is unpinned.
"""
from __future__ import annotations

import json
import os
import time

import numpy as np

from . import bop, render

VISIB_GT_MIN = 0.1                       # BOP'19: a ground-truth instance counts when at least 10 % of it is visible
RESULTS_HEADER = "scene_id,im_id,obj_id,score,R,t,time"


class BopDataError(ValueError):
    """A dataset folder or a results file that cannot be read as the BOP layout."""


def _read_json(path):
    with open(path) as f:
        return json.load(f)


def _write_json(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f)


def _int_keys(d):
    return {int(k): v for k, v in d.items()}


# ----------------------------------------------------------------------------------------------
# results CSV
# ----------------------------------------------------------------------------------------------
def make_results(scene_id, im_id, obj_id, score, R, t, time=None):
    """The results table: dict(scene_id, im_id, obj_id int64 [N], score float64 [N], R float64 [N,3,3], t float64 [N,3] (BOP's
    frame: x_cam = R x + t on the model file's vertices, t in the model's units), time float64 [N] (seconds, -1 = not given))."""
    n = len(np.asarray(scene_id).reshape(-1))
    tm = np.full(n, -1.0) if time is None else np.asarray(time, dtype=np.float64).reshape(-1)
    out = dict(scene_id=np.asarray(scene_id, dtype=np.int64).reshape(-1), im_id=np.asarray(im_id, dtype=np.int64).reshape(-1),
               obj_id=np.asarray(obj_id, dtype=np.int64).reshape(-1), score=np.asarray(score, dtype=np.float64).reshape(-1),
               R=np.asarray(R, dtype=np.float64).reshape(n, 3, 3), t=np.asarray(t, dtype=np.float64).reshape(n, 3), time=tm)
    if any(len(v) != n for v in out.values()):
        raise ValueError("make_results: columns of different lengths")
    return out


def write_results(path, results):
    """Writes the BOP results CSV; floats with repr, so read_results gives the same bits back."""
    r = results
    with open(path, "w") as f:
        f.write(RESULTS_HEADER + "\n")
        for j in range(len(r["score"])):
            f.write("%d,%d,%d,%s,%s,%s,%s\n" % (r["scene_id"][j], r["im_id"][j], r["obj_id"][j], repr(float(r["score"][j])),
                                                " ".join(repr(float(x)) for x in r["R"][j].reshape(-1)),
                                                " ".join(repr(float(x)) for x in r["t"][j].reshape(-1)),
                                                repr(float(r["time"][j]))))


def read_results(path):
    """Reads a BOP results CSV (header scene_id,im_id,obj_id,score,R,t,time; R nine and t three space-separated numbers)."""
    cols = dict(scene_id=[], im_id=[], obj_id=[], score=[], R=[], t=[], time=[])
    with open(path) as f:
        header = f.readline().strip()
        if header.replace(" ", "") != RESULTS_HEADER:
            raise BopDataError("%s: header %r is not %r" % (path, header, RESULTS_HEADER))
        for n, line in enumerate(f, 2):
            if not line.strip():
                continue
            p = line.strip().split(",")
            try:
                if len(p) != 7:
                    raise ValueError("%d fields" % len(p))
                R = [float(x) for x in p[4].split()]
                t = [float(x) for x in p[5].split()]
                if len(R) != 9 or len(t) != 3:
                    raise ValueError("R has %d numbers (9), t has %d (3)" % (len(R), len(t)))
                row = (int(p[0]), int(p[1]), int(p[2]), float(p[3]), R, t, float(p[6]))
            except ValueError as e:
                raise BopDataError("%s line %d: %s" % (path, n, e)) from None
            for k, v in zip(cols, row):
                cols[k].append(v)
    return make_results(**cols)


def read_targets(path):
    """[(scene_id, im_id, obj_id, inst_count)] of a BOP targets file (test_targets_bop19.json)."""
    return [(int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"]), int(t.get("inst_count", 1))) for t in _read_json(path)]


# ----------------------------------------------------------------------------------------------
# detections file (the BOP challenge's "default detections": COCO-style JSON with run-length encoded masks)
# ----------------------------------------------------------------------------------------------
def _detection(e, where, image_size):
    from . import masks
    try:
        seg = e["segmentation"]
        size = [int(x) for x in seg["size"]]
        if len(size) != 2 or min(size) < 1:
            raise ValueError("segmentation size %r is not [H, W]" % (seg["size"],))
        det = dict(scene_id=int(e["scene_id"]), image_id=int(e["image_id"]), category_id=int(e["category_id"]),
                   bbox=[float(x) for x in e.get("bbox", [0, 0, 0, 0])], score=float(e["score"]), time=float(e.get("time", -1.0)),
                   size=(size[0], size[1]))
        if len(det["bbox"]) != 4:
            raise ValueError("bbox %r is not [x, y, w, h]" % (e["bbox"],))
        counts = seg["counts"]
        if isinstance(counts, (str, bytes)):
            counts = masks.string_to_counts(counts)
        elif not isinstance(counts, (list, tuple)) or any(isinstance(x, bool) or not isinstance(x, int) for x in counts):
            raise ValueError("segmentation counts are a list of integers or a compressed string")
        det["counts"] = [int(x) for x in masks.check_counts(counts, size[0], size[1])]
    except (KeyError, TypeError, ValueError) as err:                  # (masks.RleError is a ValueError)
        raise BopDataError("%s: %s%s" % (where, "missing field " if isinstance(err, KeyError) else "", err)) from None
    check_detection_size(det, image_size, where)
    return det


def check_detection_size(det, image_size, where="detection"):
    """BopDataError when a detection's mask size differs from its image's.  image_size: (H, W), a callable (scene_id, image_id)
    -> (H, W), or None (not checked)."""
    if image_size is None:
        return
    want = image_size(det["scene_id"], det["image_id"]) if callable(image_size) else image_size
    if tuple(int(x) for x in want) != tuple(det["size"]):
        raise BopDataError("%s: mask size %s differs from the %s of image %d of scene %d" % (
            where, list(det["size"]), [int(x) for x in want], det["image_id"], det["scene_id"]))


def read_detections(path, image_size=None):
    """[dict(scene_id, image_id, category_id (= obj_id), bbox [x, y, w, h], score, time, size (H, W), counts [int])] of a
    detections file: a JSON list with one entry per detection, its mask under segmentation {counts, size [H, W]} as COCO run
    lengths (a list, or the compressed string: masks.string_to_counts).  BopDataError for a missing field, a mask size that
    differs from the image's (image_size: see check_detection_size), runs that do not sum to H * W, a negative run and a string
    that does not parse."""
    try:
        entries = _read_json(path)
    except ValueError as err:
        raise BopDataError("%s: not JSON (%s)" % (path, err)) from None
    if not isinstance(entries, list):
        raise BopDataError("%s: a detections file is a JSON list" % path)
    return [_detection(e, "%s entry %d" % (path, n), image_size) for n, e in enumerate(entries)]


def write_detections(path, dets, compress=True):
    """Writes a detections file read_detections gives back: dets as read_detections returns them (time and bbox optional);
    compress: counts as COCO's compressed string, else as a list."""
    from . import masks
    out = []
    for d in dets:
        H, W = (int(x) for x in d["size"])
        counts = [int(x) for x in masks.check_counts(d["counts"], H, W)]
        out.append(dict(scene_id=int(d["scene_id"]), image_id=int(d["image_id"]), category_id=int(d["category_id"]),
                        bbox=[float(x) for x in d.get("bbox", [0, 0, 0, 0])], score=float(d["score"]), time=float(d.get("time", -1.0)),
                        segmentation=dict(counts=masks.counts_to_string(counts) if compress else counts, size=[H, W])))
    _write_json(path, out)


# ----------------------------------------------------------------------------------------------
# reader
# ----------------------------------------------------------------------------------------------
class Models:
    """The models folder of a BOP-format dataset: obj_{id:06d}.ply in model units (`mesh_scale` to metres) and, when present,
    models_info.json.  Dataset reads its objects through one; eval.py's multi-object form reads a folder given on its own."""

    def __init__(self, models_dir, mesh_scale=0.001):
        self.dir, self.mesh_scale = str(models_dir), float(mesh_scale)
        info = os.path.join(self.dir, "models_info.json")
        self.models_info = _int_keys(_read_json(info)) if os.path.exists(info) else {}
        self._objects = {}

    def ids(self):
        """The object ids that have a model file, ascending."""
        names = os.listdir(self.dir) if os.path.isdir(self.dir) else []
        return sorted(int(n[4:10]) for n in names if len(n) == 14 and n.startswith("obj_") and n.endswith(".ply") and n[4:10].isdigit())

    def model_path(self, obj_id):
        return os.path.join(self.dir, "obj_%06d.ply" % int(obj_id))

    def object(self, obj_id):
        """The bop.ObjectInfo of an object id (mesh and models_info entry), loaded on first use."""
        obj_id = int(obj_id)
        if obj_id not in self._objects:
            path = self.model_path(obj_id)
            if not os.path.exists(path):
                raise BopDataError("object %d has no model (%s)" % (obj_id, path))
            mesh = render.load_mesh(path, self.mesh_scale)
            self._objects[obj_id] = bop.ObjectInfo.from_mesh(mesh, models_info=self.models_info.get(obj_id), mesh_scale=self.mesh_scale)
        return self._objects[obj_id]

    def mesh(self, obj_id):
        self.object(obj_id)
        return render.load_mesh(self.model_path(obj_id), self.mesh_scale)


class Dataset:
    """One split of a BOP-format dataset under `root`.  scene_ids: the scene folders found.  Ground-truth poses are converted to
    the record convention (bop.pose_from_bop) with each object's bounding-box centre."""

    def __init__(self, root, split, mesh_scale=0.001):
        self.root, self.split, self.mesh_scale = str(root), str(split), float(mesh_scale)
        self.split_dir = os.path.join(self.root, self.split)
        if not os.path.isdir(self.split_dir):
            raise BopDataError("%s: no such split folder" % self.split_dir)
        self.models = Models(os.path.join(self.root, "models"), self.mesh_scale)
        self.models_info = self.models.models_info
        self.scene_ids = sorted(int(d) for d in os.listdir(self.split_dir)
                                if d.isdigit() and os.path.isdir(os.path.join(self.split_dir, d)))
        self._scenes, self._info, self._masks = {}, {}, (None, None)

    def scene_dir(self, scene_id):
        return os.path.join(self.split_dir, "%06d" % int(scene_id))

    def model_path(self, obj_id):
        return self.models.model_path(obj_id)

    def object(self, obj_id):
        """The bop.ObjectInfo of an object id (mesh and models_info entry), loaded on first use."""
        return self.models.object(obj_id)

    def mesh(self, obj_id):
        return self.models.mesh(obj_id)

    def scene(self, scene_id):
        """dict(camera {im: dict(K float64 [3,3], depth_scale)}, gt {im: [dict(obj_id, R, t (record convention), cam_R_m2c,
        cam_t_m2c (the file's))]})."""
        scene_id = int(scene_id)
        if scene_id not in self._scenes:
            d = self.scene_dir(scene_id)
            gt_path, cam_path = os.path.join(d, "scene_gt.json"), os.path.join(d, "scene_camera.json")
            if not os.path.exists(gt_path):
                raise BopDataError("scene %d has no scene_gt.json (%s)" % (scene_id, gt_path))
            if not os.path.exists(cam_path):
                raise BopDataError("scene %d has no scene_camera.json (%s)" % (scene_id, cam_path))
            cam = {im: dict(K=np.asarray(c["cam_K"], dtype=np.float64).reshape(3, 3), depth_scale=float(c.get("depth_scale", 1.0)))
                   for im, c in _int_keys(_read_json(cam_path)).items()}
            gt = {}
            for im, lst in _int_keys(_read_json(gt_path)).items():
                gt[im] = []
                for g in lst:
                    obj = self.object(g["obj_id"])
                    Rb = np.asarray(g["cam_R_m2c"], dtype=np.float64).reshape(3, 3)
                    tb = np.asarray(g["cam_t_m2c"], dtype=np.float64).reshape(3)
                    R, t = bop.pose_from_bop(Rb, tb, self.mesh_scale, obj.centre)
                    gt[im].append(dict(obj_id=int(g["obj_id"]), R=R, t=t, cam_R_m2c=Rb, cam_t_m2c=tb))
            self._scenes[scene_id] = dict(camera=cam, gt=gt)
        return self._scenes[scene_id]

    def depth(self, scene_id, im_id):
        """float32 [H,W] metres (0 = no reading): value * depth_scale / 1000."""
        from PIL import Image
        path = os.path.join(self.scene_dir(scene_id), "depth", "%06d.png" % int(im_id))
        if not os.path.exists(path):
            raise BopDataError("scene %d image %d has no depth image (%s)" % (scene_id, im_id, path))
        s = self.scene(scene_id)["camera"][int(im_id)]["depth_scale"]
        return (np.array(Image.open(path)).astype(np.float64) * s / 1000.0).astype(np.float32)

    def depths(self, items):
        """float32 [N,H,W] of [(scene_id, im_id)]; every image of a batch has the same shape (BopDataError otherwise)."""
        out = [self.depth(s, i) for s, i in items]
        for (s, i), d in zip(items, out):
            if d.shape != out[0].shape:
                raise BopDataError("scene %d image %d: depth %s differs from the batch's %s" % (s, i, d.shape, out[0].shape))
        return np.stack(out) if out else np.zeros((0, 0, 0), np.float32)

    # ---- visibility ---------------------------------------------------------------------------
    def _visibility(self, scene_id, im_ids, masks):
        """bop.gt_visibility of the instances of some images of a scene: {im: dict of per-instance arrays}."""
        sc = self.scene(scene_id)
        out, groups = {}, {}
        for im in im_ids:
            d = self.depth(scene_id, im)
            groups.setdefault((sc["camera"][im]["K"].tobytes(), d.shape), []).append((im, d))
        for (_, _), lst in groups.items():
            K = sc["camera"][lst[0][0]]["K"]
            inst = [(n, g) for n, (im, _) in enumerate(lst) for g in sc["gt"].get(im, [])]
            vis = bop.gt_visibility([self.object(g["obj_id"]) for _, g in inst], np.stack([d for _, d in lst]),
                                    [n for n, _ in inst], [g["R"] for _, g in inst], [g["t"] for _, g in inst], K, masks=masks)
            a = 0
            for im, _ in lst:
                n = len(sc["gt"].get(im, []))
                out[im] = {k: (v[a:a + n] if v is not None else None) for k, v in vis.items()}
                a += n
        return out

    def gt_info(self, scene_id):
        """{im: [dict(px_count_all, px_count_valid, px_count_visib, visib_fract, bbox_obj, bbox_visib)]}: scene_gt_info.json, or
        computed on the GPU (bop.gt_visibility) when the file is absent."""
        scene_id = int(scene_id)
        if scene_id not in self._info:
            path = os.path.join(self.scene_dir(scene_id), "scene_gt_info.json")
            if os.path.exists(path):
                self._info[scene_id] = _int_keys(_read_json(path))
            else:
                sc = self.scene(scene_id)
                vis = self._visibility(scene_id, sorted(sc["gt"]), False)
                self._info[scene_id] = {im: _info_entries(v) for im, v in vis.items()}
        return self._info[scene_id]

    def mask_visib(self, scene_id, im_id, gt_index):
        """bool [H,W]: the visible mask of one ground-truth instance, from mask_visib/ or computed (the last image's are kept)."""
        from PIL import Image
        path = os.path.join(self.scene_dir(scene_id), "mask_visib", "%06d_%06d.png" % (int(im_id), int(gt_index)))
        if os.path.exists(path):
            m = np.array(Image.open(path))
            return (m[..., 0] if m.ndim == 3 else m) > 0
        if self._masks[0] != (int(scene_id), int(im_id)):
            vis = self._visibility(scene_id, [int(im_id)], True)
            self._masks = ((int(scene_id), int(im_id)), vis[int(im_id)]["mask_visib"])
        return self._masks[1][int(gt_index)] > 0

    # ---- targets ------------------------------------------------------------------------------
    def targets(self, path=None, visib_gt_min=VISIB_GT_MIN):
        """[(scene_id, im_id, obj_id, inst_count)]: a targets file, or every (scene, image, object) with at least one valid
        ground-truth instance (visib_fract >= visib_gt_min), inst_count = their number."""
        if path is not None:
            return read_targets(path)
        out = []
        for s in self.scene_ids:
            info = self.gt_info(s)
            for im, lst in sorted(self.scene(s)["gt"].items()):
                n = {}
                for g, e in zip(lst, info[im]):
                    if e["visib_fract"] >= visib_gt_min:
                        n[g["obj_id"]] = n.get(g["obj_id"], 0) + 1
                out += [(s, im, o, c) for o, c in sorted(n.items())]
        return out


def _info_entries(vis):
    """scene_gt_info entries (JSON types) of one image from bop.gt_visibility's arrays."""
    return [dict(bbox_obj=[int(x) for x in vis["bbox_obj"][g]], bbox_visib=[int(x) for x in vis["bbox_visib"][g]],
                 px_count_all=int(vis["px_count_all"][g]), px_count_valid=int(vis["px_count_valid"][g]),
                 px_count_visib=int(vis["px_count_visib"][g]), visib_fract=float(vis["visib_fract"][g]))
            for g in range(len(vis["visib_fract"]))]


# ----------------------------------------------------------------------------------------------
# writer
# ----------------------------------------------------------------------------------------------
def write_ply(path, verts, faces):
    """A binary_little_endian PLY of float64 vertices and triangles (what render.load_ply reads back bit for bit)."""
    v = np.ascontiguousarray(verts, dtype="<f8").reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"], rec["i"] = 3, f
    with open(path, "wb") as out:
        out.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                   "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f))).encode("ascii"))
        out.write(v.tobytes())
        out.write(rec.tobytes())


def _render_alone(meshes, poses, K, H, W, dev):
    """float32 [N,H,W] device renders of N (Mesh, pose [3,4]) pairs, each alone; the mesh centred on its bounding-box centre."""
    import torch
    from . import ops
    if not meshes:
        return torch.zeros((0, H, W), dtype=torch.float32, device=dev)
    verts, tris, counts, base = [], [], [], 0
    for m in meshes:
        b = m.bounds
        verts.append(torch.from_numpy((m.verts - (b[0] + b[1]) / 2).astype(np.float32)))
        tris.append(torch.from_numpy(m.faces.astype(np.int32)) + base)
        counts.append(m.faces.shape[0])
        base += m.verts.shape[0]
    P = torch.from_numpy(np.asarray(poses, dtype=np.float32).reshape(-1, 12)).to(dev)
    return render.render_depth(torch.cat(verts).to(dev), torch.cat(tris).to(dev), ops._offsets(counts, dev), P, K, H, W, cull=True)


def write_dataset(root, split, meshes, scenes, K=render.INTRINSICS, height=render.HEIGHT, width=render.WIDTH, mesh_scale=0.001,
                  models_info=None, occluders=None, holes=None, depth_scale=0.1, targets_file="test_targets_bop19.json"):
    """Writes a BOP-format dataset of rendered scenes and returns its root.

    meshes: {obj_id: render.Mesh in metres}; models_info: {obj_id: entry in model units} (diameter computed when missing).
    scenes: a list of scenes (scene id = index), each a list of images (image id = index), each a list of (obj_id, R, t):
    poses in the record convention.  occluders: {(scene, image): [(Mesh, R, t)]}, drawn into the depth image but absent from
    scene_gt.  holes: {(scene, image): bool [H,W]}, readings set to 0.  One K for all images.  Every instance is rendered with
    render.render_depth (each must lie beyond render.ZNEAR: no clipping), the image depth is the nearest non-zero depth per
    pixel, quantised to the 16-bit PNG (metres = value * depth_scale / 1000), and scene_gt_info.json and mask_visib/ come from
    bop.gt_visibility on the depth as it reads back.  The targets file lists every (scene, image, object) with a valid instance."""
    import torch
    from PIL import Image
    from . import ops
    dev = ops._dev()
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    occluders, holes, models_info = occluders or {}, holes or {}, models_info or {}
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    info_out = {}
    for oid, m in meshes.items():
        write_ply(os.path.join(root, "models", "obj_%06d.ply" % oid), m.verts / mesh_scale, m.faces)
        entry = dict(models_info.get(oid, {}))
        b = m.bounds / mesh_scale
        entry.setdefault("diameter", bop.diameter(m.verts) / mesh_scale)
        entry.update(min_x=b[0, 0], min_y=b[0, 1], min_z=b[0, 2], size_x=b[1, 0] - b[0, 0], size_y=b[1, 1] - b[0, 1],
                     size_z=b[1, 2] - b[0, 2])
        info_out[str(oid)] = entry
    _write_json(os.path.join(root, "models", "models_info.json"), info_out)
    os.makedirs(os.path.join(root, split), exist_ok=True)
    ds = Dataset(root, split, mesh_scale)                               # the objects as a reader will see them
    targets = []
    for s, images in enumerate(scenes):
        d = os.path.join(root, split, "%06d" % s)
        os.makedirs(os.path.join(d, "depth"), exist_ok=True)
        os.makedirs(os.path.join(d, "mask_visib"), exist_ok=True)
        cam, gt, ginfo = {}, {}, {}
        for im, inst in enumerate(images):
            objs = [ds.object(o) for o, _, _ in inst]
            gt[str(im)] = []
            for (o, R, t), obj in zip(inst, objs):
                Rb, tb = bop.pose_to_bop(R, t, mesh_scale, obj.centre)
                gt[str(im)].append(dict(cam_R_m2c=[float(x) for x in Rb.reshape(-1)], cam_t_m2c=[float(x) for x in tb], obj_id=int(o)))
            # every render from the poses as a reader gets them back (pose_from_bop of what is written)
            back = [bop.pose_from_bop(g["cam_R_m2c"], g["cam_t_m2c"], mesh_scale, obj.centre) for g, obj in zip(gt[str(im)], objs)]
            back = [(np.asarray(R).reshape(3, 3), np.asarray(t).reshape(3)) for R, t in back]
            occ = occluders.get((s, im), [])
            ren = _render_alone([ds.mesh(o) for o, _, _ in inst] + [m for m, _, _ in occ],
                                [np.hstack([np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3, 1)])
                                 for R, t in back + [(R, t) for _, R, t in occ]], K, height, width, dev)
            depth = torch.where(ren > 0, ren, torch.full_like(ren, float("inf"))).amin(0) if ren.shape[0] else \
                torch.full((height, width), float("inf"), device=dev)
            depth = torch.where(torch.isinf(depth), torch.zeros_like(depth), depth).cpu().numpy().astype(np.float64)
            if (s, im) in holes:
                depth[np.asarray(holes[(s, im)], dtype=bool)] = 0.0
            png = np.clip(np.rint(depth * 1000.0 / depth_scale), 0, 65535).astype(np.uint16)
            Image.fromarray(png).save(os.path.join(d, "depth", "%06d.png" % im))
            depth_q = (png.astype(np.float64) * depth_scale / 1000.0).astype(np.float32)        # Dataset.depth's arithmetic
            cam[str(im)] = dict(cam_K=[float(x) for x in K.reshape(-1)], depth_scale=float(depth_scale))
            vis = bop.gt_visibility(objs, depth_q, 0, [b_[0] for b_ in back], [b_[1] for b_ in back], K, masks=True) if inst else None
            ginfo[str(im)] = _info_entries(vis) if inst else []
            n_valid = {}
            for g, (o, _, _) in enumerate(inst):
                Image.fromarray(vis["mask_visib"][g]).save(os.path.join(d, "mask_visib", "%06d_%06d.png" % (im, g)))
                if ginfo[str(im)][g]["visib_fract"] >= VISIB_GT_MIN:
                    n_valid[int(o)] = n_valid.get(int(o), 0) + 1
            targets += [dict(scene_id=s, im_id=im, obj_id=o, inst_count=c) for o, c in sorted(n_valid.items())]
        _write_json(os.path.join(d, "scene_camera.json"), cam)
        _write_json(os.path.join(d, "scene_gt.json"), gt)
        _write_json(os.path.join(d, "scene_gt_info.json"), ginfo)
    if targets_file:
        _write_json(os.path.join(root, targets_file), targets)
    return root


# ----------------------------------------------------------------------------------------------
# scoring
# ----------------------------------------------------------------------------------------------
def select_estimates(results, targets):
    """Rule 1: per target (scene, image, object) the rows of its inst_count estimates with the highest score, by descending
    score, ties in file order.  Returns ({(scene, im, obj): [row]}, dict(estimates, kept, not_a_target, over_inst_count))."""
    want = {(int(s), int(i), int(o)): int(n) for s, i, o, n in targets}
    rows = {}
    ignored = 0
    for j in range(len(results["score"])):
        key = (int(results["scene_id"][j]), int(results["im_id"][j]), int(results["obj_id"][j]))
        if key in want:
            rows.setdefault(key, []).append(j)
        else:
            ignored += 1
    kept = {}
    for key, lst in rows.items():
        order = np.argsort(-np.asarray(results["score"], dtype=np.float64)[lst], kind="stable")
        kept[key] = [lst[k] for k in order[:want[key]]]
    n_kept = sum(len(v) for v in kept.values())
    n = len(results["score"])
    return kept, dict(estimates=n, kept=n_kept, not_a_target=ignored, over_inst_count=n - ignored - n_kept)


def greedy_matches(err, thr, valid):
    """Rule 4 for one (image, object): err float64 [n_est, T, n_gt] or [n_est, 1, n_gt] (estimates by descending score), thr
    [T], valid bool [n_gt].  Every estimate in turn takes, per threshold, the valid instance not yet taken with the lowest
    error strictly below the threshold (the lower instance index on ties).  Returns (matches int64 [T], assign int64
    [n_est, T]: the instance index or -1)."""
    err = np.asarray(err, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64).reshape(-1)
    valid = np.asarray(valid, dtype=bool).reshape(-1)
    n_est, T, n_gt = err.shape[0], len(thr), len(valid)
    assign = np.full((n_est, T), -1, dtype=np.int64)
    if n_gt == 0 or n_est == 0:
        return np.zeros(T, dtype=np.int64), assign
    taken = np.zeros((T, n_gt), dtype=bool)
    rows = np.arange(T)
    for e in range(n_est):
        E = np.broadcast_to(err[e], (T, n_gt))
        cand = (E < thr[:, None]) & valid[None, :] & ~taken
        j = np.argmin(np.where(cand, E, np.inf), axis=1)             # the first minimum: the lower index on ties
        hit = cand[rows, j]
        taken[rows[hit], j[hit]] = True
        assign[e, hit] = j[hit]
    return (assign >= 0).sum(0).astype(np.int64), assign


def _recalls(matches, targets):
    """dict of AR_VSD, AR_MSSD, AR_MSPD, AR and the recall per threshold from integer match counts: each AR is (matches
    summed over the metric's thresholds) / (targets x thresholds) -- one float64 division of integers, which is what
    bop.average_recall's mean of booleans computes."""
    out = {}
    for k, m in matches.items():
        out["AR_" + k.upper()] = float(np.float64(int(m.sum())) / np.float64(targets * m.size)) if targets else None
    out["AR"] = (out["AR_VSD"] + out["AR_MSSD"] + out["AR_MSPD"]) / 3.0 if targets else None
    out["recall"] = {k: (m.astype(np.float64) / np.float64(targets)).tolist() if targets else None for k, m in matches.items()}
    out["matches"] = {k: m.tolist() for k, m in matches.items()}
    out["targets"] = int(targets)
    return out


def recall_report(tables, thetas=bop.THETAS, mspd_px=bop.MSPD_PX):
    """Rules 3-5 over error tables, one per target (scene, image, object): dict(obj_id, score [n_est], valid bool [n_gt], vsd
    [n_est, n_gt, n_taus], mssd, mspd [n_est, n_gt], diameter (metres), width (pixels)).  Returns the overall AR_VSD, AR_MSSD,
    AR_MSPD, AR, recall (per threshold: vsd [n_taus, n_thetas], mssd, mspd [10]), matches, targets, and per_object {obj_id:
    the same}."""
    th = np.asarray(thetas, dtype=np.float64)
    px = np.asarray(mspd_px, dtype=np.float64)
    acc = {}

    def add(key, name, m, n_valid):
        a = acc.setdefault(key, dict(m={}, targets=0))
        a["m"][name] = a["m"].get(name, 0) + m
        if name == "vsd":
            a["targets"] += n_valid
    for tab in tables:
        valid = np.asarray(tab["valid"], dtype=bool).reshape(-1)
        n_gt = len(valid)
        sc = np.asarray(tab["score"], dtype=np.float64).reshape(-1)
        n_est = len(sc)
        order = np.argsort(-sc, kind="stable")
        vsd = np.asarray(tab["vsd"], dtype=np.float64)
        n_taus = vsd.shape[-1]
        vsd = vsd.reshape(n_est, n_gt, n_taus)[order]
        mssd = np.asarray(tab["mssd"], dtype=np.float64).reshape(n_est, n_gt)[order]
        mspd = np.asarray(tab["mspd"], dtype=np.float64).reshape(n_est, n_gt)[order]
        # VSD: threshold (tau k, theta j) at row k * n_thetas + j, its errors the tau's column
        e_vsd = np.repeat(vsd.transpose(0, 2, 1), len(th), axis=1)
        m_vsd = greedy_matches(e_vsd, np.tile(th, n_taus), valid)[0].reshape(n_taus, len(th))
        m_mssd = greedy_matches(mssd[:, None, :], th * float(tab["diameter"]), valid)[0]
        m_mspd = greedy_matches(mspd[:, None, :], px * (float(tab["width"]) / 640.0), valid)[0]
        for key in (int(tab["obj_id"]), None):
            for name, m in (("vsd", m_vsd), ("mssd", m_mssd), ("mspd", m_mspd)):
                add(key, name, m, int(valid.sum()))
    if None not in acc:
        raise ValueError("bop_data.recall_report: no targets")
    out = _recalls(acc[None]["m"], acc[None]["targets"])
    out["per_object"] = {k: _recalls(a["m"], a["targets"]) for k, a in sorted((k, a) for k, a in acc.items() if k is not None)}
    return out


def error_tables(dataset, results, targets=None, visib_gt_min=VISIB_GT_MIN):
    """Rules 1-3: the error table of every target (see recall_report), the errors from bop.pose_errors -- one call per object
    and distinct (K, H, W), every kept estimate against every ground-truth instance of its object in its image.  targets: a
    list of (scene_id, im_id, obj_id, inst_count), a targets file, or None (Dataset.targets).  Returns (tables, counts)."""
    if targets is None or isinstance(targets, str):
        targets = dataset.targets(targets, visib_gt_min)
    kept, counts = select_estimates(results, targets)
    depths, groups, tables = {}, {}, []
    n_inst = n_valid = 0
    for s, im, o, _ in targets:
        sc = dataset.scene(s)
        gts = [(g, e) for g, e in enumerate(sc["gt"].get(im, [])) if e["obj_id"] == o]
        info = dataset.gt_info(s)[im] if gts else []
        valid = np.array([info[g]["visib_fract"] >= visib_gt_min for g, _ in gts], dtype=bool)
        if (s, im) not in depths:
            depths[(s, im)] = dataset.depth(s, im)
        obj = dataset.object(o)
        rows = kept.get((s, im, o), [])
        tab = dict(scene_id=s, im_id=im, obj_id=o, rows=rows, score=np.asarray(results["score"], dtype=np.float64)[rows],
                   gt_index=[g for g, _ in gts], gts=[e for _, e in gts], valid=valid, diameter=obj.diameter,
                   width=depths[(s, im)].shape[1])
        n_inst += len(gts)
        n_valid += int(valid.sum())
        tables.append(tab)
        groups.setdefault((o, sc["camera"][im]["K"].tobytes(), depths[(s, im)].shape), []).append(tab)
    t_err = 0.0
    for (o, _, shape), tabs in groups.items():
        obj = dataset.object(o)
        images = sorted({(t["scene_id"], t["im_id"]) for t in tabs})
        where = {k: n for n, k in enumerate(images)}
        K = dataset.scene(tabs[0]["scene_id"])["camera"][tabs[0]["im_id"]]["K"]
        Re, te, Rg, tg, idx = [], [], [], [], []
        for t in tabs:
            for j in t["rows"]:
                R, tt = bop.pose_from_bop(results["R"][j], results["t"][j], dataset.mesh_scale, obj.centre)
                for e in t["gts"]:
                    Re.append(R); te.append(tt); Rg.append(e["R"]); tg.append(e["t"]); idx.append(where[(t["scene_id"], t["im_id"])])
        t0 = time.perf_counter()
        err = bop.pose_errors(obj, np.stack([depths[k] for k in images]), np.asarray(idx, dtype=np.int64),
                              np.asarray(Re, dtype=np.float64).reshape(-1, 3, 3), np.asarray(te, dtype=np.float64).reshape(-1, 3),
                              np.asarray(Rg, dtype=np.float64).reshape(-1, 3, 3), np.asarray(tg, dtype=np.float64).reshape(-1, 3), K)
        t_err += time.perf_counter() - t0
        a = 0
        for t in tabs:
            n_est, n_gt = len(t["rows"]), len(t["gts"])
            n = n_est * n_gt
            t["vsd"] = err["vsd"][a:a + n].reshape(n_est, n_gt, err["vsd"].shape[1])
            t["mssd"] = err["mssd"][a:a + n].reshape(n_est, n_gt)
            t["mspd"] = err["mspd"][a:a + n].reshape(n_est, n_gt)
            a += n
    counts.update(targets=len(targets), gt_instances=n_inst, gt_valid=n_valid, pose_errors_s=t_err)
    return tables, counts


def score(dataset, results, targets=None, visib_gt_min=VISIB_GT_MIN):
    """The BOP'19 average recall of a results table (read_results) over a dataset: per object and overall AR_VSD, AR_MSSD,
    AR_MSPD, AR, the recall per threshold, and the counts behind them (report["counts"]: estimates, kept, not_a_target,
    over_inst_count, targets, gt_instances, gt_valid, and the wall times pose_errors_s / total_s).  Rules: the module's
    error_tables (1-3) and recall_report (3-5); DESIGN.md section 16 states them."""
    t0 = time.perf_counter()
    tables, counts = error_tables(dataset, results, targets, visib_gt_min)
    report = recall_report(tables)
    counts["total_s"] = time.perf_counter() - t0
    report["counts"] = counts
    report["visib_gt_min"] = float(visib_gt_min)
    return report
