"""A mesh's rotational symmetries, found on the GPU: what bop.ObjectInfo.from_mesh takes from a BOP
models_info.json entry and what `--sym-axis` of pair_table / render.make_items asks the user for.  The reference has no such step.

    info = detect(render.load_mesh("obj.ply", 0.001))              # dict in models_info form, in the file's units
    obj = bop.ObjectInfo.from_mesh(mesh, models_info=info)
    python -m cppf2_amd.symmetry --mesh obj.ply --mesh-scale 0.001 --obj-id 15 --out models_info.json
    python -m cppf2_amd.symmetry --bop-models <dataset>/models --out models_info.json

The statistic is cppf_sym_deviation (include/cppf_hip_experimental.h): the largest distance of a surface sample, taken through a candidate
map, to the triangle mesh -- exact point-to-triangle distances, so a true symmetry scores at rounding level whatever the sampling.
A candidate is a symmetry when that deviation is at most tol x diameter.  Rotations only (BOP's sets), about lines through the
surface centroid along the principal axes of the surface's second moments; the polyhedral groups of objects whose three moments
agree are out of scope (report["isotropic"]).
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import _lib, bop

TOL = 0.01                       # a symmetry deviates by at most TOL x diameter (DESIGN.md section 26 has the measurements)
COUNT = 2048                     # surface samples
MAX_ORDER = 12                   # rotations by 2 pi / n, n = 2 .. MAX_ORDER
PROBES = 31                      # a continuous axis passes every rotation by 2 pi i / PROBES, i = 1 .. PROBES // 2
AZIMUTHS = 180                   # half-turns about the axes perpendicular to a principal axis, one per degree of azimuth
REFINE_SPAN, REFINE_STEP = 1.0, 0.05     # degrees: the second scan around the best azimuth of a run
DUPLICATE_DEG = 0.5              # transforms closer than this (relative rotation) are one
ISOTROPIC_RTOL = 1e-3            # three second moments within this share of the largest: the principal axes are arbitrary
AXIS_DEG = 1.0                   # --sym-axis auto: a continuous axis this close to a coordinate axis is that axis
MAX_MAPS = 65535                 # maps per kernel call


def deviations(queries, tris, maps):
    """cppf_sym_deviation: float32 [C] device tensor, the deviation (metres: the square root is taken here) of the queries
    float32 [Nq,3] from the triangles float32 [F,9] under each of the maps float64 [C,12] or [C,3,4]."""
    import torch
    from . import hostargs, ops
    dev = ops._dev()
    q = hostargs.tensor(queries, torch.float32, dev).reshape(-1, 3)
    t = hostargs.tensor(tris, torch.float32, dev).reshape(-1, 9)
    m = hostargs.tensor(maps, torch.float64, dev).reshape(-1, 12)
    C_ = m.shape[0]
    out = torch.empty((C_,), dtype=torch.float32, device=dev)
    L = _lib.load()
    for a in range(0, max(C_, 1), MAX_MAPS):
        n = min(MAX_MAPS, C_ - a)
        _lib.check(L.cppf_sym_deviation(ops._p(q), q.shape[0], ops._p(t), t.shape[0], ops._p(m[a:]), n, ops._p(out[a:]),
                                        ops._stream()), "cppf_sym_deviation")
    return torch.sqrt(out)


def _device_deviations(queries, tris, maps):
    return deviations(queries, tris, maps).cpu().numpy().astype(np.float64)


def surface_frame(verts, faces):
    """(centroid float64 [3], eigenvalues ascending [3], axes [3,3] (columns), triangles float64 [F',3,3] without the zero-area
    ones, their areas): the area-weighted centroid of the surface and the principal axes of its second moments, both in closed
    form per triangle: int x dA = A (a + b + c) / 3, int x x^T dA = A (s s^T + a a^T + b b^T + c c^T) / 12 with s = a + b + c."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tri = v[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    tri, area = tri[area > 0], area[area > 0]
    if not len(tri):
        raise ValueError("symmetry: the mesh has no triangle of non-zero area")
    total = area.sum()
    c = (area[:, None] * tri.sum(1)).sum(0) / (3.0 * total)
    t = tri - c
    s = t.sum(1)
    S = (np.einsum("f,fi,fj->ij", area, s, s) + np.einsum("f,fki,fkj->ij", area, t, t)) / (12.0 * total)
    w, E = np.linalg.eigh(S)
    return c, w, E, tri, area


def sample_surface(tri, area, count, seed):
    """float64 [count,3]: area-weighted points on the triangles, drawn as icp.ModelPoints.from_mesh draws them (numpy
    Generator(seed): the triangles, then the two barycentric uniforms)."""
    rng = np.random.default_rng(seed)
    k = rng.choice(len(tri), size=int(count), p=area / area.sum())
    r1, r2 = rng.random(int(count)), rng.random(int(count))
    s = np.sqrt(r1)
    return (1.0 - s)[:, None] * tri[k, 0] + (s * (1.0 - r2))[:, None] * tri[k, 1] + (s * r2)[:, None] * tri[k, 2]


def _rot_maps(rots):
    """float64 [C,12]: rotations [C,3,3] about the origin as 3x4 maps."""
    R = np.asarray(rots, dtype=np.float64).reshape(-1, 3, 3)
    return np.concatenate([R, np.zeros((len(R), 3, 1))], 2).reshape(-1, 12)


def _perp_axis(E, k, az_deg):
    u, v = E[:, (k + 1) % 3], E[:, (k + 2) % 3]
    a = np.deg2rad(az_deg)
    return np.cos(a) * u + np.sin(a) * v


def _angle_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))


def _runs(ok):
    """The contiguous runs of a circular boolean list, as lists of indices (one run of everything when all are set)."""
    n = len(ok)
    if all(ok):
        return [list(range(n))]
    start = next(i for i in range(n) if not ok[i])
    runs, cur = [], []
    for j in range(1, n + 1):
        i = (start + j) % n
        if ok[i]:
            cur.append(i)
        elif cur:
            runs.append(cur)
            cur = []
    return runs


def detect(mesh, count=COUNT, seed=0, tol=TOL, max_order=MAX_ORDER, _deviations=None):
    """The rotational symmetries of a render.Mesh (in metres, mesh.scale = file units -> metres) as a BOP models_info entry in
    the model file's units: dict(diameter, min_x .. size_z, symmetries_discrete: [16 floats (row-major 4x4)] per transform,
    symmetries_continuous: [dict(axis, offset)], report).  bop.symmetry_transforms(info, mesh.scale, centre) expands it.
    Deterministic for a given seed.  report: dict(accepted: deviation / diameter of each discrete transform, in order,
    continuous: the same of each continuous axis (its worst probe), smallest_rejected: of the best candidate that was refused
    (None when none was), isotropic, candidates: maps scored, tol, count, seed)."""
    dev_fn = _device_deviations if _deviations is None else _deviations
    scale = float(mesh.scale)
    c, w, E, tri, area = surface_frame(mesh.verts, mesh.faces)
    diam = bop.diameter(mesh.verts)
    if not diam > 0:
        raise ValueError("symmetry: the mesh has no extent")
    thr = float(tol) * diam
    queries = (sample_surface(tri, area, count, seed) - c).astype(np.float32)
    tris = (tri - c).reshape(-1, 9).astype(np.float32)
    isotropic = bool(w[2] - w[0] <= ISOTROPIC_RTOL * w[2])
    orders = list(range(2, int(max_order) + 1))
    half = PROBES // 2

    # first call: per principal axis the rotations 2 pi / n, the probes 2 pi i / PROBES and the perpendicular half-turns
    rots = []
    for k in range(3):
        rots += [bop._axis_rotation(E[:, k], 2.0 * np.pi / n) for n in orders]
        rots += [bop._axis_rotation(E[:, k], 2.0 * np.pi * i / PROBES) for i in range(1, half + 1)]
        rots += [bop._axis_rotation(_perp_axis(E, k, az), np.pi) for az in range(AZIMUTHS)]
    rots = np.stack(rots)
    dev1 = np.asarray(dev_fn(queries, tris, _rot_maps(rots)), dtype=np.float64)
    per = len(orders) + half + AZIMUTHS
    n_cand = len(rots)
    # Two second moments that agree leave their two axes arbitrary in their plane; every rotation of such an object (not an
    # isotropic one) is about the third axis or a half-turn across it, so only that axis' candidates are read.
    close = lambda i, j: abs(w[i] - w[j]) <= ISOTROPIC_RTOL * w[2]
    active = [k for k in range(3) if isotropic or not (close(k, (k + 1) % 3) or close(k, (k + 2) % 3))]
    split = lambda k: np.split(dev1[k * per:(k + 1) * per], [len(orders), len(orders) + half])
    rejected = []                       # deviations of refused candidates: rotations, probes, local minima of the azimuth scans
    for k in active:
        d_n, d_p, d_h = split(k)
        rejected += [float(x) for x in np.concatenate([d_n, d_p]) if not x <= thr]
        rejected += [float(d_h[i]) for i in range(AZIMUTHS)
                     if not d_h[i] <= thr and d_h[i] <= d_h[i - 1] and d_h[i] <= d_h[(i + 1) % AZIMUTHS]]

    continuous, found = [], []          # found: (R, deviation) of discrete candidates, de-duplicated at the end
    second, pending = [], []            # the second call's rotations and what each answers: a power, or a step of a run
    cont_axes = [k for k in active if (split(k)[1] <= thr).all()]
    if cont_axes:
        # a continuous axis leaves only the half-turn across it: every other discrete symmetry is one of its rotations times that
        for k in cont_axes:
            _, d_p, d_h = split(k)
            continuous.append((E[:, k].copy(), float(d_p.max())))
            if d_h[0] <= thr:
                found.append((bop._axis_rotation(_perp_axis(E, k, 0.0), np.pi), float(d_h[0])))
    else:
        steps = int(round(REFINE_SPAN / REFINE_STEP))
        for k in active:
            d_n, _, d_h = split(k)
            passing = [n for n, dn in zip(orders, d_n) if dn <= thr]
            if passing:
                n = max(passing)
                for j in range(1, n):
                    second.append(bop._axis_rotation(E[:, k], 2.0 * np.pi * j / n))
                    pending.append(("power", None))
            for run in _runs([bool(x <= thr) for x in d_h]):
                best = min(run, key=lambda i: (d_h[i], i))
                for s in range(-steps, steps + 1):
                    second.append(bop._axis_rotation(_perp_axis(E, k, best + s * REFINE_STEP), np.pi))
                    pending.append(("run", (k, best)))
        if second:
            dev2 = np.asarray(dev_fn(queries, tris, _rot_maps(np.stack(second))), dtype=np.float64)
            n_cand += len(second)
            best_of = {}
            for R, (kind, rid), dv in zip(second, pending, dev2):
                if kind == "power":
                    if dv <= thr:
                        found.append((R, float(dv)))
                    else:
                        rejected.append(float(dv))
                elif rid not in best_of or dv < best_of[rid][1]:
                    best_of[rid] = (R, float(dv))
            found += [(R, dv) for R, dv in best_of.values() if dv <= thr]

    kept = []
    for R, dv in found:
        if _angle_deg(np.eye(3), R) < DUPLICATE_DEG:
            continue                                        # never the identity
        twin = next((i for i, (Rk, _) in enumerate(kept) if _angle_deg(Rk, R) < DUPLICATE_DEG), None)
        if twin is None:
            kept.append((R, dv))
        elif dv < kept[twin][1]:
            kept[twin] = (R, dv)

    cf = c / scale                                          # the centroid in the file's units
    discrete = []
    for R, _ in kept:
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = cf - R @ cf
        discrete.append([float(x) for x in T.reshape(16)])
    b = mesh.bounds / scale
    info = dict(diameter=float(diam / scale),
                min_x=float(b[0, 0]), min_y=float(b[0, 1]), min_z=float(b[0, 2]),
                size_x=float(b[1, 0] - b[0, 0]), size_y=float(b[1, 1] - b[0, 1]), size_z=float(b[1, 2] - b[0, 2]))
    if discrete:
        info["symmetries_discrete"] = discrete
    if continuous:
        info["symmetries_continuous"] = [dict(axis=[float(x) for x in a], offset=[float(x) for x in cf]) for a, _ in continuous]
    info["report"] = dict(accepted=[float(dv / diam) for _, dv in kept], continuous=[float(wst / diam) for _, wst in continuous],
                          smallest_rejected=float(min(rejected) / diam) if rejected else None, isotropic=isotropic,
                          candidates=int(n_cand), tol=float(tol), count=int(count), seed=int(seed))
    return info


def summary(info):
    """What eval.py reports of a detected entry: counts, continuous axes, the largest accepted deviation (over the diameter)."""
    rep = info.get("report", {})
    acc = list(rep.get("accepted", [])) + list(rep.get("continuous", []))
    return dict(discrete=len(info.get("symmetries_discrete", [])), continuous=len(info.get("symmetries_continuous", [])),
                continuous_axes=[s["axis"] for s in info.get("symmetries_continuous", [])],
                largest_accepted=max(acc) if acc else None, smallest_rejected=rep.get("smallest_rejected"),
                isotropic=bool(rep.get("isotropic", False)), tol=rep.get("tol"))


def coordinate_axis(info, tol=TOL):
    """--sym-axis auto: the coordinate axis k (0, 1, 2) that a detected continuous axis of the entry `info` is -- within AXIS_DEG
    of it and passing within tol x diameter of the bounding-box centre, the point map_sym's canonical frame turns about.
    ValueError naming what was detected otherwise.  A pure function of the entry."""
    cont = info.get("symmetries_continuous", [])
    if not cont:
        raise ValueError("--sym-axis auto: no continuous symmetry axis was detected (%d discrete transforms)"
                         % len(info.get("symmetries_discrete", [])))
    centre = np.array([info["min_" + a] + 0.5 * info["size_" + a] for a in "xyz"], dtype=np.float64)
    why = []
    for s in cont:
        a = np.asarray(s["axis"], dtype=np.float64)
        a = a / np.linalg.norm(a)
        o = np.asarray(s.get("offset", (0.0, 0.0, 0.0)), dtype=np.float64)
        k = int(np.argmax(np.abs(a)))
        ang = float(np.degrees(np.arccos(min(1.0, abs(a[k])))))
        r = centre - o
        dist = float(np.linalg.norm(r - (r @ a) * a))
        if ang <= AXIS_DEG and dist <= float(tol) * float(info["diameter"]):
            return k
        why.append("axis (%.4f, %.4f, %.4f) through (%.4g, %.4g, %.4g): %.2f deg from coordinate axis %d, %.3g x diameter from "
                   "the bounding-box centre" % (a[0], a[1], a[2], o[0], o[1], o[2], ang, k, dist / float(info["diameter"])))
    raise ValueError("--sym-axis auto: the detected continuous axis is not a coordinate axis through the bounding-box centre "
                     "(within %g deg and %g x diameter): %s" % (AXIS_DEG, float(tol), "; ".join(why)))


def write_models_info(path, entries):
    """A models_info.json: {"<obj id>": entry} for the dict `entries` (int id -> detect's entry), ids ascending."""
    with open(path, "w") as f:
        json.dump({str(int(k)): entries[k] for k in sorted(entries, key=int)}, f, indent=2)
        f.write("\n")


def main(argv=None):
    import argparse
    from . import render
    ap = argparse.ArgumentParser(description="Detect meshes' rotational symmetries into a BOP models_info.json (DESIGN.md section 26)")
    ap.add_argument("--mesh")
    ap.add_argument("--mesh-scale", type=float, default=None, help="mesh units -> metres (default: 1 with --mesh, 0.001 with --bop-models)")
    ap.add_argument("--obj-id", type=int, default=1, help="the key of --mesh's entry")
    ap.add_argument("--bop-models", help="a BOP dataset's models directory: one entry per obj_%%06d.ply")
    ap.add_argument("--out", required=True, help="the models_info.json to write")
    ap.add_argument("--count", type=int, default=COUNT)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tol", type=float, default=TOL, help="a symmetry deviates by at most tol x diameter")
    a = ap.parse_args(argv)
    if bool(a.mesh) == bool(a.bop_models):
        ap.error("give --mesh or --bop-models")
    if a.mesh:
        jobs = [(int(a.obj_id), a.mesh)]
    else:
        names = sorted(n for n in os.listdir(a.bop_models) if n.startswith("obj_") and n.endswith(".ply"))
        if not names:
            ap.error("no obj_*.ply under %s" % a.bop_models)
        jobs = [(int(n[4:-4]), os.path.join(a.bop_models, n)) for n in names]
    scale = a.mesh_scale if a.mesh_scale is not None else (1.0 if a.mesh else 0.001)
    entries = {}
    for oid, path in jobs:
        entries[oid] = info = detect(render.load_mesh(path, scale), a.count, a.seed, a.tol)
        s = summary(info)
        print("%s: %d discrete, %d continuous, largest accepted %s, smallest rejected %s x diameter%s"
              % (os.path.basename(path), s["discrete"], s["continuous"], s["largest_accepted"], s["smallest_rejected"],
                 " (isotropic: the scan's findings only)" if s["isotropic"] else ""))
    write_models_info(a.out, entries)


if __name__ == "__main__":
    main()
