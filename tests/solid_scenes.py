"""The two scenes of DESIGN.md section 25, built with the rasteriser's NumPy mirror (tests/render_ref.py) on the tilted table of
tests/test_scene_gpu.py and decided by the restatement alone (tests/solid_ref.py, tests/scene_ref.py).  Everything here is CPU
work; tests/test_solid.py holds the decisions, tests/test_solid_gpu.py holds the GPU path to them.

S1: the fixture object rests on the table.  Candidate 0 (A) is the truth moved 1.5 cm into the table along the plane's normal,
candidate 1 (B) the truth moved 1.8 cm along the table.  S2: two cubes of 8 cm stand on the table, one behind the other; beside
and behind the front cube the camera sees a small patch that belongs to nothing.  Candidate 0 is the front cube, candidate 1 a
cube pose moved 2.5 cm sideways and 2.5 cm back, whose protruding faces are that patch and whose body is inside the front cube,
candidate 2 the cube behind."""
import numpy as np

import bop_data_ref as DR
import render_ref as RR
import scene_ref as SC
import segment_ref as SR
import solid_ref as SO

F = np.float32
PHI = np.deg2rad(55.0)
TABLE_N = np.array([0.0, -np.cos(PHI), -np.sin(PHI)])
TABLE_C = np.array([0.0, 0.10, 0.85])
EX, DS = np.array([1.0, 0, 0]), np.array([0.0, -np.sin(PHI), np.cos(PHI)])      # along the table: sideways, away from the camera
PLANE = np.concatenate([TABLE_N, [-TABLE_N @ TABLE_C]]).astype(F)                 # (n, d): unit n, d > 0, the camera above
KMAT = np.array([DR.K[0, 0], DR.K[1, 1], DR.K[0, 2], DR.K[1, 2]], F)
SCALE = 10000.0              # depth units per metre of the scenes' PNGs
CUBE = 0.04                  # half the cubes' edge


def rotx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


RT = rotx(np.pi / 2 + PHI)   # the model's z axis along the table's normal


def centred(verts):
    return verts - (verts.min(0) + verts.max(0)) / 2


def stand(verts, R, u, v):
    """The translation that puts the lowest vertex of R verts on the table top, u sideways and v away from the table's centre."""
    return TABLE_C + u * EX + v * DS - (verts @ R.T @ TABLE_N).min() * TABLE_N


def both(verts, faces, R, t):
    """(f, b): the renders of one pose with back faces culled and with the winding reversed."""
    pose = RR.look_pose(R, t)
    return (RR.render(verts, faces, pose, DR.K, DR.H, DR.W)[0], RR.render(verts, SO.reversed_faces(faces), pose, DR.K, DR.H, DR.W)[0])


def quantised(depth):
    """What a 16-bit PNG at SCALE units per metre gives back."""
    return (np.round(depth * SCALE).astype(np.uint16).astype(np.float64) / SCALE).astype(F)


def records(cands):
    from cppf2_amd.pipeline import RESULT_DTYPE
    recs = np.zeros(len(cands), dtype=RESULT_DTYPE)
    for r_, (R, t) in zip(recs, cands):
        r_["R"], r_["t"] = np.asarray(R, np.float64).reshape(r_["R"].shape), t
    return recs


def _background():
    table, wall = DR.box((0.6, 0.5, 0.01)), DR.box((1.5, 1.2, 0.01))
    return [(centred(table[0]), table[1], RT, TABLE_C - 0.01 * TABLE_N), (centred(wall[0]), wall[1], np.eye(3), np.array([0.0, 0.0, 1.6]))]


def _decide(s, min_gain, conflict_tau, max_overlap, max_sunk, support_tau):
    """The restatement's decisions on a scene dict (d, region, f, b): without any check, with the support check, with both."""
    from cppf2_amd import scene
    C = len(s["f"])
    s["support"] = SO.support(s["f"], s["b"], [0, C], PLANE, KMAT, support_tau)
    s["share"] = SO.sunk_share(s["support"])
    s["inter"] = SO.overlap(s["f"], s["b"], [0, C], conflict_tau)
    s["conflict"] = SO.conflicts(s["inter"], max_overlap)
    none = np.zeros((C, C), bool)
    args = (scene.TAU, min_gain, scene.VIOL_WEIGHT, scene.MAX_ROUNDS)
    s["plain"] = SO.greedy_loop(s["d"], s["region"], s["f"], *args, none)
    alive = np.flatnonzero(~(s["share"] > max_sunk))
    kept = SO.greedy_loop(s["d"], s["region"], s["f"][alive], *args, none)
    s["supported"] = ([int(alive[c]) for c in kept[0]],) + kept[1:]
    s["solid"] = SO.greedy_loop(s["d"], s["region"], s["f"], *args, s["conflict"])
    return s


def scene1():
    from cppf2_amd import render, scene, solid
    fixture = render.load_mesh(DR.FIXTURE, 0.001)
    fv = centred(fixture.verts)
    R = RT @ rotz(0.7)
    t = stand(fv, R, -0.05, 0.0)
    truth = both(fv, fixture.faces, R, t)
    bg = np.stack([RR.render(v, f_, RR.look_pose(R_, t_), DR.K, DR.H, DR.W)[0] for v, f_, R_, t_ in _background()])
    ren = np.concatenate([truth[0][None], bg])
    d = quantised(np.where(ren > 0, ren, np.inf).min(0))
    owner = np.where(ren > 0, ren, np.inf).argmin(0)
    cands = [(R, t - 0.015 * TABLE_N), (R, t + 0.018 * EX)]
    fb = [both(fv, fixture.faces, R_, t_) for R_, t_ in cands]
    ref = SR.propose(d, DR.K, 0)
    s = dict(d=d, owner=owner, region=(ref["masks"] > 0).any(0), ref=ref, f=np.stack([x[0] for x in fb]), b=np.stack([x[1] for x in fb]),
             recs=records(cands), truth=(R, t), truth_fb=truth, mesh=fixture, mesh_path=DR.FIXTURE, mesh_scale=0.001)
    s["truth_support"] = SO.support(truth[0][None], truth[1][None], [0, 1], PLANE, KMAT, solid.SUPPORT_TAU)
    return _decide(s, scene.MIN_GAIN, solid.OVERLAP_TAU, solid.MAX_OVERLAP, solid.MAX_SUNK, solid.SUPPORT_TAU)


def scene2():
    from cppf2_amd import render, scene, solid
    cv, cf = RR.cube(CUBE)
    Ra, Rb = RT @ rotz(0.35), RT @ rotz(0.35)
    ta, tb = stand(cv, Ra, 0.0, -0.04), stand(cv, Rb, -0.03, 0.10)
    # the phantom: the front cube's pose moved along its own edges, 2.5 cm sideways and 2.5 cm back
    tp = ta + Ra @ np.array([0.025, 0.025, 0.0])
    cands = [(Ra, ta), (Ra, tp), (Rb, tb)]
    fb = [both(cv, cf, R_, t_) for R_, t_ in cands]
    bg = np.stack([RR.render(v, f_, RR.look_pose(R_, t_), DR.K, DR.H, DR.W)[0] for v, f_, R_, t_ in _background()])
    ren = np.concatenate([fb[0][0][None], fb[2][0][None], bg])
    near = np.where(ren > 0, ren, np.inf).min(0)
    owner = np.where(ren > 0, ren, np.inf).argmin(0)
    # the patch: what the phantom shows in front of everything else, outside the front cube's outline
    patch = (fb[1][0] > 0) & (fb[1][0] < near) & ~(fb[0][0] > 0)
    d = quantised(np.where(patch, fb[1][0], near))
    ref = SR.propose(d, DR.K, 0)
    s = dict(d=d, owner=owner, patch=patch, region=(ref["masks"] > 0).any(0), ref=ref, f=np.stack([x[0] for x in fb]),
             b=np.stack([x[1] for x in fb]), recs=records(cands), mesh=render.Mesh(cv, cf), cube=(cv, cf))
    return _decide(s, scene.MIN_GAIN, solid.OVERLAP_TAU, solid.MAX_OVERLAP, solid.MAX_SUNK, solid.SUPPORT_TAU)
