"""CPU checks of the mesh-based ICP refinement (cppf2_amd/icp.py, cppf_icp_refine): the NumPy restatement of the kernel
(tests/icp_ref.py) recovers known poses of point sets sampled from the fixture mesh and stays at the true pose, the model
sampler, and the two new C entry points' argument checks (no GPU needed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_ref as IR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")


@pytest.fixture(scope="module")
def mesh():
    from cppf2_amd import render
    return render.load_mesh(FIXTURE, 0.001)


@pytest.fixture(scope="module")
def model(mesh):
    from cppf2_amd import icp
    return icp.ModelPoints.from_mesh(mesh)


def _rot(axis, deg):
    axis = np.asarray(axis, dtype=np.float64)
    return IR.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(deg))


def _err(R, t, Rg, tg):
    c = np.clip((np.trace(R.T @ Rg) - 1) / 2, -1, 1)
    return np.degrees(np.arccos(c)), np.linalg.norm(t - tg) * 1000          # degrees, mm


def _view(mesh, R, t, seed=1, count=3000):
    """Camera-frame points sampled from the mesh surface (other draws than the model's), those facing the camera."""
    from cppf2_amd import icp
    obs = icp.ModelPoints.from_mesh(mesh, count, seed)
    pc = obs.pts.astype(np.float64) @ R.T + t
    facing = np.einsum("ij,ij->i", obs.nrm.astype(np.float64) @ R.T, pc) < 0
    return pc[facing].astype(np.float32)


def test_model_points_from_mesh(mesh, model):
    from cppf2_amd import icp
    assert model.pts.shape == model.nrm.shape == (icp.COUNT, 3) and model.pts.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(model.nrm, axis=1), 1.0, atol=1e-6)
    b = mesh.bounds
    np.testing.assert_allclose(model.centre, (b[0] + b[1]) / 2)
    half = (b[1] - b[0]) / 2 + 1e-6
    assert np.all(np.abs(model.pts) <= half)
    again = icp.ModelPoints.from_mesh(mesh)
    assert again.pts.tobytes() == model.pts.tobytes() and again.nrm.tobytes() == model.nrm.tobytes()   # seeded
    assert icp.ModelPoints.from_mesh(mesh, seed=1).pts.tobytes() != model.pts.tobytes()


def test_schedule():
    d = IR.schedule(30, 0.05, 0.005)
    assert len(d) == 30 and d[0] == np.float32(0.05) and d[-1] == np.float32(0.005)
    assert all(a > b for a, b in zip(d, d[1:]))
    assert IR.schedule(1, 0.05, 0.005) == [np.float32(0.05)]


def test_restatement_recovers_known_poses(mesh, model):
    from cppf2_amd import icp
    rng = np.random.default_rng(5)
    Rg, tg = _rot([0.3, -1.0, 0.4], 130.0), np.array([0.05, -0.03, 0.8])
    pc = _view(mesh, Rg, tg)
    for _ in range(4):
        R0 = _rot(rng.standard_normal(3), rng.uniform(5, 10)) @ Rg
        d = rng.standard_normal(3)
        t0 = tg + d / np.linalg.norm(d) * rng.uniform(0.01, 0.02)
        R, t, st = IR.refine(pc, R0, t0, model.pts, model.nrm, icp.ITERS, *icp.MAX_DIST)
        rot, tr = _err(R, t, Rg, tg)
        assert rot < 0.5 and tr < 2.0, (rot, tr, _err(R0, t0, Rg, tg))
        assert st[3] == icp.ITERS and st[2] > 0.9 and st[1] < 1e-3
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)


def test_restatement_stays_at_the_true_pose(mesh, model):
    from cppf2_amd import icp
    Rg, tg = _rot([1.0, 0.2, -0.5], 40.0), np.array([-0.1, 0.05, 1.2])
    pc = _view(mesh, Rg, tg, seed=2)
    R, t, st = IR.refine(pc, Rg, tg, model.pts, model.nrm, icp.ITERS, *icp.MAX_DIST)
    rot, tr = _err(R, t, Rg, tg)
    assert rot < 0.1 and tr < 0.2, (rot, tr)
    assert st[2] > 0.95


def test_restatement_leaves_the_pose_without_enough_inliers(model):
    pc = np.array([[0.0, 0.0, 5.0]] * 5, dtype=np.float32)        # 5 points: fewer than 6 inliers whatever the distance
    R, t, cnt, rms, upd = IR.step(pc, np.eye(3), np.array([0.0, 0.0, 5.0]), model.pts, model.nrm, np.float32(1.0))
    assert not upd and cnt == 5 and np.array_equal(R, np.eye(3)) and np.array_equal(t, [0.0, 0.0, 5.0])


def _lib():
    from cppf2_amd import _lib as L
    return L.load()


def test_workspace_bytes():
    lib = _lib()
    assert lib.cppf_icp_workspace_bytes(1, 1) == 256
    assert lib.cppf_icp_workspace_bytes(64, 2000) == 64 * 8 * 256
    assert lib.cppf_icp_workspace_bytes(3, 257) == 3 * 2 * 256
    for B, n in ((0, 10), (-1, 10), (65536, 10), (1, 0), (1, -5)):
        assert lib.cppf_icp_workspace_bytes(B, n) == -1, (B, n)


_P = C.c_void_p(1 << 20)          # never dereferenced: every call below fails its argument checks before any launch


def _call(**kw):
    a = dict(B=2, pts=_P, pt_off=_P, max_n=100, model_pts=_P, model_nrm=_P, M=4096, iters=30, d0=0.05, d1=0.005, results=_P,
             stats=_P, workspace=_P, workspace_bytes=2 * 256)
    a.update(kw)
    lib = _lib()
    st = lib.cppf_icp_refine(a["B"], a["pts"], a["pt_off"], a["max_n"], a["model_pts"], a["model_nrm"], a["M"], a["iters"],
                             C.c_float(a["d0"]), C.c_float(a["d1"]), a["results"], a["stats"], a["workspace"],
                             a["workspace_bytes"], None)
    return st, lib.cppf_last_error_string()


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-3), dict(B=65536), dict(max_n=0), dict(M=0), dict(M=-1), dict(iters=0),
                                dict(iters=-2), dict(d1=0.0), dict(d1=-0.01), dict(d0=0.004), dict(d0=float("inf")),
                                dict(d0=float("nan")), dict(d1=float("nan")), dict(pts=None), dict(pt_off=None),
                                dict(model_pts=None), dict(model_nrm=None), dict(results=None), dict(stats=None),
                                dict(workspace=None)])
def test_refine_rejects_bad_arguments(kw):
    st, msg = _call(**kw)
    assert st == -1 and b"invalid argument" in msg, (kw, st, msg)


def test_refine_rejects_a_small_workspace():
    st, msg = _call(workspace_bytes=2 * 256 - 1)
    assert st == -4 and b"workspace" in msg, (st, msg)
    st, msg = _call(B=3, max_n=257, workspace_bytes=3 * 2 * 256 - 8)
    assert st == -4
