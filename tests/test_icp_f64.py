"""CPU checks of the independent float64 ICP reference (tests/icp_f64.py) and of the rank-aware solve the kernel and its
restatement (tests/icp_ref.py) share: known poses recovered on the fixture, the observable rank of degenerate models, steps
with no component along unobservable directions, and a plain linear solve on full-rank systems."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_f64 as F  # noqa: E402
import icp_ref as IR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
T0 = np.array([0.02, -0.01, 0.7])


def _err(R, t, Rg, tg):
    c = np.clip((np.trace(R.T @ Rg) - 1) / 2, -1, 1)
    return np.degrees(np.arccos(c)), np.linalg.norm(t - tg) * 1000


def _cloud(mp, Rg, facing=True, n=2000):
    p = mp.pts[:n].astype(np.float64) @ Rg.T + T0
    if facing:
        p = p[np.einsum("ij,ij->i", mp.nrm[:n].astype(np.float64) @ Rg.T, p) < 0]
    return p.astype(np.float32)


def test_reference_recovers_known_poses():
    from cppf2_amd import icp, render
    mesh = render.load_mesh(FIXTURE, 0.001)
    model = icp.ModelPoints.from_mesh(mesh)
    rng = np.random.default_rng(41)
    for k in range(2):
        Rg = F.random_rotation(rng)
        pc = _cloud(icp.ModelPoints.from_mesh(mesh, 3000, 7 + k), Rg, n=3000)
        ax = rng.standard_normal(3)
        R = Rg @ F.Rotation.from_rotvec(ax / np.linalg.norm(ax) * np.deg2rad(8)).as_matrix()
        t = T0 + rng.standard_normal(3) * 0.008
        for dk in IR.schedule(20, 0.05, 0.005):
            R, t, cnt, x, rank = F.step(pc, R, t, model.pts, model.nrm, dk)
            assert rank == 6
        rot, tr = _err(R, t, Rg, T0)
        assert rot < 0.5 and tr < 2.0, (rot, tr)


def _models():
    from cppf2_amd import icp
    return dict(plate=(icp.ModelPoints.from_mesh(F.plate(F.random_rotation(np.random.default_rng(1)))), 3),
                plate_exact=(icp.ModelPoints.from_mesh(F.plate()), 3),
                cylinder=(F.smooth(icp.ModelPoints.from_mesh(F.cylinder()), axis_only=True), 4),
                sphere=(F.smooth(icp.ModelPoints.from_mesh(F.sphere_cap(cap_deg=180.0))), 3),
                cylinder_facets=(icp.ModelPoints.from_mesh(F.cylinder()), 5))


@pytest.mark.parametrize("name", ["plate", "plate_exact", "cylinder", "sphere", "cylinder_facets"])
def test_rank_and_no_step_along_unobservable_directions(name):
    """Ranks 3 (plates), 4 (cylinder), 3 (sphere) with smooth normals; 5 for the 128-facet cylinder, whose facets constrain the
    spin.  The unobservable eigenvalues are rounding-level (< 1e-12 of the largest), the genuine ones above 1e-5, so TAU =
    1e-9 separates them; the step has no component along the dropped eigenvectors, and the restatement's Jacobi solve finds
    the same rank and step.  The start is 3 degrees and 3 mm off, except for the smooth cylinder and sphere: off the true pose
    the nearest sample's radial normal is not the point's, and the sampling then constrains the spin (about 6e-4)."""
    mp, want = _models()[name]
    rng = np.random.default_rng(42)
    Rg = F.random_rotation(rng)
    pc = _cloud(mp, Rg, facing=not name.startswith("plate"))
    R0 = Rg @ F.Rotation.from_rotvec(np.deg2rad([1.5, -2.0, 1.5])).as_matrix()
    t0 = T0 + np.array([0.002, -0.002, 0.001])
    if name in ("cylinder", "sphere"):
        R0, t0 = Rg, T0
    A, b, qq, inl, _ = F.normal_equations(pc, R0, t0, mp.pts, mp.nrm, 0.01)
    s = F.scale(qq, int(inl.sum()))
    x, rank, lam = F.min_norm_step(A, b, s)
    assert rank == want, lam / lam[-1]
    rel = lam / lam[-1]
    assert np.all(rel[:6 - rank] < 1e-12) and np.all(rel[6 - rank:] > 1e-5), rel
    _, V = np.linalg.eigh(s[:, None] * A * s[None, :])
    assert np.abs(V[:, :6 - rank].T @ (x / s)).max() <= 1e-12 * np.linalg.norm(x / s)
    xr, rr = IR._min_norm_solve(A, b, qq, float(inl.sum()))
    assert rr == rank and np.abs(xr - x).max() <= 1e-9 * max(1.0, np.abs(x).max()), (xr, x)
    if name.startswith("plate"):              # the physical null space, whatever the scaling: spin about n, in-plane slide
        n = mp.nrm.astype(np.float64).mean(0)
        n /= np.linalg.norm(n)
        tol = 1e-7 * np.linalg.norm(x)           # the float32 normals agree to ~1e-7
        assert abs(x[:3] @ n) <= tol and np.linalg.norm(x[3:] - (x[3:] @ n) * n) <= tol, x
    if name == "plate_exact":                 # exactly zero columns: the Jacobi solve never mixes them in, no step along them
        assert xr[2] == 0 and xr[3] == 0 and xr[4] == 0 and np.abs(x[2:5]).max() <= 1e-15


@pytest.mark.parametrize("name", ["plate", "plate_exact", "cylinder", "sphere"])
def test_restatement_stays_at_the_true_pose_of_degenerate_models(name):
    """The shared solve started at the truth: 30 iterations move the pose by less than 0.01 degrees and 0.01 mm (the Cholesky
    it replaced moved the turned plate by 1-6 degrees and 2-6 mm in one step)."""
    from cppf2_amd import icp
    mp, _ = _models()[name]
    Rg = F.random_rotation(np.random.default_rng(43))
    pc = _cloud(mp, Rg, facing=not name.startswith("plate"))
    R, t, st = IR.refine(pc, Rg, T0, mp.pts, mp.nrm, icp.ITERS, *icp.MAX_DIST)
    rot, tr = _err(R, t, Rg, T0)
    assert rot < 0.01 and tr < 0.01, (rot, tr)


def test_full_rank_step_is_a_plain_solve():
    rng = np.random.default_rng(44)
    for _ in range(20):
        J = rng.standard_normal((40, 6)) * rng.uniform(0.01, 10, 6)
        A, b = J.T @ J, rng.standard_normal(6)
        s = F.scale(float(rng.uniform(1e-4, 1.0)) * 40, 40)
        x, rank, _ = F.min_norm_step(A, b, s)
        want = np.linalg.solve(A, -b)
        assert rank == 6 and np.allclose(x, want, rtol=1e-9, atol=1e-12)
        xr, rr = IR._min_norm_solve(A, b, float(s[0]) ** -2 * 40, 40.0)
        assert rr == 6 and np.allclose(xr, want, rtol=1e-9, atol=1e-12)


def test_zero_matrix_has_rank_zero():
    x, rank, _ = F.min_norm_step(np.zeros((6, 6)), np.zeros(6), F.scale(1.0, 10))
    assert rank == 0 and not x.any()
    x, rank = IR._min_norm_solve(np.zeros((6, 6)), np.zeros(6), 1.0, 10.0)
    assert rank == 0 and not x.any()
