"""CPU checks of the independent float64 refinement reference (tests/refine_f64.py) and of everything the kernel-level GPU
tests (tests/test_refine_edges_gpu.py) take for granted before they touch the GPU: the three preconditions of every step
case, the float32 oracle's distance to the reference (which sets the GPU bars), and that the single element of the
one-element scenes does decide."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_f64 as F  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402

# The oracle's distance to the reference on the step cases, measured: at most 1.8e-7 in t (4500 pairs, 2 steps) and 6.0e-7
# in R (128 pairs, 3 steps, all coordinates; 2.6e-7 elsewhere).  The caps keep the GPU bars (4 x the distance) at or below
# 2e-6 and 4e-6, 32 ulp of a float32 at 0.9 and at 1.0: an oracle further off than that is a finding, not a wider bar.
E_T_CAP, E_R_CAP = 5e-7, 1e-6


def test_zero_steps_return_the_float32_rounded_start():
    pc, idx2, tgt, _, _ = F.banded_scene(33, 0)
    R0, t0 = F.off_grid_start()
    assert np.any(R0 != R0.astype(np.float32)) and np.any(t0 != t0.astype(np.float32))
    for y_only in (False, True):
        t, R, min_res, min_g = F.refine_f64(pc, idx2, tgt, t0, R0, y_only, 0, return_margins=True)
        assert np.array_equal(t, t0.astype(np.float32).astype(np.float64))
        assert np.array_equal(R, R0.astype(np.float32).astype(np.float64))
        assert min_res == np.inf and min_g == np.inf
    moved = R0.astype(np.float32) != F.start_pose()[0].astype(np.float32)           # 1e-9 is more than half an ulp below 2^-5
    assert moved.any() and np.all(np.abs(R0[moved]) < 2.0 ** -5) and not moved.all()


def test_so3_matrix_is_the_unnormalised_formula():
    q = np.array([0.1, -0.2, 0.3, 0.9])
    M = F.so3_matrix_f64(q).numpy()
    assert np.abs(M - O.so3_matrix(q)).max() < 1e-6                                 # the oracle's float32 statement of it
    assert np.abs(M @ M.T - np.eye(3)).max() > 1e-2                                 # |q| = 0.97: not a rotation
    qn = q / np.linalg.norm(q)
    Mn = F.so3_matrix_f64(qn).numpy()
    assert np.abs(Mn @ Mn.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(Mn) - 1) < 1e-15


@pytest.mark.parametrize("y_only", [False, True])
def test_the_first_step_moves_every_parameter_by_lr_against_its_gradient(y_only):
    """Adam's first update is lr g / (|g| + eps): its size says nothing about the gradient's, which is why the GPU cases
    that can see a missing pair run two steps or more."""
    pc, idx2, tgt, R0, t0 = F.banded_scene(129, 0)
    lr = 1e-2
    t, R, _, g = F.refine_f64(pc, idx2, tgt, t0, R0, y_only, 1, lr, return_components=True)
    step = lr * g / (g + 1e-8)
    assert np.allclose(np.abs(t - t0), step[:3], rtol=0, atol=1e-12)
    q = np.zeros(4)
    q[3] = 1
    found = False
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                q[:3] = np.array([sx, sy, sz]) * step[3:]
                found |= np.abs(F.so3_matrix_f64(q).numpy() @ R0 - R).max() < 1e-12
    assert found


@pytest.mark.parametrize("case", F.STEP_CASES, ids=F.case_id)
def test_step_cases_meet_their_preconditions_and_the_oracle_agrees(case):
    c = F.step_case(*case, O.refine_pose)                            # asserts the three preconditions
    assert c["e_t"] <= E_T_CAP and c["e_R"] <= E_R_CAP, (c["e_t"], c["e_R"])
    assert c["bar_t"] == 4 * max(c["e_t"], 2.5e-7) and c["bar_R"] == 4 * max(c["e_R"], 5e-7)
    t, R, min_res, min_g = F.refine_f64(c["pc"], c["idx2"], c["tgt"], c["t0"], c["R0"], case[2], case[1], case[4],
                                        return_margins=True)
    assert np.array_equal(t, c["t"]) and np.array_equal(R, c["R"])
    assert min_res == c["min_res"] and min_g == c["g"].min()
    assert np.abs(t - c["t0"]).max() > 100 * c["bar_t"]             # it moved: the start pose is nowhere near the bar


@pytest.mark.parametrize("case", F.OFF_GRID_CASES, ids=F.case_id)
def test_off_grid_start_cases_meet_their_preconditions(case):
    c = F.step_case(*case, O.refine_pose, start=F.off_grid_start())
    assert c["e_t"] <= E_T_CAP and c["e_R"] <= E_R_CAP, (c["e_t"], c["e_R"])
    on_grid = F.step_case(*case, O.refine_pose)
    assert np.abs(c["R"] - on_grid["R"]).max() > 0                  # the rounded-up entries of R0 are seen


def test_the_case_list_is_the_one_the_kernel_needs():
    small, big = (1, 2, 32, 33, 128, 129), (2047, 2048, 2049, 2176, 2177, 4500)
    got = {c[:3] for c in F.STEP_CASES if c[4] == 1e-2}
    want = {(k, s, y) for k in small for s in (1, 2, 3, 4) for y in (False, True)}
    want |= {(k, s, y) for k in big for s in (1, 2) for y in (False, True)}
    assert got == want and len(F.STEP_CASES) == len(want) + 2
    assert {c[2] for c in F.STEP_CASES if c[4] == 3e-3} == {False, True}


@pytest.mark.parametrize("y_only", [False, True], ids=["xyz", "y"])
@pytest.mark.parametrize("e_star", F.DECISIVE_POSITIONS)
def test_one_element_decides(e_star, y_only):
    pc, idx2, tgt, mask = F.decisive_scene(e_star)
    assert idx2.size == F.DECISIVE_NE and (idx2 == F.N_POINTS).sum() == 1 and pc[F.N_POINTS, 0] == 50
    assert np.abs(pc[:F.N_POINTS]).max() < 0.1
    R0, t0 = np.eye(3), np.zeros(3)
    t_w, R_w, res_w, _ = F.refine_f64(pc, idx2, tgt, t0, R0, y_only, 1, return_margins=True)
    t_o, R_o = F.refine_f64(pc, idx2, tgt, t0, R0, y_only, 1, mask=mask)
    assert res_w >= 0.0099                                            # float32 targets: 1 cm less their rounding at 50 m
    assert np.abs(R_w - R_o).max() > 1e-2, np.abs(R_w - R_o).max()
    assert np.array_equal(t_w, t_o) or np.abs(t_w - t_o).max() < 1e-9   # the translation's signs do not hang on it
