"""TEST INFRASTRUCTURE of tests/test_gpu_lazy_panel.py and tests/test_lazy_panel_cpu.py: the worlds and open-loop scripts at which
a lazy restore's covariance panel reaches every form of the incremental update (csrc/k_inc.hip), built from tests/step_cases.py.

Open-loop scripts (the same numbers go to both engines, so nothing needs the oracle at run time): 'j' a small jiggle that
alternates its sign, 'g' the 2 m gate move, 'b' the same move backwards.  With the quiet vehicle of INC_TUNE the ground truth stays
within centimetres of the closed-loop scripts of step_cases.py; tests/test_lazy_panel_cpu.py proves the counts with the oracle.

After step s (from 0; the reset is step -1) an environment holds s + 2 poses.
"""
import numpy as np

import step_cases as S

JIG = (0.05, 0.0, 0.01)


def actions(script, n):
    """[len(script)][n][3]: the open-loop actions of a script, the same for every environment."""
    out, sign = [], 1.0
    for kind in script:
        if kind == "j":
            a = (sign * JIG[0], 0.0, sign * JIG[2])
            sign = -sign
        else:
            a = (S.GATE_MOVE if kind == "g" else -S.GATE_MOVE, 0.0, 0.0)
        out.append(np.array([a] * n, dtype=np.float64))
    return out


# A large gate (more than INEW first sightings: the gate step is a full solve) leaves a panel of 68 landmarks - too large for the
# LDS at any pose count - of which only the ring is in range from the centre: in-place updates with 8, 12 and 16 re-observed
# landmarks.  (48, 4): an in-place update that re-observes 48 (three batches) and first-sights 4 at its gate step.  (65, 0): nf = 65,
# inc_post refuses with the panel in place.  (52, 13): nn = 13 at the gate step, the same refusal after the first sightings' check.
INPLACE_RINGS = [(8, 60), (12, 56), (16, 52), (48, 4), (65, 0), (52, 13)]
INPLACE_SCRIPT = "jgbj"


def inplace_world():
    return S.World("inplace", INPLACE_RINGS, dict(max_poses=12, max_landmarks=78, max_factors=1024, max_actions=4), S.INC_TUNE)


def small_world():
    """step_cases.small_world (panels staged in LDS at short scripts) with room for a short script only."""
    return S.World("small", S.SMALL_RINGS, dict(max_poses=12, max_landmarks=63, max_factors=1024, max_actions=4), S.INC_TUNE)


def relin_world():
    """The default vehicle noise (no INC_TUNE): every new pose's delta crosses the relinearisation threshold (step_cases.py), so the
    10th update - step 8 - is a full solve that ends in panel_from_dense."""
    return S.World("relin", [(8, 0), (17, 0), (48, 0), (24, 0)], dict(max_poses=12, max_landmarks=60, max_factors=1024, max_actions=4))


RELIN_SCRIPT = "j" * 9  # the update of its last step is the 10th


def chain_world():
    """Beyond DENSE_MAX_POSES poses: the pose-chain kernels (L_max = 63: fused, k_step_arrow; the ring of 33 streams its panel)."""
    return S.World("chain", [(8, 0), (17, 0), (33, 0), (24, 0)], dict(max_poses=58, max_landmarks=63, max_factors=2048, max_actions=4), S.INC_TUNE)


CHAIN_SCRIPT = "j" * 54  # 55 poses before the step under test


def form(world, e, P, n_re, gate_seen):
    """step_cases.inc_form for the update that brings environment e to P poses."""
    size, gate = world.rings[e]
    L0 = size + (gate if gate_seen else 0)
    return S.inc_form(P, L0, n_re, world.num_landmarks, world.caps["max_poses"], world.caps["max_landmarks"])


# What the steps under test are claimed to be: {(world, ring, poses after the step): form}; asserted on the CPU.
FORMS = {
    ("inplace", 8, 5): "two-walk wide", ("inplace", 12, 5): "two-walk wide", ("inplace", 16, 5): "two-walk wide",
    ("inplace", 48, 3): "two-walk wide", ("inplace", 48, 5): "two-walk wide",
    ("small", 8, 3): "lds wide", ("small", 17, 3): "lds wide", ("small", 33, 3): "lds wide", ("small", 32, 3): "lds wide",
}
