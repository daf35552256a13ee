"""TEST INFRASTRUCTURE of tests/test_gpu_restore_compact.py and tests/test_restore_compact_cpu.py: the worlds, open-loop scripts and
activity masks at which the compact restore (csrc/k_misc.hip: k_restore_compact) meets its edges, and a restatement of the engine's
table of per-instance fields (drlgx_engine.cpp: alloc_fields) with the generic copy kernel's live-byte formula.

Scripts are lazy_panel_cases' ('j' jiggle, 'g' the 2 m gate move, 'b' back); an environment is stepped only while its entry of
`steps_of` says so (the engine's `active` mask; None: every step), so that one engine holds instances of different counts.
After k executed steps an environment holds k + 1 poses.
"""
import numpy as np

import lazy_panel_cases as LP
import step_cases as S


class Case(object):
    def __init__(self, world, script, steps_of=None, **override):
        self.world, self.script, self.override = world, script, override
        self.steps_of = list(steps_of) if steps_of is not None else [len(script)] * world.n

    def active(self, s):
        """uint8 [n]: which environments execute step s."""
        return np.array([1 if s < k else 0 for k in self.steps_of], dtype=np.uint8)

    def engine_config(self, **kw):
        o = dict(self.override)
        o.update(kw)
        return self.world.engine_config(**o)

    def caps(self):
        c = dict(self.world.caps)
        c.update(self.override)
        return c


def mixed_case():
    """Env 0 starts a grid row away from every landmark and never moves: 1 pose, 0 landmarks, 0 factors.  Env 1 (ring of 1) never moves:
    L = 1, M = 1.  Envs 2 / 3 (rings of 3 / 5) take two steps: L = 3, M = 9 and L = 5, M = 15 - their 4-byte entries end 12 / 4 bytes
    off a 16-byte boundary.  max_landmarks = 10: those of the landmark entries whose stride is no multiple of 16 go as words."""
    w = S.World("mixed", [(1, 0), (1, 0), (3, 0), (5, 0)], dict(max_poses=8, max_landmarks=10, max_factors=64, max_actions=4), S.INC_TUNE)
    w.starts[0] = S._slot(0, 1)
    return Case(w, "jj", steps_of=[0, 0, 2, 2])


MIXED_COUNTS = [(1, 0, 0), (1, 1, 1), (3, 3, 9), (3, 5, 15)]


def wrap_case():
    """lazy_panel_cases.chain_world, 55 steps; env 0 stops after three.  max_factors = 2046 (stride 8184, no multiple of 16) sends the
    two 4-byte factor entries through the word loop: the ring of 33 then holds 2 x 1848 live words and over 2 048 16-byte items."""
    return Case(LP.chain_world(), "j" * 55, steps_of=[3, 55, 55, 55], max_factors=2046)


WRAP_COUNTS = [(4, 8, 32), (56, 17, 17 * 56), (56, 33, 33 * 56), (56, 24, 24 * 56)]


def capacity_case():
    """Ring 65 with its 12-gate: seven steps bring env 0 to P = max_poses = 8, L = max_landmarks = 77 and M = max_factors = 532."""
    w = S.World("capacity", [(65, 12), (8, 0)], dict(max_poses=8, max_landmarks=77, max_factors=532, max_actions=4), S.INC_TUNE)
    return Case(w, "jgbjjjj")


CAPACITY_COUNTS = [(8, 77, 532), (8, 8, 64)]


# ---- the engine's per-instance fields that a lazy restore copies (class 0 and 2): name, elements per instance, bytes per element,
# unit (0 the whole slice, 1 / 2 / 3 per pose / landmark / factor), elements per unit - alloc_fields restated
MT_STRIDE, CNT_STRIDE, RED_STRIDE, PRIOR_STRIDE = 626, 8, 8, 16


def fields(P, L, M, LG):
    return [("gt_pose", 4, 8, 0, 0), ("parent", 1, 4, 0, 0), ("mt", 2 * MT_STRIDE, 4, 0, 0), ("nrm_saved", 2, 8, 0, 0), ("nrm_has", 2, 4, 0, 0),
            ("cnt", CNT_STRIDE, 4, 0, 0), ("th_pose", 4 * P, 8, 1, 4), ("d_pose", 3 * P, 8, 1, 3), ("th_lm", 2 * L, 8, 2, 2),
            ("d_lm", 2 * L, 8, 2, 2), ("lm_key", L, 4, 2, 1), ("key_slot", LG, 4, 0, 0), ("prior", PRIOR_STRIDE, 8, 0, 0),
            ("odo", 4 * P, 8, 1, 4), ("meas_pose", M, 4, 3, 1), ("meas_lm", M, 4, 3, 1), ("meas_br", 2 * M, 8, 3, 2),
            ("est_pose", 4 * P, 8, 1, 4), ("est_lm", 2 * L, 8, 2, 2), ("pose_info", 6 * P, 8, 1, 6), ("lm_info", 3 * L, 8, 2, 3),
            ("pose_tr", P, 8, 1, 1), ("lm_tr", L, 8, 2, 1), ("red", RED_STRIDE, 8, 0, 0), ("gt_lm", 2 * LG, 8, 0, 0)]


def rows(caps, LG, panels=True):
    """[(name, stride, unit, unit_bytes)] of the compact restore's table, in no particular order; with panels, the pose marginals jd."""
    out = [(n, per * size, unit, per_unit * size) for n, per, size, unit, per_unit in fields(caps["max_poses"], caps["max_landmarks"], caps["max_factors"], LG)]
    if panels:
        out.append(("jd", caps["max_poses"] * 48, 4, 48))
    return out


def live_bytes(stride, unit, unit_bytes, count):
    """The generic copy kernel's arithmetic (k_copy_instances): a per-unit slice ends at the count, rounded up to 16 bytes, within the slice."""
    if unit == 0:
        return stride
    return min((max(count, 0) * unit_bytes + 15) // 16 * 16, stride)


def items(stride, live):
    """(16-byte items, 4-byte words) the slice is moved as: words when the stride does not keep every instance's slice 16-byte aligned."""
    return (0, live // 4) if stride % 16 else (live // 16, 0)


def count_of(unit, counts, panel_poses):
    return {0: 0, 1: counts[0], 2: counts[1], 3: counts[2], 4: panel_poses}[unit]


def instance_items(table_rows, counts, panel_poses):
    """(16-byte items, words) one instance's restore moves; table_rows: (stride, unit, unit_bytes) per entry."""
    q = w = 0
    for stride, unit, unit_bytes in table_rows:
        a, b = items(stride, live_bytes(stride, unit, unit_bytes, count_of(unit, counts, panel_poses)))
        q, w = q + a, w + b
    return q, w
