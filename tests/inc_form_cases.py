"""TEST INFRASTRUCTURE: worlds that put an incremental (rank-k) belief update (csrc/k_inc.hip) into the forms no other world of the
suite reaches - the panel in LDS or in place with NARROW batches (the second half of Y misses the LDS), two and three narrow batches,
a streamed update whose first walk is short because the Y image is large, streamed updates whose plan affords one or two factor tiles
per walk only, and a plan that misses the LDS altogether - shared by tests/test_inc_form_cases_cpu.py (which proves on the CPU, with
the oracle alone, that every case is what it claims) and tests/test_gpu_inc_forms.py (which runs them on the device).

Built from the World machinery of tests/step_cases.py: listed landmarks, environments closed-loop on the oracle's ground truth, the
quiet vehicle of INC_TUNE.  A step on the incremental path adds at most INF = 64 factors and INEW = 12 first sightings, while the
panel's L0 counts every landmark ever seen - so a case is a ring of r landmarks around the start (all of them in range at every
pose: n_re = r) and a GATE FIELD of g landmarks ahead of it that is seen ONCE: the script is 'g' (2 m forwards: ring and field in
range, r + g factors > 64 or g > 12 first sightings - a full solve, which leaves a panel of L0 = r + g landmarks), 'b' (back to the
centre) and jiggles.  The field lies 6.6 m and more from the centre (out of range from every pose near it, max_range = 6 m) and
within 5.9 m of the point 2 m ahead, in rows 0.3 m apart.

Environments stand in the four corner slots of step_cases' grid (28.5 m apart): no pose ever has another environment's landmark
within 13 m.  Steps are numbered from 0; after step s an environment holds s + 2 poses.
"""
import ctypes as C
import math

import numpy as np

import step_cases as S

SLOTS = [(0, 0), (3, 0), (0, 1), (3, 1)]
FIELD_R0, FIELD_DR = 6.6, 0.3          # first row of a gate field and the distance between rows (m from the centre)
FIELD_REACH = 5.9                      # ... every field landmark is closer than this to the point GATE_MOVE ahead of the centre
FIELD_FILL = 0.85                      # share of a row's arc inside that reach that is used
EXTRA = 2                              # further steps on the same form behind the check step


def _field(g, spacing):
    """(rho, alpha) of g field landmarks in polar coordinates about the centre, alpha from the start heading."""
    out, row = [], 0
    while len(out) < g:
        rho = FIELD_R0 + FIELD_DR * row
        cosa = (rho * rho + S.GATE_MOVE ** 2 - FIELD_REACH ** 2) / (2 * S.GATE_MOVE * rho)
        assert cosa < 0.97, "gate field of %d landmarks at %.3f rad: out of rows" % (g, spacing)
        n = min(g - len(out), int(2 * FIELD_FILL * math.acos(cosa) / spacing))
        out += [(rho, (j - (n - 1) / 2.0) * spacing + 0.0037) for j in range(n)]
        row += 1
    return out


class FormWorld(S.World):
    """rings: [(ring size, gate field size)], environment e in SLOTS[e]; spacing: rad between neighbours of a field row."""

    def __init__(self, name, rings, caps, script, check_step, spacing=0.02):
        self.name, self.rings, self.caps, self.tune = name, list(rings), dict(caps), dict(S.INC_TUNE)
        self.script, self.check_step = script, check_step
        self.n = len(rings)
        assert self.n <= len(SLOTS) and len(script) == check_step + 1 + EXTRA
        self.starts = np.array([S._slot(*SLOTS[e]) for e in range(self.n)])
        pts, self.ring_keys, self.gate_keys = [], [], []
        k = 0
        for (size, gate), (cx, cy, th) in zip(self.rings, self.starts):
            nl, arc = (size + 1) // 2, math.radians(180 - S.GAP_DEG - S.AHEAD_DEG)   # (the ring of step_cases.World)
            beta = np.concatenate([math.radians(S.AHEAD_DEG) + (np.arange(nl) + 0.5) * arc / nl,
                                   -math.radians(S.AHEAD_DEG) - (np.arange(size - nl) + 0.5) * arc / max(size - nl, 1)])
            pts.append(np.stack([cx + S.RADIUS * np.cos(th + beta), cy + S.RADIUS * np.sin(th + beta)], axis=1))
            self.ring_keys.append(np.arange(k, k + size))
            k += size
            f = np.array(_field(gate, spacing)).reshape(-1, 2)
            pts.append(np.stack([cx + f[:, 0] * np.cos(th + f[:, 1]), cy + f[:, 0] * np.sin(th + f[:, 1])], axis=1))
            self.gate_keys.append(np.arange(k, k + gate))
            k += gate
        self.fixed = np.concatenate(pts)
        self.num_landmarks = len(self.fixed)

    def expected(self, e, s):
        """(poses after step s, L0 = landmarks in the panel before it, n_re, first sightings) of environment e, s >= 1."""
        size, gate = self.rings[e]
        return s + 2, size + gate, size, 0


DENSE_SCRIPT = "gbjjj"                  # check step 2: 4 poses; the dense kernels (fused k_step)
CHAIN_SCRIPT = "gb" + "j" * 53          # check step 52: 54 poses, the first the pose-chain kernels serve
LONG_CHAIN_SCRIPT = "gb" + "j" * 118    # check step 117: 119 poses


def worlds():
    return [
        FormWorld("dense100", [(8, 28)], dict(max_poses=12, max_landmarks=100, max_factors=512, max_actions=4), DENSE_SCRIPT, 2),
        FormWorld("dense270", [(8, 190), (16, 184), (24, 180)], dict(max_poses=12, max_landmarks=270, max_factors=1024, max_actions=4), DENSE_SCRIPT, 2),
        FormWorld("dense400", [(8, 384)], dict(max_poses=12, max_landmarks=400, max_factors=1024, max_actions=4), DENSE_SCRIPT, 2, spacing=0.012),
        FormWorld("chain270a", [(8, 0), (8, 92), (16, 84), (24, 126)], dict(max_poses=64, max_landmarks=270, max_factors=2048, max_actions=4), CHAIN_SCRIPT, 52),
        FormWorld("chain270b", [(16, 214), (24, 206)], dict(max_poses=64, max_landmarks=270, max_factors=2048, max_actions=4), CHAIN_SCRIPT, 52),
        FormWorld("chain64", [(4, 0)], dict(max_poses=64, max_landmarks=32, max_factors=512, max_actions=4), CHAIN_SCRIPT, 52),
        FormWorld("chain32", [(8, 22)], dict(max_poses=128, max_landmarks=32, max_factors=2048, max_actions=4), LONG_CHAIN_SCRIPT, 117),
    ]


# The cells of the issue's table: (case name, world, environment, form at the check step and at the EXTRA steps behind it).
# 'none': inc_plan finds no room in the LDS, the update is a full solve.
CASES = [
    ("dense_lds_narrow", "dense100", 0, "lds narrow"),
    ("dense_two_walk_narrow_1_batch", "dense270", 0, "two-walk narrow"),
    ("dense_two_walk_narrow_2_batches", "dense270", 1, "two-walk narrow"),
    ("dense_two_walk_narrow_3_batches", "dense270", 2, "two-walk narrow"),
    ("dense_not_feasible", "dense400", 0, "none"),
    ("chain_lds_narrow", "chain270a", 0, "lds narrow"),
    ("chain_lds_narrow_fused", "chain64", 0, "lds narrow"),      # (max_landmarks <= 63: the fused pose-chain step serves it)
    ("chain_streamed_1", "chain270a", 1, "streamed 1"),
    ("chain_streamed_2", "chain270a", 2, "streamed 2"),
    ("chain_streamed_2+1", "chain270a", 3, "streamed 2+1"),
    ("chain_streamed_1+1", "chain270b", 0, "streamed 1+1"),
    ("chain_streamed_1+1+1", "chain270b", 1, "streamed 1+1+1"),
    ("chain_two_walk_narrow", "chain32", 0, "two-walk narrow"),
]
# narrow batches of a case: n_re landmarks in batches of 8
BATCHES = {"dense_two_walk_narrow_1_batch": 1, "dense_two_walk_narrow_2_batches": 2, "dense_two_walk_narrow_3_batches": 3}


def pose_bound(world, calls):
    """The pose bound pc of the (calls + 1)-th drlgx_step after the reset (csrc/drlgx_engine.cpp: every call advances every
    environment's bound, stepped or not)."""
    return min(calls + 2, world.caps["max_poses"])


def restated_form(world, P, L0, n_re, pc):
    return S.inc_form(P, L0, n_re, world.num_landmarks, world.caps["max_poses"], world.caps["max_landmarks"], pc=pc)


def host_form(P, L0, n_re, pc, P_max, L_max, LG, lds_bytes=S.LDS_BUDGET):
    """drlgx_debug_inc_form - the plan of csrc/inc_carve.h on the host - in the notation of step_cases.inc_form, and its raw output."""
    from drl_graph_exploration_amd import _lib
    out = (C.c_int32 * 14)()
    st = _lib.lib().drlgx_debug_inc_form(int(P), int(L0), int(n_re), int(pc), int(P_max), int(L_max), int(LG), int(lds_bytes), out)
    assert st == 0, (P, L0, n_re, pc, P_max, L_max, LG, st)
    o = [int(v) for v in out]
    if not o[0]:
        return "none", o
    if o[4]:
        return "streamed " + "+".join(str(t) for t in o[6:6 + o[5]]), o
    return ("lds " if o[1] else "two-walk ") + ("wide" if o[2] else "narrow"), o


# ------------------------------------------------------------------------------------------------------ the oracle's walk
_walks = {}


def walk(world):
    """The oracles of a world stepped through its script, once per process: dict(actions [step][n][3]; snaps {step: clones} at the
    check step and the EXTRA steps; rows {step: [(poses, L0, nf, n_re, nn, relinearises, distinct keys)]}; margin: the smallest
    distance of any true or measured range / bearing from a sensor limit over the whole script)."""
    if world.name in _walks:
        return _walks[world.name]
    cfg = world.oracle_config()
    sims = world.make_sims()
    out = dict(actions=[], snaps={}, rows={}, margin=math.inf, sims=sims)

    def margin(sim, M0):
        veh, lms, _ = sim.ground_truth()
        dx, dy = lms[:, 0] - veh[0], lms[:, 1] - veh[1]
        d = np.hypot(dx, dy)
        c, s = math.cos(veh[2]), math.sin(veh[2])
        b = np.arctan2(-s * dx + c * dy, c * dx + s * dy)
        inr = d < cfg.max_range
        g = min(np.abs(d - cfg.max_range).min(), np.abs(d - cfg.min_range).min(), np.abs(b[inr] - cfg.max_bearing).min(),
                np.abs(b[inr] - cfg.min_bearing).min())
        _, _, mb, mr = sim.factors()
        if len(mb) > M0:
            g = min(g, np.abs(mr[M0:] - cfg.max_range).min(), np.abs(mr[M0:] - cfg.min_range).min(),
                    np.abs(mb[M0:] - cfg.max_bearing).min(), np.abs(mb[M0:] - cfg.min_bearing).min())
        out["margin"] = min(out["margin"], float(g))

    for sim in sims:
        margin(sim, 0)
    for s, kind in enumerate(world.script):
        acts = world.actions(sims, kind, s)
        out["actions"].append(acts)
        row = []
        for e, sim in enumerate(sims):
            rl = S.relinearises(sim)[0]
            M0, L0 = len(sim.factors()[0]), sim.num_landmarks()
            assert sim.simulate(acts[e]) == 0
            margin(sim, M0)
            keys = sim.factors()[1][M0:]
            nf, nn = len(keys), sim.num_landmarks() - L0
            row.append((sim.num_poses(), L0, nf, nf - nn, nn, rl, len(set(int(k) for k in keys)) == nf))
        if s >= world.check_step:
            out["rows"][s] = row
            out["snaps"][s] = [sim.clone() for sim in sims]
    _walks[world.name] = out
    return out
