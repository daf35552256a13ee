"""TEST INFRASTRUCTURE: worlds that put a full solve of the pose-chain solver (csrc/k_slam_arrow.hip) into a chosen cell of its
run-time choices - landmark system packed / register tiles / streamed, the three placements obs_lds / xs_lds / rec_lds, the form of
the pose products and, for the staged form, zfit / zg / Tn - shared by tests/test_arrow_cases_cpu.py (which proves on the CPU, with
the oracle and drlgx_debug_arrow_form alone, that every world is in the cell it claims) and tests/test_gpu_arrow_forms.py (which
runs them on the device).

A world is a ring of L listed landmarks (all of num_landmarks: the landmark count is exact) of radius RADIUS around the point
where both environments start, and a script of P - 1 equal turns in place: P poses, no pose leaves the ring.  The sensor's field
of view is `per_pose` landmark spacings wide, so a pose observes about per_pose landmarks and M = the number of bearing-range
factors (what the kernel counts as M: csrc/k_sim.hip, cnt[C_M]; the odometry factors are not among them) is about P x per_pose:
about 10 per pose keeps the factor records in LDS where the cell wants that, about 30 per pose sends them to the workspace.  No
step brings more than 64 factors or a first sighting after the turn is complete, so the steps behind the check step are rank-k
updates of the panel the check step's solve left (Case.rank_k_after: except at 496 landmarks, where the rank-k update has no
room in LDS and every update is a full solve).  The turn sweeps 372 degrees less the field of view: every landmark is seen.

The check step is the one that brings the instance to P poses, P a multiple of 10: the iSAM policy relinearises every 10th
update where a |delta| reaches 0.1, and with the default 0.1 m translation noise one does (asserted on the CPU) - with the
incremental update on, that update is a full solve that leaves the covariance panel.

ROWS restates the twelve cells of the case table in DESIGN.md ("k_slam_arrow.hip by phase") as predicates on what
drlgx_debug_arrow_form returns.
"""
import ctypes as C
import math

import numpy as np

from oracle import oracle as O

import step_cases

MAP = 40
RADIUS = 4.0
CENTRE = (0.3183, -0.2718)
HEADINGS = (0.1234, 2.2)       # the two environments' start headings
SWEEP_DEG = 372.0              # field of view + total turn (more where 209 noisy steps let the vehicle wander further)
EXTRA_STEPS = 5                # rank-k updates behind the check step

PACKED, REG, STREAM = 0, 1, 2
VECTOR, TILES, STAGED = 0, 1, 2
FIELDS = ("system", "obs_lds", "xs_lds", "rec_lds", "form", "zfit", "zg", "Tn", "nK")


def arrow_form(P, L, M, L_max, mk_panel):
    """drlgx_debug_arrow_form as a dict over FIELDS."""
    from drl_graph_exploration_amd import _lib
    out = (C.c_int32 * 9)()
    st = _lib.lib().drlgx_debug_arrow_form(int(P), int(L), int(M), int(L_max), int(mk_panel), out)
    assert st == 0, (P, L, M, L_max, st)
    return dict(zip(FIELDS, [int(x) for x in out]))


class Case(object):
    """L landmarks, P poses at the check step, a field of view of `per_pose` landmark spacings; max_landmarks L_max.  rows: the
    cells of ROWS it claims; cell: what drlgx_debug_arrow_form must return at the check step (zfit: exact, or (lo, None) = at least lo)."""

    def __init__(self, name, rows, L, P, per_pose, cell, L_max=None, phase=0.5, radius=RADIUS, sweep_deg=SWEEP_DEG):
        self.name, self.rows, self.L, self.P, self.per_pose, self.cell = name, tuple(rows), L, P, per_pose, dict(cell)
        self.L_max = L if L_max is None else L_max
        self.n = len(HEADINGS)
        self.fov_deg = 360.0 * per_pose / L
        self.turn = math.radians((sweep_deg - self.fov_deg) / (P - 1))
        self.check_step = P - 2                     # steps from 0; after step s an instance holds s + 2 poses
        self.n_steps = P - 1 + EXTRA_STEPS
        ang = (np.arange(L) + phase) * (2.0 * math.pi / L)   # (phase: where on the ring the landmarks lie, in spacings)
        self.fixed = np.stack([CENTRE[0] + radius * np.cos(ang), CENTRE[1] + radius * np.sin(ang)], axis=1)
        self.starts = np.array([[CENTRE[0], CENTRE[1], h] for h in HEADINGS])
        self.caps = dict(max_poses=P + EXTRA_STEPS + 1, max_landmarks=self.L_max, max_factors=(P + EXTRA_STEPS + 1) * (2 * per_pose + 8))

    def _tuned(self, cfg):
        cfg.min_bearing, cfg.max_bearing = -math.radians(self.fov_deg / 2), math.radians(self.fov_deg / 2)
        return cfg

    def oracle_config(self):
        return self._tuned(O.default_config(MAP, num_landmarks=self.L))

    def engine_config(self):
        from drl_graph_exploration_amd import default_config
        return self._tuned(default_config(MAP, num_landmarks=self.L, **self.caps))

    def make_sims(self):
        cfg = self.oracle_config()
        return [O.OracleSim(cfg, e, e, start=tuple(self.starts[e]), fixed_landmarks=self.fixed) for e in range(self.n)]

    def action(self, s):
        return (0.0, 0.0, self.turn)

    @property
    def rank_k_after(self):
        """Do the steps behind the check step run as rank-k updates of the panel?  Not where the update's LDS plan has no room
        for its Y rows (csrc/k_inc.hip: inc_plan, restated by step_cases.inc_form): such an instance - 3 P + 2 L beyond about
        1000 - takes a full solve at every update, by design."""
        return all(step_cases.inc_form(P, self.L, self.per_pose, self.L, self.caps["max_poses"], self.L_max) != "none"
                   for P in range(self.P + 1, self.P + EXTRA_STEPS + 1))

    def matches(self, got):
        for k, want in self.cell.items():
            if isinstance(want, tuple):
                if got[k] < want[0] or (want[1] is not None and got[k] > want[1]):
                    return False
            elif got[k] != want:
                return False
        return True


def _cell(system, obs, xs, rec, form, Tn, nK, zfit=None, zg=None):
    c = dict(system=system, obs_lds=obs, xs_lds=xs, rec_lds=rec, form=form, Tn=Tn, nK=nK)
    if form == STAGED:
        c.update(zfit=zfit, zg=zg)
    return c


CASES = [
    Case("reg64_tiles_rec_lds", (1,), 64, 60, 10, _cell(REG, 1, 1, 1, TILES, 9, 8)),
    Case("reg64_tiles_rec_ws", (2,), 64, 60, 30, _cell(REG, 1, 1, 0, TILES, 9, 8)),
    Case("packed63_tiles_8_chunks", (3,), 63, 60, 8, _cell(PACKED, 1, 1, 1, TILES, 8, 8)),
    Case("reg65_staged_zfit2", (4,), 65, 60, 10, _cell(REG, 1, 1, 1, STAGED, 9, 9, zfit=2, zg=2)),
    Case("reg65_staged_zg3_tn9", (5.0,), 65, 60, 30, _cell(REG, 1, 1, 0, STAGED, 9, 9, zfit=(3, None), zg=3)),
    Case("reg72_staged_zg3_tn10", (5.1,), 72, 60, 30, _cell(REG, 1, 1, 0, STAGED, 10, 9, zfit=(3, None), zg=3)),
    Case("reg80_staged_zg3_tn11", (5.2,), 80, 60, 30, _cell(REG, 1, 1, 0, STAGED, 11, 10, zfit=(3, None), zg=3)),
    Case("reg127_last_register_tiles", (6.0,), 127, 60, 10, _cell(REG, 1, 1, 0, STAGED, 16, 16, zfit=(3, None), zg=3)),
    Case("stream128_zfit1", (6.1, 7), 128, 60, 10, _cell(STREAM, 1, 1, 1, STAGED, 17, 16, zfit=1, zg=1)),
    Case("stream325_zfit0_xs_x", (8,), 325, 60, 16, _cell(STREAM, 1, 0, 0, STAGED, 41, 41, zfit=0, zg=1)),
    Case("stream496_obs_ws", (9,), 496, 90, 14, _cell(STREAM, 0, 0, 0, STAGED, 63, 62, zfit=0, zg=1), L_max=500, phase=0.3),
    Case("reg123_xs_x", (10,), 123, 120, 10, _cell(REG, 1, 0, 0, STAGED, 16, 16, zfit=2, zg=2), L_max=127),
    Case("reg125_obs_ws", (11,), 125, 140, 10, _cell(REG, 0, 0, 0, STAGED, 16, 16, zfit=(3, None), zg=3), L_max=127),
    Case("packed56_obs_ws", (12,), 56, 210, 10, _cell(PACKED, 0, 1, 0, TILES, 8, 7), L_max=63, radius=3.0, sweep_deg=450.0),
]
BY_NAME = {c.name: c for c in CASES}

# The cells of the case table, as predicates on (drlgx_debug_arrow_form's dict, L).  5.0 / 5.1 / 5.2: Tn mod 3 = 0 / 1 / 2 - the
# last group of three column tiles full, one tile, two tiles; 6.0 / 6.1: either side of the register-tile sweep's reach.
ROWS = {
    1: lambda f, L: f["system"] == REG and f["form"] == TILES and L == 64 and f["rec_lds"] == 1,
    2: lambda f, L: f["system"] == REG and f["form"] == TILES and L == 64 and f["rec_lds"] == 0,
    3: lambda f, L: f["system"] == PACKED and f["form"] == TILES and f["nK"] == 8 and L == 63,
    4: lambda f, L: f["system"] == REG and f["form"] == STAGED and L == 65 and f["nK"] == 9 and f["zfit"] == 2 and f["rec_lds"] == 1,
    5.0: lambda f, L: f["system"] == REG and f["form"] == STAGED and f["zfit"] >= 3 and f["zg"] == 3 and f["Tn"] % 3 == 0,
    5.1: lambda f, L: f["system"] == REG and f["form"] == STAGED and f["zfit"] >= 3 and f["zg"] == 3 and f["Tn"] % 3 == 1,
    5.2: lambda f, L: f["system"] == REG and f["form"] == STAGED and f["zfit"] >= 3 and f["zg"] == 3 and f["Tn"] % 3 == 2,
    6.0: lambda f, L: f["system"] == REG and L == 127 and f["Tn"] == 16,
    6.1: lambda f, L: f["system"] == STREAM and L == 128 and f["Tn"] == 17,
    7: lambda f, L: f["system"] == STREAM and f["form"] == STAGED and f["zfit"] == 1 and f["zg"] == 1,
    8: lambda f, L: f["system"] == STREAM and f["form"] == STAGED and f["zfit"] == 0 and f["xs_lds"] == 0,
    9: lambda f, L: f["system"] == STREAM and f["obs_lds"] == 0,
    10: lambda f, L: f["system"] == REG and f["xs_lds"] == 0,
    11: lambda f, L: f["system"] == REG and f["obs_lds"] == 0,
    12: lambda f, L: f["system"] == PACKED and f["obs_lds"] == 0,
}


def relinearises(sim):
    """Will the NEXT update of this oracle relinearise?  (oracle/drlgx_oracle.cpp Isam::update: every 10th update, a variable
    whose |delta|_inf >= 0.1.)"""
    _, dp, _, dl, count = sim.isam_state()
    mx = max(np.abs(dp).max() if dp.size else 0.0, np.abs(dl).max() if dl.size else 0.0)
    return (count + 1) % 10 == 0 and mx >= 0.1


def margins(sim):
    """Smallest distance of any listed landmark from the range limits (m) and, of those in range, from the field-of-view limits
    (rad), at the oracle's current ground-truth pose."""
    cfg = sim.cfg
    veh, lms, _ = sim.ground_truth()
    dx, dy = lms[:, 0] - veh[0], lms[:, 1] - veh[1]
    d = np.hypot(dx, dy)
    c, s = math.cos(veh[2]), math.sin(veh[2])
    b = np.arctan2(-s * dx + c * dy, c * dx + s * dy)
    inr = (d < cfg.max_range) & (d > cfg.min_range)
    m_range = float(min(np.abs(d - cfg.max_range).min(), np.abs(d - cfg.min_range).min()))
    m_fov = float(min(np.abs(b[inr] - cfg.max_bearing).min(), np.abs(b[inr] - cfg.min_bearing).min())) if inr.any() else math.inf
    return m_range, m_fov


_runs = {}


def run_oracle(case):
    """The oracles of a case stepped through its script, once per process: dict(check = clones at the check step, end = the
    oracles after EXTRA_STEPS more, relin = per environment whether the check step's update relinearised, margin = the smallest
    (range, field-of-view) margin over every pose, new_factors / new_landmarks = the largest per-step growth behind the check step)."""
    if case.name in _runs:
        return _runs[case.name]
    sims = case.make_sims()
    out = dict(margin=[math.inf, math.inf], relin=None, check=None, new_factors=0, new_landmarks=0)

    def note():
        for sim in sims:
            mr, mf = margins(sim)
            out["margin"] = [min(out["margin"][0], mr), min(out["margin"][1], mf)]

    note()
    for s in range(case.n_steps):
        if s == case.check_step:
            out["relin"] = [relinearises(sim) for sim in sims]
        before = [(len(sim.factors()[0]), sim.num_landmarks()) for sim in sims] if s > case.check_step else None
        for sim in sims:
            assert sim.simulate(case.action(s)) == 0
        note()
        if before is not None:
            for sim, (m0, l0) in zip(sims, before):
                out["new_factors"] = max(out["new_factors"], len(sim.factors()[0]) - m0)
                out["new_landmarks"] = max(out["new_landmarks"], sim.num_landmarks() - l0)
        if s == case.check_step:
            out["check"] = [sim.clone() for sim in sims]
    out["end"] = sims
    _runs[case.name] = out
    return out


def counts(sim):
    return sim.num_poses(), sim.num_landmarks(), len(sim.factors()[0])
