"""TEST INFRASTRUCTURE: the beliefs and candidate plans at which the loops of k_fm2_update / k_fm2_prior (csrc/k_fm2.hip) wrap
and at which the 256-measurement cap is met, shared by tests/test_fm2_cpu.py (which checks on the CPU that the cases are what
they claim to be, that none sits on a knife edge, that a dropped update term would show, and how far the restatement is from a
second evaluation of itself) and tests/test_gpu_fm2.py (which runs them on the device).

Three worlds, each one engine beside its oracles (same seeds, same starts, same listed landmarks):

  * RINGS: six rings of 3 m radius, far enough apart that no environment ever sees another's ring; environment e starts at the
    centre of ring e.  Every landmark of a ring passes the gates from anywhere near its centre, so a plan of K actions that
    stays there predicts exactly K x (ring size) measurements.  Environment 0 is compared straight after the reset (P = 1); the
    others drive 12 m away first - the last two poses see no landmark and dead-reckon - and their plans back up into the ring in
    one long action, so that the predicted measurements close a loop and the old poses' update term is not lost in the noise.
  * CORRIDOR: 270 landmarks in a 20 m x 5 m strip, driven end to end: more than 256 landmarks in the belief (the second pass of
    the ordered compaction), about a hundred in view of any one pose.
  * the belief of tests/em_cases.py, unchanged (its first environment): the small candidates.
"""
import math

import numpy as np

import em_cases
from oracle import fm2_ref
from oracle import oracle as O

MAP = 40
SIGMA_RTOL, SIGMA_ATOL = 1e-6, 1e-10          # the project's tolerance for the fm2 covariances (tests/test_gpu_belief.py)
MAX_MEAS = 256                                # kFm2MaxMeas (csrc/drlgx_engine.cpp)

# ---- rings
RING_RADIUS = 3.0
RING_SIZES = [32, 32, 33, 65, 16, 17]         # environment e starts inside ring e
RING_CENTRES = np.array([[-13.3183, 5.2718], [0.3183, 5.2718], [13.3183, 5.2718], [-13.3183, -5.2718], [0.3183, -5.2718], [13.3183, -5.2718]])
RING_HEADINGS = np.array([0.6234, math.pi / 2 + 0.0234, math.pi / 2 - 0.0317, -math.pi / 2 + 0.0291, -math.pi / 2 - 0.0173, -math.pi / 2 + 0.0411])
RING_WALK = [(2.0, 0.0, 0.0)] * 6             # environments 1 .. 5: away from the other row of rings; 10 m and 12 m out are blind
RING_BACK = (-11.0, 0.0, 0.01)                # first action of their plans: backwards, to 1 m from the centre
RING_SHORT = (0.05, 0.0, 0.01)
RINGS_CAPS = dict(max_poses=8, max_landmarks=65, max_factors=512, max_actions=9)

# ---- corridor
CORRIDOR_N = 270
CORRIDOR_START = (-9.3183, 0.2718, 0.0234)
CORRIDOR_WALK = [(2.0, 0.0, 0.0)] * 9
CORRIDOR_CAPS = dict(max_poses=10, max_landmarks=CORRIDOR_N, max_factors=1536, max_actions=9)

EM_CAPS = dict(max_poses=12, max_landmarks=em_cases.NUM_LANDMARKS, max_factors=256, max_actions=9)


def ring_landmarks():
    """Every ring's landmarks, ring after ring (the listed landmarks of the RINGS world; there are no sampled ones)."""
    out = []
    for c, th, n in zip(RING_CENTRES, RING_HEADINGS, RING_SIZES):
        ang = th + (np.arange(n) + 0.5) * 2 * math.pi / n + 0.011   # off the vehicle's axis: nothing on the +-179.9 degree gate
        out.append(np.stack([c[0] + RING_RADIUS * np.cos(ang), c[1] + RING_RADIUS * np.sin(ang)], axis=1))
    return np.concatenate(out)


def ring_starts():
    return np.concatenate([RING_CENTRES, RING_HEADINGS[:, None]], axis=1)


def ring_scripts():
    """Per environment the actions it is stepped through after the reset (environment 0: none)."""
    return [[]] + [list(RING_WALK) for _ in RING_SIZES[1:]]


def corridor_landmarks():
    rng = np.random.RandomState(7)
    return np.stack([rng.uniform(-10.0, 10.0, CORRIDOR_N), rng.uniform(-2.5, 2.5, CORRIDOR_N)], axis=1)


def _short(k):
    return [RING_SHORT] * k


def ring_plans():
    """{name: (environment, plan)} of the RINGS world.  nm = (number of actions) x (ring size) for all but `blind`."""
    plans = {"fresh_K0": (0, [])}
    for k in (1, 2, 3, 4, 5, 8):
        plans["fresh_K%d" % k] = (0, _short(k))
    plans["walked_K0"] = (1, [])
    for k in (1, 2, 3, 4, 5, 8):
        plans["walked_K%d" % k] = (1, [RING_BACK] + _short(k - 1))
    plans["walked_blind"] = (1, [(0.5, 0.0, 0.2)])                   # one action that stays out of sight of everything
    for e, n in ((2, 33), (3, 65)):
        for k in (0, 1, 2):
            plans["ring%d_K%d" % (n, k)] = (e, ([RING_BACK] + _short(k - 1))[:k])
    for e, n in ((4, 16), (5, 17)):
        for k in (0, 1):
            plans["ring%d_K%d" % (n, k)] = (e, [RING_BACK][:k])
    return plans


def k0_of(case):
    """The no-action case of the same environment: `<environment>_K0`."""
    return case.split("_")[0] + "_K0"


RING_NM = {"fresh_K0": 0, "fresh_K1": 32, "fresh_K2": 64, "fresh_K3": 96, "fresh_K4": 128, "fresh_K5": 160, "fresh_K8": 256,
           "walked_K0": 0, "walked_K1": 32, "walked_K2": 64, "walked_K3": 96, "walked_K4": 128, "walked_K5": 160, "walked_K8": 256,
           "walked_blind": 0, "ring33_K0": 0, "ring65_K0": 0, "ring16_K0": 0, "ring17_K0": 0, "ring33_K1": 33, "ring33_K2": 66, "ring65_K1": 65, "ring65_K2": 130, "ring16_K1": 16, "ring17_K1": 17}
RING_OVERFLOW = (1, [RING_BACK] + _short(8))                          # 9 x 32 = 288 predicted measurements: refused

# the corridor's plans; what they have to be (counts, slots) is asserted in tests/test_fm2_cpu.py
CORRIDOR_PLANS = {"corridor_end": (0, [(0.3, 0.0, 0.02), (0.3, 0.0, -0.03)]),          # two poses at the far end: the last slots
                  "corridor_back": (0, [(0.0, 0.0, 3.1), (15.0, 0.0, 0.0)]),           # turns round, drives back: early slots
                  "corridor_K0": (0, [])}
CORRIDOR_OVERFLOW = (0, [(0.3, 0.0, 0.02), (0.3, 0.0, -0.03), (0.3, 0.0, 0.02), (0.3, 0.0, -0.03)])

EM_PLANS = {"em_plan%d" % k: (0, p) for k, p in enumerate(em_cases.FM2_PLANS)}
EM_PLANS["em_K0"] = (0, [])

BANDS = [("nm<=16", 1, 16), ("17-64", 17, 64), ("65-128", 65, 128), ("129-255", 129, 255), ("=256", 256, 256)]


def band_of(nm):
    for name, lo, hi in BANDS:
        if lo <= nm <= hi:
            return name
    return None


# ---------------------------------------------------------------------------------------------------------------- worlds
class World(object):
    """One engine's worth of oracles: `sims` (stepped through `scripts`), `starts`, `fixed` landmarks, the engine capacities
    `caps`, `num_landmarks`, and the named plans."""

    def __init__(self, name, sims, starts, scripts, fixed, num_landmarks, caps, plans):
        self.name, self.sims, self.starts, self.scripts, self.fixed = name, sims, starts, scripts, fixed
        self.num_landmarks, self.caps, self.plans = num_landmarks, caps, plans
        self._ref = {}

    def ref(self, case):
        """The restatement of one case, computed once: dict(cov, n_meas, nm, base, delta, P, K)."""
        if case not in self._ref:
            e, plan = self.plans[case]
            self._ref[case] = reference(self.sims[e], plan)
        return self._ref[case]


def rings_world():
    fixed = ring_landmarks()
    ocfg = O.default_config(MAP, num_landmarks=len(fixed))
    starts, scripts = ring_starts(), ring_scripts()
    sims = [O.OracleSim(ocfg, e, e, start=tuple(starts[e]), fixed_landmarks=fixed) for e in range(len(RING_SIZES))]
    for s, script in zip(sims, scripts):
        for act in script:
            s.simulate(act)
    return World("rings", sims, starts, scripts, fixed, len(fixed), RINGS_CAPS, ring_plans())


def corridor_world():
    fixed = corridor_landmarks()
    ocfg = O.default_config(MAP, num_landmarks=CORRIDOR_N)
    starts = np.array([CORRIDOR_START])
    sim = O.OracleSim(ocfg, 0, 0, start=CORRIDOR_START, fixed_landmarks=fixed)
    for act in CORRIDOR_WALK:
        sim.simulate(act)
    return World("corridor", [sim], starts, [list(CORRIDOR_WALK)], fixed, CORRIDOR_N, CORRIDOR_CAPS, dict(CORRIDOR_PLANS))


def em_world():
    sims, starts = em_cases.make_sims(1)
    return World("em_cases", sims, starts, [list(em_cases.SCRIPT)], None, em_cases.NUM_LANDMARKS, EM_CAPS, dict(EM_PLANS))


def make_engine(world):
    """The engine of a world, reset and stepped beside its oracles (an environment whose script has ended is masked out)."""
    import torch
    from drl_graph_exploration_amd import default_config
    from drl_graph_exploration_amd.engine import Engine
    n = len(world.sims)
    cfg = default_config(MAP, num_landmarks=world.num_landmarks, **world.caps)
    eng = Engine(cfg, n, 0)
    if world.fixed is not None:
        eng.set_fixed_landmarks(world.fixed)
    eng.reset(np.arange(n), np.arange(n), starts=world.starts)
    for s in range(max(len(sc) for sc in world.scripts)):
        odom = np.array([sc[s] if s < len(sc) else (0.0, 0.0, 0.0) for sc in world.scripts], dtype=np.float64)
        active = np.array([1 if s < len(sc) else 0 for sc in world.scripts], dtype=np.uint8)
        eng.step(torch.tensor(odom, device=eng.device), torch.tensor(active, device=eng.device))
    assert eng.status() == 0
    return eng, cfg


# ------------------------------------------------------------------------------------------------------------- reference
class _NoSightings(object):
    """An OracleSim whose sensor reaches nothing: fm2_ref.fm2_update of it returns the covariances BEFORE the measurement
    update (the prior blocks of the old poses, the odometry chain's covariances of the new ones)."""

    def __init__(self, sim):
        self._sim = sim
        self.cfg = O.OrcConfig.from_buffer_copy(sim.cfg)
        self.cfg.max_range = 0.0

    def __getattr__(self, name):
        return getattr(self._sim, name)


def reference(sim, plan):
    cov, n_meas = fm2_ref.fm2_update(sim, plan)
    base, none = fm2_ref.fm2_update(_NoSightings(sim), plan)
    assert sum(none) == 0
    return dict(cov=cov, n_meas=n_meas, nm=int(sum(n_meas)), base=base, delta=cov - base, P=sim.num_poses(), K=len(plan))


def predicted_pairs(sim, plan):
    """Every (new pose, landmark slot) pair with its range and bearing on the estimated map, and the smallest distance of any
    of them to a gate (the expressions of fm2_ref.fm2_update)."""
    cfg = sim.cfg
    est_xyt, _ = sim.poses()
    keys, est, _ = sim.landmarks()
    slot_of = {int(k): j for j, k in enumerate(sim.slot_keys())}
    origin = fm2_ref._pose(*est_xyt[-1])
    pairs, margin = [], math.inf
    for b, a in enumerate(plan):
        origin = fm2_ref._compose(origin, fm2_ref._pose(*a))
        for key, xy in zip(keys, est):
            dx, dy = xy[0] - origin[0], xy[1] - origin[1]
            rng = math.sqrt(dx * dx + dy * dy)
            bearing = math.atan2(-origin[3] * dx + origin[2] * dy, origin[2] * dx + origin[3] * dy)
            margin = min(margin, abs(rng - cfg.max_range), abs(rng - cfg.min_range))
            if rng < cfg.max_range:
                margin = min(margin, abs(bearing - cfg.max_bearing), abs(bearing - cfg.min_bearing))
            seen = cfg.min_range < rng < cfg.max_range and cfg.min_bearing < bearing < cfg.max_bearing
            pairs.append((b, slot_of[int(key)], rng, bearing, seen))
    return pairs, margin


# ------------------------------------------------------------------------- the restatement a second, independent way (C4)
def information_matrix(sim):
    """J^T W J of the belief's factors at the iSAM linearisation point, order [landmarks by slot (2 each), poses (3 each)],
    assembled from the factor lists - not from full_covariance().  The rotations that the prior and the odometry factors carry
    in their Jacobians commute with their isotropic x / y weights and drop out."""
    cfg = sim.cfg
    thp, _, thl, _, _ = sim.isam_state()
    P, L = sim.num_poses(), sim.num_landmarks()
    n = 2 * L + 3 * P
    Lam = np.zeros((n, n))
    px = lambda i: slice(2 * L + 3 * i, 2 * L + 3 * i + 3)   # noqa: E731
    assert cfg.sigma_x0 == cfg.sigma_y0
    Lam[px(0), px(0)] += np.diag([cfg.sigma_x0 ** -2, cfg.sigma_y0 ** -2, cfg.sigma_theta0 ** -2])
    W = np.diag([cfg.translation_noise ** -2, cfg.translation_noise ** -2, cfg.rotation_noise ** -2])
    for i in range(P - 1):
        _, H1 = fm2_ref._between(fm2_ref._pose(*thp[i]), fm2_ref._pose(*thp[i + 1]))
        J = np.zeros((3, n))
        J[:, px(i)], J[:, px(i + 1)] = H1, np.eye(3)
        Lam += J.T @ W @ J
    slot_of = {int(k): j for j, k in enumerate(sim.slot_keys())}
    sig_br = np.array([cfg.bearing_noise, cfg.range_noise])
    fp, fk, _, _ = sim.factors()
    for p, k in zip(fp, fk):
        j = slot_of[int(k)]
        Jx, Jl = fm2_ref._br_jacobians(fm2_ref._pose(*thp[p]), thl[j])
        J = np.zeros((2, n))
        J[:, px(p)], J[:, 2 * j:2 * j + 2] = Jx / sig_br[:, None], Jl / sig_br[:, None]
        Lam += J.T @ J
    return Lam


def _pose_blocks(Lam, L, n_poses):
    """The 3x3 diagonal blocks of Lam^-1 at the poses, by a Cholesky factor and one forward solve: Sigma_ii = X_i^T X_i with
    C X = E (no inverse is formed)."""
    n = Lam.shape[0]
    C = np.linalg.cholesky(Lam)
    E = np.zeros((n, 3 * n_poses))
    E[2 * L:, :] = np.eye(3 * n_poses)
    X = np.linalg.solve(C, E)
    return np.array([X[:, 3 * i:3 * i + 3].T @ X[:, 3 * i:3 * i + 3] for i in range(n_poses)])


def reference_information_form(sim, plan):
    """The same update in information form - the new poses appended, J^T J of the same linearised factors added, the blocks
    read off a Cholesky factor - on a prior that is assembled from the factor lists: no dense inverse, no T = I + A Sigma A^T,
    no cross covariance by F chains.  Returns dict(cov, base, delta) like reference()."""
    cfg = sim.cfg
    P, L, K = sim.num_poses(), sim.num_landmarks(), len(plan)
    thp, _, thl, _, _ = sim.isam_state()
    n0, n = 2 * L + 3 * P, 2 * L + 3 * (P + K)
    Lam0 = information_matrix(sim)
    old = _pose_blocks(Lam0, L, P)
    Lam = np.zeros((n, n))
    Lam[:n0, :n0] = Lam0
    px = lambda i: slice(2 * L + 3 * i, 2 * L + 3 * i + 3)   # noqa: E731
    sig = np.array([cfg.translation_noise, cfg.translation_noise, cfg.rotation_noise])
    sig_br = np.array([cfg.bearing_noise, cfg.range_noise])
    origin, val0 = fm2_ref._pose(*sim.poses()[0][-1]), fm2_ref._pose(*thp[-1])
    keys, est, _ = sim.landmarks()
    slot_of = {int(k): j for j, k in enumerate(sim.slot_keys())}
    base = np.zeros((P + K, 3, 3))
    base[:P] = old
    cov0 = old[P - 1]
    for k, a in enumerate(plan):
        odom = fm2_ref._pose(*a)
        end = fm2_ref._compose(origin, odom)
        hx, H1b = fm2_ref._between(val0, end)
        h, _ = fm2_ref._between(odom, hx)
        Hl = np.array([[h[2], h[3], 0], [-h[3], h[2], 0], [0, 0, 1.0]])
        A0, A1 = (Hl @ H1b) / sig[:, None], Hl / sig[:, None]
        J = np.zeros((3, n))
        J[:, px(P + k - 1)], J[:, px(P + k)] = A0, A1
        Lam += J.T @ J
        # the chain's covariance before any sighting: the marginal of the appended pose, by a solve instead of an inverse
        M = A0 @ cov0 @ A0.T + np.eye(3)
        Y = np.linalg.solve(A1, M)
        cov0 = np.linalg.solve(A1, Y.T).T
        base[P + k] = (cov0 + cov0.T) / 2
        for key, xy in zip(keys, est):
            j = slot_of[int(key)]
            dx, dy = xy[0] - end[0], xy[1] - end[1]
            rng = math.sqrt(dx * dx + dy * dy)
            bearing = math.atan2(-end[3] * dx + end[2] * dy, end[2] * dx + end[3] * dy)
            if cfg.min_range < rng < cfg.max_range and cfg.min_bearing < bearing < cfg.max_bearing:
                Jx, Jl = fm2_ref._br_jacobians(end, thl[j])
                J = np.zeros((2, n))
                J[:, px(P + k)], J[:, 2 * j:2 * j + 2] = Jx / sig_br[:, None], Jl / sig_br[:, None]
                Lam += J.T @ J
        origin, val0 = end, end
    cov = _pose_blocks(Lam, L, P + K)
    return dict(cov=cov, base=base, delta=cov - base)


# ------------------------------------------------------------------------------------------------ tolerances of the GPU test
# C4, measured on the CPU by tests/test_fm2_cpu.py::test_c4_the_restatements_own_spread (which asserts that these figures still
# bound what it measures): max |Delta_1 - Delta_2| / max |Delta_1| between the restatement and its information-form evaluation,
# per case.  The GPU test allows the update term 10 x the figure of the case (tests/test_gpu_fm2.py).
C4_DELTA_SPREAD = {
    "em_plan0": 2.0e-14, "em_plan1": 1.3e-14, "em_plan2": 2.0e-14, "ring16_K1": 3.2e-14, "ring17_K1": 1.6e-14,
    "fresh_K1": 2.6e-14, "walked_K1": 5.6e-14, "ring33_K1": 2.3e-14, "fresh_K2": 3.0e-14, "walked_K2": 1.3e-13,
    "ring65_K1": 1.3e-13, "ring33_K2": 9.3e-14, "fresh_K3": 9.8e-14, "walked_K3": 1.3e-13, "fresh_K4": 4.0e-14,
    "walked_K4": 3.5e-13, "ring65_K2": 3.4e-13, "fresh_K5": 1.1e-13, "walked_K5": 2.6e-13, "corridor_end": 2.1e-13,
    "corridor_back": 3.2e-13, "fresh_K8": 2.5e-13, "walked_K8": 5.5e-13}
# every case with a predicted measurement meets C3 (tests/test_fm2_cpu.py::test_c3_a_dropped_update_term_would_fail)
PARITY_CASES = sorted(C4_DELTA_SPREAD)
DELTA_BOUND_FACTOR = 10.0
# (world, case) handed to drlgx_em_cost: one parity case per band of nm, and the corridor
EM_COST_CASES = [("em_cases", "em_plan2"), ("rings", "ring17_K1"), ("rings", "ring65_K1"), ("rings", "walked_K5"), ("rings", "walked_K8"),
                 ("corridor", "corridor_back")]


def sensitivity(ref):
    """C3: how far the restatement with its update term dropped lies from the restatement, in units of the tolerance the GPU
    test applies to that element: max |Delta| / (SIGMA_RTOL |Sigma'| + SIGMA_ATOL) over all compared blocks, and over the old
    poses' blocks alone."""
    tol = SIGMA_RTOL * np.abs(ref["cov"]) + SIGMA_ATOL
    ratio = np.abs(ref["delta"]) / tol
    P = ref["P"]
    return float(ratio.max()), float(ratio[:P].max()) if P else 0.0
