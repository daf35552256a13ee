"""TEST INFRASTRUCTURE: the candidates at which the loops of drlgx_slam_og_cost start a second trip, shared by
tests/test_slam_og_wrap_cpu.py (which checks on the CPU that the cases are what they claim to be) and
tests/test_gpu_slam_og_wrap.py.  No new world: the CORRIDOR and the RINGS of tests/fm2_cases.py, their engines by
fm2_cases.make_engine, the restatement tests/slam_og_ref.py.

  * corridor: one environment, P = 10 = max_poses, L = 270 landmarks - P + L = 280 owners of k_fm2_prior_ordered (more than its 256
    threads), more than 256 slots for the ordered compaction of k_fm2_update<., true> and for k_slam_og_weights, five trips per lane
    of k_slam_og_blend;
  * rings: six environments (rings of 32, 32, 33, 65, 16, 17), plans of exactly 256 predicted measurements - the cap - and the
    counts on either side of the strides (16 | 17, 32 | 33, 130).
"""
import fm2_cases as F
import slam_og_ref

ALPHA = 0.3                                      # slam_og_cases.ALPHA
MAX_MEAS = F.MAX_MEAS
LM_RTOL, LM_ATOL = F.SIGMA_RTOL, F.SIGMA_ATOL   # what tests/test_gpu_fm2.py holds the pose blocks to

_ZIGZAG = [(0.3, 0.0, 0.02), (0.3, 0.0, -0.03)]
CORE9_PLAN = _ZIGZAG * 4 + _ZIGZAG[:1]
CORE9_MASK = [0, 0, 0, 1, 0, 0, 0, 0, 1]
BLIND = (0.0, 12.0, 0.0)                         # sideways out of the strip: nothing within the sensor's range

_RING_NAMES = ["fresh_K8", "walked_K8", "walked_K1", "ring65_K2", "ring33_K1", "ring16_K1", "ring17_K1", "fresh_K0", "walked_K0"]
_RING_PLANS = F.ring_plans()

# world: {name: (environment, plan, core mask or None, predicted measurements)}
CASES = {
    "corridor": {
        "corridor_K0": F.CORRIDOR_PLANS["corridor_K0"] + (None, 0),
        "corridor_end": F.CORRIDOR_PLANS["corridor_end"] + (None, 172),
        "corridor_back": F.CORRIDOR_PLANS["corridor_back"] + (None, 228),
        "corridor_core9": (0, CORE9_PLAN, CORE9_MASK, 130),
        "corridor_blind": (0, [BLIND], None, 0),
    },
    "rings": {name: _RING_PLANS[name] + (None, F.RING_NM[name]) for name in _RING_NAMES},
}
AT_THE_CAP = ["fresh_K8", "walked_K8"]           # nm == 256

# refused: more than 256 predicted measurements
OVERFLOWS = {"corridor": F.CORRIDOR_OVERFLOW + (None,), "rings": F.RING_OVERFLOW + (None,)}
# served: the corridor's overflow plan with two of its four poses masked out - only the mask brings it under the cap
MASKED_OVERFLOW = (0, F.CORRIDOR_OVERFLOW[1], [1, 0, 1, 0], 166)

_WORLDS = {"corridor": F.corridor_world, "rings": F.rings_world}


def world(name):
    return _WORLDS[name]()


def predicted(sim, plan, core=None):
    """Number of predicted measurements of a plan, as the restatement counts them."""
    return int(sum(slam_og_ref._plan_rows(sim, plan, core)[2]))


def reference(w, case, alpha=ALPHA):
    """slam_og_ref.slam_og_cost of a named case of the world, or of an (environment, plan, core, nm) tuple."""
    e, plan, core, _ = CASES[w.name][case] if isinstance(case, str) else case
    return slam_og_ref.slam_og_cost(w.sims[e], plan, alpha, core=core)
