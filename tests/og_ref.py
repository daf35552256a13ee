"""TEST INFRASTRUCTURE: numpy (fp64) restatement of `calculateUncertainty_OG_SHANNON` (src/em_exploration/Planner2D.cpp:368-392)
and `costFunction` (:418-420) for one action list on an `oracle.OracleSim`:

  * `VirtualMap::updateProbability` (VirtualMap.cpp:61-84): `num_samples` copies of the estimated map, each through
    `OccupancyMap::update(map)` (OccupancyMap.cpp:122-138) - every cell at LOGODDS_UNKNOWN, one occupied update of its cell per
    landmark inside the grid (:55-62), then `update(state)` per pose in trajectory order (:64-120): the bounding box of the origin
    cell and of the ray end points every 3 degrees, floored and clamped; within the box a cell at MIN_LOGODDS is skipped, a cell
    that fails `checkWithoutMinRange` is skipped, the others get `occupied` above OCCUPIED_THRESH + 1e-8 and `free` otherwise;
  * the leaf's trajectory: the estimates, then the noise-free predicted poses (`em_ref.leaf_poses`);
  * H = sum_v -p ln p - (1 - p) ln(1 - p); cost = H + distance * distance_weight with em_ref's distance and the distance weight of
    `initialize` (:1322-1332) from the LIVE map's probabilities.

The log-odds constants are those of OccupancyMap.h:10-19, evaluated with the C library's log / exp (`math`, not numpy's own
vector routines): the ladder's values are then the reference's bits.  Besides the values it reports by how little any decision
was taken (`margins`).
"""
import math

import numpy as np

import em_ref


def _p2l(p):
    return math.log(p / (1.0 - p))


def _l2p(l):
    return math.exp(l) / (1.0 + math.exp(l))


LOGODDS_FREE = _p2l(0.3)
LOGODDS_UNKNOWN = _p2l(0.5)
LOGODDS_OCCUPIED = _p2l(0.7)
MIN_LOGODDS = _p2l(0.05)
MAX_LOGODDS = _l2p(0.95)  # sic (OccupancyMap.h:17)
OCCUPIED_THRESH = _p2l(0.5)
DEG3 = 3 * 0.01745329251994329575  # DEG2RAD(3)


def _update_cell(logodds, v, free):
    """OccupancyMap::update(row, col, free) on flat index (or index array) v."""
    l = logodds[v] + (LOGODDS_FREE if free else LOGODDS_OCCUPIED)
    logodds[v] = np.minimum(MAX_LOGODDS, np.maximum(MIN_LOGODDS, l))


def _cell_of(cfg, x, y):
    """(row, col) before any clamp, and the distance (in metres) of the point from the nearest cell boundary."""
    fy, fx = (y - cfg.map_min_y) / cfg.resolution, (x - cfg.map_min_x) / cfg.resolution
    edge = min(fy - math.floor(fy), math.ceil(fy) - fy, fx - math.floor(fx), math.ceil(fx) - fx) * cfg.resolution
    if fy == math.floor(fy) or fx == math.floor(fx):
        edge = 0.0
    return int(math.floor(fy)), int(math.floor(fx)), edge


def occupancy_logodds(poses, landmarks, cfg, rows, cols):
    """OccupancyMap::update(map): poses [n, 4] (x, y, cos, sin) in trajectory order, landmarks [m, 2].  Returns (log-odds [rows *
    cols], margins): margins = {"range", "bearing", "floor"} in metres (the bearing gates as the arc at the cell's range),
    {"thresh"} in log-odds - the smallest distance of any decision from its gate."""
    V = rows * cols
    lo = np.full(V, LOGODDS_UNKNOWN)
    margins = {"range": math.inf, "bearing": math.inf, "floor": math.inf, "thresh": math.inf}
    for x, y in landmarks:
        r, c, edge = _cell_of(cfg, x, y)
        margins["floor"] = min(margins["floor"], edge)
        if r >= rows or r < 0 or c >= cols or c < 0:
            continue
        _update_cell(lo, r * cols + c, False)
    cx = cfg.map_min_x + cfg.resolution * (np.arange(cols) + 0.5)
    cy = cfg.map_min_y + cfg.resolution * (np.arange(rows) + 0.5)
    X, Y = np.meshgrid(cx, cy)
    X, Y = X.reshape(-1), Y.reshape(-1)
    R, C = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    R, C = R.reshape(-1), C.reshape(-1)
    for px, py, pc, ps in poses:
        r0, c0, edge = _cell_of(cfg, px, py)
        margins["floor"] = min(margins["floor"], edge)
        rs, cs = [min(max(0, r0), rows - 1)], [min(max(0, c0), cols - 1)]
        theta0 = math.atan2(ps, pc)
        b = cfg.min_bearing
        while b < cfg.max_bearing + 1e-5:
            ex = px + cfg.max_range * math.cos(theta0 + b)
            ey = py + cfg.max_range * math.sin(theta0 + b)
            r, c, edge = _cell_of(cfg, ex, ey)
            margins["floor"] = min(margins["floor"], edge)
            rs.append(min(max(0, r), rows - 1))
            cs.append(min(max(0, c), cols - 1))
            b += DEG3
        box = (R >= min(rs)) & (R <= max(rs)) & (C >= min(cs)) & (C <= max(cs))
        live = box & ~(np.abs(lo - MIN_LOGODDS) < 1e-5)
        dx, dy = X - px, Y - py
        rng = np.sqrt(dx * dx + dy * dy)
        bearing = np.arctan2(-ps * dx + pc * dy, pc * dx + ps * dy)
        if live.any():
            margins["range"] = min(margins["range"], float(np.min(np.abs(rng[live] - cfg.max_range))))
        near = live & (rng < cfg.max_range)
        if near.any():
            arc = np.minimum(np.abs(bearing[near] - cfg.max_bearing), np.abs(bearing[near] - cfg.min_bearing)) * rng[near]
            margins["bearing"] = min(margins["bearing"], float(np.min(arc)))
        seen = near & (bearing < cfg.max_bearing) & (bearing > cfg.min_bearing)  # checkWithoutMinRange
        if seen.any():
            margins["thresh"] = min(margins["thresh"], float(np.min(np.abs(lo[seen] - (OCCUPIED_THRESH + 1e-8)))))
        occ = seen & (lo > OCCUPIED_THRESH + 1e-8)
        _update_cell(lo, np.nonzero(occ)[0], False)
        _update_cell(lo, np.nonzero(seen & ~occ)[0], True)
    return lo, margins


def probabilities(logodds, num_samples):
    """VirtualMap::updateProbability: the sum over num_samples identical maps of LOGODDS2PROB(l) / num_samples, per distinct value."""
    out = np.empty_like(logodds)
    for l in np.unique(logodds):
        p1, acc = _l2p(float(l)), 0.0
        for _ in range(num_samples):
            acc += p1 / num_samples
        out[logodds == l] = acc
    return out


def entropy(prob):
    return float(np.sum(-prob * np.log(prob) - (1.0 - prob) * np.log(1.0 - prob)))


def og_cost(sim, actions):
    """(entropy, cost, prob [rows, cols], margins) of the leaf that `actions` reach from the belief of `sim`."""
    cfg = sim.cfg
    actions = [tuple(float(v) for v in a) for a in actions]
    rows, cols = sim.vm_shape()
    lo, margins = occupancy_logodds(em_ref.leaf_poses(sim, actions), sim.landmarks()[1], cfg, rows, cols)
    prob = probabilities(lo, cfg.num_samples)
    h = entropy(prob)
    known = int(np.sum(sim.virtual_map()[0] < cfg.occupancy_threshold))  # the live map's
    dw = cfg.distance_weight0 - (cfg.distance_weight0 - cfg.distance_weight1) * (known / float(rows * cols))
    return h, h + em_ref.plan_distance(actions, cfg.angle_weight) * dw, prob.reshape(rows, cols), margins
