// The EM planner's tree sampler: the growth loop that EMPlanner2D::optimize2 (src/em_exploration/Planner2D.cpp:1058-1092) and
// EMPlanner2D::rrt_planner (:866-922) share, for the non-Dubins control model at safe_distance = 0 (isSafe is then always true and
// the `failed > 1000` counters cannot fire) -
//   initialize (:1281-1357)      root = the current pose estimate, distance 0; max_nodes_ = floor(#{p_v < occupancy_threshold} max_nodes)
//   sampleNode (:101-125)        Halton point number count++ in bases 2, 3, 5: x, y over the MAP's box, theta = 2 pi h2
//   nearestNode (:267-276, Distance.cpp:5-9, :24-35)   arg-min of range^2 + (angle_weight bearing)^2, the bearing taken from the tree
//                                node's frame to the sample's position; strict <, so the lowest node index wins a tie
//   connectNode (:188-216, :250-258)   angle = relative bearing of the sample in the parent's frame, len = min(d, max_edge_length),
//                                child = parent * Pose2(angle, (len cos, len sin)), edge odometry (len cos angle, len sin angle, angle),
//                                distance = parent.distance + sqrt(sqDistanceBetweenPoses(child, parent, angle_weight))
// and the two stop rules: optimize2 stops after max_nodes_ accepted nodes; rrt_planner stops when a new node lies within
// max_edge_length of the goal Pose2(gx, gy, pi) (isReached, :88-99) and then connects the goal to that node.
// Here: tree_init, sample_point, nearest_node, connect; the stop rules are the growth loop of k_em_tree, which is one turn for every
// instantiation - sample, nearest, connect, then the refused-counter or Tree::push, then the goal test and the same connect towards
// the goal; tree_enter checks the arguments, tree_finish writes the results.
//
// The chain of accepted nodes is strictly sequential - node k + 1 is attached to the nearest of nodes 0 .. k - and the only parallel
// work per sample is that arg-min.  ONE WAVE owns a tree: the node table (x y c s distance | parent depth children) lives in LDS
// (struct Tree), lanes stride over the nodes and reduce (distance, index) by butterfly with the lowest index on equal distance
// (wave_argmin), every lane then holds the winner and computes the same child; lane 0 stores it (Tree::push).  A single wave needs
// no cross-wave exchange per sample (a 256-thread workgroup pays two barriers and an LDS round per sample to save at most three
// strides of the arg-min at a few hundred nodes; DESIGN.md section 4 has the comparison).  Every loop is bounded by the node capacity
// `cap`: each turn of the growth loop accepts exactly one node, so a tree that cannot finish ends with a capacity result instead of
// spinning.
//
//
// THE OBSTACLE LOGIC (kSafe = true; the engine launches it only behind drlgx_set_sampler_obstacles and a safe_distance > 0 - with
// kSafe = false none of it is compiled in) adds, restated from the same file:
//   isSafe(node) (:48-56; Distance.cpp:78-97)   unsafe iff an estimated landmark of the environment lies strictly nearer than
//                                safe_distance (a negative radius finds nothing).  Each lane keeps one landmark in registers (lanes
//                                stride the rest), a ballot decides: only emptiness is asked, the landmarks' order does not matter
//                                (point_safe)
//   sampleNode (:101-125)        Halton points until one is safe, every drawn point consumed; the 1001st unsafe point of one call
//                                ends the tree with SAMPLING_FAILURE (sample_point)
//   isSafe(node, parent) (:58-86), asked by connectNode after the child is scaled (:243-248): |safe_distance| < 1e-3 tests nothing;
//                                else d = range(child, parent), unit = the child's position in the PARENT's frame / d, and for
//                                l = sd/2; l < d; l += sd/2 (repeated addition, strict <) the point child.transform_from(l unit).
//                                AS WRITTEN IN THE REFERENCE these points lie BEYOND the child, in the direction of the child's
//                                heading turned by the edge's bearing once more - not between parent and child.  Reproduced as
//                                written: this project follows the reference's behaviour.  Waypoints serially, landmarks in
//                                parallel, out at the first unsafe one (the branch is wave-uniform); at most 2 max_edge_length /
//                                1e-3 turns (d <= max_edge_length, the step is at least 5e-4) (edge_safe, asked by connect)
//   the connect counter (:1070-1079, :890-899)   a refused connect adds no node; the 1001st in a row ends the tree (the growth loop)
//   the shrink (:1046-1054, :841-849)   when the root is nearer than safe_distance to its nearest estimated landmark, the call's
//                                safe_distance is that distance - 0.1 (optimize2: not below 0; rrt_planner: unclamped) - IF the
//                                landmark's KEY is smaller than the NUMBER of landmarks: searchLandmarkNearest returns the key
//                                (Simulator2D.cpp:394-403: landmarks in key order, strict <, so the lowest key wins a tie) and the
//                                planner compares it with getLandmarkSize().  Kept as it is (tree_shrink)
//   rrt_planner's goal edge (:910-922)   a goal whose edge is unsafe is not in the tree: SUCCESS, no leaf, an empty plan
// ONE DEVIATION: in rrt_planner a shrunk safe_distance below -1e-3 (the root within 0.099 m of a landmark) makes the reference's
// waypoint loop run for ever - a negative step, l < d always true.  Such a tree ends at once with SAMPLING_FAILURE, the root alone,
// no point drawn (tree_shrink).
// A tree that ends with SAMPLING_FAILURE keeps the nodes accepted so far, has no leaf and no plan; the other trees of the launch are
// not concerned, and the flag is not touched: a sampling failure is a result.  Loop bounds: cap accepted nodes, the two counters of
// 1000, the waypoint bound.
//
//
// THE DUBINS CONTROL MODEL (kDubins = true; launched when drlgx_set_dubins_library_host has loaded a library and the sampler's Dubins
// flag is set - for optimize2 behind drlgx_set_dubins_leaf_scoring as well: the same growth loop, its stop rule and its shrink) replaces the body of connectNode - connect<kSafe, true> -, restated from the same file:
//   the library (:1359-1414)     built by the engine on the host, SoA: the end point of every (v, w, duration) path from Pose2(0, 0, 0)
//   sampleNode (:41-45, :110-115)   the generator has dimension 2: the same x, y in bases 2 and 3; the sample's theta is 0 and unread
//   connectNodeDubinsPath (:157-176)   local = the sample in the parent's frame; the FIRST entry in library order with
//                                |local - end_i| < tolerance_radius (strict) wins: lanes stride the library in index order, a ballot
//                                per stride takes the lowest matching lane of the first stride that has one, and the scan ends
//                                there.  A scan that cannot match is skipped: |local| > (max_i |end_i| + tolerance_radius)(1 +
//                                2^-30) implies |local - end_i| > tolerance_radius for every i by the triangle inequality, the factor
//                                covering the roundings of the three square roots many times over (an infinite bound switches the
//                                skip off: drlgx_set_dubins_prefilter) (dubins_match).  Every thread then integrates the entry's
//                                num_steps Euler steps from the PARENT's pose - x += v dt cos, y += v dt sin, theta = atan2(sin, cos)
//                                + w dt, the angle through (cos, sin) at every step as Pose2(x, y, theta) does (dubins_step); the
//                                node is the last pose
//   isSafe(node, parent) (:59-70)   |safe_distance| < 1e-3 tests nothing; else poses 1 .. num_steps - 2 (the first and the last are
//                                not tested) each pass isSafe(point): steps serially, landmarks in parallel, out at the first
//                                unsafe one.  There is no waypoint loop, so a negative shrunk safe_distance is no deviation here
//   connectNode (:179-265, :295-300)   no scaling to max_edge_length and no bearing test; no match or an unsafe pose refuses the
//                                connect - the counter of 1000 runs at safe_distance = 0 too; key = parent.key + num_steps (the
//                                node's depth counts STEPS), distance = parent.distance + v dt n + |w dt n| angle_weight
//   the goal edge (:915)         connectNode(goal, node): the goal joins only if a library path from the node ends within
//                                tolerance_radius of it and is safe - the goal NODE is that path's last pose; else SUCCESS, no plan
// The node's edge record is (library index, num_steps, 0) instead of an odometry; k_em_leaves_dubins replays the steps for the plans
// and, for optimize2, marks each edge's last step as the core pose of the leaf evaluation (k_em.hip, k_fm2.hip).
// Loop bounds: the library size, the largest num_steps, cap, the two counters of 1000.
//
// The live belief is only read.  Built with -ffp-contract=off: the nearest-node comparison and the safety tests are gates.
#include "drlgx_dev.h"

#ifndef DRLGX_EM_TREE_THREADS
#define DRLGX_EM_TREE_THREADS 64
#endif

namespace kemt {

constexpr int kT = DRLGX_EM_TREE_THREADS;
constexpr int kWaves = kT / 64;
constexpr int kNd = 5, kNi = 3;  // per node: x y c s distance | parent depth children
constexpr int kNodeOut = 8;      // doubles per node of nodes_out
enum { M_NODES = 0, M_LEAVES = 1, M_HALTON = 2, M_RESULT = 3, M_STRIDE = 4 };
enum { R_SAMPLING_FAILURE = 0, R_SUCCESS = 3 };  // EMPlanner2D::OptimizationResult
constexpr int kMaxFailed = 1000;     // `failed > 1000` of sampleNode and of the growth loops
constexpr double kEdgeEps = 1e-3;    // |safe_distance| below which isSafe(node, parent) tests nothing

__host__ __device__ inline size_t lds_bytes(int cap) {
  return (size_t)cap * (kNd * sizeof(double) + kNi * sizeof(int)) + 2 * kWaves * sizeof(double) + 64;
}

// Radical inverse of `index` in `base`: sum_k d_k base^-(k+1) over ALL digits d_k of the index (the Halton sequence's definition).
// 32 digits cover every int in base 2.
__device__ __forceinline__ double radical_inverse(int index, int base) {
  double f = 1.0, r = 0.0;
  for (int k = 0; k < 32 && index > 0; ++k) {
    f = f / (double)base;
    r = r + f * (double)(index % base);
    index /= base;
  }
  return r;
}

// sqDistanceBetweenPoses(pose1, pose2 at pt, angle_weight) (Distance.cpp:5-9)
__device__ __forceinline__ double sq_distance(const Pose &p1, const P2 &pt, double angle_weight, double &bearing) {
  const double range = range_of<false>(p1, pt, nullptr, nullptr);
  bearing = bearing_of<false>(p1, pt, nullptr, nullptr);
  const double wb = bearing * angle_weight;
  return range * range + wb * wb;
}

// (value, index) of one wave's minimum, the lowest index on equal value, in every lane
__device__ __forceinline__ void wave_argmin(double &v, int &i) {
  for (int m = 1; m < 64; m <<= 1) {
    const double ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    if (ov < v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

// One tree in LDS, carved once from the workgroup's dynamic LDS (lds_bytes(cap)): the node table, the slots of the cross-wave
// exchanges, and the tree's act rows in memory (the edge record of every node).
struct Tree {
  double *nd;     // [cap][kNd] x y c s distance
  int *ni;        // [cap][kNi] parent depth children
  double *red_d;  // [kWaves]
  int *red_i;     // [kWaves]
  double *ta;     // [cap][3], memory
  int n;          // nodes so far

  __device__ __forceinline__ Tree(double *smem, int cap, double *act_rows)
      : nd(smem), ni(reinterpret_cast<int *>(smem + (size_t)cap * kNd + 2 * kWaves)), red_d(smem + (size_t)cap * kNd),
        red_i(reinterpret_cast<int *>(smem + (size_t)cap * kNd + kWaves)), ta(act_rows), n(0) {}

  __device__ __forceinline__ Pose pose(int j) const { return Pose{nd[kNd * j], nd[kNd * j + 1], nd[kNd * j + 2], nd[kNd * j + 3]}; }
  __device__ __forceinline__ double dist(int j) const { return nd[kNd * j + 4]; }
  __device__ __forceinline__ int parent(int j) const { return ni[kNi * j]; }
  __device__ __forceinline__ int depth(int j) const { return ni[kNi * j + 1]; }
  __device__ __forceinline__ bool is_leaf(int j) const { return ni[kNi * j + 2] == 0; }

  // node n, a child of `parent` (-1: the root); every thread calls it with the same values, lane 0 stores
  __device__ __forceinline__ void push(int parent, const Pose &child, double dist, int depth, double act0, double act1, double act2) {
    __syncthreads();  // (every thread has read the table)
    if (threadIdx.x == 0) {
      nd[kNd * n] = child.x; nd[kNd * n + 1] = child.y; nd[kNd * n + 2] = child.c; nd[kNd * n + 3] = child.s;
      nd[kNd * n + 4] = dist;
      ni[kNi * n] = parent; ni[kNi * n + 1] = depth; ni[kNi * n + 2] = 0;
      if (parent >= 0) ni[kNi * parent + 2] += 1;
      ta[3 * n] = act0; ta[3 * n + 1] = act1; ta[3 * n + 2] = act2;
    }
    __syncthreads();
    ++n;
  }
};

// (distance, index) of the whole workgroup's minimum, lowest index on equal distance, in every thread
__device__ __forceinline__ void argmin_all(double &d, int &idx, const Tree &t) {
  wave_argmin(d, idx);
  if (kWaves > 1) {
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // (the previous round's readers are done)
    if ((threadIdx.x & 63) == 0) {
      t.red_d[wave] = d;
      t.red_i[wave] = idx;
    }
    __syncthreads();
    d = t.red_d[0];
    idx = t.red_i[0];
    for (int w = 1; w < kWaves; ++w)
      if (t.red_d[w] < d || (t.red_d[w] == d && t.red_i[w] < idx)) {
        d = t.red_d[w];
        idx = t.red_i[w];
      }
  }
}

// The estimated landmarks of one environment as the safety tests read them: landmark `lane` in registers (+inf where there is
// none: its distance is never below a radius), the ones from 64 on in memory.  Every wave holds all of them.
struct Obstacles {
  double x, y;
  const double *el;
  int L;
};

// What tree_shrink leaves for the call's safety tests (kSafe = false reads none of it)
struct Safety {
  Obstacles ob;
  double sd;     // the call's safe_distance, shrunk or not
  int wp_bound;  // the waypoint loop's bound
};

// isSafe(node): no landmark strictly nearer than sd; the same answer in every thread
__device__ __forceinline__ bool point_safe(const P2 &pt, const Obstacles &ob, double sd) {
  if (sd < 0.0) return true;
  const int lane = threadIdx.x & 63;
  const double dx = ob.x - pt.x, dy = ob.y - pt.y;
  bool hit = sqrt(dx * dx + dy * dy) < sd;
  for (int j = lane + 64; j < ob.L; j += 64) {
    const double ex = ob.el[2 * j] - pt.x, ey = ob.el[2 * j + 1] - pt.y;
    hit = hit || sqrt(ex * ex + ey * ey) < sd;
  }
  return __ballot(hit) == 0ull;
}

// isSafe(node, parent), non-Dubins: the waypoints as the reference writes them (beyond the child - see the head of the file)
__device__ __forceinline__ bool edge_safe(const Pose &child, const Pose &par, const Safety &sf) {
  if (fabs(sf.sd) < kEdgeEps) return true;
  const double d = range_of<false>(child, P2{par.x, par.y}, nullptr, nullptr);
  const P2 loc = transform_to(par, P2{child.x, child.y});
  const double half = sf.sd / 2;
  double l = half;
  for (int w = 0; w < sf.wp_bound && l < d; ++w) {  // (d == 0: no waypoint)
    const double inv = 1.0 / d;
    const P2 unit{inv * loc.x, inv * loc.y};
    if (!point_safe(transform_from(child, P2{l * unit.x, l * unit.y}), sf.ob, sf.sd)) return false;
    l += half;
  }
  return true;
}

// connectNodeDubinsPath's search: the lowest library index whose end point lies strictly within the tolerance radius of `local`, or
// -1; the same answer in every thread.  At most ceil(n / kT) strides.
__device__ __forceinline__ int dubins_match(const DrlgxDubins &lib, const P2 &local, int *red_i) {
  if (sqrt(local.x * local.x + local.y * local.y) > lib.reach) return -1;  // (provably no match - see the head of the file)
  const int tid = threadIdx.x, lane = tid & 63;
  for (int base = 0; base < lib.n; base += kT) {
    const int i = base + tid;
    bool hit = false;
    if (i < lib.n) {
      const double dx = lib.end_x[i] - local.x, dy = lib.end_y[i] - local.y;
      hit = sqrt(dx * dx + dy * dy) < lib.tol;
    }
    const unsigned long long b = __ballot(hit);
    int first = b ? base + (tid - lane) + (int)__builtin_ctzll(b) : 0x7fffffff;
    if (kWaves > 1) {
      __syncthreads();  // (the previous round's readers are done)
      if (lane == 0) red_i[tid >> 6] = first;
      __syncthreads();
      first = red_i[0];
      for (int w = 1; w < kWaves; ++w) first = min(first, red_i[w]);
    }
    if (first != 0x7fffffff) return first;
  }
  return -1;
}

// One Euler step of the Dubins model, the angle through (cos, sin) as Pose2(x, y, theta) takes it
__device__ __forceinline__ Pose dubins_step(const Pose &p, double vdt, double wdt) {
  const double x = p.x + vdt * p.c, y = p.y + vdt * p.s, th = atan2(p.s, p.c) + wdt;
  return Pose{x, y, cos(th), sin(th)};
}

// What connectNode adds to its parent: the child's pose, distanceBetweenNodes, the depth the child gains (1; Dubins: the path's
// steps) and the node's act row: the edge odometry - or, Dubins, (entry, depth, 0), kept as the integers they are until the push
// (as doubles they cost the Dubins loops six registers)
struct Edge {
  Pose child;
  double dist;
  int depth;
  double ax, ay, angle;
  int entry;
};

// connectNode from `par` towards `target`, the sampled point or the goal, every thread alike: false = refused (kSafe: an unsafe
// edge; kDubins: no library path, or an unsafe intermediate pose).  Without kSafe and kDubins it cannot refuse.
template <bool kSafe, bool kDubins>
__device__ __forceinline__ bool connect(const Pose &par, const P2 &target, const drlgx_config &cfg, const Safety &sf, const DrlgxDubins &lib,
                                        int *red_i, Edge &e) {
  if (kDubins) {
    const int m = dubins_match(lib, transform_to(par, target), red_i);
    if (m < 0) return false;
    const double v = lib.v[m], w = lib.w[m];
    const int ns = min(lib.num_steps[m], lib.max_steps);
    const double vdt = v * lib.dt, wdt = w * lib.dt;
    const bool test = kSafe && !(fabs(sf.sd) < kEdgeEps);
    e.child = par;
    for (int step = 0; step < ns; ++step) {
      e.child = dubins_step(e.child, vdt, wdt);
      if (test && step >= 1 && step <= ns - 2 && !point_safe(P2{e.child.x, e.child.y}, sf.ob, sf.sd)) return false;
    }
    e.dist = vdt * (double)ns + fabs(wdt * (double)ns) * cfg.angle_weight;
    e.depth = ns;
    e.entry = m;
    return true;
  }
  const double d = range_of<false>(par, target, nullptr, nullptr);
  const double angle = bearing_of<false>(par, target, nullptr, nullptr);
  const double len = d > cfg.max_edge_length ? cfg.max_edge_length : d;
  e.ax = len * cos(angle); e.ay = len * sin(angle); e.angle = angle;
  e.child = compose(par, make_pose(e.ax, e.ay, angle));
  if (kSafe && !edge_safe(e.child, par, sf)) return false;  // isSafe(node, parent) on the scaled child
  double bb;
  e.dist = sqrt(sq_distance(e.child, P2{par.x, par.y}, cfg.angle_weight, bb));
  e.depth = 1;
  return true;
}

// The edge's child becomes node t.n, at `dist` and `depth` from the root
template <bool kDubins>
__device__ __forceinline__ void push_edge(Tree &t, int parent, const Edge &e, double dist, int depth) {
  if (kDubins) t.push(parent, e.child, dist, depth, (double)e.entry, (double)e.depth, 0.0);
  else t.push(parent, e.child, dist, depth, e.ax, e.ay, e.angle);
}

// Where one tree reads its belief and leaves its counts
struct Belief {
  int P, L;
  const double *ep, *el;  // the estimated poses (x y c s) and landmarks
  const int *lk;          // the landmarks' keys
  int *mt;                // the tree's meta row
};

// How a tree ended, for tree_finish
struct Outcome {
  int count;      // the next Halton index
  int max_depth;  // of the plans the tree offers
  int goal_node;  // rrt: the goal's node, -1: not in the tree
  bool sampling_failed, full;  // full: the table filled before the stop rule was met
};

// The argument checks, with the one invalid exit: false = this workgroup has no tree to grow
__device__ __forceinline__ bool tree_enter(const DrlgxState &S, const DrlgxTreeArgs &a, int ti, Belief &b) {
  if (ti >= a.n_sel) return false;
  const int env = a.env_sel[ti];
  b.mt = a.meta + (size_t)ti * M_STRIDE;
  bool ok = env >= 0 && env < S.n_envs && a.cap >= 1;
  if (ok) {
    const int *cnt = S.cnt + (size_t)env * DRLGX_CNT_STRIDE;
    b.P = cnt[C_P];
    b.L = cnt[C_L];
    ok = b.P >= 1 && b.P <= S.P_max && b.L >= 0 && b.L <= S.L_max;
  }
  if (!ok) {
    if (threadIdx.x == 0) {
      atomicMin(a.flag, DRLGX_E_INVALID);
      b.mt[M_NODES] = b.mt[M_LEAVES] = 0;
    }
    return false;
  }
  b.ep = S.est_pose + (size_t)env * S.P_max * 4;
  b.el = S.est_lm + (size_t)env * S.L_max * 2;
  b.lk = S.lm_key + (size_t)env * S.L_max;
  return true;
}

// initialize: max_nodes_ from the known cells (mode 0: the accepted nodes the stop rule allows), the goal from key or point (mode
// 1), the root
__device__ __forceinline__ void tree_init(const DrlgxState &S, const DrlgxTreeArgs &a, const Belief &b, int ti, Tree &t, int &budget,
                                          P2 &goal) {
  const int tid = threadIdx.x, lane = tid & 63, env = a.env_sel[ti], P = b.P, L = b.L;
  budget = 0x7fffffff;
  if (a.mode == 0) {
    const double *prob = S.vm_prob + (size_t)env * S.V;
    int known = 0;
    for (int v = tid; v < S.V; v += kT) known += prob[v] < S.cfg.occupancy_threshold ? 1 : 0;
    double kd = (double)known;
    for (int m = 1; m < 64; m <<= 1) kd += __shfl_xor(kd, m, 64);
    if (kWaves > 1) {
      __syncthreads();
      if (lane == 0) t.red_d[tid >> 6] = kd;
      __syncthreads();
      kd = 0.0;
      for (int w = 0; w < kWaves; ++w) kd += t.red_d[w];
      __syncthreads();
    }
    const double mn = floor(kd * a.max_nodes);
    budget = mn < 0.0 ? 0 : (mn > 2147483647.0 ? 0x7fffffff : (int)mn);
  }
  goal = P2{0.0, 0.0};
  if (a.mode == 1) {
    // the goal: graph node goal_key (landmarks in key order, then poses - the order of the exported graph) or the frontier point
    const int gk = a.goal_key[ti];
    goal = P2{a.goal_xy[2 * ti], a.goal_xy[2 * ti + 1]};
    if (gk >= 0 && gk < L) {
      int slot = 0x7fffffff;  // the slot whose key has rank gk
      for (int j = lane; j < L; j += 64) {
        int rank = 0;
        for (int q = 0; q < L; ++q) rank += b.lk[q] < b.lk[j] ? 1 : 0;
        if (rank == gk) slot = min(slot, j);
      }
      for (int m = 1; m < 64; m <<= 1) slot = min(slot, __shfl_xor(slot, m, 64));
      if (slot < L) goal = P2{b.el[2 * slot], b.el[2 * slot + 1]};
    } else if (gk >= L && gk < L + P) {
      goal = P2{b.ep[4 * (gk - L)], b.ep[4 * (gk - L) + 1]};
    }
  }
  const double *root = b.ep + 4 * (P - 1);
  t.push(-1, Pose{root[0], root[1], root[2], root[3]}, 0.0, 0, 0.0, 0.0, 0.0);
}

// The call's safety tests: the landmark registers and - the shrink - the call's safe_distance.  kSafe = false: nothing to test.
// failed: rrt_planner's deviation, the tree ends before a point is drawn.
template <bool kSafe, bool kDubins>
__device__ __forceinline__ Safety tree_shrink(const drlgx_config &cfg, const DrlgxTreeArgs &a, const Belief &b, bool &failed) {
  Safety sf{Obstacles{__builtin_huge_val(), __builtin_huge_val(), b.el, b.L}, a.safe_distance, 0};
  if (!kSafe) return sf;
  const int lane = threadIdx.x & 63, L = b.L;
  if (lane < L) {
    sf.ob.x = b.el[2 * lane];
    sf.ob.y = b.el[2 * lane + 1];
  }
  // searchLandmarkNearest: the landmarks in key order, strict < - the arg-min of (distance, key); what comes back is the KEY
  const double rx = b.ep[4 * (b.P - 1)], ry = b.ep[4 * (b.P - 1) + 1];
  double bd = __builtin_huge_val();
  int bk = 0x7fffffff;
  for (int j = lane; j < L; j += 64) {
    const double dx = b.el[2 * j] - rx, dy = b.el[2 * j + 1] - ry;
    const double dj = sqrt(dx * dx + dy * dy);
    if (dj < bd || (dj == bd && b.lk[j] < bk)) {
      bd = dj;
      bk = b.lk[j];
    }
  }
  wave_argmin(bd, bk);
  // (no landmark: the reference's search answers 1, which is not below 0.)  The key against the NUMBER of landmarks, as written
  if (L > 0 && bk >= 0 && bk < L && bd < sf.sd) sf.sd = a.mode == 0 ? (bd - 0.1 > 0.0 ? bd - 0.1 : 0.0) : bd - 0.1;
  // the deviation: rrt_planner's waypoint loop would not end
  if (!kDubins && a.mode == 1 && sf.sd < -kEdgeEps) failed = true;
  const double wb = 2.0 * cfg.max_edge_length / kEdgeEps + 2.0;
  sf.wp_bound = wb < 2147483647.0 ? (int)wb : 0x7fffffff;
  return sf;
}

// sampleNode: Halton point number count++ over the map's box.  (The sample's own heading, theta = 2 pi h2 with h2 the radical
// inverse in base 5, enters nothing - nearestNode and connectNode read the sample's position only, the child's heading is the
// parent's plus the bearing - so the third coordinate of the point is not evaluated; the point is consumed all the same.)
// kSafe: points are drawn until one is safe, each one consumed; false = the 1001st unsafe one, which ends the tree.
template <bool kSafe>
__device__ __forceinline__ bool sample_point(const drlgx_config &cfg, const Safety &sf, int &count, P2 &sp) {
  const double span_x = cfg.map_max_x - cfg.map_min_x, span_y = cfg.map_max_y - cfg.map_min_y;
  for (int u = 0; u <= (kSafe ? kMaxFailed : 0); ++u) {
    const double h0 = radical_inverse(count, 2), h1 = radical_inverse(count, 3);
    ++count;
    sp = P2{cfg.map_min_x + h0 * span_x, cfg.map_min_y + h1 * span_y};
    if (!kSafe || point_safe(sp, sf.ob, sf.sd)) return true;
  }
  return false;
}

// nearestNode: the node with the smallest sq_distance to the sample, the lowest index on equal distance
__device__ __forceinline__ int nearest_node(const Tree &t, const P2 &sp, double angle_weight) {
  double best = __builtin_huge_val();
  int bi = 0x7fffffff;
  for (int j = threadIdx.x; j < t.n; j += kT) {
    double b;
    const double dj = sq_distance(t.pose(j), sp, angle_weight, b);
    if (dj < best) {
      best = dj;
      bi = j;
    }
  }
  argmin_all(best, bi, t);
  return bi < 0 || bi >= t.n ? 0 : bi;  // (only a NaN distance to every node could leave no winner)
}

// The results: the tables to memory, the leaves in node order, meta and the flag
template <bool kDubins>
__device__ __forceinline__ void tree_finish(const DrlgxState &S, const DrlgxTreeArgs &a, const Belief &b, int ti, const Tree &t,
                                            const Outcome &r) {
  const int tid = threadIdx.x, lane = tid & 63, n = t.n, cap = a.cap;
  int *tl = a.link + (size_t)ti * cap * 2, *lf = a.leaf + (size_t)ti * cap;
  for (int j = tid; j < n; j += kT) {
    const Pose p = t.pose(j);
    tl[2 * j] = t.parent(j);
    tl[2 * j + 1] = t.depth(j);
    if (kDubins) {
      double *o = a.lib.pose + ((size_t)ti * cap + j) * 4;
      o[0] = p.x; o[1] = p.y; o[2] = p.c; o[3] = p.s;
    }
    if (a.nodes_out) {
      double *o = a.nodes_out + ((size_t)ti * cap + j) * kNodeOut;
      o[0] = p.x; o[1] = p.y;
      o[2] = atan2(p.s, p.c);
      o[3] = (double)t.parent(j);
      o[4] = t.dist(j);
      o[5] = t.ta[3 * j]; o[6] = t.ta[3 * j + 1]; o[7] = t.ta[3 * j + 2];
    }
  }
  int n_leaves = 0;
  if (a.mode == 0 && !r.sampling_failed) {
    if (tid < 64) {  // (one wave lists: node order)
      for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const bool is_leaf = j < n && t.is_leaf(j);
        const unsigned long long bl = __ballot(is_leaf);
        if (is_leaf) lf[n_leaves + __popcll(bl & ((1ull << lane) - 1ull))] = j;
        n_leaves += __popcll(bl);
      }
    }
  } else if (r.goal_node >= 0) {
    if (tid == 0) lf[0] = r.goal_node;
    n_leaves = 1;
  }
  if (tid == 0) {
    const int res = ((a.mode == 1 && r.full) || r.sampling_failed) ? R_SAMPLING_FAILURE : R_SUCCESS;
    b.mt[M_NODES] = n;
    b.mt[M_LEAVES] = n_leaves;
    b.mt[M_HALTON] = r.count;
    b.mt[M_RESULT] = res;
    if (a.n_nodes_out) a.n_nodes_out[ti] = n;
    if (a.result_out) a.result_out[ti] = res;
    if (a.halton_next_out) a.halton_next_out[ti] = r.count;
    // what the whole call is refused for: optimize2's tree does not fit the table; a plan deeper than max_actions
    // (a tree that failed to sample offers no plan: nothing of it can be too deep)
    if ((a.mode == 0 && r.full) || (((a.mode == 0 && !r.sampling_failed) || r.goal_node >= 0) && r.max_depth > S.A_max))
      atomicMin(a.flag, DRLGX_E_CAPACITY);
  }
}

// One tree per workgroup (DrlgxTreeArgs in drlgx_dev.h).  kSafe: the obstacle logic with the planner parameter safe_distance (> 0);
// kSafe = false never reads it.  kDubins: the Dubins control model with the library a.lib (either mode; kDubins = false never reads
// it).  Growth: one accepted node per turn - or, kSafe || kDubins, one refused connect, at most kMaxFailed in a row.
template <bool kSafe, bool kDubins>
__global__ __launch_bounds__(kT) void k_em_tree(DrlgxState S, DrlgxTreeArgs a) {
  extern __shared__ __attribute__((aligned(16))) double tree_smem[];
  const int ti = blockIdx.x, cap = a.cap, mode = a.mode;
  Belief b;
  if (!tree_enter(S, a, ti, b)) return;
  const drlgx_config &cfg = S.cfg;
  Tree t(tree_smem, cap, a.act + (size_t)ti * cap * 3);
  int budget;
  P2 goal;
  tree_init(S, a, b, ti, t, budget, goal);
  Outcome r{a.halton_start[ti], 0, -1, false, false};
  const Safety sf = tree_shrink<kSafe, kDubins>(cfg, a, b, r.sampling_failed);
  bool goal_refused = false;
  int failed = 0;
  const long long max_turns = kSafe || kDubins ? (long long)cap * (kMaxFailed + 2) : (long long)cap;
  for (long long turn = 0; turn < max_turns && !r.sampling_failed; ++turn) {
    if (mode == 0 && t.n - 1 >= budget) break;
    if (t.n >= cap) {
      r.full = true;
      break;
    }
    P2 sp{0.0, 0.0};
    if (!sample_point<kSafe>(cfg, sf, r.count, sp)) {
      r.sampling_failed = true;
      break;
    }
    const int bi = nearest_node(t, sp, cfg.angle_weight);
    const Pose par = t.pose(bi);
    Edge e;
    if (!connect<kSafe, kDubins>(par, sp, cfg, sf, a.lib, t.red_i, e)) {  // a refused connect adds no node
      if (++failed > kMaxFailed) {
        r.sampling_failed = true;
        break;
      }
      continue;
    }
    failed = 0;
    const int node = t.n, depth = t.depth(bi) + e.depth;
    const double dist = t.dist(bi) + e.dist;
    push_edge<kDubins>(t, bi, e, dist, depth);
    r.max_depth = max(r.max_depth, depth);
    // isReached(goal, node), then connectNode(goal, node): the goal Pose2(gx, gy, pi) becomes a child of the node that reached it
    const double gx = e.child.x - goal.x, gy = e.child.y - goal.y;
    if (mode == 1 && sqrt(gx * gx + gy * gy) <= cfg.max_edge_length) {
      if (t.n >= cap) {
        r.full = true;
        break;
      }
      Edge g;
      if (!connect<kSafe, kDubins>(e.child, goal, cfg, sf, a.lib, t.red_i, g)) {
        goal_refused = true;  // the loop ends all the same (:910-922, :915): SUCCESS, the goal not in the tree, no plan
        break;
      }
      r.goal_node = t.n;
      r.max_depth = depth + g.depth;  // (of the plan: the path to the goal, in edges or - Dubins - steps)
      push_edge<kDubins>(t, node, g, dist + g.dist, depth + g.depth);
      break;
    }
  }
  if (mode == 1 && r.goal_node < 0 && !r.sampling_failed && !goal_refused) r.full = true;  // (the turns ran out: the table is full)
  tree_finish<kDubins>(S, a, b, ti, t, r);
}

// The sum of the leaf counts before tree ti: its first candidate.  One wave, the same answer in every lane
__device__ __forceinline__ int leaf_offset(const int *meta, int ti) {
  int off = 0;
  for (int q = threadIdx.x; q < ti; q += 64) off += meta[(size_t)q * M_STRIDE + M_LEAVES];
  for (int m = 1; m < 64; m <<= 1) off += __shfl_xor(off, m, 64);
  return off;
}

// An empty plan: the row zero, n_actions = 0.  One wave
__device__ __forceinline__ void empty_plan(double *row, int32_t *n_actions, int A_max) {
  for (int q = threadIdx.x; q < 3 * A_max; q += 64) row[q] = 0.0;
  if (threadIdx.x == 0) *n_actions = 0;
}

// The action lists root -> leaf of every listed leaf, in the [cand][max_actions][3] layout drlgx_em_cost reads (zero behind the
// plan), with cand_env and n_actions.  Tree ti's first candidate is the sum of the leaf counts before it - or, per_tree_row, row ti
// (rrt: one plan per tree, none for a tree that failed).
__global__ __launch_bounds__(64) void k_em_leaves(int n_sel, const int32_t *env_sel, int cap, int A_max, const double *act, const int *link,
                                                  const int *leaf, const int *meta, int per_tree_row, int32_t *cand_env, double *actions,
                                                  int32_t *n_actions) {
  const int ti = blockIdx.x, lane = threadIdx.x;
  if (ti >= n_sel) return;
  const int off = per_tree_row ? ti : leaf_offset(meta, ti);
  const int nl = meta[(size_t)ti * M_STRIDE + M_LEAVES];
  const double *ta = act + (size_t)ti * cap * 3;
  const int *tl = link + (size_t)ti * cap * 2, *lf = leaf + (size_t)ti * cap;
  if (per_tree_row && nl == 0) {
    empty_plan(actions + (size_t)off * A_max * 3, n_actions + off, A_max);
    return;
  }
  for (int k = lane; k < nl; k += 64) {
    const int node = lf[k], depth = tl[2 * node + 1];
    const size_t c = (size_t)off + k;
    double *row = actions + c * A_max * 3;
    if (cand_env) cand_env[c] = env_sel[ti];
    n_actions[c] = depth;
    int j = node;
    for (int s = depth - 1; s >= 0 && j > 0; --s) {  // (at most depth <= cap - 1 parents)
      if (s < A_max) {
        row[3 * s] = ta[3 * j]; row[3 * s + 1] = ta[3 * j + 1]; row[3 * s + 2] = ta[3 * j + 2];
      }
      j = tl[2 * j];
    }
    for (int s = depth; s < A_max; ++s) row[3 * s] = row[3 * s + 1] = row[3 * s + 2] = 0.0;
  }
}

// The plans under the Dubins model: one row per STEP root -> leaf, Edge::getOdoms (Planner2D.h:143-151) - between(previous pose,
// this pose), the origin moving along -, the steps integrated again from the parent's stored pose and the node's library entry.
// per_tree_row (rrt_planner): row ti of the outputs is the path to the goal; a tree without a goal node has the empty plan.  Else
// (optimize2) every listed leaf is a candidate of drlgx_em_cost_steps, tree ti's first at the sum of the leaf counts before it, with
// cand_env, the core mask - 1 at the last step of every edge, the only pose of an edge that updateTrajectory_EM puts into the
// leaf's map (Planner2D.cpp:498) - and the leaf's distance, the edges' v dt n + |w dt n| angle_weight summed from the root down as
// the tree summed them (:293-303).  One wave per tree, the leaves one after the other; lane q takes the q-th node of the path from
// the leaf up (at most cap - 1 parents); n_actions = the leaf's depth in steps (<= A_max: a deeper leaf has refused the call).
__global__ __launch_bounds__(64) void k_em_leaves_dubins(int n_sel, const int32_t *env_sel, int cap, int A_max, double angle_weight,
                                                         const double *act, const int *link, const int *leaf, const int *meta,
                                                         DrlgxDubins lib, int per_tree_row, int32_t *cand_env, double *actions,
                                                         int32_t *n_actions, uint8_t *core, double *distance) {
  const int ti = blockIdx.x, lane = threadIdx.x;
  if (ti >= n_sel) return;
  const int off = per_tree_row ? ti : leaf_offset(meta, ti);
  const int nl = meta[(size_t)ti * M_STRIDE + M_LEAVES];
  const double *ta = act + (size_t)ti * cap * 3, *tp = lib.pose + (size_t)ti * cap * 4;
  const int *tl = link + (size_t)ti * cap * 2, *lf = leaf + (size_t)ti * cap;
  if (per_tree_row && nl == 0) {
    empty_plan(actions + (size_t)off * A_max * 3, n_actions + off, A_max);
    return;
  }
  for (int k = 0; k < nl; ++k) {
    const size_t c = (size_t)off + k;
    const int node = lf[k], total = tl[2 * node + 1];
    double *row = actions + c * A_max * 3;
    for (int q = lane; q < 3 * A_max; q += 64)
      if (q >= 3 * total) row[q] = 0.0;
    if (core) {
      for (int q = lane; q < A_max; q += 64) core[c * A_max + q] = 0;
      __syncthreads();  // (the ones below come from other lanes)
    }
    if (lane == 0) {
      n_actions[c] = total;
      if (cand_env) cand_env[c] = env_sel[ti];
    }
    int j = node;
    for (int q = 0; q < lane && j > 0; ++q) j = tl[2 * j];
    for (int turn = 0; turn < cap && j > 0; turn += 64) {
      const int par = tl[2 * j], m = (int)ta[3 * j];
      const int ns = min((int)ta[3 * j + 1], lib.max_steps), first = tl[2 * j + 1] - ns;
      if (m >= 0 && m < lib.n && par >= 0 && par < cap) {
        const double vdt = lib.v[m] * lib.dt, wdt = lib.w[m] * lib.dt;
        Pose p{tp[4 * par], tp[4 * par + 1], tp[4 * par + 2], tp[4 * par + 3]};
        for (int s = 0; s < ns; ++s) {
          const Pose nx = dubins_step(p, vdt, wdt);
          const Pose od = between(p, nx, nullptr);
          if (first + s >= 0 && first + s < A_max) {
            row[3 * (first + s)] = od.x; row[3 * (first + s) + 1] = od.y; row[3 * (first + s) + 2] = theta_of(od);
          }
          p = nx;
        }
        if (core && ns > 0 && first + ns - 1 >= 0 && first + ns - 1 < A_max) core[c * A_max + first + ns - 1] = 1;
      }
      for (int q = 0; q < 64 && j > 0; ++q) j = tl[2 * j];
    }
    if (distance && lane == 0) {
      int ne = 0;  // edges root -> leaf (at most cap - 1)
      for (int q = node; q > 0 && ne < cap; q = tl[2 * q]) ++ne;
      double d = 0.0;
      for (int i = ne - 1; i >= 0; --i) {  // the edge i parents above the leaf; the root's first
        int q = node;
        for (int u = 0; u < i; ++u) q = tl[2 * q];
        const int m = (int)ta[3 * q];
        if (m < 0 || m >= lib.n) continue;
        const int ns = min((int)ta[3 * q + 1], lib.max_steps);
        const double vdt = lib.v[m] * lib.dt, wdt = lib.w[m] * lib.dt;
        d = d + (vdt * (double)ns + fabs(wdt * (double)ns) * angle_weight);
      }
      distance[c] = d;
    }
  }
}

// optimize2's choice (Planner2D.cpp:1095-1111): per tree the first leaf in node order with the strictly smallest cost - the first
// leaf is always taken, a NaN cost never replaces a held one.  One wave per tree.
__global__ __launch_bounds__(64) void k_em_pick(int n_sel, int A_max, const int *meta, const double *cost, const double *actions,
                                                const int32_t *n_actions, double *plan_out, int32_t *n_actions_out, double *cost_out,
                                                int32_t *n_leaves_out) {
  const int ti = blockIdx.x, lane = threadIdx.x;
  if (ti >= n_sel) return;
  const int off = leaf_offset(meta, ti);
  const int nl = meta[(size_t)ti * M_STRIDE + M_LEAVES];
  double best = __builtin_huge_val();
  int bi = 0x7fffffff;
  for (int k = lane; k < nl; k += 64) {
    const double c = cost[off + k];
    if (c < best || (c == best && k < bi)) {  // (a NaN compares false: never taken here)
      best = c;
      bi = k;
    }
  }
  wave_argmin(best, bi);
  // the first leaf is held whatever its cost: a NaN there is never replaced, an infinite one only by a smaller cost
  const double c0 = nl > 0 ? cost[off] : 0.0;
  if (nl > 0 && (c0 != c0 || bi >= nl || !(best < c0))) bi = 0;
  if (nl <= 0) {  // (a tree that failed to sample: no leaf, an empty plan)
    empty_plan(plan_out + (size_t)ti * A_max * 3, n_actions_out + ti, A_max);
    if (lane == 0) {
      if (cost_out) cost_out[ti] = 0.0;
      if (n_leaves_out) n_leaves_out[ti] = 0;
    }
    return;
  }
  const size_t c = (size_t)off + bi;
  for (int q = lane; q < 3 * A_max; q += 64) plan_out[(size_t)ti * A_max * 3 + q] = actions[c * A_max * 3 + q];
  if (lane == 0) {
    n_actions_out[ti] = n_actions[c];
    if (cost_out) cost_out[ti] = cost[c];
    if (n_leaves_out) n_leaves_out[ti] = nl;
  }
}

}  // namespace kemt

size_t drlgx_em_tree_lds_bytes(int cap) { return kemt::lds_bytes(cap); }

void drlgx_launch_em_tree(const DrlgxState &S, hipStream_t st, DrlgxTreeArgs args, bool obstacles, bool dubins) {
  using Kernel = void (*)(DrlgxState, DrlgxTreeArgs);
  static const Kernel kernels[4] = {kemt::k_em_tree<false, false>, kemt::k_em_tree<true, false>, kemt::k_em_tree<false, true>,
                                    kemt::k_em_tree<true, true>};  // [obstacles + 2 dubins]
  static bool attr_set[32] = {false};
  const void *fns[4];
  for (int i = 0; i < 4; ++i) fns[i] = reinterpret_cast<const void *>(kernels[i]);
  drlgx_ensure_lds_attr(attr_set, fns, 4, 160 * 1024);
  if (!obstacles) args.safe_distance = 0.0;
  hipLaunchKernelGGL(kernels[(obstacles ? 1 : 0) + (dubins ? 2 : 0)], dim3(args.n_sel), dim3(kemt::kT), kemt::lds_bytes(args.cap), st, S, args);
}
void drlgx_launch_em_leaves_dubins(hipStream_t st, int n_sel, const int32_t *env_sel, int cap, int A_max, double angle_weight,
                                   const double *act, const int *link, const int *leaf, const int *meta, const DrlgxDubins &lib,
                                   int per_tree_row, int32_t *cand_env, double *actions, int32_t *n_actions, uint8_t *core,
                                   double *distance) {
  hipLaunchKernelGGL(kemt::k_em_leaves_dubins, dim3(n_sel), dim3(64), 0, st, n_sel, env_sel, cap, A_max, angle_weight, act, link, leaf,
                     meta, lib, per_tree_row, cand_env, actions, n_actions, core, distance);
}
void drlgx_launch_em_leaves(hipStream_t st, int n_sel, const int32_t *env_sel, int cap, int A_max, const double *act, const int *link,
                            const int *leaf, const int *meta, int per_tree_row, int32_t *cand_env, double *actions, int32_t *n_actions) {
  hipLaunchKernelGGL(kemt::k_em_leaves, dim3(n_sel), dim3(64), 0, st, n_sel, env_sel, cap, A_max, act, link, leaf, meta, per_tree_row,
                     cand_env, actions, n_actions);
}
void drlgx_launch_em_pick(hipStream_t st, int n_sel, int A_max, const int *meta, const double *cost, const double *actions,
                          const int32_t *n_actions, double *plan_out, int32_t *n_actions_out, double *cost_out, int32_t *n_leaves_out) {
  hipLaunchKernelGGL(kemt::k_em_pick, dim3(n_sel), dim3(64), 0, st, n_sel, A_max, meta, cost, actions, n_actions, plan_out, n_actions_out,
                     cost_out, n_leaves_out);
}
