/* ccmp_graph.h — the roadmap graph's bookkeeping: what growTree does after its traversals (stefanBiPRM.cpp:303-372 and milestonesToAdd,
 * :420-445) and the vertex scan of closestFromGoal (:675-684), one text for host and device in the rounding model of ccmp_detmath.h.
 * The kernels of ccmp_kernels_graph.hip and the *_ref forms of ccmp_roadmap.cpp both compile it: they cannot differ in a bit.
 *
 * Arithmetic:
 *   edge weight     opt_->motionCost of the joint components = RealVectorStateSpace::distance over the 14 joints: the k-NN's rule
 *                   (ccmp_kernels_knn.hip) — dist = fma(diff_i, diff_i, dist), i = 0..13, then the correctly rounded root;
 *   pose of a state pose_from_joints_kernel's text (compute_t_wo of the left arm, then Quaterniond(Matrix3d));
 *   pose distance   ccmp_pose_dist (ccmp_pose.h).
 *
 * Labels: label[v] = the smallest vertex index of v's connected component — a function of the edge set alone.
 *
 * Slot kinds, for query q and slot r < k (edge e = q k + r), N = the store's size at call entry:
 *   empty      nbr_idx < 0 or nbr_idx >= N (the second cannot come out of the store's own k-NN; it keeps every read in bounds)
 *   unsettled  ok == 2 or n_states > max_states: a continuation is still due
 *   reached    ok == 1
 *   failed     otherwise
 *
 * The rule.  L = the labels at call entry; root(l) = l is the label of one of the caller's root vertices (the planner's startM_).
 *   vertex_ok[q] == 0            -> TRAPPED, nothing committed
 *   any slot unsettled           -> UNSETTLED, nothing committed for q
 *   joined = {}, joined_start = false
 *   for r = 0 .. k-1:
 *     reached: edge (nbr, t), weight = joint distance; joined += L[nbr]; joined_start |= root(L[nbr])
 *     failed, a goal pose given, n_states > 1, and (root(L[nbr]) or (L[nbr] in joined and joined_start)):
 *         m = pose of states[q][r][n_states-1]
 *         if dist(m, goal) < dist(pose[nbr], goal)  (strict; a NaN never passes):
 *             mid-stone r = vertex (that state, m) + edge (nbr, mid), weight = joint distance
 *   added = any slot reached;  t is kept iff added or KEEP_ISOLATED
 *   state = !added ? TRAPPED : joined_start ? SREACHED : GREACHED
 * The second arm of the component test is the reference's own: sameComponent_start(n) is asked inside the neighbour loop, after the
 * earlier successful edges of the same vertex have been united.  New indices, ascending q: t if kept, then its mid-stones in r order;
 * edges: the reached edges of q in r order, then its mid-stone edges.  The queries of one call do not see each other. */
#ifndef CCMP_GRAPH_H
#define CCMP_GRAPH_H
#include "../../include/ccmp.h"
#include "ccmp_pose.h"

namespace ccmp {

/* the caller's root vertices, by value */
struct graph_roots {
  int32_t v[CCMP_GRAPH_MAX_ROOTS];
  int32_t n;
};

enum : uint32_t {
  kSlotEmpty = 0, kSlotUnsettled = 1, kSlotReached = 2, kSlotFailed = 3, kSlotKindMask = 3,
  kSlotRoot = 4,   /* root(L[nbr]) */
  kSlotCloser = 8, /* failed, with a last state whose pose is strictly closer to the goal than the neighbour's */
};

/* what the per-query pass hands the scan and the scatter */
struct graph_decision {
  uint32_t reached, mid; /* bit r: slot r gives an edge to t / a mid-stone */
  int32_t keep;          /* t gets an index */
  int32_t state;         /* CCMP_GROW_* */
};

CCMP_HD uint32_t graph_slot_kind(int32_t nbr, uint32_t N, uint8_t ok, int32_t n_states, int max_states)
{
  if (nbr < 0 || (uint32_t)nbr >= N) return kSlotEmpty;
  if (ok == 2 || n_states > max_states) return kSlotUnsettled;
  return ok == 1 ? kSlotReached : kSlotFailed;
}

CCMP_HD double graph_joint_dist(const double *a, const double *b)
{
  double d2 = 0.0;
  for (int c = 0; c < 14; c++) {
    const double e = a[c] - b[c];
    d2 = CCMP_FMA(e, e, d2);
  }
  return ccmp_sqrt(d2);
}

/* pose_from_joints_kernel's text */
CCMP_HD void graph_pose_of_joints(const ccmp_consts &K, const double *joints, double *pose)
{
  double x[7], Rw[9], pw[3], T[12];
  for (int e = 0; e < 7; e++) x[e] = joints[e];
  fk_arm(K, 0, x, Rw, pw);
  mul33(Rw, K.t_o7i_R, T);
  T[9] = pw[0]; T[10] = pw[1]; T[11] = pw[2];
  mulvec_acc(Rw, K.t_o7i_p, T + 9);
  ccmp_pose_of_t_wo(T, pose);
}

CCMP_HD bool graph_is_root(const int32_t *labels, const graph_roots &R, int32_t l)
{
  bool hit = false;
  for (int i = 0; i < R.n; i++) hit = hit || labels[R.v[i]] == l;
  return hit;
}

/* The per-slot pass: the slot's flags; *label = L[nbr], *weight = the weight of the edge the slot would give (reached: neighbour to the
 * new state; failed with a last state: neighbour to that state), mid_pose[8] = that state's pose.  mids == false (no goal pose, or no
 * state lists: slot_states, the slot's [max_states][14] list, and goal are then not read): no mid-stone is considered.  Outputs of a
 * slot that does not need them are left alone. */
CCMP_HD uint32_t graph_slot_eval(const ccmp_consts &K, bool mids, const double *joints, const double *poses, const int32_t *labels, uint32_t N, const graph_roots &R,
                                 int32_t nbr, uint8_t ok, int32_t n_states, int max_states, const double *slot_states, const double *new_joints,
                                 const double *goal, int32_t *label, double *weight, double *mid_pose)
{
  const uint32_t kind = graph_slot_kind(nbr, N, ok, n_states, max_states);
  if (kind == kSlotEmpty || kind == kSlotUnsettled) return kind;
  uint32_t f = kind;
  const int32_t l = labels[nbr];
  *label = l;
  if (graph_is_root(labels, R, l)) f |= kSlotRoot;
  if (kind == kSlotReached) {
    *weight = graph_joint_dist(joints + (size_t)nbr * 14, new_joints);
  } else if (mids && n_states > 1) {
    const double *last = slot_states + (size_t)(n_states - 1) * 14; /* n_states <= max_states: inside the list */
    graph_pose_of_joints(K, last, mid_pose);
    if (ccmp_pose_dist(mid_pose, goal) < ccmp_pose_dist(poses + (size_t)nbr * 8, goal)) f |= kSlotCloser;
    *weight = graph_joint_dist(joints + (size_t)nbr * 14, last);
  }
  return f;
}

/* The per-query pass on the slots' flags and labels (flags[r], label[r], r < k <= 16). */
CCMP_HD graph_decision graph_decide(const uint32_t *flags, const int32_t *label, int k, int vertex_ok, int keep_isolated)
{
  graph_decision d;
  d.reached = d.mid = 0;
  d.keep = 0;
  d.state = CCMP_GROW_TRAPPED;
  if (!vertex_ok) return d;
  for (int r = 0; r < k; r++)
    if ((flags[r] & kSlotKindMask) == kSlotUnsettled) { d.state = CCMP_GROW_UNSETTLED; return d; }
  bool joined_start = false;
  for (int r = 0; r < k; r++) {
    const uint32_t f = flags[r], kind = f & kSlotKindMask;
    if (kind == kSlotReached) {
      d.reached |= 1u << r;
      joined_start = joined_start || (f & kSlotRoot);
    } else if (kind == kSlotFailed && (f & kSlotCloser)) {
      bool in_joined = false; /* the labels of the reached slots before r */
      for (int s = 0; s < r; s++) in_joined = in_joined || ((d.reached >> s & 1u) && label[s] == label[r]);
      if ((f & kSlotRoot) || (in_joined && joined_start)) d.mid |= 1u << r;
    }
  }
  const bool added = d.reached != 0;
  d.keep = added || keep_isolated;
  d.state = !added ? CCMP_GROW_TRAPPED : joined_start ? CCMP_GROW_SREACHED : CCMP_GROW_GREACHED;
  return d;
}

CCMP_HD int graph_popcount(uint32_t x)
{
  int n = 0;
  for (; x; x &= x - 1) n++;
  return n;
}

/* closestFromGoal's candidate order: (distance, index) ascending; a NaN distance is never a candidate */
CCMP_HD bool graph_closer(double da, int32_t ia, double db, int32_t ib) { return da < db || (da == db && ia < ib); }

}  // namespace ccmp

#endif /* CCMP_GRAPH_H */
