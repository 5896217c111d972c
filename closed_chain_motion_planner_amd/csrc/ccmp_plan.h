/* ccmp_plan.h — the planner's loop on the roadmap store: the decisions of stefanBiPRM::solve / constructRoadmap / checkForSolution
 * (stefanBiPRM.cpp:692-899) that are neither a traversal, an IK, a k-NN nor a mesh test, one text for host and device.  The kernels of
 * ccmp_kernels_plan.hip and the *_ref forms of ccmp_plan.cpp both compile it: they cannot differ in a bit.  include/ccmp.h states the
 * whole sequence (open, growth, check, solution test) and its two differences from the reference; what is stated HERE is
 *
 *   the gate        the check runs iff size > size_at_check + 3 (strict; checkForSolution's `tree_->size() > size + 3`, :712)
 *   the carry rule  closestFromGoal(froms, {to}) (:641-690) from ccmp_roadmap_closest's per-from answers: val = +inf; per from f in the
 *                   list's order: h = from_dist, if h < val then val = h; closest = f; if idx >= 0 and dist < val then (closest, val) =
 *                   (idx, dist).  The LAST from's component therefore decides `closest` even where an earlier one was nearer: that is
 *                   the reference's behaviour and is kept.  A from outside [0, size) is skipped, an idx outside it is no candidate.
 *   the thresholds  d < prev - 0.1, one IEEE subtraction then a strict compare; a NaN never passes
 *   the caps        a side that fires with its list full (8) does not try its IK; counters.push_refused counts it
 *   the indices     a check that ran advances next_index by 11: goal, ladder 1 .. 9, start, in that order, fired or not
 *   the prefix      the longest run from the ladder's first pose in which valid and ik_ok are both non-zero
 *   the solution    the first pair (s, g), s major and g minor, whose labels agree — stated as templates over the state type: RRT-Connect's
 *                   state block (ccmp_rrtc.h) takes the same test, in the same kernel text and the same host fold
 *
 * No arithmetic here rounds differently on host and device: comparisons, one subtraction of two doubles, integer sums. */
#ifndef CCMP_PLAN_H
#define CCMP_PLAN_H
#include "../../include/ccmp.h"
#include "ccmp_detmath.h"

namespace ccmp {

constexpr int kPlanTargets = 2 + CCMP_PLAN_LADDER; /* the IK targets of a check: goal, ladder 1 .. 9, start */
constexpr int kPlanGoalRow = 0, kPlanLadderRow = 1, kPlanStartRow = 1 + CCMP_PLAN_LADDER;
constexpr double kPlanImprove = 0.1;               /* checkForSolution's `dist < previous - 0.1` */

/* ---- what the planners on the store share.  ccmp_plan_state and ccmp_rrtc_state both hold n_starts, n_goals, starts, goals, status, cycle,
 * solved_start and solved_goal (at different offsets: the shared text below is a template over the state type S, no overlay), and both
 * spell their status values and caps alike; the shared text names them as ccmp_plan does. */
static_assert((int)CCMP_PLAN_OPEN == (int)CCMP_RRTC_OPEN && (int)CCMP_PLAN_SOLVED == (int)CCMP_RRTC_SOLVED && (int)CCMP_PLAN_BUDGET == (int)CCMP_RRTC_BUDGET &&
                  (int)CCMP_PLAN_FULL == (int)CCMP_RRTC_FULL && CCMP_PLAN_MAX_STARTS == CCMP_RRTC_MAX_ROOTS && CCMP_PLAN_MAX_GOALS == CCMP_RRTC_MAX_ROOTS,
              "one status and one cap for every planner");

CCMP_HD int planner_clamp(int n) { return n < 0 ? 0 : n > CCMP_PLAN_MAX_STARTS ? CCMP_PLAN_MAX_STARTS : n; } /* a list's length as it is used */

CCMP_HD bool plan_gate(unsigned long long size, int32_t size_at_check) { return size_at_check >= 0 && size > (unsigned long long)size_at_check + 3ull; }

/* the cycle's worst case: width (1 + k) rows of a growth step, nine ladder rows, one goal and one start vertex */
CCMP_HD bool plan_full(unsigned long long size, int width, int k, unsigned long long max_vertices)
{
  return size + (unsigned long long)width * (unsigned long long)(1 + k) + (unsigned long long)kPlanTargets > max_vertices;
}

CCMP_HD void plan_carry(const int32_t *froms, int n, const int32_t *idx, const double *dist, const double *from_dist, unsigned long long size, int32_t *closest,
                        double *val)
{
  int32_t c = -1;
  double v = __builtin_inf();
  for (int i = 0; i < n && i < CCMP_PLAN_MAX_STARTS; i++) {
    const int32_t f = froms[i];
    if (f < 0 || (unsigned long long)f >= size) continue;
    const double h = from_dist[i];
    if (h < v) v = h;
    c = f;
    const int32_t j = idx[i];
    if (j >= 0 && (unsigned long long)j < size && dist[i] < v) { c = j; v = dist[i]; }
  }
  *closest = c;
  *val = v;
}

/* step 2's decisions on the state; trig = {ran, goal side fired, start side fired, the vertex that seeds the goal side or -1}.
 * nearest_pose is the caller's to copy (pose[trig[3]]) where the goal side fired. */
CCMP_HD void plan_check(ccmp_plan_state *s, unsigned long long size, const int32_t *a_idx, const double *a_dist, const double *a_from, const int32_t *b_idx,
                        const double *b_dist, const double *b_from, int32_t trig[4])
{
  trig[0] = trig[1] = trig[2] = 0;
  trig[3] = -1;
  if (!plan_gate(size, s->size_at_check)) return;
  trig[0] = 1;
  s->counters.checks += 1;
  const int S = planner_clamp(s->n_starts), G = planner_clamp(s->n_goals);
  if (G > 0 && S > 0) {
    int32_t c, p;
    double d, d2;
    plan_carry(s->starts, S, a_idx, a_dist, a_from, size, &c, &d);
    if (c >= 0 && d < s->prev_from_goal - kPlanImprove) {
      s->nearest = c;
      s->prev_from_goal = d;
      trig[1] = 1;
      trig[3] = c;
      if (G >= CCMP_PLAN_MAX_GOALS) s->counters.push_refused += 1;
    }
    plan_carry(s->goals, G, b_idx, b_dist, b_from, size, &p, &d2);
    if (p >= 0) {
      s->sprevious = p;
      if (d2 < s->prev_from_start - kPlanImprove) {
        s->prev_from_start = d2;
        trig[2] = 1;
        if (S >= CCMP_PLAN_MAX_STARTS) s->counters.push_refused += 1;
      }
    }
  }
  s->size_at_check = (int32_t)size;
  s->next_index += (uint64_t)kPlanTargets;
}

CCMP_HD int plan_prefix(const uint8_t *valid, const uint8_t *ik_ok, uint8_t *vertex_ok)
{
  int n = 0;
  while (n < CCMP_PLAN_LADDER && valid[n] && ik_ok[n]) n++;
  for (int i = 0; i < CCMP_PLAN_LADDER; i++) vertex_ok[i] = i < n ? 1 : 0;
  return n;
}

/* the solution test: pair (si, gi) of the state's lists is connected under `labels` [N] */
template <class S> CCMP_HD bool pair_connected(const S *s, int si, int gi, const int32_t *labels, unsigned long long N)
{
  const int32_t a = s->starts[si], b = s->goals[gi];
  if (a < 0 || b < 0 || (unsigned long long)a >= N || (unsigned long long)b >= N) return false;
  return labels[a] == labels[b];
}

template <class S> CCMP_HD void solved(S *s, int si, int gi)
{
  s->status = CCMP_PLAN_SOLVED;
  s->solved_start = s->starts[si];
  s->solved_goal = s->goals[gi];
}

/* the host's fold: the first connected pair, start-major; a state that is SOLVED stays as it is */
template <class S> CCMP_HD void first_connected(S *s, const int32_t *labels, unsigned long long N)
{
  if (s->status == CCMP_PLAN_SOLVED) return;
  for (int si = 0; si < s->n_starts; si++)
    for (int gi = 0; gi < s->n_goals; gi++)
      if (pair_connected(s, si, gi, labels, N)) { solved(s, si, gi); return; }
}

/* a committed vertex onto starts (which == 0) or goals (1), under the cap; new_index < 0: nothing was committed */
CCMP_HD void plan_push(ccmp_plan_state *s, int which, int32_t new_index)
{
  if (new_index < 0) return;
  if (which == 0) {
    if (s->n_starts >= CCMP_PLAN_MAX_STARTS) { s->counters.push_refused += 1; return; }
    s->starts[s->n_starts++] = new_index;
    s->counters.start_pushes += 1;
  } else {
    if (s->n_goals >= CCMP_PLAN_MAX_GOALS) { s->counters.push_refused += 1; return; }
    s->goals[s->n_goals++] = new_index;
    s->counters.goal_pushes += 1;
  }
}

}  // namespace ccmp

struct ccmp_ctx;

namespace ccmp_launch { struct GraphStore; }
namespace ccmp_host {
#pragma GCC visibility push(hidden)
/* the store's arrays as they stand (a commit or an append may move them), its context, and an object's device: what ccmp_plan.cpp needs
 * of the handles that ccmp_roadmap.cpp and ccmp_object.cpp define */
void roadmap_arrays(const ccmp_roadmap *rm, ccmp_launch::GraphStore *out);
ccmp_ctx *roadmap_ctx(const ccmp_roadmap *rm);
int object_device(const ccmp_object *obj);
#pragma GCC visibility pop
}  // namespace ccmp_host

#endif /* CCMP_PLAN_H */
