/* ccmp_ik_vet.h — the collision gate of growTree's sampleCalibGoal, on the proxy scene: one text for host and device in the rounding model
 * of ccmp_detmath.h (-ffp-contract=off -DCCMP_USE_FMA).  ccmp_arm_clearance_ref / ccmp_pose_ik_vetted_ref run it on the host,
 * ik_vet_kernel / ik_assemble_kernel / ik_pick_kernel (ccmp_kernels_ik_vet.hip) on the device: the same bits.
 *
 * The reference (jy_ConstrainedValidStateSampler.h:147-199): every IK candidate of an arm is ik_task_->solve(...) && IKvc_->IKValid(arm,
 * solution) — IKValid a collision test of that one arm (KinematicChain.cpp:129-161, req.group_name = arm) — and the assembled 14-joint
 * state must pass si_->isValid(result) (:188).  ccmp_ik.h restates the rule without the gate; here it is with the proxy scene in
 * MoveIt's place.
 *
 * Arm clearance.  A sphere is static on the world frame or on either arm's base, moving on arm a on CCMP_FRAME(a, 0..7).  Arm a's pair
 * set is the scene's tested pairs (already filtered by its allowed matrix; boxes included) that contain no sphere moving on the other
 * arm (ccmp_scene.h: scene_arm_dev); arm_clearance(a, q7) is the smallest signed distance over it: +inf for an empty set, NaN when one
 * of the seven joints is not finite.  It reads arm a's seven joints only, and is ccmp_clearance's arithmetic (ccmp_scene_math.h: the
 * chain of joint_step, t_wb (o + R c), the distances; scene_arm_clearance on the host, ik_vet_kernel on the device) on the same
 * operands: the bits of orc_clearance on the sub-scene without the other arm's moving spheres, whatever the work layout (the minimum of
 * a set of doubles is exact).  The scene's pairs are arm 0's set, arm 1's set and the cross pairs (one sphere moving on each arm): full
 * clearance = min(arm 0, arm 1, cross).
 *
 * Unlike MoveIt's IKValid, which tests the arm against a robot state that still holds whatever the other arm was last set to, the arm
 * is tested ALONE here; the pair of arms is tested on the assembled state.
 *
 * Vetted selection, over the records of ccmp_ik.h and an arm clearance per converged candidate:
 *   admissible   a candidate that converged (rounds >= 0) and whose arm clearance > margin (the rule of free_out);
 *   per arm      candidate 0 if admissible, else the admissible restart with the smallest rec_d2 (ties to the lowest r), else failure;
 *   assembled    a slot whose two arms succeed; its slot clearance is the full clearance of the 14-joint row, and the slot succeeds iff
 *                that is > margin (si_->isValid(result): what catches the cross pairs);
 *   answer       the first slot that succeeds in the order given; otherwise a NaN row, ok = 0, which = -1.
 * margin = -inf admits every converged candidate and every assembled slot: ik_select's answer bit for bit.  margin = +inf admits none.
 * Where ik_select's answer has a full clearance > margin (hence arm clearances > margin: each arm's set is a subset), every slot in
 * front of it fails on an arm here as it does there, and the slot's own picks are the same: the same row, ok and which. */
#ifndef CCMP_IK_VET_H
#define CCMP_IK_VET_H
#include "ccmp_ik.h"

namespace ccmp {

/* ---- the selection ------------------------------------------------------------------------------------------------------------------- */
CCMP_HD bool ik_vet_admissible(int32_t rounds, double clear, double margin) { return rounds >= 0 && clear > margin; }

/* the per-arm part of the rule for slot ts = t S + s over the records and cand_clear [c]: the slot's state into q14 and true, or a row
 * of zeros and false (a row that is never reported: no NaN reaches a clearance kernel) */
CCMP_HD bool ik_vet_assemble(const double *rec_q, const int32_t *rec_rounds, const double *rec_d2, const double *cand_clear, size_t ts, int R, double margin,
                             double *q14)
{
  size_t pick[2];
  bool both = true;
  for (int a = 0; a < 2; a++) {
    const size_t base = (ts * 2 + (size_t)a) * (size_t)(1 + R);
    bool have = false;
    size_t best = base;
    if (ik_vet_admissible(rec_rounds[base], cand_clear[base], margin)) have = true;
    else {
      for (int r = 1; r <= R; r++) {
        if (!ik_vet_admissible(rec_rounds[base + r], cand_clear[base + r], margin)) continue;
        if (!have || rec_d2[base + r] < rec_d2[best]) { best = base + r; have = true; }
      }
    }
    pick[a] = best;
    both = both && have;
  }
  for (int a = 0; a < 2; a++)
    for (int i = 0; i < 7; i++) q14[7 * a + i] = both ? rec_q[pick[a] * 7 + i] : 0.0;
  return both;
}

/* the first slot of target t with a state and a slot clearance > margin -> q_out[14], ok, which, clearance (nullable); slot_out
 * (nullable, [T][S]): the slot clearances as the caller sees them, NaN where the slot was not assembled */
CCMP_HD void ik_vet_pick(const double *slot_q, const uint8_t *slot_has, const double *slot_clear, size_t t, int S, double margin, double *q_out, uint8_t *ok,
                         int32_t *which, double *clearance, double *slot_out)
{
  int won = -1;
  for (int s = 0; s < S; s++) {
    const size_t ts = t * (size_t)S + (size_t)s;
    const bool has = slot_has[ts] != 0;
    if (slot_out) slot_out[ts] = has ? slot_clear[ts] : __builtin_nan("");
    if (won < 0 && has && slot_clear[ts] > margin) won = s;
  }
  const size_t ts = t * (size_t)S + (size_t)(won < 0 ? 0 : won);
  for (int i = 0; i < 14; i++) q_out[i] = won < 0 ? __builtin_nan("") : slot_q[ts * 14 + i];
  *ok = won < 0 ? 0 : 1;
  *which = won;
  if (clearance) *clearance = won < 0 ? __builtin_nan("") : slot_clear[ts];
}

} /* namespace ccmp */
#endif /* CCMP_IK_VET_H */
