/* ccmp_scene.h — device-side description of a proxy scene (ccmp_scene.cpp builds it, ccmp_kernels_scene.hip reads it);
 * not part of the public ABI. */
#ifndef CCMP_SCENE_H
#define CCMP_SCENE_H
#include <stdint.h>

#include "../../include/ccmp.h"

namespace ccmp {

constexpr int kSceneSlots = 19;                                                   // 2 arms x (7 bodies, hand, base) + world
constexpr int kSceneMaxPairs = CCMP_MAX_SPHERES * (CCMP_MAX_SPHERES - 1) / 2 + CCMP_MAX_SPHERES * CCMP_MAX_BOXES;

/* Spheres are stored sorted by frame slot (slot = frame code, world last), so that a wavefront walking one arm's chain
 * places the spheres of a frame the moment that frame exists; `user` maps a stored index back to the caller's. */
struct scene_dev {
  int32_t n_spheres, n_boxes, n_pairs, n_pairs_ss; /* the first n_pairs_ss pairs are sphere-sphere, the rest sphere-box */
  int32_t slot_begin[kSceneSlots + 1];
  int32_t user[CCMP_MAX_SPHERES];
  int32_t slot[CCMP_MAX_SPHERES]; /* frame slot of each stored sphere (the per-state kernel walks to it) */
  double c[CCMP_MAX_SPHERES][3];
  double r[CCMP_MAX_SPHERES];
  double box_c[CCMP_MAX_BOXES][3];
  double box_R[CCMP_MAX_BOXES][9];
  double box_half[CCMP_MAX_BOXES][3];
  /* tested pairs in the public numbering (include/ccmp.h): stored index of the first sphere | (stored index of the
   * second, or 64 + box) << 8 — one dword, so that the kernel fetches it with a scalar load; code = the value reported
   * to the caller (the caller's own indices) */
  uint32_t pair_ij[kSceneMaxPairs];
  int32_t pair_code[kSceneMaxPairs];
  double pair_rsum[kSceneMaxPairs]; /* r_i + r_j (sphere-sphere) or r_i (sphere-box): what is subtracted from the distance */
};

/* Derived from scene_dev for the vetted IK (the rule: csrc/ccmp_ik_vet.h; the arm clearance over it: csrc/ccmp_scene_math.h): the tested
 * pairs of ONE arm — those that contain no sphere moving on the other arm (frame slots 9 a' .. 9 a' + 7) — as positions in scene_dev's
 * pair table, ascending.  The two lists and the cross pairs (one sphere moving on each arm) partition the table.  A table of its own:
 * scene_dev's layout is what every scene kernel reads. */
struct scene_arm_dev {
  int32_t n_pairs[2];
  uint16_t pair[2][kSceneMaxPairs];
};
/* the arm a sphere on frame slot `slot` moves with (slots 9 a .. 9 a + 7: the bodies and the hand), -1 for a static one (a base, the world) */
constexpr int scene_moving_arm(int slot) { return slot == kSceneSlots - 1 || slot % 9 == 8 ? -1 : slot / 9; }
/* the arm whose frames and base a slot indexes (slots 9 a .. 9 a + 8); 0 for the world, which has neither */
constexpr int scene_slot_arm(int slot) { return slot >= 9 && slot < kSceneSlots - 1 ? 1 : 0; }
static_assert(kSceneMaxPairs < 65536, "scene_arm_dev keeps pair positions in 16 bits");

}  // namespace ccmp

struct ccmp_scene {
  int device = 0;
  ccmp_ctx *ctx = nullptr; // the context the scene was created on: its resident service kernel is stopped before the scene's hipFree (ccmp_resident.h rule 2); the context must outlive the scene or be destroyed first with the service off
  ccmp::scene_dev host;
  ccmp::scene_dev *dev = nullptr;
  ccmp::scene_arm_dev arm_host; // the per-arm pair lists (ik_vet_kernel); filled by ccmp_scene_create with the tables above
  ccmp::scene_arm_dev *arm_dev = nullptr;
  // The scene's share of the bound on `best + rsum` (ccmp_scene.cpp: clearance_magnitude_bound; the tile kernel's prune holds below
  // 2^22 only): the largest |centre| of the spheres on each kind of frame, in that frame (-1: none there), the largest pair_rsum,
  // and over the boxes the largest |centre| and the largest max(1, |R|_F)
  double c_world = -1.0, c_base[2] = {-1.0, -1.0}, c_moving[2] = {-1.0, -1.0};
  double rsum_max = 0.0, box_c = 0.0, box_gain = 1.0;
};

namespace ccmp_host {
/* what ccmp_scene_create checks of the caller's arrays and the tables it derives from them (no device): shared with the *_ref forms
 * that take a scene as the caller's arrays (ccmp_arm_clearance_ref, ccmp_pose_ik_vetted_ref) */
int scene_tables(const ccmp_sphere *spheres, int n_spheres, const ccmp_box *boxes, int n_boxes, const uint32_t allowed[32], ccmp::scene_dev &H,
                 ccmp::scene_arm_dev &A);
}  // namespace ccmp_host

#endif /* CCMP_SCENE_H */
