// scene_math_check.cpp — host check of the proxy scene's shared arithmetic (csrc/ccmp_scene_math.h) in the det oracle's rounding model
// (-ffp-contract=off -DCCMP_USE_FMA).  Two kernels build an arm's frames row by row (state_clearance<NT>, ik_vet_kernel); everything
// else walks joint_step.  Here, on the host and for three arm models (stock, calibrated, tilted base), both arms:
//   1. scene_joint_rot for the seven joints, then scene_chain_row for rows 0, 1, 2 in turn, gives the eight frames of the one-thread
//      joint_step walk (scene_arm_frames) in all 96 doubles, byte for byte;
//   2. scene_place on those frames equals frame -> base followed by base -> world applied by hand (ccmp_kin.h: mulvec_acc), for every
//      slot kind: each of the arm's eight frames, its base, the world — once with the arm's own frames and once with both arms' frames
//      and the offset kSceneArmFrames * scene_slot_arm(slot).
// usage: scene_math_check <config.yaml> <joint vectors per model and arm>; prints one line of counts, exit status 0 iff nothing
// differed.  (tests/test_scene_math_host.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ccmp_host.h"
#include "ccmp_scene_math.h"

using namespace ccmp;

namespace {

uint64_t g_state = 0x5CE7E0A7ull;
uint64_t next_u64() { return g_state = splitmix64(g_state); }
double uniform(double lo, double hi) { return lo + (hi - lo) * ((double)(next_u64() >> 11) * 0x1p-53); }

struct Counts { long vectors = 0, frames_differ = 0, places = 0, place_differ = 0; };

// the frames of arm `arm` at q7, both ways, in their place among both arms' frames (the other arm's are never read); then every slot kind
void check_vector(const ccmp_consts &K, int arm, const double *q7, const char *model, Counts &n)
{
  double walk[2 * kSceneArmFrames], rows[2 * kSceneArmFrames], rj[7 * 9];
  memset(walk, 0xff, sizeof walk);
  memset(rows, 0xff, sizeof rows); // every double of the arm's frames must be written
  scene_arm_frames(K, arm, q7, walk + kSceneArmFrames * arm);
  for (int i = 0; i < 7; i++) scene_joint_rot(K, arm, i, q7[i], rj + 9 * i);
  for (int r = 0; r < 3; r++) scene_chain_row(K, arm, r, rj, rows + kSceneArmFrames * arm);
  n.vectors++;
  if (memcmp(walk + kSceneArmFrames * arm, rows + kSceneArmFrames * arm, kSceneArmFrames * sizeof(double)) != 0) {
    if (n.frames_differ++ < 5) fprintf(stderr, "%s arm %d: the row-wise chain differs at q = %a %a %a %a %a %a %a\n", model, arm, q7[0], q7[1], q7[2], q7[3], q7[4], q7[5], q7[6]);
  }
  const double c[3] = {uniform(-0.3, 0.3), uniform(-0.3, 0.3), uniform(-0.3, 0.3)};
  for (int k = 0; k <= 9; k++) { // frames 0..7 of the arm, its base, the world
    const int slot = k == 9 ? kSceneSlots - 1 : 9 * arm + k;
    double want[3], v[3], one[3], both[3];
    if (k == 9) {
      memcpy(want, c, sizeof want);
    } else {
      if (k == 8) {
        memcpy(v, c, sizeof v);
      } else {
        const double *f = walk + kSceneArmFrames * arm + kSceneFrame * k;
        v[0] = f[9]; v[1] = f[10]; v[2] = f[11];
        mulvec_acc(f, c, v);
      }
      want[0] = K.base_p[arm][0]; want[1] = K.base_p[arm][1]; want[2] = K.base_p[arm][2];
      mulvec_acc(K.base_R[arm], v, want);
    }
    scene_place(K, slot, c, rows + kSceneArmFrames * arm, one);
    scene_place(K, slot, c, rows + kSceneArmFrames * scene_slot_arm(slot), both);
    n.places++;
    if (memcmp(want, one, sizeof want) != 0 || memcmp(want, both, sizeof want) != 0) {
      if (n.place_differ++ < 5) fprintf(stderr, "%s arm %d: scene_place differs on slot %d\n", model, arm, slot);
    }
  }
}

} // namespace

int main(int argc, char **argv)
{
  if (argc < 3) return 2;
  ccmp_problem P;
  if (ccmp_problem_from_yaml(argv[1], &P) != CCMP_OK) return 3;
  const long n_vectors = atol(argv[2]);
  const double pi = 3.14159265358979323846;

  ccmp_problem M[3] = {P, P, P}; // stock, calibrated (offsets that differ per arm), stock arms with arm 1 on a tilted base
  const char *name[3] = {"stock", "calibrated", "tilted"};
  for (int arm = 0; arm < 2; arm++) {
    double dh[7][4];
    for (int i = 0; i < 28; i++) dh[i / 4][i % 4] = 1e-3 * (double)((5 * i + 2 * arm) % 7 - 3);
    if (ccmp_set_calibration(&M[1], arm, dh) != CCMP_OK) return 5;
  }
  {
    const double a = 0.3, b = -0.7;
    const double Rx[9] = {1, 0, 0, 0, std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a)};
    const double Rz[9] = {std::cos(b), -std::sin(b), 0, std::sin(b), std::cos(b), 0, 0, 0, 1};
    double R[9];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) R[3 * i + j] = Rz[3 * i] * Rx[j] + Rz[3 * i + 1] * Rx[3 + j] + Rz[3 * i + 2] * Rx[6 + j];
    if (ccmp_set_base_frame(&M[2], 1, R, P.base_p[1]) != CCMP_OK) return 5;
  }
  ccmp_consts K[3];
  for (int m = 0; m < 3; m++) ccmp_host::make_consts(M[m], K[m]);
  if (!K[0].stock || K[1].stock || !K[2].stock || ((K[2].base_diag >> 1) & 1)) { fprintf(stderr, "the three models are not what they are meant to be\n"); return 4; }

  Counts n;
  for (int m = 0; m < 3; m++)
    for (int arm = 0; arm < 2; arm++) {
      const ccmp_consts &Km = K[m];
      // the corners: all zero, both joint limits, +-pi/2 and +-pi on every joint, and each of those on one joint at a time
      const double vals[7] = {0.0, pi / 2, -pi / 2, pi, -pi, 0.0, 0.0};
      double q[7];
      for (int v = 0; v < 7; v++) {
        for (int i = 0; i < 7; i++) q[i] = v == 5 ? Km.lb[i] : (v == 6 ? Km.ub[i] : vals[v]);
        check_vector(Km, arm, q, name[m], n);
        for (int one = 0; one < 7; one++) {
          double q1[7] = {0, 0, 0, 0, 0, 0, 0};
          q1[one] = q[one];
          check_vector(Km, arm, q1, name[m], n);
        }
      }
      for (long k = 0; k < n_vectors; k++) {
        for (int i = 0; i < 7; i++) {
          switch ((k + i) & 7) {
          case 0: q[i] = uniform(-pi, pi); break;
          case 1: q[i] = pi * (double)((long)(next_u64() % 5) - 2) / 2.0 + uniform(-1e-7, 1e-7); break; // beside multiples of pi/2
          case 2: q[i] = std::ldexp(uniform(1.0, 2.0), -(int)(next_u64() % 60)) * ((next_u64() & 1) ? 1.0 : -1.0); break; // every magnitude down to 2^-59
          default: q[i] = uniform(Km.lb[i], Km.ub[i]); break; // the joint's range
          }
        }
        check_vector(Km, arm, q, name[m], n);
      }
    }

  printf("{\"vectors\": %ld, \"frames_differ\": %ld, \"places\": %ld, \"place_differ\": %ld}\n", n.vectors, n.frames_differ, n.places, n.place_differ);
  return (n.frames_differ || n.place_differ) ? 1 : 0;
}
