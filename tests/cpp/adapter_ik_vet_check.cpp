// ccmp::ProxyScene::ikValid, the vetted ccmp::Projector::sampleCalibGoal and the vetted ccmp::Roadmap::grow (include/ccmp_ompl_adapter.hpp)
// against the host forms of the rule they stand on (ccmp_arm_clearance_ref, ccmp_pose_ik_vetted_ref: no device behind them), compiled
// against the interface mock in tests/cpp/mock_ompl (tests/test_cpp_adapter_ik_vet.py).  The scene: one sphere on each arm's elbow frame
// (k = 3), one on each hand, a world sphere and the reference's sub_table; every group against every other.  A store of projected
// samples is built; its vertices' poses are the targets, their pose-nearest other vertices' joints the seeds.  A failing call must
// return false, fill NaN and keep the first error.
// usage: adapter_ik_vet_check <config.yaml>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <iostream>
#include <algorithm>
#include <utility>
#include <vector>
#include <string>
#include <fstream>
#include <memory>

#include <ompl/base/Constraint.h>
#include <ompl/base/ConstrainedSpaceInformation.h>
#include <ompl/base/spaces/constraint/ConstrainedStateSpace.h>
#include <ompl/base/spaces/constraint/ProjectedStateSpace.h>

#include <closed_chain_motion_planner/kinematics/panda_rbdl.h>

using namespace std;
#define CCMP_WITH_OMPL
#include "ccmp_ompl_adapter.hpp"

static bool same_bits(const double *a, const double *b, size_t n) { return memcmp(a, b, n * sizeof(double)) == 0; }
static bool all_nan(const double *a, size_t n)
{
  for (size_t i = 0; i < n; i++)
    if (!std::isnan(a[i])) return false;
  return true;
}
static ccmp_sphere sphere(int frame, int group, double x, double y, double z, double r)
{
  ccmp_sphere s;
  memset(&s, 0, sizeof s);
  s.frame = frame; s.group = group; s.c[0] = x; s.c[1] = y; s.c[2] = z; s.r = r;
  return s;
}

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  ccmp::Projector proj{std::string(argv[1])};
  const uint64_t kSeed = 0xABCDull;
  proj.setIkStream(kSeed, 3);
  int mismatches = 0, errors_before = 0;

  const std::vector<ccmp_sphere> spheres = {sphere(CCMP_FRAME(0, 3), 0, 0, 0, 0, 0.07), sphere(CCMP_FRAME(1, 3), 1, 0, 0, 0, 0.07),
                                            sphere(CCMP_FRAME(0, 7), 2, 0, 0, 0.05, 0.03), sphere(CCMP_FRAME(1, 7), 3, 0, 0, 0.05, 0.03),
                                            sphere(CCMP_FRAME_WORLD, 4, 0.45, 0.0, 1.45, 0.12)};
  const std::vector<ccmp_box> boxes = {ccmp::ProxyScene::subTable(5)};
  ccmp::ProxyScene scene(proj, spheres, boxes, nullptr);
  const double margin = 0.01;

  // a store: the valid ones of 512 projected samples
  const size_t B = 512;
  std::vector<double> q(B * 14), joints;
  std::vector<uint8_t> okp(B), jv(B);
  if (ccmp_sample_project_host(proj.ctx(), &proj.problem(), 0x17, 0, q.data(), okp.data(), nullptr, B) != CCMP_OK) return 3;
  if (ccmp_joint_valid_host(proj.ctx(), &proj.problem(), q.data(), jv.data(), B) != CCMP_OK) return 3;
  for (size_t i = 0; i < B; i++)
    if (okp[i] && jv[i]) joints.insert(joints.end(), q.begin() + i * 14, q.begin() + (i + 1) * 14);
  const size_t N = joints.size() / 14;
  printf("store %zu\n", N);
  if (N < 8) return 4;
  ccmp::Roadmap rm(proj, N);
  if (!rm.append(joints.data(), nullptr, N)) return 5;
  std::vector<double> poses(N * 8);
  if (!rm.read(0, N, nullptr, poses.data())) return 5;

  // ---- ikValid: both arms of the first vertices
  int free_rows = 0, refused_rows = 0;
  for (size_t t = 0; t < 8; t++)
    for (int arm = 0; arm < 2; arm++) {
      double want = 0.0, got = 0.0;
      uint8_t wfree = 0;
      if (ccmp_arm_clearance_ref(&proj.problem(), spheres.data(), (int)spheres.size(), boxes.data(), (int)boxes.size(), nullptr, arm,
                                 &joints[t * 14 + 7 * arm], 1, margin, &want, &wfree) != CCMP_OK)
        return 6;
      const bool r = scene.ikValid(arm, &joints[t * 14 + 7 * arm], margin, &got);
      const bool agree = r == (wfree != 0) && same_bits(&want, &got, 1);
      if (!agree) mismatches++;
      (r ? free_rows : refused_rows)++;
      printf("valid t=%zu arm=%d free=%d agree=%d\n", t, arm, (int)r, (int)agree);
    }

  // ---- the vetted sampleCalibGoal: one seed (the reference's signature) and three
  int solved = 0;
  for (size_t t = 0; t < 4; t++) {
    const double *pose = &poses[t * 8];
    double seeds[3 * 14];
    std::vector<int32_t> near;
    if (!rm.nearestK(CCMP_METRIC_OBJECT, pose, 3, &near, nullptr, CCMP_KNN_NOT_SELF, t)) return 5;
    for (int s = 0; s < 3; s++) memcpy(seeds + s * 14, &joints[(size_t)near[s] * 14], 14 * sizeof(double));
    for (int S = 1; S <= 3; S += 2) {
      double want[14], got[14], wclr = 0.0, clr = 0.0;
      uint8_t ok = 0;
      int32_t which = -7;
      const uint64_t index = proj.ikNextIndex();
      if (ccmp_pose_ik_vetted_ref(&proj.problem(), &proj.ikOptions(), pose, seeds, 1, S, kSeed, index, spheres.data(), (int)spheres.size(), boxes.data(),
                                  (int)boxes.size(), nullptr, margin, want, &ok, &which, nullptr, nullptr, nullptr, nullptr, &wclr) != CCMP_OK)
        return 6;
      int slot = -7;
      bool r;
      if (S == 1) {
        r = proj.sampleCalibGoal(pose, seeds, got, scene, margin);
        slot = which;
        clr = wclr;
      } else {
        r = proj.sampleCalibGoal(pose, seeds, S, got, &slot, scene, margin, &clr);
      }
      const bool agree = r == (ok != 0) && slot == which && same_bits(want, got, 14) && same_bits(&wclr, &clr, 1) && proj.ikNextIndex() == index + 1 &&
                         (r || all_nan(got, 14));
      if (!agree) mismatches++;
      solved += r;
      printf("goal t=%zu S=%d ok=%d which=%d agree=%d\n", t, S, (int)r, slot, (int)agree);
    }
  }
  errors_before += proj.lastError() != CCMP_OK;
  errors_before += scene.lastError() != CCMP_OK;

  // ---- the vetted Roadmap::grow against the composition: the plain grow's neighbours, the rule on the host from their joints
  const unsigned k = 5;
  const int ms = 12;
  for (size_t t = 0; t < 3; t++) {
    double pose[8];
    memcpy(pose, &poses[(N - 1 - t) * 8], sizeof pose);
    if (t == 2) pose[0] += 10.0; // no state: empty slots
    const uint64_t index = proj.ikNextIndex();
    std::vector<int32_t> near;
    if (!rm.nearestK(CCMP_METRIC_OBJECT, pose, k, &near, nullptr, CCMP_KNN_ALL, 0)) return 7;
    std::vector<double> seeds((size_t)k * 14);
    for (unsigned s = 0; s < k; s++) memcpy(&seeds[(size_t)s * 14], &joints[(size_t)near[s] * 14], 14 * sizeof(double));
    double wq[14], wclr = 0.0;
    uint8_t wik = 0;
    int32_t wwhich = -7;
    if (ccmp_pose_ik_vetted_ref(&proj.problem(), &proj.ikOptions(), pose, seeds.data(), 1, (int)k, kSeed, index, spheres.data(), (int)spheres.size(), boxes.data(),
                                (int)boxes.size(), nullptr, margin, wq, &wik, &wwhich, nullptr, nullptr, nullptr, nullptr, &wclr) != CCMP_OK)
      return 7;
    std::vector<int32_t> idx, n;
    std::vector<uint8_t> ok;
    std::vector<double> st;
    double gq[14], clr = 0.0;
    int which = -7;
    const bool r = rm.grow(pose, k, ms, &idx, gq, &which, &n, &ok, &st, scene.handle(), margin, true, &clr);
    bool agree = r == (wik != 0) && which == wwhich && same_bits(gq, wq, 14) && same_bits(&clr, &wclr, 1) && idx == near && proj.ikNextIndex() == index + 1;
    for (unsigned e = 0; e < k && agree && r; e++) agree = n[e] >= 1 && same_bits(&st[(size_t)e * ms * 14], &joints[(size_t)near[e] * 14], 14); // every edge starts at its neighbour
    if (!r)
      for (unsigned e = 0; e < k; e++) agree = agree && n[e] == 0 && ok[e] == 0;
    if (!agree) mismatches++;
    int reached = 0;
    for (unsigned e = 0; e < k; e++) reached += ok[e] == 1;
    printf("grow t=%zu ok=%d which=%d reached=%d agree=%d\n", t, (int)r, which, reached, (int)agree);
  }
  errors_before += rm.lastError() != CCMP_OK;

  // ---- failing calls: false, NaN, the first error kept until cleared
  double clr = 0.0;
  const bool f0 = scene.ikValid(2, &joints[0], margin, &clr); // no such arm
  const bool nan0 = std::isnan(clr);
  const int e0 = scene.lastError();
  const bool f0b = scene.ikValid(0, &joints[0], std::numeric_limits<double>::quiet_NaN(), &clr);
  const bool kept0 = scene.lastError() == e0 && !scene.lastErrorMessage().empty() && std::isnan(clr);
  scene.clearError();
  double got[14] = {0};
  std::vector<double> many(17 * 14, 0.1);
  int which = 5;
  const bool f1 = proj.sampleCalibGoal(&poses[0], many.data(), 17, got, &which, scene, margin, &clr); // S beyond CCMP_IK_MAX_SEEDS
  const bool nan1 = all_nan(got, 14) && which == -1 && std::isnan(clr);
  const int e1 = proj.lastError();
  double got2[14] = {0};
  const bool f2 = proj.sampleCalibGoal(&poses[0], &joints[14], got2, scene, std::numeric_limits<double>::quiet_NaN()); // a NaN margin
  const bool nan2 = all_nan(got2, 14);
  const bool kept = proj.lastError() == e1 && !proj.lastErrorMessage().empty();
  proj.clearError();
  const int cleared = proj.lastError();
  std::vector<int32_t> idx, n;
  std::vector<uint8_t> ok;
  std::vector<double> st;
  double gq[14] = {0};
  clr = 0.0;
  const bool f3 = rm.grow(&poses[0], k, ms, &idx, gq, &which, &n, &ok, &st, nullptr, margin, true, &clr); // the vetted grow needs its scene
  const bool nan3 = all_nan(gq, 14) && which == -1 && std::isnan(clr);
  const int e3 = rm.lastError();
  rm.clearError();
  printf("summary solved %d free %d refused %d mismatches %d before %d failed %d%d%d%d%d nan %d%d%d%d sticky %d %d kept %d%d cleared %d %d roadmap %d cleared %d\n",
         solved, free_rows, refused_rows, mismatches, errors_before, (int)f0, (int)f0b, (int)f1, (int)f2, (int)f3, (int)nan0, (int)nan1, (int)nan2, (int)nan3, e0,
         e1, (int)kept0, (int)kept, scene.lastError(), cleared, e3, rm.lastError());
  return 0;
}
