// ccmp::Projector::sampleCalibGoal and ccmp::Roadmap::grow (include/ccmp_ompl_adapter.hpp) against the C calls they stand on, compiled
// against the interface mock in tests/cpp/mock_ompl (tests/test_cpp_adapter_ik.py).  A store of projected samples is built; for a few
// of its vertices the object pose is the target and its pose-nearest other vertices' joints are the seeds.  Every adapter call must give the bits of
// ccmp_pose_ik_host / ccmp_roadmap_grow_host on the same stream index; a failing call must return false, fill NaN and keep the error.
// usage: adapter_ik_check <config.yaml>
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

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  ccmp::Projector proj{std::string(argv[1])};
  const uint64_t kSeed = 0xABCDull;
  proj.setIkStream(kSeed, 3);
  int mismatches = 0, errors_before = 0;

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

  // ---- sampleCalibGoal: one seed (the reference's signature) and three
  int solved = 0;
  double solved_pose[8], solved_q[14];
  for (size_t t = 0; t < 4; t++) {
    const double *pose = &poses[t * 8];
    double seeds[3 * 14];
    std::vector<int32_t> near;
    if (!rm.nearestK(CCMP_METRIC_OBJECT, pose, 3, &near, nullptr, CCMP_KNN_NOT_SELF, t)) return 5;
    for (int s = 0; s < 3; s++) memcpy(seeds + s * 14, &joints[(size_t)near[s] * 14], 14 * sizeof(double));
    for (int S = 1; S <= 3; S += 2) {
      double want[14], got[14];
      uint8_t ok = 0;
      int32_t which = -7;
      const uint64_t index = proj.ikNextIndex();
      if (ccmp_pose_ik_host(proj.ctx(), &proj.problem(), &proj.ikOptions(), pose, seeds, 1, S, kSeed, index, want, &ok, &which, nullptr, nullptr) != CCMP_OK) return 6;
      int slot = -7;
      const bool r = S == 1 ? proj.sampleCalibGoal(pose, seeds, got) : proj.sampleCalibGoal(pose, seeds, S, got, &slot);
      if (S == 1) slot = which;
      const bool agree = r == (ok != 0) && slot == which && same_bits(want, got, 14) && proj.ikNextIndex() == index + 1 && (r || all_nan(got, 14));
      if (!agree) mismatches++;
      solved += r;
      if (r) { memcpy(solved_pose, pose, sizeof solved_pose); memcpy(solved_q, got, sizeof solved_q); }
      printf("goal t=%zu S=%d ok=%d which=%d agree=%d\n", t, S, (int)r, slot, (int)agree);
    }
  }
  // a seed that already solves the target (a state this call returned: a projected sample meets the hand targets to the constraint's
  // tolerance only) comes back unchanged
  if (solved) {
    double got[14];
    const bool r = proj.sampleCalibGoal(solved_pose, solved_q, got);
    printf("goal own-state ok=%d same=%d\n", (int)r, (int)same_bits(got, solved_q, 14));
    if (!r || !same_bits(got, solved_q, 14)) mismatches++;
  }
  // a pose out of reach: false, NaN, and NO error (the call ran)
  {
    double far[8], got[14];
    memcpy(far, &poses[0], sizeof far);
    far[2] += 10.0;
    const bool r = proj.sampleCalibGoal(far, &joints[14], got);
    printf("goal unreachable ok=%d nan=%d error=%d\n", (int)r, (int)all_nan(got, 14), proj.lastError());
    if (r || !all_nan(got, 14)) mismatches++;
  }
  errors_before += proj.lastError() != CCMP_OK;

  // ---- Roadmap::grow against ccmp_roadmap_grow_host
  const unsigned k = 5;
  const int ms = 12;
  for (size_t t = 0; t < 3; t++) {
    double pose[8];
    memcpy(pose, &poses[(N - 1 - t) * 8], sizeof pose);
    if (t == 2) pose[0] += 10.0; // no state: empty slots
    const uint64_t index = proj.ikNextIndex();
    std::vector<int32_t> widx(k), wn(k);
    std::vector<uint8_t> wok(k);
    std::vector<double> wst((size_t)k * ms * 14);
    double wq[14];
    uint8_t wik = 0;
    int32_t wwhich = -7;
    if (ccmp_roadmap_grow_host(rm.handle(), &proj.problem(), nullptr, 0.0, &proj.ikOptions(), pose, 1, (int)k, CCMP_KNN_ALL, 0, kSeed, index, 0, ms, 0, widx.data(),
                               nullptr, wq, &wik, &wwhich, wst.data(), wn.data(), wok.data(), nullptr, nullptr, nullptr) != CCMP_OK)
      return 7;
    std::vector<int32_t> idx, n;
    std::vector<uint8_t> ok;
    std::vector<double> st;
    double gq[14];
    int which = -7;
    const bool r = rm.grow(pose, k, ms, &idx, gq, &which, &n, &ok, &st);
    bool agree = r == (wik != 0) && which == wwhich && same_bits(gq, wq, 14) && idx == widx && n == wn && ok == wok && proj.ikNextIndex() == index + 1;
    for (unsigned e = 0; e < k && agree; e++) agree = same_bits(&st[(size_t)e * ms * 14], &wst[(size_t)e * ms * 14], (size_t)std::min(n[e], ms) * 14);
    if (!r)
      for (unsigned e = 0; e < k; e++) agree = agree && n[e] == 0 && ok[e] == 0;
    if (!agree) mismatches++;
    int reached = 0;
    for (unsigned e = 0; e < k; e++) reached += ok[e] == 1;
    printf("grow t=%zu ok=%d which=%d reached=%d agree=%d\n", t, (int)r, which, reached, (int)agree);
  }
  errors_before += rm.lastError() != CCMP_OK;

  // ---- failing calls: false, NaN, the first error kept until cleared
  double got[14] = {0};
  std::vector<double> many(17 * 14, 0.1);
  int which = 5;
  const bool f1 = proj.sampleCalibGoal(&poses[0], many.data(), 17, got, &which); // S beyond CCMP_IK_MAX_SEEDS
  const bool nan1 = all_nan(got, 14) && which == -1;
  const int e1 = proj.lastError();
  proj.ikOptions().max_rounds = 0;
  double got2[14] = {0};
  const bool f2 = proj.sampleCalibGoal(&poses[0], &joints[14], got2);
  const bool nan2 = all_nan(got2, 14);
  const bool kept = proj.lastError() == e1 && !proj.lastErrorMessage().empty();
  proj.clearError();
  const int cleared = proj.lastError();
  ccmp_ik_opts_default(&proj.ikOptions());
  std::vector<int32_t> idx, n;
  std::vector<uint8_t> ok;
  std::vector<double> st;
  double gq[14] = {0};
  const bool f3 = rm.grow(&poses[0], 17, ms, &idx, gq, &which, &n, &ok, &st); // k beyond CCMP_IK_MAX_SEEDS
  const bool nan3 = all_nan(gq, 14) && which == -1;
  const int e3 = rm.lastError();
  rm.clearError();
  printf("summary solved %d mismatches %d before %d failed %d%d%d nan %d%d%d sticky %d kept %d cleared %d roadmap %d cleared %d\n", solved, mismatches,
         errors_before, (int)f1, (int)f2, (int)f3, (int)nan1, (int)nan2, (int)nan3, e1, (int)kept, cleared, e3, rm.lastError());
  return 0;
}
