// The extend step with the proxy pre-filter on the device, through part 2 of include/ccmp_ompl_adapter.hpp against the interface mock
// in tests/cpp/mock_ompl: a planner-shaped loop (growTree's discreteGeodesics, checkMotion, single discreteGeodesic calls) runs twice,
// once with a PrefilteredValidityChecker installed (jy_ProjectedStateSpace runs the proxies inside the traversal) and once with the
// same kind of checker behind a wrapper that hides its type (the host path: one clearance call per listed state).  Every result is
// printed with a section tag; the two sections must agree line by line (tests/test_cpp_adapter_scene.py).
// usage: adapter_scene_check <margin> <start_joint 14 values...>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <iostream>
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

namespace ob = ompl::base;

static uint64_t bits(double v)
{
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return u;
}
static uint64_t hash_state(uint64_t h, const ob::State *s)
{
  const auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
  for (int i = 0; i < 14; i++) h = (h ^ bits(x[i])) * 0x100000001b3ull;
  return h;
}

// ambient space stand-in: KinematicChainSpace's enforceBounds (KinematicChain.h:118-130) and a fixed "sampler"
class AmbientSampler : public ob::StateSampler {
public:
  using ob::StateSampler::StateSampler;
  void sampleUniform(ob::State *s) override { fill(s, 0.1); }
  void sampleUniformNear(ob::State *s, const ob::State *near, double d) override
  {
    auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
    const auto &n = *near->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) x[i] = n[i] + ((i & 1) ? d : -d) * 0.5;
  }
  void sampleGaussian(ob::State *s, const ob::State *mean, double sd) override { sampleUniformNear(s, mean, sd); }
private:
  static void fill(ob::State *s, double v)
  {
    auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) x[i] = v;
  }
};
class AmbientSpace : public ob::StateSpace {
public:
  AmbientSpace() { setName("KinematicChainSpace"); }
  ob::StateSamplerPtr allocDefaultStateSampler() const override { return std::make_shared<AmbientSampler>(this); }
  void enforceBounds(ob::State *s) const override
  {
    auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) {
      double v = std::fmod(x[i], 2.0 * M_PI);
      if (v < -M_PI) v += 2.0 * M_PI;
      else if (v >= M_PI) v -= 2.0 * M_PI;
      x[i] = v;
    }
  }
  ob::State *allocState() const override { return new ob::ConstrainedStateSpace::StateType(); }
};
// the exact checker (MoveIt in the reference): a deterministic rule on the state, and a log of what it was asked, in order
class ExactChecker : public ob::StateValidityChecker {
public:
  bool isValid(const ob::State *s) const override
  {
    calls_++;
    hash_ = hash_state(hash_, s);
    const auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
    return std::fmod(std::fabs(x[3]) * 1000.0, 11.0) >= 1.0; // refuses about one state in eleven
  }
  mutable int calls_ = 0;
  mutable uint64_t hash_ = 0xcbf29ce484222325ull;
};
// hides the type of the checker it wraps: jy_ProjectedStateSpace cannot see the proxies and takes the host path
class Hidden : public ob::StateValidityChecker {
public:
  explicit Hidden(ob::StateValidityCheckerPtr inner) : inner_(std::move(inner)) {}
  bool isValid(const ob::State *s) const override { return inner_->isValid(s); }
private:
  ob::StateValidityCheckerPtr inner_;
};

static void print_list(const char *tag, const std::vector<ob::State *> &l)
{
  uint64_t h = 0xcbf29ce484222325ull;
  for (const ob::State *s : l) h = hash_state(h, s);
  std::printf("%s n %zu hash %016" PRIx64 "\n", tag, l.size(), h);
}

int main(int argc, char **argv)
{
  if (argc < 16) return 2;
  try {
    const double margin = std::atof(argv[1]);
    Eigen::VectorXd start(14);
    for (int i = 0; i < 14; i++) start[i] = std::atof(argv[2 + i]);
    auto arm1 = std::make_shared<ArmModel>();
    auto arm2 = std::make_shared<ArmModel>();
    arm1->name = "panda_left"; arm1->index = 0;
    arm2->name = "panda_right"; arm2->index = 1;
    arm1->t_wb.translation()(1) = 0.3;  arm1->t_wb.translation()(2) = 1.006;
    arm2->t_wb.translation()(1) = -0.3; arm2->t_wb.translation()(2) = 1.006;
    ChainConstraintPtr constraint = std::make_shared<KinematicChainConstraint>(14);
    constraint->setArmModels(arm1, arm2);
    constraint->setInitialPosition(start);
    constraint->setTolerance(1e-3, 5e-3);
    auto ambient = std::make_shared<AmbientSpace>();
    auto space = std::make_shared<jy_ProjectedStateSpace>(ambient, constraint);
    auto si_ptr = std::make_shared<ob::SpaceInformation>();
    ob::SpaceInformation &si = *si_ptr;
    si.setStateSpace(space);
    space->setSpaceInformation(&si);
    space->setDelta(0.05);
    space->setLambda(2.0);
    // proxies: spheres along both arms' links and hands, the sub_table; neighbouring links and the two bases allowed
    std::vector<ccmp_sphere> sph;
    for (int arm = 0; arm < 2; arm++)
      for (int k = 0; k < 8; k++) {
        ccmp_sphere s;
        std::memset(&s, 0, sizeof s);
        s.frame = CCMP_FRAME(arm, k);
        s.group = arm * 9 + k;
        s.r = k == 7 ? 0.06 : 0.07;
        sph.push_back(s);
      }
    uint32_t allowed[32] = {0};
    for (int arm = 0; arm < 2; arm++)
      for (int k = 0; k < 8; k++)
        for (int j = k + 1; j < 8 && j <= k + 3; j++) ccmp::ProxyScene::allow(allowed, arm * 9 + k, arm * 9 + j);
    std::vector<ccmp_box> boxes{ccmp::ProxyScene::subTable(19)};
    auto scene = std::make_shared<ccmp::ProxyScene>(constraint->impl(), sph, boxes, allowed);

    ob::State *a = space->allocState();
    auto &xa = *a->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) xa[i] = start[i];
    ob::StateSamplerPtr sampler = space->allocDefaultStateSampler();
    // the planner's vertices: projected samples near the start, the same for both sections
    std::vector<ob::State *> verts;
    for (int v = 0; v < 24; v++) {
      ob::State *s = space->allocState();
      sampler->sampleUniformNear(s, v == 0 ? a : verts[(v * 7) % v], 0.5);
      verts.push_back(s);
    }
    for (int section = 0; section < 2; section++) {
      const char *tag = section == 0 ? "device" : "host";
      auto exact = std::make_shared<ExactChecker>();
      auto pre = std::make_shared<PrefilteredValidityChecker>(si_ptr, scene, exact, margin);
      if (section == 0) si.setStateValidityChecker(pre);
      else si.setStateValidityChecker(std::make_shared<Hidden>(pre));
      // growTree: a new vertex against up to five earlier ones, in one call
      for (int v = 5; v < 24; v++) {
        std::vector<const ob::State *> from;
        for (int k = 1; k <= 5; k++) from.push_back(verts[v - k]);
        std::vector<std::vector<ob::State *>> lists;
        std::vector<char> reached;
        space->discreteGeodesics(from, verts[v], false, &lists, &reached);
        for (size_t e = 0; e < from.size(); e++) {
          char t[64];
          std::snprintf(t, sizeof t, "%s grow %d %zu ok %d", tag, v, e, (int)reached[e]);
          print_list(t, lists[e]);
          for (ob::State *s : lists[e]) space->freeState(s);
        }
      }
      // checkMotion (isSatisfied(s2) && discreteGeodesic(s1, s2, false)) and single edges with their lists
      jy_MotionValidator mv(si_ptr);
      for (int v = 0; v + 3 < 24; v++) {
        std::vector<ob::State *> geo;
        const bool g = space->discreteGeodesic(verts[v], verts[v + 3], false, &geo);
        char t[64];
        std::snprintf(t, sizeof t, "%s edge %d ok %d motion %d", tag, v, g ? 1 : 0, mv.checkMotion(verts[v + 3], verts[v]) ? 1 : 0);
        print_list(t, geo);
        for (ob::State *s : geo) space->freeState(s);
      }
      std::printf("%s counters asked %llu rejected %llu exact_calls %d exact_hash %016" PRIx64 "\n", tag,
                  (unsigned long long)pre->askedExact(), (unsigned long long)pre->rejectedByProxies(), exact->calls_, exact->hash_);
    }
    for (ob::State *s : verts) space->freeState(s);
    space->freeState(a);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
