// The connection step through part 2 of include/ccmp_ompl_adapter.hpp against the interface mock in tests/cpp/mock_ompl:
// addMilestone's neighbour loop runs twice over the same growing roadmap, once as jy_ProjectedStateSpace::connectMilestone (nearestK +
// checkMotion of all neighbours in one launch) and once as the reference writes it (nearestK, then checkMotion per neighbour).  Every
// result is printed with a section tag; the two sections must agree line by line, the checker's questions included
// (tests/test_cpp_adapter_connect.py).  nearestK itself is compared with a ranking computed here.
// usage: adapter_connect_check <start_joint 14 values...>
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

static uint64_t list_hash(const std::vector<ob::State *> &l)
{
  uint64_t h = 0xcbf29ce484222325ull;
  for (const ob::State *s : l) h = hash_state(h, s);
  return h;
}

// KinematicChainSpace::distance as the CPU checker states it: the FMA chain over the 14 joints, then the square root
static double joint_distance(const ob::State *a, const ob::State *b)
{
  const auto &x = *a->as<ob::ConstrainedStateSpace::StateType>();
  const auto &y = *b->as<ob::ConstrainedStateSpace::StateType>();
  double d = 0.0;
  for (int i = 0; i < 14; i++) {
    const double diff = x[i] - y[i];
    d = std::fma(diff, diff, d);
  }
  return std::sqrt(d);
}

int main(int argc, char **argv)
{
  if (argc < 15) return 2;
  try {
    Eigen::VectorXd start(14);
    for (int i = 0; i < 14; i++) start[i] = std::atof(argv[1 + i]);
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

    ob::State *a = space->allocState();
    auto &xa = *a->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) xa[i] = start[i];
    ob::StateSamplerPtr sampler = space->allocDefaultStateSampler();
    // the roadmap: projected samples near the start; vertex 20 is moved off the manifold (checkMotion must refuse it as a target);
    // vertex 9 repeats vertex 4 (equal distances: the lower index first)
    const int V = 32;
    std::vector<ob::State *> verts;
    for (int v = 0; v < V; v++) {
      ob::State *s = space->allocState();
      sampler->sampleUniformNear(s, v == 0 ? a : verts[(v * 7) % v], 0.5);
      verts.push_back(s);
    }
    {
      auto &x = *verts[20]->as<ob::ConstrainedStateSpace::StateType>();
      for (int i = 0; i < 14; i++) x[i] += 0.05;
      auto &y = *verts[9]->as<ob::ConstrainedStateSpace::StateType>();
      const auto &z = *verts[4]->as<ob::ConstrainedStateSpace::StateType>();
      for (int i = 0; i < 14; i++) y[i] = z[i];
    }
    const unsigned k = 5;
    int bad_rank = 0;
    for (int section = 0; section < 2; section++) {
      const char *tag = section == 0 ? "connect" : "loop";
      auto exact = std::make_shared<ExactChecker>();
      si.setStateValidityChecker(exact);
      jy_MotionValidator mv(si_ptr);
      for (int v = 3; v < V; v++) { // (v = 3, 4: fewer nodes than k)
        std::vector<const ob::State *> nodes(verts.begin(), verts.begin() + v);
        std::vector<unsigned> nb;
        std::vector<char> reached;
        std::vector<std::vector<ob::State *>> lists;
        if (section == 0) {
          space->connectMilestone(nodes, verts[v], k, &nb, &reached, &lists);
        } else {
          space->nearestK(nodes, verts[v], k, &nb);
          // the ranking itself: ascending (distance, index)
          std::vector<std::pair<double, unsigned>> all;
          for (int j = 0; j < v; j++) all.emplace_back(joint_distance(nodes[j], verts[v]), (unsigned)j);
          std::sort(all.begin(), all.end());
          if (nb.size() != std::min<size_t>(k, all.size())) bad_rank++;
          for (size_t r = 0; r < nb.size() && r < all.size(); r++)
            if (nb[r] != all[r].second) bad_rank++;
          for (unsigned j : nb) reached.push_back(mv.checkMotion(nodes[j], verts[v]) ? 1 : 0); // the reference's loop
        }
        for (size_t r = 0; r < nb.size(); r++) std::printf("%s v %d r %zu nb %u ok %d\n", tag, v, r, nb[r], (int)reached[r]);
        if (section == 0) { // the lists of connectMilestone against single discreteGeodesic calls (a checker of their own)
          auto other = std::make_shared<ExactChecker>();
          si.setStateValidityChecker(other);
          const bool target_ok = constraint->isSatisfied(verts[v]);
          for (size_t r = 0; r < nb.size(); r++) {
            std::vector<ob::State *> geo;
            space->discreteGeodesic(nodes[nb[r]], verts[v], false, &geo);
            const bool same = target_ok ? (geo.size() == lists[r].size() && list_hash(geo) == list_hash(lists[r]))
                                        : (lists[r].size() == 1 && hash_state(0, lists[r][0]) == hash_state(0, nodes[nb[r]]) && !reached[r]);
            std::printf("lists v %d r %zu n %zu same %d target %d\n", v, r, lists[r].size(), same ? 1 : 0, target_ok ? 1 : 0);
            for (ob::State *s : geo) space->freeState(s);
            for (ob::State *s : lists[r]) space->freeState(s);
          }
          si.setStateValidityChecker(exact);
        }
      }
      std::printf("%s counters exact_calls %d exact_hash %016" PRIx64 "\n", tag, exact->calls_, exact->hash_);
    }
    std::printf("rank mismatches %d errors %d\n", bad_rank, constraint->lastError());
    for (ob::State *s : verts) space->freeState(s);
    space->freeState(a);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
