// The resident service in analytic mode through include/ccmp_ompl_adapter.hpp against the interface mock in tests/cpp/mock_ompl: a
// planner-shaped sequence — project and isSatisfied one state at a time, growTree's discreteGeodesics of five edges (lists that
// overflow their first call, so that continuation calls with carry_in run), checkMotion, single edges — runs twice on the same
// vertices after setJacobianMode(1): with setResident(false), section "launched", and with setResident(true), section "resident".
// Every result is printed in hex behind its section tag; the two sections must agree line by line, the constraint's lastError()
// must stay 0, and the context's "resident_served" must have risen in the resident section only
// (tests/test_cpp_adapter_resident_analytic.py).
// usage: adapter_resident_analytic_check <start_joint 14 values...>
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

class AmbientSampler : public ob::StateSampler {
public:
  using ob::StateSampler::StateSampler;
  void sampleUniform(ob::State *s) override
  {
    auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) x[i] = 0.1;
  }
  void sampleUniformNear(ob::State *s, const ob::State *near, double d) override
  {
    auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
    const auto &n = *near->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) x[i] = n[i] + ((i & 1) ? d : -d) * 0.5;
  }
  void sampleGaussian(ob::State *s, const ob::State *mean, double sd) override { sampleUniformNear(s, mean, sd); }
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
class AllValid : public ob::StateValidityChecker {
public:
  bool isValid(const ob::State *) const override { return true; }
};

static void print_list(const char *tag, const std::vector<ob::State *> &l)
{
  uint64_t h = 0xcbf29ce484222325ull;
  for (const ob::State *s : l) h = hash_state(h, s);
  std::printf("%s n %zu hash %016" PRIx64 "\n", tag, l.size(), h);
}

static long served(const ChainConstraintPtr &constraint)
{
  long v = -1;
  if (ccmp_ctx_get_option(constraint->impl().ctx(), "resident_served", &v) != CCMP_OK) return -1;
  return v;
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
    constraint->impl().setJacobianMode(1);
    if (ccmp_ctx_set_option(constraint->impl().ctx(), "resident_idle_ms", 200) != CCMP_OK) return 3;
    auto ambient = std::make_shared<AmbientSpace>();
    auto space = std::make_shared<jy_ProjectedStateSpace>(ambient, constraint);
    auto si_ptr = std::make_shared<ob::SpaceInformation>();
    ob::SpaceInformation &si = *si_ptr;
    si.setStateSpace(space);
    space->setSpaceInformation(&si);
    space->setDelta(0.01); // short steps: edges between vertices ~1 rad apart list more than the 64 states of a first call
    space->setLambda(2.0);
    si.setStateValidityChecker(std::make_shared<AllValid>());

    ob::State *a = space->allocState();
    auto &xa = *a->as<ob::ConstrainedStateSpace::StateType>();
    for (int i = 0; i < 14; i++) xa[i] = start[i];
    ob::StateSamplerPtr sampler = space->allocDefaultStateSampler();
    std::vector<ob::State *> verts;
    for (int v = 0; v < 16; v++) {
      ob::State *s = space->allocState();
      sampler->sampleUniformNear(s, v == 0 ? a : verts[(v * 7) % v], 0.5);
      verts.push_back(s);
    }
    size_t longest = 0;
    for (int section = 0; section < 2; section++) {
      const char *tag = section == 0 ? "launched" : "resident";
      constraint->setResident(section == 1);
      const long served_before = served(constraint);
      // project / isSatisfied / jointValid / function of single states: the vertices, pushed off the manifold
      for (int v = 0; v < 16; v++) {
        Eigen::VectorXd x(14), f(2);
        const auto &sv = *verts[v]->as<ob::ConstrainedStateSpace::StateType>();
        for (int i = 0; i < 14; i++) x[i] = sv[i] + 0.03 * ((i + v) % 3 - 1);
        const bool sat0 = constraint->isSatisfied(x);
        constraint->function(x, f);
        const bool ok = constraint->project(x);
        const bool sat1 = constraint->isSatisfied(x);
        uint64_t h = 0xcbf29ce484222325ull;
        for (int i = 0; i < 14; i++) h = (h ^ bits(x[i])) * 0x100000001b3ull;
        std::printf("%s state %d sat %d f %016" PRIx64 " %016" PRIx64 " project %d x %016" PRIx64 " sat %d valid %d\n", tag, v, sat0 ? 1 : 0, bits(f[0]), bits(f[1]),
                    ok ? 1 : 0, h, sat1 ? 1 : 0, constraint->jointValid(x) ? 1 : 0);
      }
      // growTree: a new vertex against five earlier ones, in one call
      for (int v = 5; v < 16; v++) {
        std::vector<const ob::State *> from;
        for (int k = 1; k <= 5; k++) from.push_back(verts[v - k]);
        std::vector<std::vector<ob::State *>> lists;
        std::vector<char> reached;
        space->discreteGeodesics(from, verts[v], false, &lists, &reached);
        for (size_t e = 0; e < from.size(); e++) {
          char t[64];
          std::snprintf(t, sizeof t, "%s grow %d %zu ok %d", tag, v, e, (int)reached[e]);
          print_list(t, lists[e]);
          if (lists[e].size() > longest) longest = lists[e].size();
          for (ob::State *s : lists[e]) space->freeState(s);
        }
      }
      // ... and with lists of three states per call through the batch function itself: every edge that moves is continued
      {
        std::vector<double> fr(5 * 14), to(5 * 14);
        for (int e = 0; e < 5; e++) {
          const auto &f = *verts[e]->as<ob::ConstrainedStateSpace::StateType>();
          const auto &t = *verts[e + 6]->as<ob::ConstrainedStateSpace::StateType>();
          for (int i = 0; i < 14; i++) { fr[14 * e + i] = f[i]; to[14 * e + i] = t[i]; }
        }
        std::vector<std::vector<std::vector<double>>> lists;
        std::vector<char> reached;
        const bool done = constraint->guarded([&] {
          ccmp::discreteGeodesicBatch(constraint->impl(), fr.data(), to.data(), 5, true, [](const double *) { return true; }, &lists, &reached, 3, false, 0.05, 2.0);
        });
        for (int e = 0; done && e < 5; e++) {
          uint64_t h = 0xcbf29ce484222325ull;
          for (const auto &row : lists[e])
            for (int i = 0; i < 14; i++) h = (h ^ bits(row[i])) * 0x100000001b3ull;
          std::printf("%s short %d ok %d n %zu hash %016" PRIx64 "\n", tag, e, (int)reached[e], lists[e].size(), h);
        }
      }
      jy_MotionValidator mv(si_ptr);
      for (int v = 0; v + 3 < 16; v++) {
        std::vector<ob::State *> geo;
        const bool g = space->discreteGeodesic(verts[v], verts[v + 3], false, &geo);
        char t[64];
        std::snprintf(t, sizeof t, "%s edge %d ok %d motion %d", tag, v, g ? 1 : 0, mv.checkMotion(verts[v + 3], verts[v]) ? 1 : 0);
        print_list(t, geo);
        for (ob::State *s : geo) space->freeState(s);
      }
      std::printf("%s_counters served %ld error %d longest %zu\n", tag, served(constraint) - served_before, constraint->lastError(), longest);
      if (constraint->lastError() != 0) std::fprintf(stderr, "lastError: %s\n", constraint->lastErrorMessage().c_str());
    }
    constraint->setResident(false);
    for (ob::State *s : verts) space->freeState(s);
    space->freeState(a);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
