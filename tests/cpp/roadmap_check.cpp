// ccmp::Roadmap and the jy_ProjectedStateSpace overloads that take one (include/ccmp_ompl_adapter.hpp) against the interface mock in
// tests/cpp/mock_ompl.  A roadmap grows vertex by vertex twice: once as a node vector through connectMilestone(nodes, ...) and once as
// a device-resident ccmp::Roadmap through connectMilestone(rm, ..., pose8 = nullptr, ...): on the joint metric the two must agree line
// by line (tests/test_cpp_adapter_roadmap.py).  The object metric is compared with a ranking computed here from ccmp_pose_distance
// over the poses the store derived; then the planner's remove-the-last-vertex, growTree's pose-only vertex and the sticky error.
// usage: roadmap_check <start_joint 14 values...>
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

// what ompl::base::SE3StateSpace::StateType offers, as far as ccmp::poseOf reads it
struct Se3Like {
  struct Rot { double x, y, z, w; } rot;
  double p[3];
  double getX() const { return p[0]; }
  double getY() const { return p[1]; }
  double getZ() const { return p[2]; }
  const Rot &rotation() const { return rot; }
};

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
class ExactChecker : public ob::StateValidityChecker {
public:
  bool isValid(const ob::State *s) const override
  {
    calls_++;
    const auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
    return std::fmod(std::fabs(x[3]) * 1000.0, 11.0) >= 1.0; // refuses about one state in eleven
  }
  mutable int calls_ = 0;
};

static void joints_of(const ob::State *s, double *q)
{
  const auto &x = *s->as<ob::ConstrainedStateSpace::StateType>();
  for (int i = 0; i < 14; i++) q[i] = x[i];
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
    const int V = 24;
    std::vector<ob::State *> verts;
    for (int v = 0; v < V; v++) {
      ob::State *s = space->allocState();
      sampler->sampleUniformNear(s, v == 0 ? a : verts[(v * 7) % v], 0.5);
      verts.push_back(s);
    }
    {
      auto &y = *verts[9]->as<ob::ConstrainedStateSpace::StateType>();
      const auto &z = *verts[4]->as<ob::ConstrainedStateSpace::StateType>();
      for (int i = 0; i < 14; i++) y[i] = z[i]; // equal distances: the lower index first
    }
    const unsigned k = 5;
    int mismatches = 0, self_returned = 0;
    ccmp::Roadmap rm(constraint->impl(), 4); // grows on the way
    for (int section = 0; section < 2; section++) {
      const char *tag = section == 0 ? "vector" : "roadmap";
      auto exact = std::make_shared<ExactChecker>();
      si.setStateValidityChecker(exact);
      for (int v = 0; v < V; v++) {
        std::vector<unsigned> nb;
        std::vector<char> reached;
        std::vector<std::vector<ob::State *>> lists;
        if (section == 0) {
          std::vector<const ob::State *> nodes(verts.begin(), verts.begin() + v);
          if (v > 0) space->connectMilestone(nodes, verts[v], k, &nb, &reached, &lists);
        } else {
          if (rm.size() != (size_t)v) mismatches++;
          space->connectMilestone(rm, verts[v], nullptr, k, &nb, &reached, &lists);
          double q[14];
          size_t first = 99;
          joints_of(verts[v], q);
          // the documented sequence — query, THEN append (the reference's order, stefanBiPRM.cpp:390-410) — never returns the vertex itself
          for (unsigned j : nb) self_returned += j >= (unsigned)v;
          if (!rm.append(q, nullptr, 1, &first) || first != (size_t)v) mismatches++; // the pose is derived on the device
          // ... and a caller that appends first says so: NOT_SELF at the new index gives the same neighbours, without the vertex
          std::vector<unsigned> after;
          if (!space->nearestK(rm, verts[v], nullptr, k, &after, CCMP_KNN_NOT_SELF, first) || after != nb) mismatches++;
          for (unsigned j : after) self_returned += j == (unsigned)v;
        }
        for (size_t r = 0; r < nb.size(); r++) {
          std::printf("%s v %d r %zu nb %u ok %d n %zu\n", tag, v, r, nb[r], (int)reached[r], lists[r].size());
          for (ob::State *s : lists[r]) space->freeState(s);
        }
      }
      std::printf("%s counters exact_calls %d\n", tag, exact->calls_);
    }
    // read-back: the joints are the vertices', bit for bit
    std::vector<double> J((size_t)V * 14), P((size_t)V * 8);
    if (!rm.read(0, V, J.data(), P.data())) mismatches++;
    for (int v = 0; v < V; v++) {
      double q[14];
      joints_of(verts[v], q);
      if (std::memcmp(q, &J[(size_t)v * 14], sizeof q) != 0 || P[(size_t)v * 8 + 7] != 0.0) mismatches++;
    }
    // the object metric: every vertex's pose as the query, against (ccmp_pose_distance, index) sorted here
    int object_queries = 0;
    for (int v = 0; v < V; v++) {
      std::vector<int32_t> idx;
      std::vector<double> dist;
      if (!rm.nearestK(CCMP_METRIC_OBJECT, &P[(size_t)v * 8], k, &idx, &dist, CCMP_KNN_NOT_SELF, (size_t)v)) mismatches++;
      std::vector<std::pair<double, int32_t>> all;
      for (int j = 0; j < V; j++)
        if (j != v) all.emplace_back(ccmp_pose_distance(&P[(size_t)v * 8], &P[(size_t)j * 8]), j);
      std::sort(all.begin(), all.end());
      for (unsigned r = 0; r < k; r++)
        if (idx[r] != all[r].second || std::memcmp(&dist[r], &all[r].first, 8) != 0) mismatches++;
      object_queries++;
      // the space's overload on the same pose: the same indices, self included this time (distance 0 first, vertex 9 behind its twin 4)
      std::vector<unsigned> nb;
      if (!space->nearestK(rm, verts[v], &P[(size_t)v * 8], k, &nb) || nb.size() != k) mismatches++;
      else if (nb[0] != (unsigned)(v == 9 ? 4 : v)) mismatches++;
    }
    // ccmp::poseOf / poseDistance on an SE3-like state
    Se3Like s1{{P[3], P[4], P[5], P[6]}, {P[0], P[1], P[2]}}, s2{{P[11], P[12], P[13], P[14]}, {P[8], P[9], P[10]}};
    double pose[8];
    ccmp::poseOf(s1, pose);
    if (std::memcmp(pose, &P[0], 64) != 0) mismatches++;
    const double d12 = ccmp::poseDistance(s1, s2), want = ccmp_pose_distance(&P[0], &P[8]);
    if (std::memcmp(&d12, &want, 8) != 0) mismatches++;
    // remove_vertex of the vertex just appended, then growTree's pose-only vertex: no joint neighbour until its joints arrive
    if (!rm.truncate(V - 1) || rm.size() != (size_t)V - 1) mismatches++;
    size_t first = 0;
    if (!rm.append(nullptr, &P[(size_t)(V - 1) * 8], 1, &first) || first != (size_t)V - 1) mismatches++;
    double qlast[14];
    joints_of(verts[V - 1], qlast);
    std::vector<int32_t> idx;
    if (!rm.nearestK(CCMP_METRIC_JOINT, qlast, 1, &idx) || idx[0] == V - 1) mismatches++;
    if (!rm.nearestK(CCMP_METRIC_OBJECT, &P[(size_t)(V - 1) * 8], 1, &idx) || idx[0] != V - 1) mismatches++;
    if (!rm.setJoints(V - 1, qlast)) mismatches++;
    if (!rm.nearestK(CCMP_METRIC_JOINT, qlast, 1, &idx) || idx[0] != V - 1) mismatches++;
    // one-call neighbours + checkMotion: the neighbours are nearestK's
    {
      std::vector<int32_t> cidx, n_states, want_idx;
      std::vector<uint8_t> ok;
      std::vector<double> states;
      if (!rm.connect(CCMP_METRIC_OBJECT, qlast, nullptr, k, true, 16, &cidx, &n_states, &ok, &states)) mismatches++;
      if (!rm.nearestK(CCMP_METRIC_OBJECT, &P[(size_t)(V - 1) * 8], k, &want_idx) || cidx != want_idx) mismatches++;
      int reached = 0;
      for (unsigned r = 0; r < k; r++) reached += ok[r] == 1;
      std::printf("connect reached %d of %u\n", reached, k);
    }
    const int before = rm.lastError();
    // the sticky error: the first failure stays until it is cleared, and nothing throws
    const bool t1 = rm.truncate(1000), t2 = rm.read(5000, 1, J.data(), nullptr);
    const int sticky = rm.lastError();
    rm.clearError();
    std::printf("object queries %d\n", object_queries);
    std::printf("self returned %d\n", self_returned);
    std::printf("summary mismatches %d errors %d before %d failed %d%d sticky %d cleared %d\n", mismatches, constraint->lastError(), before, (int)t1, (int)t2,
                sticky, rm.lastError());
    for (ob::State *s : verts) space->freeState(s);
    space->freeState(a);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
