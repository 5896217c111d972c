// ccmp::Roadmap's solution step (include/ccmp_ompl_adapter.hpp: shortestPath, constructSolution) against the interface mock in
// tests/cpp/mock_ompl.  A store of sampled vertices gets a ring with chords, a chain and an isolated vertex; every pair goes through
// shortestPath and, on the edges read back from the store, through ccmp_graph_shortest_paths_ref: the "adapter" and "ref" lines must
// agree line by line (tests/test_cpp_adapter_path.py); the returned rows are compared here with the store's, bit for bit;
// constructSolution against its definition on the ref form; then the sticky error on deliberate bad calls.
// usage: path_check <start_joint 14 values...>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <limits>

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
    int mismatches = 0;
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (int v = 0; v < V; v++) {
      double q[14];
      joints_of(verts[v], q);
      if (!rm.append(q, nullptr)) mismatches++;
    }
    // two components and an isolated vertex: a ring over 0..11 with chords (several routes, the equal rows 4 and 9 make a real tie), a
    // chain over 12..22; vertex 23 alone
    std::vector<int32_t> uv;
    for (int v = 0; v < 12; v++) { uv.push_back(v); uv.push_back((v + 1) % 12); }
    for (int v = 0; v < 12; v += 3) { uv.push_back((v + 5) % 12); uv.push_back(v); }
    uv.push_back(3); uv.push_back(4); // a parallel edge
    for (int v = 12; v < 22; v++) { uv.push_back(v + 1); uv.push_back(v); }
    if (!rm.addEdges(uv.data(), uv.size() / 2) || rm.numEdges() != uv.size() / 2) mismatches++;
    const size_t N = rm.size(), E = rm.numEdges();
    std::vector<int32_t> euv(2 * E);
    std::vector<double> ew(E), J(N * 14);
    if (!rm.readEdges(0, E, euv.data(), ew.data()) || !rm.read(0, N, J.data(), nullptr)) mismatches++;
    const int32_t pairs[][2] = {{0, 6}, {6, 0}, {2, 9}, {9, 4}, {12, 22}, {22, 15}, {7, 7}, {0, 12}, {23, 1}, {5, 23}};
    const size_t F = sizeof pairs / sizeof pairs[0];
    for (size_t f = 0; f < F; f++) {
      const int32_t s = pairs[f][0], t = pairs[f][1];
      std::vector<int32_t> path, want((size_t)N, -1);
      std::vector<std::array<double, 14>> rows;
      double cost = -1.0, want_cost = -1.0;
      int32_t want_len = -1;
      const bool found = rm.shortestPath(s, t, path, cost, &rows);
      if (ccmp_graph_shortest_paths_ref(euv.data(), ew.data(), E, N, &s, &t, 1, (int)N, &want_cost, &want_len, want.data(), nullptr, nullptr) != CCMP_OK) mismatches++;
      std::printf("adapter pair %d %d found %d cost %a path", s, t, (int)found, cost);
      for (int32_t v : path) std::printf(" %d", v);
      std::printf("\nref pair %d %d found %d cost %a path", s, t, (int)(want_len > 0), want_cost);
      for (int32_t i = 0; i < want_len; i++) std::printf(" %d", want[(size_t)i]);
      std::printf("\n");
      if (rows.size() != path.size()) mismatches++;
      for (size_t i = 0; i < rows.size() && i < path.size(); i++)
        if (std::memcmp(rows[i].data(), J.data() + (size_t)path[i] * 14, 14 * sizeof(double)) != 0) mismatches++;
    }
    // constructSolution against its definition on the ref form: the connected pairs in starts-major order, the first cheapest
    {
      const std::vector<int32_t> starts = {23, 0, 14, 3}, goals = {8, 20, 6};
      std::vector<int32_t> lab(N), got_idx, best_path;
      if (!rm.readLabels(0, N, lab.data())) mismatches++;
      double best = std::numeric_limits<double>::infinity();
      for (int32_t s : starts)
        for (int32_t t : goals) {
          if (lab[(size_t)s] != lab[(size_t)t]) continue;
          std::vector<int32_t> want((size_t)N, -1);
          double c = -1.0;
          int32_t len = -1;
          if (ccmp_graph_shortest_paths_ref(euv.data(), ew.data(), E, N, &s, &t, 1, (int)N, &c, &len, want.data(), nullptr, nullptr) != CCMP_OK) mismatches++;
          if (len > 0 && c < best) { best = c; best_path.assign(want.begin(), want.begin() + len); }
        }
      std::vector<std::array<double, 14>> states;
      double cost = -1.0;
      const bool found = rm.constructSolution(starts, goals, states, &cost, &got_idx);
      std::printf("adapter solution found %d cost %a path", (int)found, cost);
      for (int32_t v : got_idx) std::printf(" %d", v);
      std::printf("\nref solution found %d cost %a path", (int)!best_path.empty(), best);
      for (int32_t v : best_path) std::printf(" %d", v);
      std::printf("\n");
      if (states.size() != got_idx.size()) mismatches++;
      for (size_t i = 0; i < states.size() && i < got_idx.size(); i++)
        if (std::memcmp(states[i].data(), J.data() + (size_t)got_idx[i] * 14, 14 * sizeof(double)) != 0) mismatches++;
      // no pair in one component: "no", and no error
      std::vector<std::array<double, 14>> none;
      if (rm.constructSolution({23}, {0, 13}, none) || !none.empty() || rm.constructSolution({}, {0}, none)) mismatches++;
    }
    const int before = rm.lastError();
    // the sticky error: a vertex that does not exist — refused on the host, the first code stays until it is cleared, nothing throws
    std::vector<int32_t> path;
    double cost = 0.0;
    const bool t1 = rm.shortestPath(0, (int32_t)N, path, cost), t2 = rm.shortestPath(-1, 0, path, cost);
    const bool shape = path.empty() && std::isinf(cost);
    const int sticky = rm.lastError();
    rm.clearError();
    const bool t3 = rm.shortestPath(0, 6, path, cost); // and the store still answers
    std::printf("summary mismatches %d errors %d before %d failed %d%d shape %d sticky %d cleared %d again %d\n", mismatches, constraint->lastError(), before, (int)t1,
                (int)t2, (int)shape, sticky, rm.lastError(), (int)t3);
    for (ob::State *s : verts) space->freeState(s);
    space->freeState(a);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
