// ccmp::Roadmap's graph verbs (include/ccmp_ompl_adapter.hpp: commit, addEdges, closest, numEdges, readEdges, readLabels) against the
// interface mock in tests/cpp/mock_ompl.  A store of sampled vertices gets a start component; then twelve new states go through
// connect() -> commit(), and the same arrays through ccmp_roadmap_commit_ref: the "adapter" and "ref" lines must agree line by line
// (tests/test_cpp_adapter_graph.py), the rows and edges in the store are compared here bit for bit, the labels against
// ccmp_graph_labels_ref; closest() against ccmp_roadmap_closest_ref; then the sticky error on deliberate bad calls.
// usage: graph_check <start_joint 14 values...>
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
    const int MS = 16;
    int mismatches = 0;
    ccmp::Roadmap rm(constraint->impl(), 4); // rows and edges grow on the way
    for (int v = 0; v < V; v++) {
      double q[14];
      joints_of(verts[v], q);
      if (!rm.append(q, nullptr)) mismatches++;
    }
    // the planner's start component: a chain over the first six vertices, and one more edge elsewhere
    const int32_t seed_edges[6][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {10, 11}};
    if (!rm.addEdges(&seed_edges[0][0], 6) || rm.numEdges() != 6) mismatches++;
    const std::vector<int32_t> roots = {0};
    double goal[8];
    {
      std::vector<double> P(8);
      if (!rm.read(V - 1, 1, nullptr, P.data())) mismatches++;
      std::memcpy(goal, P.data(), sizeof goal);
      goal[0] += 0.02;
    }
    // new vertices: states sampled near existing ones; connect() supplies what grow() would, commit() decides; the same arrays through
    // ccmp_roadmap_commit_ref give the "ref" lines
    for (int step = 0; step < 12; step++) {
      ob::State *s = space->allocState();
      sampler->sampleUniformNear(s, verts[(step * 5) % V], 0.3);
      double q[14], pose[8];
      joints_of(s, q);
      space->freeState(s);
      size_t at = 0;
      if (!rm.append(q, nullptr, 1, &at) || !rm.read(at, 1, nullptr, pose) || !rm.truncate(at)) mismatches++; // the pose as the store derives it
      std::vector<int32_t> idx, n_states;
      std::vector<uint8_t> ok;
      std::vector<double> states;
      if (!rm.connect(CCMP_METRIC_OBJECT, q, pose, k, false, MS, &idx, &n_states, &ok, &states)) mismatches++;
      const size_t N = rm.size(), E = rm.numEdges();
      std::vector<double> J(N * 14), P(N * 8);
      std::vector<int32_t> L(N);
      if (!rm.read(0, N, J.data(), P.data()) || !rm.readLabels(0, N, L.data())) mismatches++;
      int32_t ref_new = -1, ref_state = -1;
      std::vector<int32_t> ref_mid(k, -1), ref_uv(2 * k);
      std::vector<double> ref_rj((1 + k) * 14), ref_rp((1 + k) * 8), ref_w(k);
      size_t ref_nv = 0, ref_ne = 0;
      const bool keep = step % 5 == 4;
      const int rc = ccmp_roadmap_commit_ref(&constraint->impl().problem(), J.data(), P.data(), L.data(), N, idx.data(), ok.data(), n_states.data(), states.data(), MS,
                                             q, pose, nullptr, 1, (int)k, goal, roots.data(), (int)roots.size(), keep ? CCMP_COMMIT_KEEP_ISOLATED : 0, &ref_new,
                                             ref_mid.data(), &ref_state, ref_rj.data(), ref_rp.data(), ref_uv.data(), ref_w.data(), &ref_nv, &ref_ne);
      if (rc != CCMP_OK) mismatches++;
      int32_t got_new = -1;
      std::vector<int32_t> got_mid;
      const int got_state = rm.commit(idx, ok, n_states, &states, MS, q, pose, goal, roots, &got_new, &got_mid, keep);
      std::printf("adapter step %d state %d new %d mids", step, got_state, got_new);
      for (int32_t m : got_mid) std::printf(" %d", m);
      std::printf(" size %zu edges %zu\n", rm.size(), rm.numEdges());
      std::printf("ref step %d state %d new %d mids", step, ref_state, ref_new);
      for (int32_t m : ref_mid) std::printf(" %d", m);
      std::printf(" size %zu edges %zu\n", N + ref_nv, E + ref_ne);
      // the rows and edges the store now holds are the ref's, bit for bit
      if (rm.size() == N + ref_nv && rm.numEdges() == E + ref_ne) {
        std::vector<double> rj(ref_nv * 14), rp(ref_nv * 8), w(ref_ne);
        std::vector<int32_t> uv(2 * ref_ne);
        if (ref_nv && (!rm.read(N, ref_nv, rj.data(), rp.data()) || std::memcmp(rj.data(), ref_rj.data(), rj.size() * 8) != 0 ||
                       std::memcmp(rp.data(), ref_rp.data(), rp.size() * 8) != 0)) mismatches++;
        if (ref_ne && (!rm.readEdges(E, ref_ne, uv.data(), w.data()) || std::memcmp(uv.data(), ref_uv.data(), uv.size() * 4) != 0 ||
                       std::memcmp(w.data(), ref_w.data(), w.size() * 8) != 0)) mismatches++;
      } else mismatches++;
      // the labels against the host union-find over every edge
      {
        const size_t N2 = rm.size(), E2 = rm.numEdges();
        std::vector<int32_t> uv(2 * E2), lab(N2), want(N2);
        if (!rm.readEdges(0, E2, uv.data(), nullptr) || !rm.readLabels(0, N2, lab.data()) || ccmp_graph_labels_ref(uv.data(), E2, N2, want.data()) != CCMP_OK ||
            lab != want) mismatches++;
      }
    }
    // closest: every vertex's component against the ref on the arrays read back
    {
      const size_t N = rm.size();
      std::vector<double> P(N * 8);
      std::vector<int32_t> L(N), froms = {0, 7, 10, (int32_t)N - 1, 3};
      if (!rm.read(0, N, nullptr, P.data()) || !rm.readLabels(0, N, L.data())) mismatches++;
      std::vector<int32_t> idx, want_idx(froms.size());
      std::vector<double> dist, fd, want_dist(froms.size()), want_fd(froms.size());
      if (!rm.closest(froms, goal, &idx, &dist, &fd)) mismatches++;
      if (ccmp_roadmap_closest_ref(P.data(), L.data(), N, froms.data(), froms.size(), goal, want_idx.data(), want_dist.data(), want_fd.data()) != CCMP_OK) mismatches++;
      for (size_t f = 0; f < froms.size(); f++) {
        std::printf("adapter closest from %d idx %d dist %a from_dist %a\n", froms[f], idx[f], dist[f], fd[f]);
        std::printf("ref closest from %d idx %d dist %a from_dist %a\n", froms[f], want_idx[f], want_dist[f], want_fd[f]);
      }
    }
    const int before = rm.lastError();
    // the sticky error: a loop edge, then an edge to nowhere — both refused, the first code stays until it is cleared, nothing throws
    const int32_t loop[2] = {3, 3}, nowhere[2] = {0, 1 << 20};
    const size_t edges_before = rm.numEdges();
    const bool t1 = rm.addEdges(loop), t2 = rm.addEdges(nowhere);
    const bool t3 = rm.truncate(1); // below the edge floor
    const int sticky = rm.lastError();
    if (rm.numEdges() != edges_before) mismatches++;
    rm.clearError();
    std::printf("summary mismatches %d errors %d before %d failed %d%d%d sticky %d cleared %d\n", mismatches, constraint->lastError(), before, (int)t1, (int)t2,
                (int)t3, sticky, rm.lastError());
    for (ob::State *s : verts) space->freeState(s);
    space->freeState(a);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
