// The adapter's shortcut solution paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::shortcutPath,
// ccmp::Roadmap::constructShortcutSolution) against the interface mock in tests/cpp/mock_ompl.  The program reads waypoints, roadmap nodes
// and undirected edges from a text file, runs shortcutPath on the waypoints with every span and with span 2 and constructShortcutSolution
// on the roadmap, prints kept indices and rows as hex floats (tests/test_cpp_adapter_shortcut.py compares them with the oracle's verdicts
// under the restated rule) and compares each with ccmp_path_shortcut_host called directly.  Then the answers that are "unchanged path"
// with the sticky error set; nothing throws.
// usage: adapter_shortcut_check <start_joint 14 values...> <delta> <input file>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <limits>

#include <iostream>
#include <sstream>
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
  void enforceBounds(ob::State *) const override {}
  ob::State *allocState() const override { return new ob::ConstrainedStateSpace::StateType(); }
};

typedef std::vector<std::array<double, 14>> Rows;

static void print_rows(const char *tag, const Rows &rows, const std::vector<int32_t> &kept)
{
  std::printf("%s rows %zu kept", tag, rows.size());
  for (int32_t v : kept) std::printf(" %d", (int)v);
  std::printf("\n");
  for (size_t r = 0; r < rows.size(); r++) {
    std::printf("%s row %zu", tag, r);
    for (double v : rows[r]) std::printf(" %a", v);
    std::printf("\n");
  }
}

static bool read_rows(std::istream &in, size_t n, Rows &rows)
{
  rows.resize(n);
  for (auto &r : rows)
    for (double &v : r) {
      std::string tok;
      if (!(in >> tok)) return false;
      v = std::strtod(tok.c_str(), nullptr); // hex floats: the exact bits
    }
  return true;
}

static bool same_rows(const Rows &a, const Rows &b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a[0].data(), b[0].data(), a.size() * 14 * sizeof(double)) == 0);
}

// the C ABI called directly on the same waypoints: kept rows and indices
static int direct(const ccmp::Projector &proj, const Rows &in, int max_span, double delta, double lambda, Rows &rows, std::vector<int32_t> &kept, double *cost)
{
  ccmp_problem P = proj.problem();
  P.delta = delta;
  P.lambda = lambda;
  ccmp_shortcut_opts o;
  ccmp_shortcut_opts_default(&o);
  o.max_span = max_span;
  o.chunk_states = 3; // another cut than the adapter's: the result does not depend on it
  o.tile_edges = 2;
  const int32_t len = (int32_t)in.size();
  int32_t out_len = 0;
  double ci = 0.0;
  rows.assign(in.size(), std::array<double, 14>());
  kept.assign(in.size(), -1);
  std::lock_guard<std::mutex> hold(proj.mutex());
  const int rc = ccmp_path_shortcut_host(proj.ctx(), &P, nullptr, 0.0, in[0].data(), &len, 1, len, &o, rows[0].data(), &out_len, kept.data(), &ci, cost, nullptr,
                                         nullptr, nullptr);
  if (rc != CCMP_OK) return rc;
  rows.resize((size_t)out_len);
  kept.resize((size_t)out_len);
  return CCMP_OK;
}

int main(int argc, char **argv)
{
  if (argc < 17) return 2;
  try {
    Eigen::VectorXd start(14);
    for (int i = 0; i < 14; i++) start[i] = std::atof(argv[1 + i]);
    const double delta = std::atof(argv[15]);
    std::ifstream in(argv[16]);
    size_t W = 0, N = 0, E = 0;
    Rows waypoints, nodes;
    if (!(in >> W >> N >> E) || !read_rows(in, W, waypoints) || !read_rows(in, N, nodes)) return 2;
    std::vector<int32_t> uv(2 * E);
    for (int32_t &v : uv)
      if (!(in >> v)) return 2;

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
    si_ptr->setStateSpace(space);
    space->setSpaceInformation(si_ptr.get());
    space->setDelta(delta);
    space->setLambda(2.0);

    int mismatches = 0;
    // shortcutPath: every span, and span 2, on the same waypoints; each against the C ABI called directly
    for (int span : {0, 2}) {
      Rows got = waypoints, want;
      std::vector<int32_t> kept(3, 7), kept_want;
      double cost = -1.0;
      const bool r = space->shortcutPath(got, span, &kept);
      const int rc = direct(constraint->impl(), waypoints, span, space->getDelta(), space->getLambda(), want, kept_want, &cost);
      if (!r || rc != CCMP_OK || !same_rows(got, want) || kept != kept_want) mismatches++;
      print_rows(span == 0 ? "every" : "span2", got, kept);
    }
    // one waypoint: itself; none: nothing — answers, not errors
    Rows one(1, waypoints[0]), none;
    std::vector<int32_t> k1(3, 7), k0(3, 7);
    const bool r3 = space->shortcutPath(one, 0, &k1), r4 = space->shortcutPath(none, 0, &k0);
    if (!r3 || !r4 || one.size() != 1 || std::memcmp(one[0].data(), waypoints[0].data(), 14 * sizeof(double)) != 0 || !none.empty() ||
        k1 != std::vector<int32_t>(1, 0) || !k0.empty())
      mismatches++;

    // constructShortcutSolution on the recorded roadmap
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (size_t v = 0; v < N; v++)
      if (!rm.append(nodes[v].data(), nullptr)) mismatches++;
    if (!rm.addEdges(uv.data(), E) || rm.numEdges() != E) mismatches++;
    const std::vector<int32_t> starts = {0, 1}, goals = {9, 6};
    Rows sol, plain, want;
    std::vector<int32_t> idx, idx_plain, kept_want;
    double cost = -1.0, cost_plain = -2.0, cost_want = -3.0;
    const bool found = rm.constructShortcutSolution(starts, goals, sol, 0, &cost, &idx, space->getDelta(), space->getLambda());
    const bool found_plain = rm.constructSolution(starts, goals, plain, &cost_plain, &idx_plain);
    if (!found || !found_plain || !(cost <= cost_plain) || sol.size() > plain.size() || idx.size() != sol.size()) mismatches++;
    if (found_plain) {
      const int rc = direct(constraint->impl(), plain, 0, space->getDelta(), space->getLambda(), want, kept_want, &cost_want);
      if (rc != CCMP_OK || !same_rows(sol, want) || cost != cost_want || idx.size() != kept_want.size()) mismatches++;
      for (size_t k = 0; k < idx.size() && k < kept_want.size(); k++)
        if (idx[k] != idx_plain[(size_t)kept_want[k]]) mismatches++;
    }
    std::printf("solution found %d cost %a plain", (int)found, cost);
    for (int32_t v : idx_plain) std::printf(" %d", v);
    std::printf("\n");
    print_rows("solution", sol, idx);
    // no connected pair: "no", no states, and no error
    Rows nothing(2, waypoints[0]);
    if (rm.constructShortcutSolution({}, {0}, nothing) || !nothing.empty()) mismatches++;
    const int before = rm.lastError(), before_c = constraint->lastError();
    // the sticky error: a path longer than CCMP_SHORTCUT_MAX_LEN comes back unchanged, false, with the error kept
    Rows longp((size_t)CCMP_SHORTCUT_MAX_LEN + 1, waypoints[0]);
    const bool t1 = space->shortcutPath(longp);
    if (longp.size() != (size_t)CCMP_SHORTCUT_MAX_LEN + 1) mismatches++;
    std::printf("summary mismatches %d before %d %d long %d %d\n", mismatches, before, before_c, (int)t1, constraint->lastError());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
