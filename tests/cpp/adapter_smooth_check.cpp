// The adapter's smooth solution paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::smoothPath,
// ccmp::Roadmap::constructSmoothSolution) against the interface mock in tests/cpp/mock_ompl.  The program reads waypoints, roadmap nodes
// and undirected edges from a text file, runs smoothPath on the waypoints and constructSmoothSolution on the roadmap, prints the rows as
// hex floats (tests/test_cpp_adapter_smooth.py compares them with the mirror's host form) and compares each with ccmp_path_smooth_host
// called directly under another cut.  Then the answers that are "unchanged path" with the sticky error set; nothing throws.
// usage: adapter_smooth_check <start_joint 14 values...> <delta> <input file>
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

static void print_rows(const char *tag, const Rows &rows, int passes, int moved)
{
  std::printf("%s rows %zu passes %d moved %d\n", tag, rows.size(), passes, moved);
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

// the C ABI called directly on the same waypoints, under another cut than the adapter's: the result does not depend on it
static int direct(const ccmp::Projector &proj, const Rows &in, int max_steps, double min_change, double delta, double lambda, Rows &rows, int32_t *passes,
                  int32_t *moved, double *length_out)
{
  ccmp_problem P = proj.problem();
  P.delta = delta;
  P.lambda = lambda;
  ccmp_smooth_opts o;
  ccmp_smooth_opts_default(&o);
  o.max_steps = max_steps;
  o.min_change = min_change;
  o.chunk_states = 3;
  o.tile_edges = 2;
  const int32_t len = (int32_t)in.size();
  const int cap = ccmp_smooth_len_after(len, max_steps);
  int32_t out_len = 0, stop = 0;
  double li = 0.0;
  rows.assign((size_t)cap, std::array<double, 14>());
  std::lock_guard<std::mutex> hold(proj.mutex());
  const int rc = ccmp_path_smooth_host(proj.ctx(), &P, nullptr, 0.0, in[0].data(), &len, 1, len, &o, cap, rows[0].data(), &out_len, passes, moved, &stop, &li,
                                       length_out, nullptr);
  if (rc != CCMP_OK) return rc;
  rows.resize((size_t)out_len);
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
    // smoothPath: three passes and the default five on the same waypoints; each against the C ABI called directly
    for (int steps : {3, 5}) {
      Rows got = waypoints, want;
      int passes = -1, moved = -1;
      int32_t passes_want = -2, moved_want = -2;
      double lo = 0.0;
      const bool r = steps == 5 ? space->smoothPath(got) : space->smoothPath(got, steps, 0.005, &passes, &moved);
      const int rc = direct(constraint->impl(), waypoints, steps, 0.005, space->getDelta(), space->getLambda(), want, &passes_want, &moved_want, &lo);
      if (!r || rc != CCMP_OK || !same_rows(got, want) || (steps == 3 && (passes != passes_want || moved != moved_want))) mismatches++;
      print_rows(steps == 3 ? "three" : "five", got, steps == 3 ? passes : (int)passes_want, steps == 3 ? moved : (int)moved_want);
    }
    // two waypoints, one, none: themselves — answers, not errors
    Rows two(waypoints.begin(), waypoints.begin() + 2), one(1, waypoints[0]), none;
    const Rows two_in = two;
    const bool r2 = space->smoothPath(two), r3 = space->smoothPath(one), r4 = space->smoothPath(none);
    if (!r2 || !r3 || !r4 || !same_rows(two, two_in) || one.size() != 1 || std::memcmp(one[0].data(), waypoints[0].data(), 14 * sizeof(double)) != 0 ||
        !none.empty())
      mismatches++;

    // constructSmoothSolution on the recorded roadmap: the shortcut solution, then two passes
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (size_t v = 0; v < N; v++)
      if (!rm.append(nodes[v].data(), nullptr)) mismatches++;
    if (!rm.addEdges(uv.data(), E) || rm.numEdges() != E) mismatches++;
    const std::vector<int32_t> starts = {0, 1}, goals = {9, 6};
    Rows sol, shortcut, want;
    std::vector<int32_t> idx, idx_shortcut;
    double cost = -1.0, cost_shortcut = -2.0, lo = -3.0;
    int32_t p_want = 0, m_want = 0;
    const bool found = rm.constructSmoothSolution(starts, goals, sol, 2, 0.005, 0, &cost, &idx, space->getDelta(), space->getLambda());
    const bool found_sc = rm.constructShortcutSolution(starts, goals, shortcut, 0, &cost_shortcut, &idx_shortcut, space->getDelta(), space->getLambda());
    if (!found || !found_sc || idx != idx_shortcut) mismatches++;
    if (found_sc) {
      const int rc = direct(constraint->impl(), shortcut, 2, 0.005, space->getDelta(), space->getLambda(), want, &p_want, &m_want, &lo);
      if (rc != CCMP_OK || !same_rows(sol, want) || cost != lo) mismatches++;
    }
    std::printf("solution found %d cost %a shortcut", (int)found, cost);
    for (int32_t v : idx_shortcut) std::printf(" %d", v);
    std::printf("\n");
    print_rows("solution", sol, (int)p_want, (int)m_want);
    const int before = rm.lastError(), before_c = constraint->lastError();
    // the sticky error: the library refuses a negative number of passes — the path comes back unchanged, false, with the error kept;
    // on the roadmap the answer is the unchanged shortcut solution, true, with the error kept
    Rows bad = waypoints;
    const bool t1 = space->smoothPath(bad, -1);
    if (!same_rows(bad, waypoints)) mismatches++;
    Rows sol_bad;
    const bool t2 = rm.constructSmoothSolution(starts, goals, sol_bad, -1, 0.005, 0, nullptr, nullptr, space->getDelta(), space->getLambda());
    if (!same_rows(sol_bad, shortcut)) mismatches++;
    std::printf("summary mismatches %d before %d %d bad %d %d roadmap %d %d\n", mismatches, before, before_c, (int)t1, constraint->lastError(), (int)t2,
                rm.lastError());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
