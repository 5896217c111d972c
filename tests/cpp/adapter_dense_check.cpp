// The adapter's dense solution paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::interpolatePath,
// ccmp::Roadmap::constructDenseSolution) against the interface mock in tests/cpp/mock_ompl.  The program reads waypoints, roadmap nodes and
// undirected edges from a text file, runs interpolatePath on the waypoints in both layouts and constructDenseSolution on the roadmap, and
// prints every row as hex floats; tests/test_cpp_adapter_dense.py compares them bit for bit with the oracle's segments joined by the rule.
// Then the answers that are "no" without being errors, and the sticky error of a deliberate bad call; nothing throws.
// usage: adapter_dense_check <start_joint 14 values...> <delta> <input file>
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

static void print_rows(const char *tag, const Rows &rows, const std::vector<uint8_t> &ok)
{
  std::printf("%s rows %zu ok", tag, rows.size());
  for (uint8_t v : ok) std::printf(" %d", (int)v);
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
    // interpolatePath: both layouts on the same waypoints
    std::vector<uint8_t> ok_ref, ok_dis;
    Rows ref = waypoints, dis = waypoints;
    const bool r1 = space->interpolatePath(ref, false, &ok_ref), r2 = space->interpolatePath(dis, true, &ok_dis);
    if (!r1 || !r2 || ok_ref != ok_dis) mismatches++;
    print_rows("reference", ref, ok_ref);
    print_rows("distinct", dis, ok_dis);
    {
      std::ostringstream text; // ccmp::printAsMatrix over the result is the reference's <obj>_path.txt: one line per row, one empty line
      ccmp::printAsMatrix(text, ref.empty() ? nullptr : ref[0].data(), ref.size());
      const std::string s = text.str();
      std::printf("matrix lines %zu\n", (size_t)std::count(s.begin(), s.end(), '\n'));
    }
    // one waypoint: itself; none: nothing — answers, not errors
    Rows one(1, waypoints[0]), none;
    std::vector<uint8_t> ok1(3, 7), ok0(3, 7);
    const bool r3 = space->interpolatePath(one, false, &ok1), r4 = space->interpolatePath(none, false, &ok0);
    if (!r3 || !r4 || one.size() != 1 || std::memcmp(one[0].data(), waypoints[0].data(), 14 * sizeof(double)) != 0 || !none.empty() || !ok1.empty() || !ok0.empty())
      mismatches++;

    // constructDenseSolution on the recorded roadmap
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (size_t v = 0; v < N; v++)
      if (!rm.append(nodes[v].data(), nullptr)) mismatches++;
    if (!rm.addEdges(uv.data(), E) || rm.numEdges() != E) mismatches++;
    const std::vector<int32_t> starts = {0, 1}, goals = {9, 6};
    Rows sol, plain;
    std::vector<int32_t> idx, idx_plain;
    std::vector<uint8_t> ok_sol;
    double cost = -1.0, cost_plain = -2.0;
    const bool found = rm.constructDenseSolution(starts, goals, sol, false, &cost, &idx, &ok_sol, space->getDelta(), space->getLambda());
    const bool found_plain = rm.constructSolution(starts, goals, plain, &cost_plain, &idx_plain);
    if (!found || !found_plain || cost != cost_plain || idx != idx_plain || ok_sol.size() + 1 != idx.size()) mismatches++;
    std::printf("solution found %d cost %a path", (int)found, cost);
    for (int32_t v : idx) std::printf(" %d", v);
    std::printf("\n");
    print_rows("solution", sol, ok_sol);
    // no connected pair: "no", no states, and no error
    Rows nothing(2, waypoints[0]);
    if (rm.constructDenseSolution({}, {0}, nothing) || !nothing.empty()) mismatches++;
    const int before = rm.lastError(), before_c = constraint->lastError();
    // the sticky error: a start that is not a vertex is ignored by constructSolution ("no"); a roadmap whose store is gone is an error
    ccmp::Roadmap empty(constraint->impl(), 4);
    Rows e;
    const bool t1 = empty.constructDenseSolution({0}, {0}, e);
    std::printf("summary mismatches %d before %d %d empty %d %d\n", mismatches, before, before_c, (int)t1, empty.lastError());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
