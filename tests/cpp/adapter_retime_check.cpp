// The adapter's resampled and time-stamped paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::resamplePath / timePath,
// ccmp::Roadmap::constructTimedSolution, ccmp::printTrajectory) against the interface mock in tests/cpp/mock_ompl.  The program reads
// waypoints, roadmap nodes and undirected edges from a text file, resamples the waypoints by count and by spacing, stamps the rows, runs
// constructTimedSolution on the roadmap and prints rows and times as hex floats (tests/test_cpp_adapter_retime.py compares them with the
// mirror's host form).  Then printTrajectory against printAsMatrix, and the answers that are "unchanged path" / "times untouched" /
// "the smooth solution without times" with the sticky error set; nothing throws.
// usage: adapter_retime_check <start_joint 14 values...> <delta> <input file>
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

// the robot's data sheet, both arms (the reference holds no limits)
static const double kVmax[14] = {2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61, 2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61};
static const double kAmax[14] = {15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0, 15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0};

static void print_rows(const char *tag, const Rows &rows, const std::vector<double> &times)
{
  std::printf("%s rows %zu times %zu\n", tag, rows.size(), times.size());
  for (size_t r = 0; r < rows.size(); r++) {
    std::printf("%s row %zu", tag, r);
    for (double v : rows[r]) std::printf(" %a", v);
    std::printf("\n");
  }
  std::printf("%s time", tag);
  for (double t : times) std::printf(" %a", t);
  std::printf("\n");
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

// printTrajectory's lines are printAsMatrix's with one more column
static bool trajectory_extends_matrix(const Rows &rows, const std::vector<double> &times)
{
  std::ostringstream a, b;
  ccmp::printAsMatrix(a, rows.empty() ? nullptr : rows[0].data(), rows.size());
  ccmp::printTrajectory(b, rows.empty() ? nullptr : rows[0].data(), times.data(), rows.size());
  std::istringstream la(a.str()), lb(b.str());
  std::string x, y;
  size_t lines = 0;
  while (std::getline(la, x)) {
    if (!std::getline(lb, y)) return false;
    if (y.compare(0, x.size(), x) != 0) return false; // the first 14 columns, character for character
    if (!x.empty()) {
      std::istringstream rest(y.substr(x.size()));
      double t = -1.0;
      std::string more;
      if (!(rest >> t) || (rest >> more)) return false; // exactly one more column
      std::ostringstream again;
      again << times[lines];
      if (std::strtod(again.str().c_str(), nullptr) != t) return false;
      lines++;
    } else if (!y.empty()) {
      return false;
    }
  }
  return lines == rows.size() && !std::getline(lb, y);
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
    // resamplePath by count and by spacing, timePath on the rows
    Rows by_count = waypoints, by_spacing = waypoints;
    std::vector<uint8_t> kinds;
    std::vector<double> t_count, t_spacing;
    double duration = -1.0;
    if (!space->resamplePath(by_count, 17, 0.0, &kinds) || by_count.size() != 17 || kinds.size() != 17 || kinds.front() != CCMP_SAMPLE_COPIED ||
        kinds.back() != CCMP_SAMPLE_COPIED)
      mismatches++;
    if (!space->resamplePath(by_spacing, 0, 0.125)) mismatches++;
    if (!space->timePath(by_count, kVmax, kAmax, &t_count, 0.5, &duration) || t_count.size() != by_count.size() || t_count.front() != 0.0 ||
        duration != t_count.back())
      mismatches++;
    if (!space->timePath(by_spacing, kVmax, kAmax, &t_spacing, 0.2)) mismatches++;
    print_rows("count", by_count, t_count);
    print_rows("spacing", by_spacing, t_spacing);
    if (!trajectory_extends_matrix(by_count, t_count)) mismatches++;
    // no waypoints: an answer, not an error
    Rows none;
    std::vector<double> t_none(3, 7.0);
    if (!space->resamplePath(none) || !none.empty() || !space->timePath(none, kVmax, kAmax, &t_none) || !t_none.empty()) mismatches++;

    // constructTimedSolution on the recorded roadmap: the smooth solution of two passes, resampled at the space's delta, stamped
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (size_t v = 0; v < N; v++)
      if (!rm.append(nodes[v].data(), nullptr)) mismatches++;
    if (!rm.addEdges(uv.data(), E) || rm.numEdges() != E) mismatches++;
    const std::vector<int32_t> starts = {0, 1}, goals = {9, 6};
    Rows sol, smooth;
    std::vector<double> t_sol;
    std::vector<int32_t> idx, idx_smooth;
    double cost = -1.0, cost_smooth = -2.0;
    const bool found = rm.constructTimedSolution(starts, goals, sol, t_sol, kVmax, kAmax, 0.5, 0, 0.0, 2, 0.005, 0, &cost, &idx, space->getDelta(), space->getLambda());
    const bool found_sm = rm.constructSmoothSolution(starts, goals, smooth, 2, 0.005, 0, &cost_smooth, &idx_smooth, space->getDelta(), space->getLambda());
    if (!found || !found_sm || idx != idx_smooth || t_sol.size() != sol.size() || t_sol.empty() || cost != t_sol.back()) mismatches++;
    print_rows("smooth", smooth, std::vector<double>());
    print_rows("solution", sol, t_sol);
    const int before = rm.lastError(), before_c = constraint->lastError();
    // the sticky error: the library refuses count == 1 — the path comes back unchanged, false, with the error kept; a limit of zero leaves
    // `times` untouched; on the roadmap the answer is the smooth solution without times, true, with the error kept
    Rows bad = waypoints;
    const bool t1 = space->resamplePath(bad, 1);
    if (!same_rows(bad, waypoints)) mismatches++;
    double vbad[14];
    std::memcpy(vbad, kVmax, sizeof vbad);
    vbad[3] = 0.0;
    std::vector<double> t_bad(2, 7.0);
    const bool t2 = space->timePath(by_count, vbad, kAmax, &t_bad);
    if (t_bad.size() != 2 || t_bad[0] != 7.0 || t_bad[1] != 7.0) mismatches++;
    Rows sol_bad;
    std::vector<double> t_sol_bad(1, 7.0);
    double cost_bad = -1.0;
    const bool t3 = rm.constructTimedSolution(starts, goals, sol_bad, t_sol_bad, kVmax, kAmax, 0.5, 1, 0.0, 2, 0.005, 0, &cost_bad, nullptr, space->getDelta(),
                                              space->getLambda());
    if (!same_rows(sol_bad, smooth) || !t_sol_bad.empty() || cost_bad != cost_smooth) mismatches++;
    std::printf("summary mismatches %d before %d %d bad %d %d %d roadmap %d %d\n", mismatches, before, before_c, (int)t1, (int)t2, constraint->lastError(), (int)t3,
                rm.lastError());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
