// The adapter's setpoints and execution audit (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::setpointPath,
// ccmp::Roadmap::constructExecutableSolution, ccmp::printSetpoints) against the interface mock in tests/cpp/mock_ompl.  The program reads a
// timed path (rows and stamps), roadmap nodes and undirected edges from a text file, takes the path's setpoints at the given period, runs
// constructExecutableSolution on the roadmap and prints ticks and audits as hex floats (tests/test_cpp_adapter_setpoints.py compares them
// with the mirror's host form).  Then printSetpoints' shape, and the answers that are "*out untouched" / "the timed solution without
// setpoints" with the sticky error set, and a path out of order, which is an answer and not an error; nothing throws.
// usage: adapter_setpoints_check <start_joint 14 values...> <delta> <period> <input file>
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

// one line per tick: tau, q, qd, f, clearance, satisfied; then the audit
static void print_setpoints(const char *tag, const ccmp::Setpoints &s)
{
  std::printf("%s ticks %zu status %d\n", tag, s.tau.size(), (int)s.status);
  for (size_t j = 0; j < s.tau.size(); j++) {
    std::printf("%s tick %zu %a", tag, j, s.tau[j]);
    for (double v : s.q[j]) std::printf(" %a", v);
    for (double v : s.qd[j]) std::printf(" %a", v);
    std::printf(" %a %a %a %d\n", s.f[j][0], s.f[j][1], s.clearance[j], (int)s.satisfied[j]);
  }
  std::printf("%s audit", tag);
  for (double v : s.peak) std::printf(" %a", v);
  std::printf(" %a", s.stretch);
  for (int32_t v : s.peak_tick) std::printf(" %d", (int)v);
  std::printf(" %d %d\n", (int)s.n_off, (int)s.n_below);
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

static bool read_values(std::istream &in, size_t n, std::vector<double> &out)
{
  out.resize(n);
  for (double &v : out) {
    std::string tok;
    if (!(in >> tok)) return false;
    v = std::strtod(tok.c_str(), nullptr);
  }
  return true;
}

// printSetpoints: one line of 1 + 14 + 14 columns per tick, the first of which reads back as tau, and the empty line after the last
static bool setpoints_print_shape(const ccmp::Setpoints &s)
{
  std::ostringstream a;
  ccmp::printSetpoints(a, s);
  std::istringstream la(a.str());
  std::string x;
  size_t lines = 0;
  bool blank = false;
  while (std::getline(la, x)) {
    if (x.empty()) {
      if (blank) return false;
      blank = true;
      continue;
    }
    if (blank) return false;
    std::istringstream cols(x);
    double v = 0.0, first = 0.0;
    size_t n = 0;
    while (cols >> v) {
      if (n == 0) first = v;
      n++;
    }
    std::ostringstream again;
    again << s.tau[lines];
    if (n != 29 || std::strtod(again.str().c_str(), nullptr) != first) return false;
    lines++;
  }
  return blank && lines == s.tau.size();
}

int main(int argc, char **argv)
{
  if (argc < 18) return 2;
  try {
    Eigen::VectorXd start(14);
    for (int i = 0; i < 14; i++) start[i] = std::atof(argv[1 + i]);
    const double delta = std::atof(argv[15]), period = std::atof(argv[16]);
    std::ifstream in(argv[17]);
    size_t W = 0, N = 0, E = 0;
    Rows path, nodes;
    std::vector<double> stamps;
    if (!(in >> W >> N >> E) || !read_rows(in, W, path) || !read_values(in, W, stamps) || !read_rows(in, N, nodes)) return 2;
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
    // setpointPath on the timed path
    ccmp::Setpoints sp;
    if (!space->setpointPath(path, stamps, kVmax, kAmax, &sp, period) || sp.status != CCMP_SETPOINTS_OK || sp.tau.size() < 2 || sp.q.size() != sp.tau.size() ||
        sp.qd.size() != sp.tau.size() || sp.f.size() != sp.tau.size() || sp.satisfied.size() != sp.tau.size() || sp.tau.front() != 0.0 ||
        sp.tau.back() != stamps.back() || sp.peak_tick[4] != -1 || !(sp.stretch >= 1.0))
      mismatches++;
    print_setpoints("path", sp);
    if (!setpoints_print_shape(sp)) mismatches++;
    // a path out of order is an answer, not an error: its status and no tick
    std::vector<double> reversed(stamps.rbegin(), stamps.rend());
    ccmp::Setpoints un;
    if (!space->setpointPath(path, reversed, kVmax, kAmax, &un, period) || un.status != CCMP_SETPOINTS_UNORDERED || !un.tau.empty() || un.peak_tick[0] != -1) mismatches++;
    // no rows: EMPTY
    ccmp::Setpoints none;
    if (!space->setpointPath(Rows(), std::vector<double>(), kVmax, kAmax, &none, period) || none.status != CCMP_SETPOINTS_EMPTY || !none.tau.empty()) mismatches++;

    // constructExecutableSolution on the recorded roadmap: the timed solution of two smoothing passes, then its setpoints
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (size_t v = 0; v < N; v++)
      if (!rm.append(nodes[v].data(), nullptr)) mismatches++;
    if (!rm.addEdges(uv.data(), E) || rm.numEdges() != E) mismatches++;
    const std::vector<int32_t> starts = {0, 1}, goals = {9, 6};
    Rows sol, timed;
    std::vector<double> t_sol, t_timed;
    ccmp::Setpoints sp_sol;
    double cost = -1.0;
    const bool found = rm.constructExecutableSolution(starts, goals, sol, t_sol, sp_sol, kVmax, kAmax, period, 65536, nullptr, 0.0, 0.5, 0, 0.0, 2, 0.005, 0, &cost,
                                                      nullptr, space->getDelta(), space->getLambda());
    const bool found_t = rm.constructTimedSolution(starts, goals, timed, t_timed, kVmax, kAmax, 0.5, 0, 0.0, 2, 0.005, 0, nullptr, nullptr, space->getDelta(),
                                                   space->getLambda());
    if (!found || !found_t || sol.size() != timed.size() || t_sol != t_timed || t_sol.empty() || sp_sol.status != CCMP_SETPOINTS_OK || sp_sol.tau.empty() ||
        sp_sol.tau.back() != t_sol.back() || cost != t_sol.back())
      mismatches++;
    print_rows("solution", sol, t_sol);
    print_setpoints("executable", sp_sol);
    const int before = rm.lastError(), before_c = constraint->lastError();
    // the sticky error: the library refuses a period of zero — *out stays as it was, false, the error kept; on the roadmap the answer is the
    // timed solution without setpoints, true, with the error kept
    ccmp::Setpoints kept = sp;
    const bool t1 = space->setpointPath(path, stamps, kVmax, kAmax, &kept, 0.0);
    if (kept.tau != sp.tau || kept.status != sp.status) mismatches++;
    Rows sol_bad;
    std::vector<double> t_sol_bad;
    ccmp::Setpoints sp_bad = sp;
    const bool t2 = rm.constructExecutableSolution(starts, goals, sol_bad, t_sol_bad, sp_bad, kVmax, kAmax, 0.0, 65536, nullptr, 0.0, 0.5, 0, 0.0, 2, 0.005, 0, nullptr,
                                                   nullptr, space->getDelta(), space->getLambda());
    if (sol_bad.size() != sol.size() || t_sol_bad != t_sol || !sp_bad.tau.empty() || sp_bad.status != CCMP_SETPOINTS_EMPTY) mismatches++;
    std::printf("summary mismatches %d before %d %d bad %d %d roadmap %d %d\n", mismatches, before, before_c, (int)t1, constraint->lastError(), (int)t2, rm.lastError());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
