// The adapter's fitted time stamps (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::fitPath and the overload of
// ccmp::Roadmap::constructExecutableSolution that takes fit options) against the interface mock in tests/cpp/mock_ompl.  The program reads
// a timed path (rows and stamps), roadmap nodes and undirected edges from a text file, fits the path's stamps at the given period, runs both
// constructTimedSolution and the fitting constructExecutableSolution on the roadmap and prints stamps, factors and answers as hex floats
// (tests/test_cpp_adapter_fit.py compares them with the mirror's host form).  Then the answers that are "*out untouched" / "the time-stamp
// rule's stamps and their setpoints" with the sticky error set, and a path out of order, which is an answer and not an error; nothing throws.
// usage: adapter_fit_check <start_joint 14 values...> <delta> <period> <input file>
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

static void print_fit(const char *tag, const ccmp::FittedTimes &f)
{
  std::printf("%s fit %d %d %a %a %a\n", tag, (int)f.status, (int)f.passes, f.peak[0], f.peak[1], f.duration);
  std::printf("%s fitted", tag);
  for (double t : f.times) std::printf(" %a", t);
  std::printf("\n%s factor", tag);
  for (double t : f.factor) std::printf(" %a", t);
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
    ccmp::FitOptions opts;
    opts.period = period;
    // fitPath on the timed path: FITTED, the stamps dilated and ordered, the peaks within the limits
    ccmp::FittedTimes fit;
    if (!space->fitPath(path, stamps, kVmax, kAmax, &fit, opts) || fit.status != CCMP_FIT_FITTED || fit.passes < 1 || fit.times.size() != stamps.size() ||
        fit.factor.size() != stamps.size() || fit.times.front() != 0.0 || fit.times.back() != fit.duration || !(fit.duration > stamps.back()) ||
        !(fit.peak[0] <= 1.0) || !(fit.peak[1] <= 1.0) || !std::is_sorted(fit.times.begin(), fit.times.end()))
      mismatches++;
    print_fit("path", fit);
    // the audit of the fitted stamps reports the fit's peaks; fitted again they come back bit for bit without a dilation
    ccmp::Setpoints sp;
    if (!space->setpointPath(path, fit.times, kVmax, kAmax, &sp, period) || sp.status != CCMP_SETPOINTS_OK || sp.peak[0] != fit.peak[0] || sp.peak[1] != fit.peak[1] ||
        sp.stretch != 1.0)
      mismatches++;
    ccmp::FittedTimes again;
    if (!space->fitPath(path, fit.times, kVmax, kAmax, &again, opts) || again.status != CCMP_FIT_FITTED || again.passes != 0 || again.times != fit.times) mismatches++;
    // no dilation allowed: PASSES is a status, not an error, and the stamps are the input's
    ccmp::FitOptions none_allowed = opts;
    none_allowed.max_passes = 0;
    ccmp::FittedTimes spent;
    if (!space->fitPath(path, stamps, kVmax, kAmax, &spent, none_allowed) || spent.status != CCMP_FIT_PASSES || spent.passes != 0 || spent.times != stamps) mismatches++;
    // a path out of order is an answer, not an error: its status and its stamps
    std::vector<double> reversed(stamps.rbegin(), stamps.rend());
    ccmp::FittedTimes un;
    if (!space->fitPath(path, reversed, kVmax, kAmax, &un, opts) || un.status != CCMP_SETPOINTS_UNORDERED || un.times != reversed || un.passes != 0) mismatches++;
    // no rows: EMPTY
    ccmp::FittedTimes none;
    if (!space->fitPath(Rows(), std::vector<double>(), kVmax, kAmax, &none, opts) || none.status != CCMP_SETPOINTS_EMPTY || !none.times.empty()) mismatches++;

    // the recorded roadmap: the timed solution of two smoothing passes, and the same with the fit before its setpoints
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (size_t v = 0; v < N; v++)
      if (!rm.append(nodes[v].data(), nullptr)) mismatches++;
    if (!rm.addEdges(uv.data(), E) || rm.numEdges() != E) mismatches++;
    const std::vector<int32_t> starts = {0, 1}, goals = {9, 6};
    Rows sol, timed;
    std::vector<double> t_sol, t_timed;
    ccmp::Setpoints sp_sol;
    ccmp::FittedTimes fit_sol;
    double cost = -1.0;
    const bool found_t = rm.constructTimedSolution(starts, goals, timed, t_timed, kVmax, kAmax, 0.5, 0, 0.0, 2, 0.005, 0, nullptr, nullptr, space->getDelta(),
                                                   space->getLambda());
    const bool found = rm.constructExecutableSolution(starts, goals, sol, t_sol, sp_sol, fit_sol, opts, kVmax, kAmax, nullptr, 0.0, 0.5, 0, 0.0, 2, 0.005, 0, &cost,
                                                      nullptr, space->getDelta(), space->getLambda());
    if (!found || !found_t || sol != timed || t_sol.size() != t_timed.size() || t_sol != fit_sol.times || fit_sol.status != CCMP_FIT_FITTED ||
        sp_sol.status != CCMP_SETPOINTS_OK || sp_sol.tau.empty() || sp_sol.tau.back() != t_sol.back() || cost != fit_sol.duration ||
        sp_sol.peak[0] != fit_sol.peak[0] || sp_sol.peak[1] != fit_sol.peak[1])
      mismatches++;
    print_rows("timed", timed, t_timed);
    print_fit("executable", fit_sol);
    std::printf("executable audit %zu %a %a %a\n", sp_sol.tau.size(), sp_sol.peak[0], sp_sol.peak[1], sp_sol.stretch);
    const int before = rm.lastError(), before_c = constraint->lastError();
    // the sticky error: the library refuses aim = 0 — *out stays as it was, false, the error kept; on the roadmap the answer is the
    // time-stamp rule's stamps with their setpoints, true, with the error kept
    ccmp::FitOptions bad = opts;
    bad.aim = 0.0;
    ccmp::FittedTimes kept = fit;
    const bool t1 = space->fitPath(path, stamps, kVmax, kAmax, &kept, bad);
    if (kept.times != fit.times || kept.status != fit.status || kept.passes != fit.passes) mismatches++;
    Rows sol_bad;
    std::vector<double> t_sol_bad;
    ccmp::Setpoints sp_bad;
    ccmp::FittedTimes fit_bad = fit;
    const bool t2 = rm.constructExecutableSolution(starts, goals, sol_bad, t_sol_bad, sp_bad, fit_bad, bad, kVmax, kAmax, nullptr, 0.0, 0.5, 0, 0.0, 2, 0.005, 0, nullptr,
                                                   nullptr, space->getDelta(), space->getLambda());
    if (sol_bad != timed || t_sol_bad != t_timed || !fit_bad.times.empty() || fit_bad.status != CCMP_SETPOINTS_EMPTY || sp_bad.status != CCMP_SETPOINTS_OK ||
        sp_bad.tau.empty() || sp_bad.tau.back() != t_timed.back())
      mismatches++;
    std::printf("summary mismatches %d before %d %d bad %d %d roadmap %d %d\n", mismatches, before, before_c, (int)t1, constraint->lastError(), (int)t2, rm.lastError());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
