// The adapter's jerk-bounded setpoints (include/ccmp_ompl_adapter.hpp: ccmp::jerkSetpointPath, jy_ProjectedStateSpace::jerkSetpointPath, the
// overload of ccmp::Roadmap::constructExecutableSolution that takes jmax and JerkOptions, printSetpoints for ccmp::JerkSetpoints) against the
// interface mock in tests/cpp/mock_ompl.  The program reads a timed path (rows and stamps), roadmap nodes and undirected edges from a text
// file, takes the path's jerk-bounded setpoints at the given period, runs constructTimedSolution and the new overload (without and with the
// fit) on the roadmap and prints ticks and answers as hex floats (tests/test_cpp_adapter_jerk.py compares them with the mirror's host
// form).  Then the answers that are "*out untouched" / "the timed solution with empty setpoints" with the sticky error set, and a path out
// of order, which is an answer and not an error; nothing throws.
// usage: adapter_jerk_check <start_joint 14 values...> <delta> <period> <input file>
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
static const double kJmax[14] = {7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0, 7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0};

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

// the answer and every tick: tau, q, qd, f, clearance as hex floats
static void print_jerk(const char *tag, const ccmp::JerkSetpoints &s)
{
  std::printf("%s jerk %d %d %d %zu %d %d", tag, (int)s.status, (int)s.window, (int)s.passes, s.tau.size(), (int)s.n_off, (int)s.n_below);
  for (int k = 0; k < 6; k++) std::printf(" %a", s.peak[k]);
  for (int k = 0; k < 6; k++) std::printf(" %d", (int)s.peak_tick[k]);
  std::printf("\n");
  for (size_t j = 0; j < s.tau.size(); j++) {
    std::printf("%s tick %zu %a", tag, j, s.tau[j]);
    for (double v : s.q[j]) std::printf(" %a", v);
    for (double v : s.qd[j]) std::printf(" %a", v);
    std::printf(" %a %a %d\n", s.f[j][0], s.f[j][1], (int)s.satisfied[j]);
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

static bool same_ticks(const ccmp::JerkSetpoints &a, const ccmp::JerkSetpoints &b)
{
  return a.q == b.q && a.qd == b.qd && a.tau == b.tau && a.status == b.status && a.window == b.window && a.passes == b.passes &&
         std::memcmp(a.peak, b.peak, 3 * sizeof(double)) == 0; // (the clearance peak of a call without a scene is +inf on both sides; the NaN clearances are not compared)
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
    ccmp::JerkOptions opts;
    opts.period = period;
    // jerkSetpointPath on the timed path: OK with a window the search grew, both ends copies at rest, the jerk ratio within 1
    ccmp::JerkSetpoints js;
    if (!space->jerkSetpointPath(path, stamps, kVmax, kAmax, kJmax, &js, opts) || js.status != CCMP_JERK_OK || js.window < 2 || js.passes < 1 || js.tau.empty() ||
        js.q.size() != js.tau.size() || js.qd.size() != js.tau.size() || js.f.size() != js.tau.size() || js.satisfied.size() != js.tau.size() ||
        js.q.front() != path.front() || js.q.back() != path.back() || js.tau.front() != 0.0 || !(js.peak[2] <= 1.0) || !(js.peak[2] > 0.0) || js.peak_tick[2] < 1)
      mismatches++;
    print_jerk("path", js);
    // against the plain setpoints: the window adds W - 1 ticks and neither peak rises beyond a rounding (the margin is derived in
    // tests/test_jerk_ref.py; here: a part in 1e9)
    ccmp::Setpoints sp;
    if (!space->setpointPath(path, stamps, kVmax, kAmax, &sp, period) || sp.status != CCMP_SETPOINTS_OK || js.tau.size() != sp.tau.size() + (size_t)js.window - 1 ||
        !(js.peak[0] <= sp.peak[0] * (1.0 + 1e-9)) || !(js.peak[1] <= sp.peak[1] * (1.0 + 1e-9)))
      mismatches++;
    // the free function under the caller's lock gives the same answer; window 1 is the setpoints rule on the grid
    ccmp::JerkSetpoints free_form, one;
    {
      const ccmp::Projector &proj = constraint->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      if (ccmp::jerkSetpointPath(proj, path, stamps, kVmax, kAmax, kJmax, &free_form, opts) != CCMP_OK || !same_ticks(free_form, js)) mismatches++;
    }
    ccmp::JerkOptions fixed = opts;
    fixed.window = 1;
    if (!space->jerkSetpointPath(path, stamps, kVmax, kAmax, kJmax, &one, fixed) || one.status != CCMP_JERK_WINDOW || one.window != 1 || one.passes != 0 ||
        one.q != sp.q || one.qd != sp.qd || !(one.peak[2] > 1.0))
      mismatches++;
    // printSetpoints for the new struct: one line per tick and the empty line
    std::ostringstream text;
    printSetpoints(text, js);
    const std::string printed = text.str();
    if ((size_t)std::count(printed.begin(), printed.end(), '\n') != js.tau.size() + 1) mismatches++;
    // a path out of order is an answer, not an error: its status and no tick; no rows: EMPTY
    std::vector<double> reversed(stamps.rbegin(), stamps.rend());
    ccmp::JerkSetpoints un, none;
    if (!space->jerkSetpointPath(path, reversed, kVmax, kAmax, kJmax, &un, opts) || un.status != CCMP_JERK_UNORDERED || !un.tau.empty() || un.window != 0) mismatches++;
    if (!space->jerkSetpointPath(Rows(), std::vector<double>(), kVmax, kAmax, kJmax, &none, opts) || none.status != CCMP_JERK_EMPTY || !none.tau.empty()) mismatches++;

    // the recorded roadmap: the timed solution of two smoothing passes, its jerk-bounded setpoints, and the same behind the fit
    ccmp::Roadmap rm(constraint->impl(), 4);
    for (size_t v = 0; v < N; v++)
      if (!rm.append(nodes[v].data(), nullptr)) mismatches++;
    if (!rm.addEdges(uv.data(), E) || rm.numEdges() != E) mismatches++;
    const std::vector<int32_t> starts = {0, 1}, goals = {9, 6};
    Rows sol, sol_fit, timed;
    std::vector<double> t_sol, t_fit, t_timed;
    ccmp::JerkSetpoints js_sol, js_fit;
    ccmp::FittedTimes fit_sol;
    ccmp::FitOptions fit_opts;
    fit_opts.period = period;
    double cost = -1.0;
    const bool found_t = rm.constructTimedSolution(starts, goals, timed, t_timed, kVmax, kAmax, 0.5, 0, 0.0, 2, 0.005, 0, nullptr, nullptr, space->getDelta(),
                                                   space->getLambda());
    const bool found = rm.constructExecutableSolution(starts, goals, sol, t_sol, js_sol, kVmax, kAmax, kJmax, opts, nullptr, nullptr, nullptr, 0.0, 0.5, 0, 0.0, 2,
                                                      0.005, 0, nullptr, nullptr, space->getDelta(), space->getLambda());
    const bool found_f = rm.constructExecutableSolution(starts, goals, sol_fit, t_fit, js_fit, kVmax, kAmax, kJmax, opts, &fit_opts, &fit_sol, nullptr, 0.0, 0.5, 0,
                                                        0.0, 2, 0.005, 0, &cost, nullptr, space->getDelta(), space->getLambda());
    if (!found || !found_t || sol != timed || t_sol != t_timed || js_sol.status != CCMP_JERK_OK || js_sol.tau.empty() || !(js_sol.peak[2] <= 1.0)) mismatches++;
    if (!found_f || sol_fit != timed || fit_sol.status != CCMP_FIT_FITTED || t_fit != fit_sol.times || cost != fit_sol.duration || js_fit.status != CCMP_JERK_OK ||
        !(js_fit.peak[0] <= 1.0) || !(js_fit.peak[1] <= 1.0) || !(js_fit.peak[2] <= 1.0) || js_fit.window > 5)  // (a fitted Panda path passes with every W >= 4 at 1 ms; the search's first step from P <= 4 is at most ceil(4 / 0.95) = 5)
      mismatches++;
    print_rows("timed", timed, t_timed);
    print_jerk("executable", js_sol);
    print_rows("fitted", sol_fit, t_fit);
    print_jerk("executable_fit", js_fit);
    const int before = rm.lastError(), before_c = constraint->lastError();
    // the sticky error: the library refuses max_window = 0 — *out stays as it was, false, the error kept; on the roadmap the answer is the
    // timed solution with empty setpoints, true, with the error kept
    ccmp::JerkOptions bad = opts;
    bad.max_window = 0;
    ccmp::JerkSetpoints kept = js;
    const bool t1 = space->jerkSetpointPath(path, stamps, kVmax, kAmax, kJmax, &kept, bad);
    if (!same_ticks(kept, js)) mismatches++;
    Rows sol_bad;
    std::vector<double> t_sol_bad;
    ccmp::JerkSetpoints js_bad = js;
    const bool t2 = rm.constructExecutableSolution(starts, goals, sol_bad, t_sol_bad, js_bad, kVmax, kAmax, kJmax, bad, nullptr, nullptr, nullptr, 0.0, 0.5, 0, 0.0, 2,
                                                   0.005, 0, nullptr, nullptr, space->getDelta(), space->getLambda());
    if (sol_bad != timed || t_sol_bad != t_timed || !js_bad.tau.empty() || js_bad.status != CCMP_JERK_EMPTY || js_bad.window != 0) mismatches++;
    std::printf("summary mismatches %d before %d %d bad %d %d roadmap %d %d\n", mismatches, before, before_c, (int)t1, constraint->lastError(), (int)t2, rm.lastError());
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
