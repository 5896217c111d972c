// ccmp_ompl_adapter.hpp — header-only C++ host side above the C ABI (include/ccmp.h).
//
// Part 1 (always available, no third-party headers): ccmp::Projector, an RAII owner of a
// ccmp_ctx + ccmp_problem with the reference's method names on raw double[14] buffers;
// ccmp::SampleBuffer / ccmp::RefSampleBuffer, refill-on-empty batches of GPU-projected samples;
// ccmp::discreteGeodesic; ccmp::ShardedProjector (one process, several GPUs, RCCL all-gather of the valid states);
// ccmp::ProxyScene (sphere / box pre-filter ahead of the MoveIt validity test); and
// the dump formats of the reference's planner run (ccmp::printAsMatrix, ccmp::printGraphML, ccmp::printGraphviz).
//
// Part 2 (compiled only with CCMP_WITH_OMPL defined, i.e. inside the reference's catkin workspace where OMPL and Eigen
// exist): drop-in replacements that keep the reference's class names and virtual signatures, so
// src/planner/stefanBiPRM.cpp, src/base/constraints/ConstrainedPlanningCommon.cpp and src/main.cpp compile unchanged
// against them.  They replace the class bodies of TWO headers and the members of ONE source file of the reference:
//   class KinematicChainConstraint : public ompl::base::Constraint, typedef ChainConstraintPtr
//       (include/closed_chain_motion_planner/base/constraints/ConstraintFunction.h:21-140)
//   typedef jy_ProjectedStateSpacePtr, class jy_ProjectedStateSampler : public ompl::base::WrapperStateSampler,
//   class jy_ProjectedStateSpace : public ompl::base::ConstrainedStateSpace,
//   class jy_MotionValidator : public ompl::base::ConstrainedMotionValidator
//       (include/closed_chain_motion_planner/base/jy_ProjectedStateSpace.h:15-69; members: src/base/jy_ProjectedStateSpace.cpp:5-96,
//        which therefore leaves the build)
// The replacement headers and the CMake edit are in include/reference_overlay/ (INTEGRATION.md section 2).
// Neither OMPL nor Eigen is installed in the build image of this repository: part 2 is compiled against an interface mock
// (tests/cpp/mock_ompl) — two translation units including both replacement headers, linked into one program — and run on
// the GPU box by tests/test_cpp_adapter.py; part 1 is compiled and run there as plain C++14.
#ifndef CCMP_OMPL_ADAPTER_HPP
#define CCMP_OMPL_ADAPTER_HPP

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <limits>
#include <mutex>
#include <ostream>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ccmp.h"

namespace ccmp {

namespace detail {
// the text of every error of this header: "<entry point>: <the library's word for the code>"
inline std::string describe(int code, const std::string &what) { return what + ": " + ccmp_strerror(code); }
}  // namespace detail

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &what) : std::runtime_error(detail::describe(c, what)), code(c) {}
};
inline void check(int rc, const char *what)
{
  if (rc != CCMP_OK) throw Error(rc, what);
}

namespace detail {
// The sticky error of the verbs that never throw: the FIRST failure stays until clear().  Not synchronised: the owner's calls are
// (KinematicChainConstraint, the one class touched from two threads, keeps a mutex of its own around it).
class ErrorLatch {
public:
  void record(int code, const char *what) noexcept
  {
    if (code_ != CCMP_OK) return;
    code_ = code;
    try { what_ = describe(code, what); } catch (...) {}
  }
  // the same rule with the message as given
  void recordAs(int code, const char *message) noexcept
  {
    if (code_ != CCMP_OK) return;
    code_ = code;
    try { what_ = message; } catch (...) {}
  }
  int code() const noexcept { return code_; }
  std::string message() const { return what_; }
  void clear() noexcept { code_ = CCMP_OK; what_.clear(); }

private:
  int code_ = CCMP_OK;
  std::string what_;
};
// One library call of a verb that never throws: without a handle CCMP_EINVAL; else `body` (returns the library's code) under `mu`, an
// exception counting as CCMP_EHIP; whatever is not CCMP_OK goes to the latch under the name `what`.  true = the call ran and succeeded.
template <class F>
inline bool guardedCall(bool have_handle, std::mutex &mu, ErrorLatch &err, const char *what, F &&body) noexcept
{
  if (!have_handle) { err.record(CCMP_EINVAL, what); return false; }
  int rc;
  try {
    std::lock_guard<std::mutex> hold(mu);
    rc = body();
  } catch (...) {
    rc = CCMP_EHIP;
  }
  if (rc != CCMP_OK) err.record(rc, what);
  return rc == CCMP_OK;
}
inline void fillNaN(double *x, int n = 14)
{
  if (x)
    for (int i = 0; i < n; i++) x[i] = std::numeric_limits<double>::quiet_NaN();
}
// 14 joints between a double[14] and anything indexable (an OMPL StateType, an Eigen::Ref)
template <class Src>
inline void load14(double *dst, const Src &src)
{
  for (int i = 0; i < 14; ++i) dst[i] = src[i];
}
template <class Dst>
inline void store14(Dst &&dst, const double *src)
{
  for (int i = 0; i < 14; ++i) dst[i] = src[i];
}
}  // namespace detail

// SplitMix64 (the generator behind the kernels' counter-based samplers) and a process-wide source of sampler seeds:
// every sampler owns its own stream, as every OMPL StateSampler owns its own ompl::RNG.  CCMP_SEED in the
// environment makes runs reproducible (the counterpart of ompl::RNG::setSeed).
inline uint64_t splitmix64(uint64_t z)
{
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline uint64_t next_sampler_seed()
{
  static const uint64_t process_seed = [] {
    if (const char *env = std::getenv("CCMP_SEED")) return (uint64_t)std::strtoull(env, nullptr, 0);
    std::random_device rd;
    return ((uint64_t)rd() << 32) ^ (uint64_t)rd();
  }();
  static std::atomic<uint64_t> counter{0};
  return splitmix64(process_seed + counter.fetch_add(1, std::memory_order_relaxed));
}

class ProxyScene; // the proxy pre-filter, below: the vetted sampleCalibGoal takes one

// Owner of one execution context and one problem description.  The drop-in KinematicChainConstraint is touched from
// more than one thread in the reference (the jy_GoalLazySamples sampling thread; checkForSolution beside
// constructRoadmap, src/planner/stefanBiPRM.cpp:848) and one ccmp_ctx holds per-call state (pinned I/O block, queue
// words, stream): every call that uses the context takes the Projector's mutex for its duration — negligible next to
// a ~100 us launch.  The problem is passed by value into every launch and may be changed between calls.
class Projector {
public:
  explicit Projector(int device = 0)
  {
    check(ccmp_ctx_create(device, &ctx_), "ccmp_ctx_create");
    std::memset(&problem_, 0, sizeof problem_);
    ccmp_ik_opts_default(&ik_opts_);
  }
  Projector(const std::string &yaml_path, int device = 0) : Projector(device) { loadConfig(yaml_path); }
  ~Projector() { ccmp_ctx_destroy(ctx_); }
  Projector(const Projector &) = delete;
  Projector &operator=(const Projector &) = delete;

  // grasping_point::loadConfig + ConstrainedProblem set-up (src/kinematics/grasping_point.cpp:34-65,
  // src/base/constraints/ConstrainedPlanningCommon.cpp:85-132)
  void loadConfig(const std::string &yaml_path)
  {
    check(ccmp_problem_from_yaml(yaml_path.c_str(), &problem_), "ccmp_problem_from_yaml");
    configured_ = true;
  }
  // KinematicChainConstraint::setArmModels (ConstraintFunction.h:122-126): arm1 = the first seven joints, arm2 the other
  // seven — the order given, as the reference stores them (sorting by name is ConstrainedProblem::_setEnvironment's
  // business, ConstrainedPlanningCommon.cpp:89-91).  On a configured problem (the reference calls it after loadConfig,
  // ConstrainedPlanningCommon.cpp:126) only the arm / base-frame fields change: object poses, tolerances, delta / lambda,
  // calibration and mode are kept, init_chain_ and t_o7 are recomputed.
  void setArmModels(const std::string &name1, int index1, const std::string &name2, int index2)
  {
    if (!configured_) {
      const double q0[14] = {0};
      check(ccmp_problem_init(&problem_, name1.c_str(), index1, name2.c_str(), index2, q0, nullptr, nullptr, nullptr, nullptr), "ccmp_problem_init");
      configured_ = true;
    }
    check(ccmp_set_arms(&problem_, name1.c_str(), index1, name2.c_str(), index2), "ccmp_set_arms");
  }
  // ArmModel::t_wb of the arm in `slot` (panda_model.h:15; row-major rotation, translation): what function() multiplies
  // with (ConstraintFunction.h:89-90).  After setArmModels.
  void setBaseFrame(int slot, const double *R9, const double *p3) { check(ccmp_set_base_frame(&problem_, slot, R9, p3), "ccmp_set_base_frame"); }
  void setInitialPosition(const double *init_joint14) { check(ccmp_set_start(&problem_, init_joint14), "ccmp_set_start"); }
  // throws where the reference throws ompl::Exception (ConstraintFunction.h:106-108)
  void setTolerance(double tolerance1, double tolerance2) { check(ccmp_set_tolerance(&problem_, tolerance1, tolerance2), "setTolerance: tolerance must be positive"); }
  void setJacobianMode(int mode) { problem_.jacobian_mode = mode; }
  // The unchanged planner calls the constraint one state at a time (project(State*), isSatisfied(State*):
  // src/base/jy_ProjectedStateSpace.cpp:13,20,27,65, src/planner/stefanBiPRM.cpp:397-398), and each such call is a kernel launch
  // plus a completion poll.  setResident(true) turns on the context's resident service kernel (include/ccmp.h, option "resident"):
  // the same calls, the same bits, no launch on the call path (project(x) ~10 us less, isSatisfied 21 -> 9 us).  In the reference
  // arithmetic it also serves discreteGeodesic / checkMotion of ONE pair; after setJacobianMode(1) it serves discreteGeodesicBatch
  // of up to eight edges (growTree's five) and the continuation calls below, which carry carry_in — they reach it through
  // ccmp_geodesic_host_ex by themselves.  ccmp_ctx_get_option(ctx(), "resident_served", &n) counts the served requests.  Opt-in because a
  // kernel that stays on the device makes a device-wide synchronise of the APPLICATION's own (hipDeviceSynchronize, hipFree) wait
  // until the service has idled out ("resident_idle_ms", default 10 ms); the library's own calls stop it first.
  void setResident(bool on)
  {
    std::lock_guard<std::mutex> hold(mu_);
    check(ccmp_ctx_set_option(ctx_, "resident", on ? 1 : 0), "ccmp_ctx_set_option(resident)");
  }
  // what the scheduling policy does with a batched call of n samples / edges (CCMP_CALL_*), in one line — ccmp_ctx_describe
  std::string describe(int call_kind, size_t n) const
  {
    char buf[2048];
    const int len = ccmp_ctx_describe(ctx_, call_kind, n, buf, sizeof buf);
    return len < 0 ? std::string() : std::string(buf);
  }

  // bool KinematicChainConstraint::project(Eigen::Ref<VectorXd> x) const — in place
  bool project(double *x14) const
  {
    uint8_t ok = 0;
    std::lock_guard<std::mutex> hold(mu_);
    check(ccmp_project_host(ctx_, &problem_, x14, x14, &ok, nullptr, 1), "ccmp_project_host");
    return ok != 0;
  }
  void function(const double *x14, double *out2) const
  {
    std::lock_guard<std::mutex> hold(mu_);
    check(ccmp_function_host(ctx_, &problem_, x14, out2, 1), "ccmp_function_host");
  }
  bool isSatisfied(const double *x14) const
  {
    uint8_t ok = 0;
    std::lock_guard<std::mutex> hold(mu_);
    check(ccmp_is_satisfied_host(ctx_, &problem_, x14, &ok, 1), "ccmp_is_satisfied_host");
    return ok != 0;
  }
  bool jointValid(const double *x14) const
  {
    uint8_t ok = 0;
    std::lock_guard<std::mutex> hold(mu_);
    check(ccmp_joint_valid_host(ctx_, &problem_, x14, &ok, 1), "ccmp_joint_valid_host");
    return ok != 0;
  }
  // batches on host buffers (q row-major [B][14])
  void projectBatch(const double *q_in, double *q_out, uint8_t *ok, uint16_t *iters, size_t B) const
  {
    std::lock_guard<std::mutex> hold(mu_);
    check(ccmp_project_host(ctx_, &problem_, q_in, q_out, ok, iters, B), "ccmp_project_host");
  }
  // ---- growTree's IK: bool jy_ValidStateSampler::sampleCalibGoal(obj_state, start, result) (jy_ConstrainedValidStateSampler.h:147-189) ----
  // pose8 = the object pose (x y z qx qy qz qw pad: poseOf), start14 = the neighbour's joints, result14 = the new joints.  Per arm the
  // hand target is T_obj * t_o7; the seeded solve first, else the closest converged one of ikOptions().restarts Gaussian restarts; both
  // arms must succeed (ccmp_pose_ik_host; the solver is this library's own, not TRAC-IK: include/ccmp.h).  The multi-seed form tries
  // `S` seeds [S][14] in order in ONE call — the reference's loop over the neighbours (stefanBiPRM.cpp:294-302) — and reports the slot
  // that won in *which (-1: none).  The reference's IKValid / si_->isValid(result) stay the caller's, on the returned state.
  // Never throw: false when no state was found OR the call failed; a failed call also leaves the FIRST error in lastError() /
  // lastErrorMessage() until clearError().  Whenever false is returned result14 is NaN-filled.
  // The restarts draw from the stream (ikSeed(), running index): one index per call; setIkStream makes runs reproducible.
  bool sampleCalibGoal(const double *pose8, const double *start14, double *result14) const noexcept { return sampleCalibGoal(pose8, start14, 1, result14, nullptr); }
  bool sampleCalibGoal(const double *pose8, const double *seeds, int S, double *result14, int *which) const noexcept
  {
    uint8_t ok = 0;
    int32_t slot = -1;
    const bool ran = detail::guardedCall(true, mu_, err_, "ccmp_pose_ik_host", [&] {
      const int rc = ccmp_pose_ik_host(ctx_, &problem_, &ik_opts_, pose8, seeds, 1, S, ikSeed(), ik_index_, result14, &ok, &slot, nullptr, nullptr);
      if (rc == CCMP_OK) ik_index_++;
      return rc;
    });
    if (!ran) {
      ok = 0;
      slot = -1;
      detail::fillNaN(result14);
    }
    if (which) *which = slot;
    return ok != 0;
  }
  // The same with the collision gates the reference has INSIDE sampleCalibGoal (jy_ConstrainedValidStateSampler.h:188,192-199), on the
  // PROXY scene (ccmp_pose_ik_vetted_host): a candidate of an arm counts only if that arm's clearance exceeds `margin` (IKValid), the
  // assembled state only if its full clearance does (si_->isValid(result)); a seeded solution that collides loses to a restart that does
  // not, and a refused slot hands over to the next seed.  Proxies, not MoveIt: the exact si_->isValid(result) of the returned state stays
  // the caller's.  Unlike MoveIt's IKValid, which sees whatever the other arm was last set to, the arm is tested alone and the pair of
  // arms on the assembled state.  *clearance (nullable): the returned state's clearance, NaN without one.  Same stream, same error rules.
  bool sampleCalibGoal(const double *pose8, const double *start14, double *result14, const ProxyScene &scene, double margin) const noexcept
  {
    return sampleCalibGoal(pose8, start14, 1, result14, nullptr, scene, margin, nullptr);
  }
  inline bool sampleCalibGoal(const double *pose8, const double *seeds, int S, double *result14, int *which, const ProxyScene &scene, double margin,
                              double *clearance = nullptr) const noexcept;
  ccmp_ik_opts &ikOptions() noexcept { return ik_opts_; }
  const ccmp_ik_opts &ikOptions() const noexcept { return ik_opts_; }
  void setIkStream(uint64_t seed, uint64_t next_index = 0) noexcept { ik_seed_ = seed; ik_index_ = next_index; ik_seeded_ = true; }
  // (drawn from the process-wide source at first use, not at construction: the samplers' seeds keep their order)
  uint64_t ikSeed() const noexcept
  {
    if (!ik_seeded_) { ik_seed_ = next_sampler_seed(); ik_seeded_ = true; }
    return ik_seed_;
  }
  uint64_t ikNextIndex() const noexcept { return ik_index_; }
  // for ccmp::Roadmap::grow, under mutex(): the index of the next call's restarts
  uint64_t takeIkIndex() const noexcept { return ik_index_++; }
  int lastError() const noexcept { return err_.code(); }
  std::string lastErrorMessage() const { return err_.message(); }
  void clearError() noexcept { err_.clear(); }

  unsigned getCoDimension() const { return 2; }
  unsigned getAmbientDimension() const { return 14; }
  const ccmp_problem &problem() const { return problem_; }
  ccmp_problem &problem() { return problem_; }
  ccmp_ctx *ctx() const { return ctx_; }
  // for callers that use ctx() directly (the buffers and discreteGeodesic below): hold this across the call
  std::mutex &mutex() const { return mu_; }

private:
  mutable std::mutex mu_;
  ccmp_ctx *ctx_ = nullptr;
  ccmp_problem problem_;
  bool configured_ = false;
  ccmp_ik_opts ik_opts_;
  mutable uint64_t ik_seed_ = 0;
  mutable bool ik_seeded_ = false;
  mutable uint64_t ik_index_ = 0;
  mutable detail::ErrorLatch err_; // the IK verbs' sticky error (the other verbs throw)
};

namespace detail {
// the Projector's problem with this delta / lambda where positive (the OMPL space's setDelta / setLambda): a per-call copy, nothing
// shared is written.  The CALLER holds proj.mutex().
inline ccmp_problem problemWith(const Projector &proj, double delta, double lambda)
{
  ccmp_problem pb = proj.problem();
  if (delta > 0) pb.delta = delta;
  if (lambda > 0) pb.lambda = lambda;
  return pb;
}
}  // namespace detail

// jy_ProjectedStateSampler::sampleUniform served from a buffer that ONE launch of `batch` fused
// sample -> project -> enforceBounds refills when empty (src/base/jy_ProjectedStateSpace.cpp:10-15).
// The stream of samples depends on (seed, running index) only, not on `batch`.
class SampleBuffer {
public:
  SampleBuffer(const Projector &proj, uint64_t seed, size_t batch = 4096) : proj_(proj), seed_(seed), batch_(batch) {}
  // writes 14 doubles; returns project()'s result for that sample (the reference ignores it)
  bool next(double *state14)
  {
    if (pos_ >= filled_) refill();
    std::memcpy(state14, &buf_[14 * pos_], 14 * sizeof(double));
    return ok_[pos_++] != 0;
  }

private:
  void refill()
  {
    filled_ = 0;  // a refill that throws leaves the buffer EMPTY (the next call tries again with the same indices), never half-valid
    pos_ = 0;
    buf_.resize(batch_ * 14);
    ok_.resize(batch_);
    std::lock_guard<std::mutex> hold(proj_.mutex());
    check(ccmp_sample_project_host(proj_.ctx(), &proj_.problem(), seed_, next_index_, buf_.data(), ok_.data(), nullptr, batch_),
          "ccmp_sample_project_host");
    next_index_ += batch_;
    filled_ = batch_;
  }
  const Projector &proj_;
  uint64_t seed_, next_index_ = 0;
  size_t batch_, pos_ = 0, filled_ = 0;
  std::vector<double> buf_;
  std::vector<uint8_t> ok_;
};

// jy_ProjectedStateSampler::sampleUniformNear / sampleGaussian (src/base/jy_ProjectedStateSpace.cpp:17-29) through the
// batched counter-based kernels.  The reference state may change from call to call, so nothing can be drawn ahead of
// the call; but `lookahead` samples around one state cost what one does (a 128-thread block per sample on an
// otherwise idle GPU), so a call with a new (state, parameter) draws `lookahead` samples in one launch and the
// following calls with the same arguments pop from that buffer.  Every refill takes fresh indices of the sampler's
// stream: no sample is handed out twice, whatever the call pattern.
class RefSampleBuffer {
public:
  enum Kind { Near = 0, Gaussian = 1 };
  RefSampleBuffer(const Projector &proj, uint64_t seed, Kind kind, size_t lookahead = 32)
    : proj_(proj), seed_(seed ^ (kind == Near ? 0x4E454152ull : 0x47415553ull)), kind_(kind), lookahead_(lookahead)
  {
  }
  // writes 14 doubles: a sample around ref14 (Near: within `param` per dimension; Gaussian: std dev `param`),
  // projected and wrapped by enforceBounds; returns project()'s result
  bool next(double *state14, const double *ref14, double param)
  {
    if (pos_ >= filled_ || param != param_ || std::memcmp(ref_, ref14, sizeof ref_) != 0) refill(ref14, param);
    std::memcpy(state14, &buf_[14 * pos_], 14 * sizeof(double));
    return ok_[pos_++] != 0;
  }

private:
  void refill(const double *ref14, double param)
  {
    filled_ = 0;  // a refill that throws leaves the buffer EMPTY, never filled with samples around another state
    pos_ = 0;
    std::memcpy(ref_, ref14, sizeof ref_);
    param_ = param;
    buf_.resize(lookahead_ * 14);
    ok_.resize(lookahead_);
    std::lock_guard<std::mutex> hold(proj_.mutex());
    check(ccmp_sample_ref_project_host(proj_.ctx(), &proj_.problem(), (int)kind_, seed_, next_index_, ref_, param_, buf_.data(), ok_.data(),
                                       nullptr, lookahead_),
          "ccmp_sample_ref_project_host");
    next_index_ += lookahead_;
    filled_ = lookahead_;
    pos_ = 0;
  }
  const Projector &proj_;
  uint64_t seed_, next_index_ = 0;
  Kind kind_;
  size_t lookahead_, pos_ = 0, filled_ = 0;
  double ref_[14] = {0}, param_ = 0;
  std::vector<double> buf_;
  std::vector<uint8_t> ok_;
};

// jy_ProjectedStateSpace::discreteGeodesic (src/base/jy_ProjectedStateSpace.cpp:32-96) for E edges in ONE launch on raw
// buffers (from / to: E x 14, row-major): growTree tries its (up to five) nearest neighbours one after the other
// (src/planner/stefanBiPRM.cpp:307-351, each a discreteGeodesic(neighbour, new vertex, false, &states)); handed over
// together they cost the longest edge's serial chain instead of the sum.  `valid` is the host StateValidityChecker; it is
// consulted only when !interpolate, and it sees the same states in the same order as in the reference's loop — edge by
// edge, state by state, an edge stopping at its first rejected state, where the reference's loop breaks.  reached[e] is
// the bool of edge e, (*geodesics)[e] its list.
// The traversal on the GPU lists max_states states per call (edges of the reference's roadmaps have 3-7; the work spent
// beyond a state the checker rejects is bounded by this).  An edge that needs more is CONTINUED from its last stored
// state (ccmp_geodesic_host_ex: the states of one uninterrupted traversal, bit for bit) — after the checker has passed
// what is there, so that a long or creeping edge the checker cuts early costs nothing more.  A cut list never reaches
// the caller as if it were complete.
// check_target: ConstrainedMotionValidator::checkMotion in one launch — isSatisfied(to) is tested first and an edge whose
// target fails it returns false with only `from` in the list (src/planner/stefanBiPRM.cpp:397-398).
// delta / lambda > 0 override the problem's values for this call (the space's setDelta / setLambda) through a per-call
// copy of the problem: nothing shared is written, whichever thread calls.
namespace detail {
// The host loop of every discreteGeodesicBatch / discreteGeodesic.  scene != nullptr (never with interpolate): the traversal itself
// refuses a state whose clearance does not exceed `margin` (ccmp_geodesic_scene_host) and (*blocked)[e] (nullable) = 1 where edge e
// ended at such a state; else ccmp_geodesic_host_ex — the first pass and the continuations alike.
template <class ValidFn>
inline void traverseBatch(const Projector &proj, const double *from, const double *to, size_t E, bool interpolate, ValidFn valid,
                          std::vector<std::vector<std::vector<double>>> *geodesics, std::vector<char> *reached, int max_states, bool check_target,
                          double delta, double lambda, const ccmp_scene *scene, double margin, std::vector<char> *blocked)
{
  // one library call, by the caller under proj.mutex(): bl = the edges' blocked bytes (with a scene), carry as ccmp_geodesic_host_ex has it
  const auto traversal = [&](const ccmp_problem &pb, const double *a, const double *b, size_t edges, int cap, double *st, int32_t *n, uint8_t *ok,
                             uint8_t *bl, const double *carry_in, double *carry_out, int budget, int target, bool continued) {
    if (scene)
      check(ccmp_geodesic_scene_host(proj.ctx(), &pb, scene, margin, a, b, edges, cap, st, n, ok, nullptr, bl, nullptr, carry_in, carry_out, budget, target),
            continued ? "ccmp_geodesic_scene_host(continue)" : "ccmp_geodesic_scene_host");
    else
      check(ccmp_geodesic_host_ex(proj.ctx(), &pb, a, b, edges, cap, st, n, ok, carry_in, carry_out, budget, target),
            continued ? "ccmp_geodesic_host_ex(continue)" : "ccmp_geodesic_host_ex");
  };
  if (blocked) blocked->assign(E, 0);
  if (reached) reached->assign(E, 0);
  if (geodesics) geodesics->assign(E, {});
  if (E == 0) return;
  if (max_states < 2) max_states = 2; // a continuation starts from a stored state other than `from`
  // A large batch takes the shape the library is fastest with: a first pass with lists of 16 states and at
  // most 128 Newton rounds per edge — one launch that no creeping edge can hold — and the few edges that stop short
  // (list full: n = cap + 1; rounds spent: ok = 2) are continued below, which gives the states of one uninterrupted
  // traversal bit for bit.  growTree's handful of neighbours goes through unchanged.
  const bool big = E >= 1024;
  const int first_cap = big && max_states > 16 ? 16 : max_states;
  const int first_budget = big ? 128 : 0;
  ccmp_problem pb;
  std::vector<double> states(E * (size_t)first_cap * 14), carry(E * 2);
  std::vector<int32_t> n(E);
  std::vector<uint8_t> ok(E), bl(scene ? E : 0);
  {
    std::lock_guard<std::mutex> hold(proj.mutex());
    pb = problemWith(proj, delta, lambda);
    traversal(pb, from, to, E, first_cap, states.data(), n.data(), ok.data(), bl.data(), nullptr, carry.data(), first_budget, check_target ? 1 : 0, false);
  }
  std::vector<double> more((size_t)max_states * 14);
  for (size_t e = 0; e < E; ++e) {
    std::vector<std::vector<double>> list;
    const double *st = &states[e * (size_t)first_cap * 14];
    const double *to_e = to + 14 * e;
    double cr[2] = {carry[2 * e], carry[2 * e + 1]};
    int32_t ne = n[e];
    uint8_t oke = ok[e], ble = scene ? bl[e] : 0;
    bool good = false, cut = false;
    std::vector<double> last(14);
    int first = 0; // a continuation's row 0 repeats the state it started from
    int cap = first_cap;
    for (;;) {
      const int have = ne > cap ? cap : ne;
      for (int k = first; k < have && !cut; ++k) {
        const double *row = st + (size_t)k * 14;
        if (!interpolate && !(list.empty() && k == 0) && !valid(row)) {
          // the reference's loop breaks here, before `dist` is updated: the answer is about the last accepted state
          double d = 0;
          for (int i = 0; i < 14; ++i) { const double df = last[i] - to_e[i]; d += df * df; }
          good = std::sqrt(d) <= pb.delta;
          cut = true;
          break;
        }
        last.assign(row, row + 14);
        list.emplace_back(row, row + 14);
      }
      if (cut) break;
      // the edge ended here: a blocked edge is final too (the traversal's ok is the reference's answer behind the break)
      if (ne <= cap && oke != 2) { good = oke != 0; if (blocked) (*blocked)[e] = (char)ble; break; }
      // ne == cap + 1: the list was full and the traversal stopped there; ok == 2: it had spent the call's Newton rounds —
      // either way go on from its last state
      double cr_out[2];
      {
        std::lock_guard<std::mutex> hold(proj.mutex());
        traversal(pb, last.data(), to_e, 1, max_states, more.data(), &ne, &oke, &ble, cr, cr_out, 0, 0, true);
      }
      cr[0] = cr_out[0];
      cr[1] = cr_out[1];
      st = more.data();
      cap = max_states;
      first = 1;
    }
    if (reached) (*reached)[e] = good ? 1 : 0;
    if (geodesics) (*geodesics)[e] = std::move(list);
  }
}
}  // namespace detail

// E edges, as described above
template <class ValidFn>
inline void discreteGeodesicBatch(const Projector &proj, const double *from, const double *to, size_t E, bool interpolate, ValidFn valid,
                                  std::vector<std::vector<std::vector<double>>> *geodesics, std::vector<char> *reached, int max_states = 64,
                                  bool check_target = false, double delta = -1.0, double lambda = -1.0)
{
  detail::traverseBatch(proj, from, to, E, interpolate, valid, geodesics, reached, max_states, check_target, delta, lambda, nullptr, 0.0, nullptr);
}

// one edge
template <class ValidFn>
inline bool discreteGeodesic(const Projector &proj, const double *from14, const double *to14, bool interpolate, ValidFn valid,
                             std::vector<std::vector<double>> *geodesic, int max_states = 64, bool check_target = false,
                             double delta = -1.0, double lambda = -1.0)
{
  std::vector<std::vector<std::vector<double>>> lists;
  std::vector<char> reached;
  detail::traverseBatch(proj, from14, to14, 1, interpolate, valid, geodesic ? &lists : nullptr, &reached, max_states, check_target, delta, lambda, nullptr,
                        0.0, nullptr);
  if (geodesic) *geodesic = std::move(lists[0]);
  return reached[0] != 0;
}

// The reference's connectionStrategy_(m) — a KStrategy over tree_ (src/planner/stefanBiPRM.cpp:292,390,457) — on the joint distance
// (ccmp_knn_host): the k nearest of N host states for one state, nearest first, ties to the lower index; idx has k entries, -1
// where fewer than k nodes exist.  The joint term only, and the nodes are uploaded with every call: ccmp::Roadmap below keeps them on
// the device and ranks on the reference's own metric, the object's SE3 distance.
inline void nearestK(const Projector &proj, const double *nodes, size_t N, const double *q14, unsigned k, std::vector<int32_t> *idx)
{
  idx->assign(k, -1);
  std::lock_guard<std::mutex> hold(proj.mutex());
  check(ccmp_knn_host(proj.ctx(), nodes, N, q14, 1, (int)k, CCMP_KNN_ALL, 0, idx->data(), nullptr), "ccmp_knn_host");
}

// PathGeometric::interpolate on a solution path (include/ccmp.h: ccmp_path_densify_host): `states` = the waypoints on entry and the dense
// path on return — w_0, G_0, w_1, G_1, .., w_{L-1} with every w_i before the last twice in a row, as printAsMatrix then writes them, or
// with `distinct` G_0, G_1, .., w_{L-1}; G_i = the state list of discreteGeodesic(w_i, w_{i+1}, interpolate = true), traversed to its end
// inside the library.  seg_ok (nullable) = the return value of each of the L - 1 traversals: a 0 is a segment that stopped short of its
// target — its rows are there and the path jumps, as the reference's does.  delta / lambda > 0 replace the problem's (the OMPL space's
// setDelta / setLambda).  Returns the library's code and leaves `states` untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int densifyPathLocked(const Projector &proj, std::vector<std::array<double, 14>> &states, bool distinct, std::vector<uint8_t> *seg_ok,
                             double delta = 0.0, double lambda = 0.0)
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double), "rows are contiguous");
  const ccmp_problem P = detail::problemWith(proj, delta, lambda);
  ccmp_dense_opts o;
  ccmp_dense_opts_default(&o);
  o.flags = distinct ? CCMP_DENSE_DISTINCT : 0;
  static const double none[14] = {0};
  const int32_t len = (int32_t)states.size();
  ccmp_dense_paths *h = nullptr;
  int rc = ccmp_path_densify_host(proj.ctx(), &P, nullptr, 0.0, len ? states[0].data() : none, &len, 1, len > 0 ? len : 1, &o, &h);
  if (rc != CCMP_OK) return rc;
  size_t rows = 0;
  std::vector<std::array<double, 14>> dense;
  std::vector<uint8_t> ok;
  try {
    rc = ccmp_dense_paths_info(h, nullptr, nullptr, &rows, nullptr);
    dense.resize(rows);
    ok.resize(len > 1 ? (size_t)len - 1 : 0);
  } catch (...) {
    rc = CCMP_ENOMEM;
  }
  if (rc == CCMP_OK)
    rc = ccmp_dense_paths_copy_host(h, rows ? dense[0].data() : nullptr, nullptr, nullptr, ok.empty() ? nullptr : ok.data(), nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr);
  ccmp_dense_paths_destroy(h);
  if (rc != CCMP_OK) return rc;
  states.swap(dense);
  if (seg_ok) seg_ok->swap(ok);
  return CCMP_OK;
}

// The removal of interior vertices from a solution path (include/ccmp.h: ccmp_path_shortcut_host): `states` = the waypoints on entry and
// the kept waypoints on return — every pair (i, j) with 2 <= j - i <= max_span (0: every span) is put to one checkMotion(w_i, w_j), all
// pairs in one batch, and the cheapest path from w_0 to w_{L-1} over the path's own edges and the pairs that passed is taken: the optimum
// any sequence of PathSimplifier::reduceVertices removals could reach, deterministic.  kept (nullable) = the indices of the kept waypoints
// in the path as it came in; cost_in / cost_out (nullable) = the joint length before and after.  delta / lambda > 0 replace the problem's.
// A shortcut leaves the edges the host validated: interpolate the result and put the dense rows to the host's isValid.
// Returns the library's code and leaves `states` untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int shortcutPathLocked(const Projector &proj, std::vector<std::array<double, 14>> &states, int max_span, std::vector<int32_t> *kept,
                              double *cost_in, double *cost_out, double delta = 0.0, double lambda = 0.0)
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double), "rows are contiguous");
  if (states.empty()) {
    if (kept) kept->clear();
    if (cost_in) *cost_in = 0.0;
    if (cost_out) *cost_out = 0.0;
    return CCMP_OK;
  }
  if (states.size() > (size_t)CCMP_SHORTCUT_MAX_LEN) return CCMP_EINVAL;
  const ccmp_problem P = detail::problemWith(proj, delta, lambda);
  ccmp_shortcut_opts o;
  ccmp_shortcut_opts_default(&o);
  o.max_span = max_span;
  const int32_t len = (int32_t)states.size();
  int32_t out_len = 0;
  double ci = 0.0, co = 0.0;
  std::vector<std::array<double, 14>> rows;
  std::vector<int32_t> idx;
  try {
    rows.resize(states.size());
    idx.assign(states.size(), -1);
  } catch (...) {
    return CCMP_ENOMEM;
  }
  const int rc = ccmp_path_shortcut_host(proj.ctx(), &P, nullptr, 0.0, states[0].data(), &len, 1, len, &o, rows[0].data(), &out_len, idx.data(), &ci, &co,
                                         nullptr, nullptr, nullptr);
  if (rc != CCMP_OK) return rc;
  if (out_len < 0 || out_len > len) return CCMP_EHIP;
  rows.resize((size_t)out_len);
  idx.resize((size_t)out_len);
  states.swap(rows);
  if (kept) kept->swap(idx);
  if (cost_in) *cost_in = ci;
  if (cost_out) *cost_out = co;
  return CCMP_OK;
}

// B-spline smoothing passes on the manifold (include/ccmp.h: ccmp_path_smooth_host; the structure of PathSimplifier::smoothBSpline with
// the library's midpoint): `states` = the waypoints on entry and the smoothed path on return — at most max_steps passes, each L -> 2L - 1
// vertices, a vertex moving only by more than min_change and only when both checkMotions to its new neighbours pass.  passes / moved /
// stop / length_in / length_out (nullable) as the library reports them.  delta / lambda > 0 replace the problem's.  Order of use:
// shortcut -> smooth -> interpolate -> the host's isValid over the dense rows.  Returns the library's code and leaves
// `states` untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int smoothPathLocked(const Projector &proj, std::vector<std::array<double, 14>> &states, int max_steps, double min_change, int *passes = nullptr,
                            int *moved = nullptr, int *stop = nullptr, double *length_in = nullptr, double *length_out = nullptr, double delta = 0.0,
                            double lambda = 0.0)
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double), "rows are contiguous");
  const ccmp_problem P = detail::problemWith(proj, delta, lambda);
  ccmp_smooth_opts o;
  ccmp_smooth_opts_default(&o);
  o.max_steps = max_steps;
  o.min_change = min_change;
  if (states.empty()) {
    if (passes) *passes = 0;
    if (moved) *moved = 0;
    if (stop) *stop = 0;
    if (length_in) *length_in = 0.0;
    if (length_out) *length_out = 0.0;
    return (max_steps < 0 || !(min_change >= 0.0)) ? CCMP_EINVAL : CCMP_OK;
  }
  if (states.size() > (size_t)0x3fffffff) return CCMP_EINVAL;
  const int32_t len = (int32_t)states.size();
  const int cap = ccmp_smooth_len_after(len, max_steps < 0 ? 0 : max_steps);
  if (cap == 0x7fffffff) return CCMP_EINVAL; // the result would not fit any buffer
  int32_t out_len = 0, n_pass = 0, n_moved = 0, why = 0;
  double li = 0.0, lo = 0.0;
  std::vector<std::array<double, 14>> rows;
  try {
    rows.resize((size_t)cap);
  } catch (...) {
    return CCMP_ENOMEM;
  }
  const int rc = ccmp_path_smooth_host(proj.ctx(), &P, nullptr, 0.0, states[0].data(), &len, 1, len, &o, cap, rows[0].data(), &out_len, &n_pass, &n_moved, &why,
                                       &li, &lo, nullptr);
  if (rc != CCMP_OK) return rc;
  if (out_len < 0 || out_len > cap) return CCMP_EHIP;
  rows.resize((size_t)out_len);
  states.swap(rows);
  if (passes) *passes = n_pass;
  if (moved) *moved = n_moved;
  if (stop) *stop = why;
  if (length_in) *length_in = li;
  if (length_out) *length_out = lo;
  return CCMP_OK;
}

// A solution path resampled at even arc (include/ccmp.h: ccmp_path_densify_host, then ccmp_path_resample on the dense result where the
// library keeps it — PathGeometric::interpolate(count) with the library's blend): `states` = the waypoints on entry (the smoothed path,
// say) and the resampled rows on return: `count` rows, or with count == 0 one every `spacing` of arc (spacing <= 0: the problem's delta).
// The first and the last row are the path's own; every other row is a NEW state — the blend at its arc put back on the manifold, or the
// nearer dense row where that fails — and goes to the host's isValid before use.  status (nullable) = CCMP_RETIME_*;
// kinds (nullable) = CCMP_SAMPLE_* per row.  A path that is empty, broken (a segment that stopped short), not finite or over 65 536 rows
// comes back as it was, with CCMP_OK and its status.  delta / lambda > 0 replace the problem's.  Returns the library's code and leaves
// `states` untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int resamplePathLocked(const Projector &proj, std::vector<std::array<double, 14>> &states, int count, double spacing, int *status = nullptr,
                              std::vector<uint8_t> *kinds = nullptr, double delta = 0.0, double lambda = 0.0)
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double), "rows are contiguous");
  const ccmp_problem P = detail::problemWith(proj, delta, lambda);
  ccmp_resample_opts ro;
  ccmp_resample_opts_default(&P, &ro);
  ro.count = count;
  if (spacing > 0.0) ro.spacing = spacing;
  ccmp_dense_opts o;
  ccmp_dense_opts_default(&o);
  o.flags = CCMP_DENSE_DISTINCT;
  static const double none[14] = {0};
  const int32_t len = (int32_t)states.size();
  ccmp_dense_paths *dense = nullptr;
  int rc = ccmp_path_densify_host(proj.ctx(), &P, nullptr, 0.0, len ? states[0].data() : none, &len, 1, len > 0 ? len : 1, &o, &dense);
  if (rc != CCMP_OK) return rc;
  ccmp_sampled_paths *h = nullptr;
  rc = ccmp_path_resample(proj.ctx(), &P, dense, &ro, &h, nullptr);
  ccmp_dense_paths_destroy(dense);
  if (rc != CCMP_OK) return rc;
  size_t rows = 0;
  int32_t st = CCMP_RETIME_EMPTY;
  std::vector<std::array<double, 14>> out;
  std::vector<uint8_t> kd;
  try {
    rc = ccmp_sampled_paths_info(h, nullptr, &rows);
    out.resize(rows);
    kd.resize(rows);
  } catch (...) {
    rc = CCMP_ENOMEM;
  }
  if (rc == CCMP_OK) rc = ccmp_sampled_paths_copy_host(h, rows ? out[0].data() : nullptr, nullptr, nullptr, nullptr, rows ? kd.data() : nullptr, &st, nullptr);
  ccmp_sampled_paths_destroy(h);
  if (rc != CCMP_OK) return rc;
  if (status) *status = st;
  if (st == CCMP_RETIME_OK || st == CCMP_RETIME_POINT) {
    states.swap(out);
    if (kinds) kinds->swap(kd);
  } else if (kinds) {
    kinds->clear();
  }
  return CCMP_OK;
}

// Time stamps for a path's rows under joint velocity and acceleration limits (include/ccmp.h: ccmp_path_timestamps_host; the path starts
// and ends at rest): vmax / amax = 14 numbers each, beta in (0, 1) the share of the acceleration budget given to curvature.  times = one
// per row, times[0] = 0; duration (nullable) = the last.  The limits bound the speed profile at the rows; they are not a bound on finite
// differences of the sampled trajectory.  A row that is not finite is CCMP_EINVAL.  Returns the library's code and leaves `times`
// untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int timestampPath(const Projector &proj, const std::vector<std::array<double, 14>> &states, const double *vmax, const double *amax, double beta,
                         std::vector<double> *times, double *duration = nullptr)
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double), "rows are contiguous");
  if (!times || states.size() > (size_t)0x7fffffff) return CCMP_EINVAL;
  const int32_t first[2] = {0, (int32_t)states.size()};
  std::vector<double> t;
  try {
    t.assign(states.size(), 0.0);
  } catch (...) {
    return CCMP_ENOMEM;
  }
  double total = 0.0;
  int32_t st = CCMP_RETIME_EMPTY;
  const int rc = ccmp_path_timestamps_host(proj.ctx(), states.empty() ? nullptr : states[0].data(), first, 1, states.size(), vmax, amax, beta,
                                           t.empty() ? nullptr : t.data(), &total, nullptr, nullptr, &st);
  if (rc != CCMP_OK) return rc;
  if (st == CCMP_RETIME_NONFINITE) return CCMP_EINVAL;
  times->swap(t);
  if (duration) *duration = total;
  return CCMP_OK;
}

// What a controller is commanded at every tick of its period along a timed path, and the audit of that motion (include/ccmp.h:
// ccmp_path_setpoints_host): q, qd = one row of 14 per tick, tau = the tick times (tau[0] = 0, the last = the duration); f = the
// constraint gap (|dp|, angle) per tick, satisfied = isSatisfied, clearance = against `scene` (NaN without one); peak / peak_tick in the
// order speed ratio, acceleration ratio, |dp|, angle, clearance; n_off / n_below = ticks isSatisfied refuses / with clearance < margin;
// stretch = the factor on all stamps that would bring the measured peaks to the limits (a report).  status = CCMP_SETPOINTS_*.
struct Setpoints {
  std::vector<std::array<double, 14>> q, qd;
  std::vector<double> tau, clearance;
  std::vector<std::array<double, 2>> f;
  std::vector<uint8_t> satisfied;
  int32_t status = CCMP_SETPOINTS_EMPTY;
  double peak[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int32_t peak_tick[5] = {-1, -1, -1, -1, -1};
  int32_t n_off = 0, n_below = 0;
  double stretch = 1.0;
};

// The setpoints of ONE path: states and times as ccmp::timestampPath leaves them (any stamps that start at 0 and do not decrease), vmax /
// amax = 14 numbers each, period > 0 the controller's, max_ticks >= 2; scene (nullable) and margin for the ticks' clearance.  The
// setpoints are NOT projected: between rows they leave the manifold by what the resample spacing allows, and out->peak says by how much.
// A path that is empty, not finite, out of order or over max_ticks comes back with CCMP_OK, its status and no tick.  Returns the library's
// code and leaves *out untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int setpointPath(const Projector &proj, const std::vector<std::array<double, 14>> &states, const std::vector<double> &times, const double *vmax,
                        const double *amax, Setpoints *out, double period = 0.001, int max_ticks = 65536, const ccmp_scene *scene = nullptr,
                        double margin = 0.0)
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double) && sizeof(std::array<double, 2>) == 2 * sizeof(double), "rows are contiguous");
  if (!out || states.size() != times.size() || states.size() > (size_t)0x7fffffff) return CCMP_EINVAL;
  const ccmp_problem P = detail::problemWith(proj, 0.0, 0.0);
  const int32_t first[2] = {0, (int32_t)states.size()};
  const ccmp_setpoint_opts o = {period, max_ticks};
  ccmp_setpoints *h = nullptr;
  int rc = ccmp_path_setpoints_host(proj.ctx(), &P, scene, margin, states.empty() ? nullptr : states[0].data(), first, times.empty() ? nullptr : times.data(), 1,
                                    states.size(), vmax, amax, &o, &h);
  if (rc != CCMP_OK) return rc;
  Setpoints s;
  size_t ticks = 0;
  try {
    rc = ccmp_setpoints_info(h, nullptr, &ticks);
    s.q.resize(ticks);
    s.qd.resize(ticks);
    s.tau.resize(ticks);
    s.clearance.resize(ticks);
    s.f.resize(ticks);
    s.satisfied.resize(ticks);
  } catch (...) {
    rc = CCMP_ENOMEM;
  }
  int32_t counts[2] = {0, 0};
  if (rc == CCMP_OK)
    rc = ccmp_setpoints_copy_host(h, ticks ? s.q[0].data() : nullptr, ticks ? s.qd[0].data() : nullptr, ticks ? s.tau.data() : nullptr, nullptr,
                                  ticks ? s.f[0].data() : nullptr, ticks ? s.satisfied.data() : nullptr, ticks ? s.clearance.data() : nullptr, &s.status, s.peak,
                                  s.peak_tick, counts, &s.stretch);
  ccmp_setpoints_destroy(h);
  if (rc != CCMP_OK) return rc;
  s.n_off = counts[0];
  s.n_below = counts[1];
  *out = std::move(s);
  return CCMP_OK;
}

// Time stamps fitted to the limits at the controller's rate (include/ccmp.h: ccmp_path_fit_timestamps_host), the step between
// timestampPath and setpointPath: times = the fitted stamps, factor = the dilation of each row interval at its right row, status =
// CCMP_FIT_FITTED, CCMP_FIT_PASSES or the setpoints status that ended the path, passes = the dilations applied, peak = the speed and
// acceleration ratios of the last measurement (what setpointPath's audit reports for `times`), duration = the last stamp.
struct FittedTimes {
  std::vector<double> times, factor;
  int32_t status = CCMP_SETPOINTS_EMPTY, passes = 0;
  double peak[2] = {0.0, 0.0};
  double duration = 0.0;
};

// The options of a fit: the controller's period and tick bound as setpointPath takes them, the share `aim` of a limit an interval in
// excess is dilated to (0 < aim <= 1) and the dilations at most.
struct FitOptions {
  double period = 0.001;
  int max_ticks = 65536;
  double aim = 0.95;
  int max_passes = 8;
};

// The fit of ONE path: states and times as ccmp::timestampPath leaves them.  Only the row intervals in which the commanded motion exceeds
// a limit are dilated; a path already within the limits comes back bit for bit.  It is not TOPP-RA, has no jerk limit, bounds the motion
// only at the ticks of the stated period, and its convergence is observed, not proven: out->status says whether the audit passes.  A path
// that is empty, not finite, out of order or over max_ticks comes back with CCMP_OK, that status and its stamps.  Returns the library's
// code and leaves *out untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int fitPath(const Projector &proj, const std::vector<std::array<double, 14>> &states, const std::vector<double> &times, const double *vmax,
                   const double *amax, FittedTimes *out, const FitOptions &opts = FitOptions())
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double), "rows are contiguous");
  if (!out || states.size() != times.size() || states.size() > (size_t)0x7fffffff) return CCMP_EINVAL;
  const int32_t first[2] = {0, (int32_t)states.size()};
  const ccmp_fit_opts o = {opts.period, opts.max_ticks, opts.aim, opts.max_passes};
  FittedTimes r;
  try {
    r.times.assign(times.size(), 0.0);
    r.factor.assign(times.size(), 1.0);
  } catch (...) {
    return CCMP_ENOMEM;
  }
  const int rc = ccmp_path_fit_timestamps_host(proj.ctx(), states.empty() ? nullptr : states[0].data(), first, times.empty() ? nullptr : times.data(), 1,
                                               states.size(), vmax, amax, &o, r.times.empty() ? nullptr : r.times.data(), &r.status, &r.passes, r.peak,
                                               &r.duration, r.factor.empty() ? nullptr : r.factor.data());
  if (rc != CCMP_OK) return rc;
  *out = std::move(r);
  return CCMP_OK;
}

// Jerk-bounded setpoints (include/ccmp.h: ccmp_path_jerk_setpoints_host), the unit beside setpointPath for a controller that limits jerk:
// Setpoints' per-tick arrays for the moving average of `window` consecutive ticks of the interpolant, plus the window the search chose, its
// passes and SIX peaks in the order speed ratio, acceleration ratio, jerk ratio, |dp|, angle, clearance — the last three of the FILTERED
// positions.  status = CCMP_JERK_*.  There is no stretch.
struct JerkSetpoints {
  std::vector<std::array<double, 14>> q, qd;
  std::vector<double> tau, clearance;
  std::vector<std::array<double, 2>> f;
  std::vector<uint8_t> satisfied;
  int32_t status = CCMP_JERK_EMPTY, window = 0, passes = 0;
  double peak[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int32_t peak_tick[6] = {-1, -1, -1, -1, -1, -1};
  int32_t n_off = 0, n_below = 0;
};

// The options of the call: the controller's period and tick bound as setpointPath takes them, window (0: chosen per path, else 1 ..
// max_window), max_window (1 .. 256) and the share `aim` of the jerk limit the next window of the search aims at (0 < aim <= 1).
struct JerkOptions {
  double period = 0.001;
  int max_ticks = 65536;
  int window = 0;
  int max_window = 64;
  double aim = 0.95;
};

// The jerk-bounded setpoints of ONE path: states and times as ccmp::timestampPath or ccmp::fitPath leave them, vmax / amax / jmax = 14
// numbers each.  By construction the speed and acceleration peaks do not rise above setpointPath's and the jerk is at most 2 A / (W period);
// it is a bound at the ticks of the stated period on the qd sequence, not a third difference of positions; the filtered ticks lag by
// (W - 1) / 2 ticks and cut corners — out->f, satisfied and clearance say whether that matters; it is not a jerk-optimal profile.  A path
// that is empty, not finite, out of order or over max_ticks comes back with CCMP_OK, its status and no tick; CCMP_JERK_WINDOW still delivers
// the ticks of max_window.  Returns the library's code and leaves *out untouched unless it is CCMP_OK.  The CALLER holds proj.mutex().
inline int jerkSetpointPath(const Projector &proj, const std::vector<std::array<double, 14>> &states, const std::vector<double> &times, const double *vmax,
                            const double *amax, const double *jmax, JerkSetpoints *out, const JerkOptions &opts = JerkOptions(),
                            const ccmp_scene *scene = nullptr, double margin = 0.0)
{
  static_assert(sizeof(std::array<double, 14>) == 14 * sizeof(double) && sizeof(std::array<double, 2>) == 2 * sizeof(double), "rows are contiguous");
  if (!out || states.size() != times.size() || states.size() > (size_t)0x7fffffff) return CCMP_EINVAL;
  const ccmp_problem P = detail::problemWith(proj, 0.0, 0.0);
  const int32_t first[2] = {0, (int32_t)states.size()};
  const ccmp_jerk_opts o = {opts.period, opts.max_ticks, opts.window, opts.max_window, opts.aim, 0};
  ccmp_jerk_setpoints *h = nullptr;
  int rc = ccmp_path_jerk_setpoints_host(proj.ctx(), &P, scene, margin, states.empty() ? nullptr : states[0].data(), first, times.empty() ? nullptr : times.data(),
                                         1, states.size(), vmax, amax, jmax, &o, &h);
  if (rc != CCMP_OK) return rc;
  JerkSetpoints s;
  size_t ticks = 0;
  try {
    rc = ccmp_jerk_setpoints_info(h, nullptr, &ticks);
    s.q.resize(ticks);
    s.qd.resize(ticks);
    s.tau.resize(ticks);
    s.clearance.resize(ticks);
    s.f.resize(ticks);
    s.satisfied.resize(ticks);
  } catch (...) {
    rc = CCMP_ENOMEM;
  }
  int32_t counts[2] = {0, 0};
  if (rc == CCMP_OK)
    rc = ccmp_jerk_setpoints_copy_host(h, ticks ? s.q[0].data() : nullptr, ticks ? s.qd[0].data() : nullptr, ticks ? s.tau.data() : nullptr, nullptr,
                                       ticks ? s.f[0].data() : nullptr, ticks ? s.satisfied.data() : nullptr, ticks ? s.clearance.data() : nullptr, &s.status,
                                       &s.window, &s.passes, s.peak, s.peak_tick, counts);
  ccmp_jerk_setpoints_destroy(h);
  if (rc != CCMP_OK) return rc;
  s.n_off = counts[0];
  s.n_below = counts[1];
  *out = std::move(s);
  return CCMP_OK;
}

// ---- the device-resident roadmap (include/ccmp.h: ccmp_roadmap_*) ------------------------------------------------------------------
// The object pose of a vertex as the store keeps it (x y z qx qy qz qw pad) from any state type that offers getX / getY / getZ and
// rotation().x / y / z / w — ompl::base::SE3StateSpace::StateType, i.e. components[1] of the reference's compound states.
template <class SE3State>
inline void poseOf(const SE3State &s, double pose[8])
{
  pose[0] = s.getX();
  pose[1] = s.getY();
  pose[2] = s.getZ();
  pose[3] = s.rotation().x;
  pose[4] = s.rotation().y;
  pose[5] = s.rotation().z;
  pose[6] = s.rotation().w;
  pose[7] = 0.0;
}
// obj_space_->distance(a, b) of the reference's tree metric (stefanBiPRM.h:194-201) on two such states: host arithmetic, no device
template <class SE3State>
inline double poseDistance(const SE3State &a, const SE3State &b)
{
  double pa[8], pb[8];
  poseOf(a, pa);
  poseOf(b, pb);
  return ccmp_pose_distance(pa, pb);
}

// The planner's tree_ on the device: joints and object pose of every vertex, appended one at a time, ranked on the reference's own
// metric (CCMP_METRIC_OBJECT) or on the joint distance (CCMP_METRIC_JOINT).  Replaces tree_->add (append), tree_->remove of the vertex
// just added (truncate: ONLY the tail can go) and connectionStrategy_ (nearestK).  The reference queries BEFORE it adds — tree_->add(m)
// follows the neighbour loop and only on success (stefanBiPRM.cpp:410,476; growTree :361) — so a query never sees the new vertex; a
// caller that appends first passes mode = CCMP_KNN_NOT_SELF and self_base = the new index, or the vertex is its own nearest neighbour.  Never throws: every verb returns false when it
// failed and the FIRST failure stays in lastError() / lastErrorMessage() until clearError().  Host pointers throughout; the calls
// take the Projector's mutex and upload only what is new.  The Projector must outlive the Roadmap.
class Roadmap {
public:
  explicit Roadmap(const Projector &proj, size_t capacity_hint = 0) noexcept : proj_(proj)
  {
    std::lock_guard<std::mutex> hold(proj_.mutex());
    rm_ = ccmp_roadmap_create(proj_.ctx(), capacity_hint);
    if (!rm_) err_.record(CCMP_EHIP, "ccmp_roadmap_create");
  }
  ~Roadmap()
  {
    if (!rm_) return;
    std::lock_guard<std::mutex> hold(proj_.mutex());
    ccmp_roadmap_destroy(rm_);
  }
  Roadmap(const Roadmap &) = delete;
  Roadmap &operator=(const Roadmap &) = delete;

  size_t size() const noexcept { return ccmp_roadmap_size(rm_); }
  bool reserve(size_t n) noexcept { return call([&] { return ccmp_roadmap_reserve(rm_, n); }, "ccmp_roadmap_reserve"); }
  // n vertices: joints [n][14] and / or poses [n][8].  poses == nullptr: derived on the device from the joints; joints == nullptr:
  // growTree's pose-only vertices (stefanBiPRM.cpp:283-292), no joint-metric neighbour of anything until setJoints.  *first = index of the first
  bool append(const double *joints, const double *poses, size_t n = 1, size_t *first = nullptr) noexcept
  {
    return call([&] { return ccmp_roadmap_append_host(rm_, &proj_.problem(), joints, poses, n, first); }, "ccmp_roadmap_append_host");
  }
  bool setJoints(size_t index, const double *joints14) noexcept
  {
    return call([&] { return ccmp_roadmap_set_joints_host(rm_, index, joints14); }, "ccmp_roadmap_set_joints_host");
  }
  // remove_vertex(t) of the vertex just appended (stefanBiPRM.cpp:353-359): drops the vertices from index n on
  bool truncate(size_t n) noexcept { return call([&] { return ccmp_roadmap_truncate(rm_, n); }, "ccmp_roadmap_truncate"); }
  bool read(size_t first, size_t count, double *joints, double *poses) const noexcept
  {
    return call([&] { return ccmp_roadmap_read_host(rm_, first, count, joints, poses); }, "ccmp_roadmap_read_host");
  }
  // connectionStrategy_(m): the k nearest vertices of ONE query (a pose [8] under CCMP_METRIC_OBJECT, joints [14] under
  // CCMP_METRIC_JOINT), nearest first, ties to the lower index; idx / dist (nullable) get k entries, -1 / +inf where fewer exist
  bool nearestK(int metric, const double *query, unsigned k, std::vector<int32_t> *idx, std::vector<double> *dist = nullptr, int mode = CCMP_KNN_ALL,
                size_t self_base = 0) const noexcept
  {
    try {
      idx->assign(k, -1);
      if (dist) dist->assign(k, 0.0);
    } catch (...) {
      err_.record(CCMP_ENOMEM, "Roadmap::nearestK");
      return false;
    }
    return call([&] { return ccmp_roadmap_knn_host(rm_, metric, query, 1, (int)k, mode, self_base, idx->data(), dist ? dist->data() : nullptr); },
                "ccmp_roadmap_knn_host");
  }
  // neighbours and checkMotion (check_target) / discreteGeodesic of all of them towards ONE query in one call (ccmp_roadmap_connect_host):
  // the raw outputs of ccmp_connect_host for k edges — n_states, ok [k], states [k][max_states][14].  query_pose may be nullptr (derived).
  bool connect(int metric, const double *query_joints, const double *query_pose, unsigned k, bool check_target, int max_states, std::vector<int32_t> *idx,
               std::vector<int32_t> *n_states, std::vector<uint8_t> *ok, std::vector<double> *states, const ccmp_scene *scene = nullptr,
               double margin = 0.0, int mode = CCMP_KNN_ALL, size_t self_base = 0) const noexcept
  {
    if (!resetSlots("Roadmap::connect", k, max_states, idx, n_states, ok, states)) return false;
    return call([&] {
      return ccmp_roadmap_connect_host(rm_, &proj_.problem(), scene, margin, metric, query_joints, query_pose, 1, (int)k, mode, self_base, check_target ? 1 : 0,
                                       max_states, 0, idx->data(), nullptr, states->data(), n_states->data(), ok->data(), nullptr, nullptr, nullptr);
    }, "ccmp_roadmap_connect_host");
  }

  // growTree's device part for ONE object pose in one call (ccmp_roadmap_grow_host; stefanBiPRM.cpp:283-351): the k pose-nearest
  // vertices, Projector::sampleCalibGoal's rule over their joints as seeds in rank order, then discreteGeodesic (check_target:
  // checkMotion) from every neighbour to the new state.  idx [k], q_new14 [14], *ik_which (nullable) = the neighbour slot whose joints
  // seeded the state, n_states / ok [k], states [k][max_states][14] as connect() reports them; a pose without a state gives NaN joints,
  // *ik_which = -1 and empty slots.  Returns true when the call ran AND a state was found; a failed call leaves q_new14 NaN-filled and
  // the error in lastError().  It does not append: the reference adds the vertex only after an edge succeeded (:361).  The restarts'
  // stream is the Projector's (setIkStream).
  bool grow(const double *pose8, unsigned k, int max_states, std::vector<int32_t> *idx, double *q_new14, int *ik_which, std::vector<int32_t> *n_states,
            std::vector<uint8_t> *ok, std::vector<double> *states, bool check_target = false, const ccmp_scene *scene = nullptr, double margin = 0.0,
            int mode = CCMP_KNN_ALL, size_t self_base = 0) const noexcept
  {
    return growWith(false, nullptr, pose8, k, max_states, idx, q_new14, ik_which, n_states, ok, states, check_target, scene, margin, mode, self_base);
  }

  // grow() with the vetted IK (ccmp_roadmap_grow_vetted_host): `scene` (required; ProxyScene::handle()) stands where the reference has
  // IKValid inside sampleCalibGoal and si_->isValid(result) behind it, and serves the traversals too, all under the one `margin`.  With
  // vet = false this is grow() above with the scene on the traversals alone.  *ik_clearance (nullable): the new state's clearance, NaN
  // without one.  Proxies, not MoveIt: the caller's exact validity test of the new state stays.  Same outputs, stream and error rules.
  bool grow(const double *pose8, unsigned k, int max_states, std::vector<int32_t> *idx, double *q_new14, int *ik_which, std::vector<int32_t> *n_states,
            std::vector<uint8_t> *ok, std::vector<double> *states, const ccmp_scene *scene, double margin, bool vet, double *ik_clearance = nullptr,
            bool check_target = false, int mode = CCMP_KNN_ALL, size_t self_base = 0) const noexcept
  {
    detail::fillNaN(ik_clearance, 1);
    return growWith(vet, vet ? ik_clearance : nullptr, pose8, k, max_states, idx, q_new14, ik_which, n_states, ok, states, check_target, scene, margin, mode,
                    self_base);
  }

  // ---- the graph (include/ccmp.h: ccmp_roadmap_commit / _add_edges / _closest) --------------------------------------------------------
  // What growTree does with grow()'s outputs (stefanBiPRM.cpp:303-372 and milestonesToAdd), for ONE pose: idx / ok / n_states / states
  // as grow() or connect() left them, the new state's joints and pose, the planner's goal pose (nullptr: no mid-stones) and startM_
  // (roots).  Returns the GrowState (CCMP_GROW_*); CCMP_GROW_TRAPPED when the call failed (the error in lastError()).  *new_index
  // (nullable): the new vertex or -1; *mid_index (nullable): k entries, the mid-stone of every slot or -1.  keep_isolated:
  // startgoalMilestone's vertex, which stays without an edge.  have_state = false: the IK found no state (vertex_ok = 0).
  int commit(const std::vector<int32_t> &idx, const std::vector<uint8_t> &ok, const std::vector<int32_t> &n_states, const std::vector<double> *states,
             int max_states, const double *q_new14, const double *pose8, const double *goal_pose8, const std::vector<int32_t> &roots,
             int32_t *new_index = nullptr, std::vector<int32_t> *mid_index = nullptr, bool keep_isolated = false, bool have_state = true) noexcept
  {
    const size_t k = idx.size();
    int32_t t = -1, state = CCMP_GROW_TRAPPED;
    std::vector<int32_t> mids;
    if (new_index) *new_index = -1;
    try {
      mids.assign(k, -1);
      if (mid_index) mid_index->assign(k, -1);
    } catch (...) {
      err_.record(CCMP_ENOMEM, "Roadmap::commit");
      return CCMP_GROW_TRAPPED;
    }
    if (ok.size() != k || n_states.size() != k || (states && states->size() < k * (size_t)(max_states > 0 ? max_states : 0) * 14)) {
      err_.record(CCMP_EINVAL, "Roadmap::commit");
      return CCMP_GROW_TRAPPED;
    }
    const uint8_t vertex_ok = have_state ? 1 : 0;
    const bool ran = call([&] {
      return ccmp_roadmap_commit_host(rm_, &proj_.problem(), idx.data(), ok.data(), n_states.data(), states ? states->data() : nullptr, max_states, q_new14,
                                      pose8, &vertex_ok, 1, (int)k, goal_pose8, roots.data(), (int)roots.size(),
                                      keep_isolated ? (unsigned int)CCMP_COMMIT_KEEP_ISOLATED : 0u, &t, mids.data(), &state, nullptr, nullptr);
    }, "ccmp_roadmap_commit_host");
    if (!ran) return CCMP_GROW_TRAPPED;
    if (new_index) *new_index = t;
    if (mid_index) mid_index->swap(mids);
    return state;
  }
  // explicit edges uv [n][2] between existing vertices, weighted by the joint distance on the device
  bool addEdges(const int32_t *uv, size_t n = 1) noexcept { return call([&] { return ccmp_roadmap_add_edges_host(rm_, uv, n); }, "ccmp_roadmap_add_edges_host"); }
  size_t numEdges() const noexcept { return ccmp_roadmap_num_edges(rm_); }
  bool readEdges(size_t first, size_t count, int32_t *uv, double *w) const noexcept
  {
    return call([&] { return ccmp_roadmap_read_edges_host(rm_, first, count, uv, w); }, "ccmp_roadmap_read_edges_host");
  }
  bool readLabels(size_t first, size_t count, int32_t *labels) const noexcept
  {
    return call([&] { return ccmp_roadmap_read_labels_host(rm_, first, count, labels); }, "ccmp_roadmap_read_labels_host");
  }
  // closestFromGoal's vertex scan for every `from` (at most CCMP_CLOSEST_MAX_FROM): the vertex of from's component nearest to
  // target_pose8 by (distance, index), its distance, and from's own distance (nullable); false and -1 / +inf / NaN when the call failed
  bool closest(const std::vector<int32_t> &froms, const double *target_pose8, std::vector<int32_t> *idx, std::vector<double> *dist,
               std::vector<double> *from_dist = nullptr) const noexcept
  {
    std::vector<double> fd;
    try {
      idx->assign(froms.size(), -1);
      dist->assign(froms.size(), std::numeric_limits<double>::infinity());
      fd.assign(froms.size(), std::numeric_limits<double>::quiet_NaN());
      if (from_dist) *from_dist = fd;
    } catch (...) {
      err_.record(CCMP_ENOMEM, "Roadmap::closest");
      return false;
    }
    const bool ran = call([&] { return ccmp_roadmap_closest_host(rm_, froms.data(), froms.size(), target_pose8, idx->data(), dist->data(), fd.data()); },
                          "ccmp_roadmap_closest_host");
    if (ran && from_dist) from_dist->swap(fd);
    return ran;
  }
  // ---- the solution step (include/ccmp.h: ccmp_roadmap_shortest_paths) ----------------------------------------------------------------
  // The cheapest path src -> dst on the store's graph, on the device: path = its vertex indices, start first, cost = the sum of its
  // weights (ties: the fewest hops, then the smallest predecessor — csrc/ccmp_path.h; not boost's A*, whose heuristic here is not
  // admissible).  states (nullable) = the joint rows of those vertices.  false with an empty path and cost +inf when dst cannot be
  // reached OR the call failed (the error in lastError()).
  bool shortestPath(int32_t src, int32_t dst, std::vector<int32_t> &path, double &cost, std::vector<std::array<double, 14>> *states = nullptr) const noexcept
  {
    cost = std::numeric_limits<double>::infinity();
    path.clear();
    if (states) states->clear();
    int32_t len = 0;
    double c = cost;
    std::vector<double> rows;
    try {
      for (int room = 64, tries = 0; tries < 2; tries++) { // a path that did not fit reports its length: once more with that room
        path.assign((size_t)room, -1);
        rows.assign(states ? (size_t)room * 14 : 0, 0.0);
        const bool ran = call([&] { return ccmp_roadmap_shortest_paths_host(rm_, &src, &dst, 1, room, &c, &len, path.data(), states ? rows.data() : nullptr, nullptr, nullptr, nullptr); },
                              "ccmp_roadmap_shortest_paths_host");
        if (!ran) { path.clear(); return false; }
        if (len <= room) break;
        room = len;
      }
      path.resize((size_t)len);
      if (states) {
        states->resize((size_t)len);
        for (size_t i = 0; i < (size_t)len; i++) std::memcpy((*states)[i].data(), rows.data() + i * 14, 14 * sizeof(double));
      }
    } catch (...) {
      err_.record(CCMP_ENOMEM, "Roadmap::shortestPath");
      path.clear();
      return false;
    }
    cost = c;
    return len > 0;
  }
  // maybeConstructSolution (stefanBiPRM.cpp:480-603): of the pairs (start, goal) in one component, the cheapest path's joint states, start
  // first — what PathGeometric::append takes; constructDenseSolution below adds PathGeometric::interpolate.  The first
  // pair in starts-major order wins a tie.  false with no states when no pair is connected (at most CCMP_PATH_MAX_PAIRS connected pairs are
  // considered) OR a call failed (lastError()).  cost / indices (nullable) = the path's cost and vertices.
  bool constructSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states, double *cost = nullptr,
                         std::vector<int32_t> *indices = nullptr) const noexcept
  {
    states.clear();
    if (indices) indices->clear();
    if (cost) *cost = std::numeric_limits<double>::infinity();
    try {
      const size_t N = size();
      std::vector<int32_t> lab(N), src, dst;
      if (N == 0 || !readLabels(0, N, lab.data())) return false;
      for (int32_t s : starts)
        for (int32_t g : goals)
          if (s >= 0 && g >= 0 && (size_t)s < N && (size_t)g < N && lab[(size_t)s] == lab[(size_t)g] && src.size() < (size_t)CCMP_PATH_MAX_PAIRS) {
            src.push_back(s);
            dst.push_back(g);
          }
      const size_t F = src.size();
      if (F == 0) return false;
      std::vector<double> c(F), rows;
      std::vector<int32_t> len(F), path;
      int room = 64;
      for (int tries = 0; tries < 2; tries++) {
        path.assign(F * (size_t)room, -1);
        rows.assign(F * (size_t)room * 14, 0.0);
        if (!call([&] { return ccmp_roadmap_shortest_paths_host(rm_, src.data(), dst.data(), F, room, c.data(), len.data(), path.data(), rows.data(), nullptr, nullptr, nullptr); },
                  "ccmp_roadmap_shortest_paths_host")) return false;
        const int longest = *std::max_element(len.begin(), len.end());
        if (longest <= room) break;
        room = longest;
      }
      size_t best = F;
      for (size_t f = 0; f < F; f++)
        if (len[f] > 0 && (best == F || c[f] < c[best])) best = f;
      if (best == F) return false;
      states.resize((size_t)len[best]);
      for (size_t i = 0; i < states.size(); i++) std::memcpy(states[i].data(), rows.data() + (best * (size_t)room + i) * 14, 14 * sizeof(double));
      if (indices) indices->assign(path.begin() + (std::ptrdiff_t)(best * (size_t)room), path.begin() + (std::ptrdiff_t)(best * (size_t)room + states.size()));
      if (cost) *cost = c[best];
      return true;
    } catch (...) {
      err_.record(CCMP_ENOMEM, "Roadmap::constructSolution");
      states.clear();
      return false;
    }
  }
  // constructSolution followed by PathGeometric::interpolate (ccmp::densifyPathLocked above): `states` = the dense path, in the layout
  // ccmp::printAsMatrix writes as the reference's <obj>_path.txt, or with `distinct` without the repeated waypoint rows.  seg_ok (nullable)
  // = one flag per segment of the waypoint path; delta / lambda > 0 replace the problem's (pass the OMPL space's getDelta() / getLambda()).
  // false with no states when no pair is connected OR a call failed (lastError()).
  bool constructDenseSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states,
                              bool distinct = false, double *cost = nullptr, std::vector<int32_t> *indices = nullptr, std::vector<uint8_t> *seg_ok = nullptr,
                              double delta = 0.0, double lambda = 0.0) const noexcept
  {
    if (seg_ok) seg_ok->clear();
    if (!constructSolution(starts, goals, states, cost, indices)) return false;
    const bool ran = call([&] { return densifyPathLocked(proj_, states, distinct, seg_ok, delta, lambda); }, "ccmp_path_densify_host");
    if (!ran) {
      states.clear();
      if (indices) indices->clear();
      if (cost) *cost = std::numeric_limits<double>::infinity();
    }
    return ran;
  }

  // constructSolution followed by the removal of interior vertices (ccmp::shortcutPathLocked above): `states` = the kept waypoints, cost =
  // their joint length, indices = their vertices.  On a library error in the shortcut step the answer is the UNCHANGED solution path (true,
  // with lastError() set): a planner that cannot simplify still has its path.  false with no states when no pair is connected or the
  // solution step itself failed.  Interpolate the result (ccmp::densifyPathLocked) and validate the dense rows on the host.
  bool constructShortcutSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states,
                                 int max_span = 0, double *cost = nullptr, std::vector<int32_t> *indices = nullptr, double delta = 0.0,
                                 double lambda = 0.0) const noexcept
  {
    std::vector<int32_t> path;
    if (!constructSolution(starts, goals, states, cost, &path)) {
      if (indices) indices->clear();
      return false;
    }
    try {
      std::vector<int32_t> kept;
      double co = 0.0;
      if (call([&] { return shortcutPathLocked(proj_, states, max_span, &kept, nullptr, &co, delta, lambda); }, "ccmp_path_shortcut_host")) {
        std::vector<int32_t> idx(kept.size());
        for (size_t k = 0; k < kept.size(); k++) idx[k] = path[(size_t)kept[k]];
        path.swap(idx);
        if (cost) *cost = co;
      }
      if (indices) indices->swap(path);
    } catch (...) {
      err_.record(CCMP_ENOMEM, "Roadmap::constructShortcutSolution");
      if (indices) indices->clear();
    }
    return true;
  }

  // constructShortcutSolution followed by smoothing passes (ccmp::smoothPathLocked above): `states` = the smoothed path, cost = its joint
  // length, indices = the vertices the shortcut kept (the smoothed vertices between the first and the last are not roadmap vertices).  On
  // a library error in the smoothing step the answer is the UNCHANGED shortcut path (true, with lastError() set).  false with no states
  // when no pair is connected or the solution step itself failed.  Interpolate the result and validate the dense rows on the host.
  bool constructSmoothSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states,
                               int max_steps = 5, double min_change = 0.005, int max_span = 0, double *cost = nullptr,
                               std::vector<int32_t> *indices = nullptr, double delta = 0.0, double lambda = 0.0) const noexcept
  {
    if (!constructShortcutSolution(starts, goals, states, max_span, cost, indices, delta, lambda)) return false;
    double lo = 0.0;
    if (call([&] { return smoothPathLocked(proj_, states, max_steps, min_change, nullptr, nullptr, nullptr, nullptr, &lo, delta, lambda); },
             "ccmp_path_smooth_host")) {
      if (cost) *cost = lo;
    }
    return true;
  }

  // constructSmoothSolution followed by the resampling at even arc and the time stamps (ccmp::resamplePathLocked, ccmp::timestampPath
  // above): `states` = the resampled rows, `times` = one per row, cost = the duration.  On a library error in either step — or a path the
  // resampling gives no rows for — the answer FALLS BACK to the smooth solution without times (true, `times` empty, cost = the smoothed
  // length, lastError() set on an error).  false with no states when no pair is connected or the solution step itself failed.  The
  // resampled rows are new states: validate them on the host before the times are used.
  bool constructTimedSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states,
                              std::vector<double> &times, const double *vmax, const double *amax, double beta = 0.5, int count = 0, double spacing = 0.0,
                              int max_steps = 5, double min_change = 0.005, int max_span = 0, double *cost = nullptr,
                              std::vector<int32_t> *indices = nullptr, double delta = 0.0, double lambda = 0.0) const noexcept
  {
    times.clear();
    if (!constructSmoothSolution(starts, goals, states, max_steps, min_change, max_span, cost, indices, delta, lambda)) return false;
    try {
      std::vector<std::array<double, 14>> rows(states);
      std::vector<double> t;
      int status = CCMP_RETIME_EMPTY;
      double total = 0.0;
      if (call([&] { return resamplePathLocked(proj_, rows, count, spacing, &status, nullptr, delta, lambda); }, "ccmp_path_resample") &&
          (status == CCMP_RETIME_OK || status == CCMP_RETIME_POINT) &&
          call([&] { return timestampPath(proj_, rows, vmax, amax, beta, &t, &total); }, "ccmp_path_timestamps_host")) {
        states.swap(rows);
        times.swap(t);
        if (cost) *cost = total;
      }
    } catch (...) {
      err_.record(CCMP_ENOMEM, "Roadmap::constructTimedSolution");
    }
    return true;
  }

  // constructTimedSolution followed by the setpoints of its rows at the controller's period and their audit (ccmp::setpointPath above):
  // what is executed, and what that motion does between the rows.  On a library error in that step — or a solution that came back
  // without times — the answer FALLS BACK to the timed solution with `setpoints` empty (true, status CCMP_SETPOINTS_EMPTY, lastError() set
  // on an error).  false with no states when no pair is connected or the solution step itself failed.
  bool constructExecutableSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states,
                                   std::vector<double> &times, Setpoints &setpoints, const double *vmax, const double *amax, double period = 0.001,
                                   int max_ticks = 65536, const ccmp_scene *scene = nullptr, double margin = 0.0, double beta = 0.5, int count = 0,
                                   double spacing = 0.0, int max_steps = 5, double min_change = 0.005, int max_span = 0, double *cost = nullptr,
                                   std::vector<int32_t> *indices = nullptr, double delta = 0.0, double lambda = 0.0) const noexcept
  {
    setpoints = Setpoints();  // (empty vectors: nothing is allocated)
    if (!constructTimedSolution(starts, goals, states, times, vmax, amax, beta, count, spacing, max_steps, min_change, max_span, cost, indices, delta, lambda))
      return false;
    if (times.size() == states.size() && !states.empty())
      call([&] { return setpointPath(proj_, states, times, vmax, amax, &setpoints, period, max_ticks, scene, margin); }, "ccmp_path_setpoints_host");
    return true;
  }

  // The same with the fit between the time stamps and the setpoints (ccmp::fitPath above): `times` = the FITTED stamps, `fitted` = the
  // fit's answer, the setpoints those of the fitted stamps (period and max_ticks are the fit options').  On a library error in the fit the
  // answer FALLS BACK to the time-stamp rule's stamps and their setpoints (`fitted` as constructed, lastError() set).
  bool constructExecutableSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states,
                                   std::vector<double> &times, Setpoints &setpoints, FittedTimes &fitted, const FitOptions &fit, const double *vmax,
                                   const double *amax, const ccmp_scene *scene = nullptr, double margin = 0.0, double beta = 0.5, int count = 0,
                                   double spacing = 0.0, int max_steps = 5, double min_change = 0.005, int max_span = 0, double *cost = nullptr,
                                   std::vector<int32_t> *indices = nullptr, double delta = 0.0, double lambda = 0.0) const noexcept
  {
    setpoints = Setpoints();
    fitted = FittedTimes();
    if (!constructTimedSolution(starts, goals, states, times, vmax, amax, beta, count, spacing, max_steps, min_change, max_span, cost, indices, delta, lambda))
      return false;
    if (times.size() == states.size() && !states.empty()) {
      if (call([&] { return fitPath(proj_, states, times, vmax, amax, &fitted, fit); }, "ccmp_path_fit_timestamps_host") && fitted.times.size() == times.size()) {
        times = fitted.times;  // (same size: no allocation)
        if (cost) *cost = fitted.duration;
      }
      call([&] { return setpointPath(proj_, states, times, vmax, amax, &setpoints, fit.period, fit.max_ticks, scene, margin); }, "ccmp_path_setpoints_host");
    }
    return true;
  }

  // constructTimedSolution followed by the JERK-BOUNDED setpoints of its rows (ccmp::jerkSetpointPath above) for a controller that limits
  // jerk: jmax = 14 numbers, the period, tick bound and window search are the JerkOptions'.  `fit` non-null: the stamps go through the
  // fit first (its period and max_ticks should be the JerkOptions'), `times` = the fitted stamps and *fitted (nullable) = the fit's answer;
  // on a library error in the fit the answer falls back to the time-stamp rule's stamps.  On a library error in the setpoints step the
  // answer FALLS BACK to the timed solution with `setpoints` empty (true, status CCMP_JERK_EMPTY, lastError() set).
  bool constructExecutableSolution(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, std::vector<std::array<double, 14>> &states,
                                   std::vector<double> &times, JerkSetpoints &setpoints, const double *vmax, const double *amax, const double *jmax,
                                   const JerkOptions &jerk = JerkOptions(), const FitOptions *fit = nullptr, FittedTimes *fitted = nullptr,
                                   const ccmp_scene *scene = nullptr, double margin = 0.0, double beta = 0.5, int count = 0, double spacing = 0.0,
                                   int max_steps = 5, double min_change = 0.005, int max_span = 0, double *cost = nullptr,
                                   std::vector<int32_t> *indices = nullptr, double delta = 0.0, double lambda = 0.0) const noexcept
  {
    setpoints = JerkSetpoints();
    if (fitted) *fitted = FittedTimes();
    if (!constructTimedSolution(starts, goals, states, times, vmax, amax, beta, count, spacing, max_steps, min_change, max_span, cost, indices, delta, lambda))
      return false;
    if (times.size() == states.size() && !states.empty()) {
      if (fit) {
        FittedTimes answer;
        if (call([&] { return fitPath(proj_, states, times, vmax, amax, &answer, *fit); }, "ccmp_path_fit_timestamps_host") && answer.times.size() == times.size()) {
          times = answer.times;  // (same size: no allocation)
          if (cost) *cost = answer.duration;
          if (fitted) *fitted = std::move(answer);
        }
      }
      call([&] { return jerkSetpointPath(proj_, states, times, vmax, amax, jmax, &setpoints, jerk, scene, margin); }, "ccmp_path_jerk_setpoints_host");
    }
    return true;
  }

  // stefanBiPRM::solve on this store in one call (ccmp::Planner below: open, then up to max_cycles cycles): the status (CCMP_PLAN_*) and,
  // when it is CCMP_PLAN_SOLVED, the connected (start vertex, goal vertex) in *start / *goal — the path is shortestPaths' on that pair.
  // object: ObjectChecker::handle(); scene: ProxyScene::handle() or nullptr; goal_joints14: the goal state, or nullptr for the pose IK
  // towards the problem's goal pose.  -1 when a call failed (the error in lastError()).
  int solve(const ccmp_object *object, int max_cycles, int32_t *start = nullptr, int32_t *goal = nullptr, const ccmp_plan_opts *opts = nullptr,
            const ccmp_scene *scene = nullptr, double margin = 0.0, const double *goal_joints14 = nullptr, uint64_t rng_seed = 0,
            ccmp_plan_report *report = nullptr) noexcept;

  // RRT-Connect on this store in one call (ccmp::RRTConnectPlanner below: open on the given start and goal vertices, then up to
  // max_cycles cycles): the status (CCMP_RRTC_*) and, when it is CCMP_RRTC_SOLVED, the connected pair in *start / *goal — the path is
  // shortestPaths' on that pair.  No object checker and no IK; scene: ProxyScene::handle() or nullptr.  -1 when a call failed.
  int solveRRTConnect(const int32_t *starts, int n_starts, const int32_t *goals, int n_goals, int max_cycles, int32_t *start = nullptr, int32_t *goal = nullptr,
                      const ccmp_rrtc_opts *opts = nullptr, const ccmp_scene *scene = nullptr, double margin = 0.0, uint64_t rng_seed = 0,
                      ccmp_rrtc_report *report = nullptr) noexcept;

  int lastError() const noexcept { return err_.code(); }
  std::string lastErrorMessage() const { return err_.message(); }
  void clearError() noexcept { err_.clear(); }
  ccmp_roadmap *handle() const noexcept { return rm_; }
  const Projector &projector() const noexcept { return proj_; }

private:
  template <class F>
  bool call(F &&body, const char *what) const noexcept
  {
    return detail::guardedCall(rm_ != nullptr, proj_.mutex(), err_, what, std::forward<F>(body));
  }
  // connect's and grow's outputs for k slots, empty; false (CCMP_ENOMEM under the verb's name) when they cannot be had
  bool resetSlots(const char *verb, unsigned k, int max_states, std::vector<int32_t> *idx, std::vector<int32_t> *n_states, std::vector<uint8_t> *ok,
                  std::vector<double> *states) const noexcept
  {
    try {
      idx->assign(k, -1);
      n_states->assign(k, 0);
      ok->assign(k, 0);
      states->assign((size_t)k * (size_t)(max_states > 0 ? max_states : 0) * 14, 0.0);
      return true;
    } catch (...) {
      err_.record(CCMP_ENOMEM, verb);
      return false;
    }
  }
  // both grow() forms: vet chooses ccmp_roadmap_grow_vetted_host, which alone writes *ik_clearance (nullable)
  bool growWith(bool vet, double *ik_clearance, const double *pose8, unsigned k, int max_states, std::vector<int32_t> *idx, double *q_new14, int *ik_which,
                std::vector<int32_t> *n_states, std::vector<uint8_t> *ok, std::vector<double> *states, bool check_target, const ccmp_scene *scene,
                double margin, int mode, size_t self_base) const noexcept
  {
    uint8_t ik_ok = 0;
    int32_t slot = -1;
    detail::fillNaN(q_new14);
    if (ik_which) *ik_which = -1;
    if (!resetSlots("Roadmap::grow", k, max_states, idx, n_states, ok, states)) return false;
    const bool ran = call([&] {
      const int target = check_target ? 1 : 0;
      const int rc = vet ? ccmp_roadmap_grow_vetted_host(rm_, &proj_.problem(), scene, margin, &proj_.ikOptions(), pose8, 1, (int)k, mode, self_base,
                                                         proj_.ikSeed(), proj_.ikNextIndex(), target, max_states, 0, idx->data(), nullptr, q_new14, &ik_ok,
                                                         &slot, ik_clearance, states->data(), n_states->data(), ok->data(), nullptr, nullptr, nullptr)
                         : ccmp_roadmap_grow_host(rm_, &proj_.problem(), scene, margin, &proj_.ikOptions(), pose8, 1, (int)k, mode, self_base, proj_.ikSeed(),
                                                  proj_.ikNextIndex(), target, max_states, 0, idx->data(), nullptr, q_new14, &ik_ok, &slot, states->data(),
                                                  n_states->data(), ok->data(), nullptr, nullptr, nullptr);
      if (rc == CCMP_OK) (void)proj_.takeIkIndex();
      return rc;
    }, vet ? "ccmp_roadmap_grow_vetted_host" : "ccmp_roadmap_grow_host");
    if (!ran) {
      detail::fillNaN(q_new14);
      detail::fillNaN(ik_clearance, 1);
      return false;
    }
    if (ik_which) *ik_which = slot;
    return ik_ok != 0;
  }
  const Projector &proj_;
  ccmp_roadmap *rm_ = nullptr;
  mutable detail::ErrorLatch err_;
};

// ---- the head of growTree (include/ccmp.h: ccmp_object_*) ---------------------------------------------------------------------------
// stefan_checker_ (stefanFCL: the object's triangle mesh against the static workspace boxes) with its questions, and the two places the
// planner asks them from: the head of growTree() (stefanBiPRM.cpp:255-276: interpolate 30 % towards the goal, draw around that, ask, two
// attempts — propose) and checkForSolution's ladder (:733-752 — ladder).  The mesh ([M][9], object frame) and the boxes (half extents) are
// the caller's.  The mesh test is this library's exact separating-axis test, not FCL; the draw is its counter-based Gaussian, not OMPL's
// RNG (csrc/ccmp_object.h).  Never throws: every question answers "no" (false / 0) when the call failed, and the FIRST failure stays in
// lastError() / lastErrorMessage() until clearError(), as Projector::sampleCalibGoal does.  Host pointers throughout.  Built on a
// Projector (its context and its mutex; it must outlive the checker) or on a bare context.
class ObjectChecker {
public:
  ObjectChecker(const Projector &proj, const double *tri, int M, const ccmp_box *boxes, int n_boxes) noexcept : ctx_(proj.ctx()), mu_(&proj.mutex())
  {
    create(tri, M, boxes, n_boxes);
  }
  ObjectChecker(ccmp_ctx *ctx, const double *tri, int M, const ccmp_box *boxes, int n_boxes) noexcept : ctx_(ctx), mu_(&own_mu_)
  {
    create(tri, M, boxes, n_boxes);
  }
  ~ObjectChecker()
  {
    if (!obj_) return;
    std::lock_guard<std::mutex> hold(*mu_);
    ccmp_object_destroy(obj_);
  }
  ObjectChecker(const ObjectChecker &) = delete;
  ObjectChecker &operator=(const ObjectChecker &) = delete;

  // the half extents of every box grow by this much in every question (0 by default)
  void setInflate(double inflate) noexcept { inflate_ = inflate; }
  // position bounds of propose's draw (the planner's object space bounds; unbounded by default)
  void setBounds(const double lo[3], const double hi[3]) noexcept
  {
    for (int i = 0; i < 3; i++) { lo_[i] = lo[i]; hi_[i] = hi[i]; }
  }
  // the draws' stream: propose number n of this checker uses index first_index + n (as every OMPL sampler owns its RNG)
  void setStream(uint64_t seed, uint64_t first_index = 0) noexcept { seed_ = seed; next_ = first_index; }
  uint64_t nextIndex() const noexcept { return next_; }

  // stefanFCL::isValid on a pose row (x y z qx qy qz qw pad)
  bool isValidPose(const double pose8[8]) const noexcept
  {
    uint8_t valid = 0;
    const bool ran = call([&] { return ccmp_object_valid_host(ctx_, obj_, pose8, 1, inflate_, &valid, nullptr); }, "ccmp_object_valid_host");
    return ran && valid != 0;
  }
  // stefanFCL::isValid(Eigen::Isometry3d): any type with linear()(r, c) and translation()(i).  The rotation goes through Eigen's
  // Quaterniond(Matrix3d) arithmetic (ccmp_pose_from_t_wo), the inverse of the StateToIsometry that produced it (utils.h:22)
  template <class Isometry>
  bool isValid(const Isometry &T) const noexcept
  {
    double t_wo[12], pose[8];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) t_wo[3 * r + c] = T.linear()(r, c);
      t_wo[9 + r] = T.translation()(r);
    }
    ccmp_pose_from_t_wo(t_wo, pose);
    return isValidPose(pose);
  }
  // stefanFCL::isValid(ob::State *): state->as<ob::SE3StateSpace::StateType>(), read by the adapter's poseOf
  template <class SE3State>
  bool isValid(const SE3State *state) const noexcept
  {
    double pose[8];
    poseOf(*state, pose);
    return isValidPose(pose);
  }
  template <class SE3State>
  bool isValid(SE3State *state) const noexcept { return isValid(static_cast<const SE3State *>(state)); }
  // stefanFCL::is_Valid(pos, quat): quat as x y z w
  bool is_Valid(const double pos[3], const double quat_xyzw[4]) const noexcept
  {
    const double pose[8] = {pos[0], pos[1], pos[2], quat_xyzw[0], quat_xyzw[1], quat_xyzw[2], quat_xyzw[3], 0.0};
    return isValidPose(pose);
  }
  // The head of growTree() for one nearest pose: out8 = the first of `attempts` candidates (interpolate from8 -> goal8 at t, then the
  // SE(3) Gaussian draw with sigma) whose mesh is free; *which (nullable) = its attempt.  false = TRAPPED (out8 NaN-filled, *which = -1)
  // or a failed call (the error in lastError()).  One index of the stream per call that ran.
  bool propose(const double from8[8], const double goal8[8], double out8[8], int *which = nullptr, double t = 0.3, double sigma = 0.2,
               int attempts = 2) noexcept
  {
    int32_t w = -1;
    detail::fillNaN(out8, 7);
    out8[7] = 0.0;
    if (which) *which = -1;
    const bool ran = call([&] {
      const int rc = ccmp_object_propose_host(ctx_, obj_, from8, goal8, 0, 1, t, sigma, lo_, hi_, attempts, seed_, next_, inflate_, out8, &w, nullptr, nullptr);
      if (rc == CCMP_OK) next_++;
      return rc;
    }, "ccmp_object_propose_host");
    if (!ran) {
      detail::fillNaN(out8, 7);
      return false;
    }
    if (which) *which = w;
    return w >= 0;
  }
  // checkForSolution's ladder: poses [steps][8] (nullable) = the interpolation from8 -> goal8 at 0.1 i, i = 1..steps; returns how many of
  // them are valid before the first one refused (0 also when the call failed)
  int ladder(const double from8[8], const double goal8[8], std::vector<double> *poses = nullptr, int steps = 9) const noexcept
  {
    if (steps < 1) return 0;
    std::vector<double> own;
    std::vector<uint8_t> valid;
    std::vector<double> *rows = poses ? poses : &own;
    try {
      rows->assign((size_t)steps * 8, 0.0);
      valid.assign((size_t)steps, 0);
    } catch (...) {
      err_.record(CCMP_ENOMEM, "ObjectChecker::ladder");
      return 0;
    }
    for (int i = 1; i <= steps; i++) ccmp_pose_interpolate(from8, goal8, 0.1 * i, rows->data() + (size_t)(i - 1) * 8);
    if (!call([&] { return ccmp_object_valid_host(ctx_, obj_, rows->data(), (size_t)steps, inflate_, valid.data(), nullptr); }, "ccmp_object_valid_host")) return 0;
    int n = 0;
    while (n < steps && valid[(size_t)n]) n++;
    return n;
  }

  int numTriangles() const noexcept { return ccmp_object_num_triangles(obj_); }
  int lastError() const noexcept { return err_.code(); }
  std::string lastErrorMessage() const { return err_.message(); }
  void clearError() noexcept { err_.clear(); }
  ccmp_object *handle() const noexcept { return obj_; }

private:
  void create(const double *tri, int M, const ccmp_box *boxes, int n_boxes) noexcept
  {
    for (int i = 0; i < 3; i++) { lo_[i] = -1e30; hi_[i] = 1e30; }
    // (the library itself answers for a null context)
    if (!detail::guardedCall(true, *mu_, err_, "ccmp_object_create", [&] { return ccmp_object_create(ctx_, tri, M, boxes, n_boxes, &obj_); })) obj_ = nullptr;
  }
  template <class F>
  bool call(F &&body, const char *what) const noexcept
  {
    return detail::guardedCall(obj_ != nullptr, *mu_, err_, what, std::forward<F>(body));
  }
  ccmp_ctx *ctx_ = nullptr;
  std::mutex *mu_ = nullptr;
  mutable std::mutex own_mu_;
  ccmp_object *obj_ = nullptr;
  double inflate_ = 0.0, lo_[3], hi_[3];
  uint64_t seed_ = 0, next_ = 0;
  mutable detail::ErrorLatch err_;
};

// One planner process, several GPUs (the reference's shape: src/main.cpp is one process): one context per device and an
// RCCL communicator over them.  sampleProjectSharded / projectSharded spread a batch over the GPUs in contiguous shards,
// every GPU compacts its valid states into a fixed-capacity block and ONE all-gather brings them together; the valid
// states come back in global sample order — what the host tree consumes.  Results are bit-identical to one GPU.
class ShardedProjector {
public:
  // devices: one entry per GPU (RCCL wants distinct devices)
  ShardedProjector(const std::string &yaml_path, const std::vector<int> &devices)
  {
    check(ccmp_problem_from_yaml(yaml_path.c_str(), &problem_), "ccmp_problem_from_yaml");
    try {
      for (int d : devices) {
        ccmp_ctx *c = nullptr;
        check(ccmp_ctx_create(d, &c), "ccmp_ctx_create");
        ctxs_.push_back(c);
      }
      check(ccmp_comm_create(ctxs_.data(), (int)ctxs_.size(), &comm_), "ccmp_comm_create");
    } catch (...) {
      release();
      throw;
    }
  }
  ~ShardedProjector() { release(); }
  ShardedProjector(const ShardedProjector &) = delete;
  ShardedProjector &operator=(const ShardedProjector &) = delete;
  ccmp_problem &problem() { return problem_; }
  size_t devices() const { return ctxs_.size(); }

  // jy_ProjectedStateSampler::sampleUniform x B over the GPUs: returns the valid states (row-major [n][14], global sample
  // order); counts (optional) receives the valid states per shard.  A shard holding more valid states than the block
  // (block_fraction of the shard; ~22 % of uniform samples are valid) is retried once with full-size blocks.
  std::vector<double> sampleProjectSharded(uint64_t seed, uint64_t first_index, size_t B, std::vector<uint64_t> *counts = nullptr,
                                           double block_fraction = 0.5)
  {
    return run(nullptr, seed, first_index, B, counts, block_fraction);
  }
  // KinematicChainConstraint::project x B (host buffer q_in [B][14]) over the GPUs: the valid projected states
  std::vector<double> projectSharded(const double *q_in, size_t B, std::vector<uint64_t> *counts = nullptr, double block_fraction = 0.5)
  {
    return run(q_in, 0, 0, B, counts, block_fraction);
  }

private:
  std::vector<double> run(const double *q_in, uint64_t seed, uint64_t first, size_t B, std::vector<uint64_t> *counts, double fraction)
  {
    std::lock_guard<std::mutex> hold(mu_);
    const size_t n = ctxs_.size(), shard = (B + n - 1) / n;
    std::vector<uint64_t> cnt(n, 0);
    for (int attempt = 0; attempt < 2; ++attempt) {
      const size_t rows = attempt == 0 ? std::max<size_t>(1, (size_t)(shard * fraction)) : std::max<size_t>(1, shard);
      std::vector<double> valid(n * rows * 14);
      uint64_t nv = 0;
      const int rc = q_in ? ccmp_project_sharded(comm_, &problem_, q_in, B, nullptr, nullptr, nullptr, rows, valid.data(), n * rows, cnt.data(), &nv)
                          : ccmp_sample_project_sharded(comm_, &problem_, seed, first, B, nullptr, nullptr, nullptr, rows, valid.data(), n * rows,
                                                        cnt.data(), &nv);
      if (rc == CCMP_EOVERFLOW && attempt == 0) continue;
      check(rc, "ccmp_project_sharded");
      valid.resize((size_t)nv * 14);
      if (counts) *counts = cnt;
      return valid;
    }
    return {};
  }
  void release()
  {
    if (comm_) ccmp_comm_destroy(comm_);
    comm_ = nullptr;
    for (ccmp_ctx *c : ctxs_) ccmp_ctx_destroy(c);
    ctxs_.clear();
  }
  std::vector<ccmp_ctx *> ctxs_;
  ccmp_comm *comm_ = nullptr;
  ccmp_problem problem_;
  std::mutex mu_;
};

// ---- proxy-geometry pre-filter in front of KinematicChainValidityChecker::isValid ---------------------------------
// (src/kinematics/KinematicChain.cpp:94-123: MoveIt's checkCollision under acm_).  Spheres on link frames, static
// boxes, an allowed-pair matrix (include/ccmp.h: ccmp_scene_create); clearance() is the smallest signed distance over
// the tested pairs.  With spheres inscribed in the links a negative clearance proves a collision, so the state can be
// refused without asking MoveIt; everything else still goes to MoveIt (PrefilteredValidityChecker in part 2).
// The scene borrows the Projector (context, problem, mutex): keep the Projector alive for as long as the scene is used.
class ProxyScene {
public:
  ProxyScene(const Projector &proj, const std::vector<ccmp_sphere> &spheres, const std::vector<ccmp_box> &boxes,
             const uint32_t *allowed32 = nullptr)
    : proj_(proj)
  {
    check(ccmp_scene_create(proj.ctx(), spheres.data(), (int)spheres.size(), boxes.data(), (int)boxes.size(), allowed32, &scene_),
          "ccmp_scene_create");
  }
  ~ProxyScene() { ccmp_scene_destroy(scene_); }
  ProxyScene(const ProxyScene &) = delete;
  ProxyScene &operator=(const ProxyScene &) = delete;
  int numPairs() const { return ccmp_scene_num_pairs(scene_); }
  // one state; pair (nullable) = i | j << 8 of the closest pair (j >= 64: box j - 64), -1 if nothing is tested
  double clearance(const double *x14, int32_t *pair = nullptr) const
  {
    double clr = 0.0;
    std::lock_guard<std::mutex> hold(proj_.mutex());
    check(ccmp_clearance_host(proj_.ctx(), &proj_.problem(), scene_, x14, 1, 0.0, &clr, pair, nullptr), "ccmp_clearance_host");
    return clr;
  }
  // B host states: clearance[B], free[B] = clearance > margin (both caller-owned; pair nullable)
  void clearanceBatch(const double *q, size_t B, double margin, double *clearance, int32_t *pair, uint8_t *free_out) const
  {
    std::lock_guard<std::mutex> hold(proj_.mutex());
    check(ccmp_clearance_host(proj_.ctx(), &proj_.problem(), scene_, q, B, margin, clearance, pair, free_out), "ccmp_clearance_host");
  }
  // KinematicChainValidityChecker::IKValid(arm_index, sol) (KinematicChain.cpp:129-161: a collision test of that ONE arm) on the proxies
  // (ccmp_arm_clearance_host): true when the clearance of arm `arm` alone at the seven joints q7 — over the tested pairs that hold no
  // sphere moving on the other arm — exceeds `margin`.  Unlike MoveIt's, which sees whatever the other arm was last set to, the other
  // arm's links are not part of the test.  *clearance (nullable): the value, NaN when the call failed.  Never throws: false on a failed
  // call, whose FIRST error stays in lastError() / lastErrorMessage() until clearError().
  bool ikValid(int arm, const double *q7, double margin = 0.0, double *clearance = nullptr) const noexcept
  {
    double clr = std::numeric_limits<double>::quiet_NaN();
    uint8_t free_flag = 0;
    const bool ran = detail::guardedCall(true, proj_.mutex(), err_, "ccmp_arm_clearance_host", [&] {
      return ccmp_arm_clearance_host(proj_.ctx(), &proj_.problem(), scene_, arm, q7, 1, margin, &clr, &free_flag);
    });
    if (!ran) {
      clr = std::numeric_limits<double>::quiet_NaN();
      free_flag = 0;
    }
    if (clearance) *clearance = clr;
    return free_flag != 0;
  }
  int lastError() const noexcept { return err_.code(); }
  std::string lastErrorMessage() const { return err_.message(); }
  void clearError() noexcept { err_.clear(); }
  const ccmp_scene *handle() const { return scene_; }
  const Projector &projector() const { return proj_; }

  // AllowedCollisionMatrix::setEntry(g, h, true) on a 32-word matrix
  static void allow(uint32_t *allowed32, int g, int h)
  {
    allowed32[g] |= 1u << h;
    allowed32[h] |= 1u << g;
  }
  // the reference constructor's "sub_table" (KinematicChain.cpp:25-30: addBox(dim (0.65, 1.0, 0.2), pose (0.65, 0, 1.1)))
  static ccmp_box subTable(int group)
  {
    ccmp_box b;
    std::memset(&b, 0, sizeof b);
    b.group = group;
    b.c[0] = 0.65; b.c[1] = 0.0; b.c[2] = 1.1;
    b.R[0] = b.R[4] = b.R[8] = 1.0;
    b.half[0] = 0.325; b.half[1] = 0.5; b.half[2] = 0.1;
    return b;
  }

private:
  const Projector &proj_;
  ccmp_scene *scene_ = nullptr;
  mutable detail::ErrorLatch err_; // ikValid's sticky error (the other verbs throw)
};

// ---- the planners on the store (include/ccmp.h: ccmp_plan_*, ccmp_rrtc_*) -----------------------------------------------------------
namespace detail {

// One resumable planner object over the C handle that the traits T name: Handle, Report, State; run / stateRead / destroy (the C entries)
// with kRun / kState (their texts in an error) and kCreate (the text recorded on a failed open); kSolved; blank(report): the fields
// beyond status and the solved pair of a planner never opened.  ccmp::Planner and ccmp::RRTConnectPlanner add their constructors.
// Never throws: a planner that could not be opened answers "no" to every verb and keeps the FIRST failure in lastError() /
// lastErrorMessage() until clearError(), as ccmp::Roadmap does.  The handle is destroyed under the lock.
template <class T> class PlannerBase {
public:
  ~PlannerBase()
  {
    if (!plan_) return;
    std::lock_guard<std::mutex> hold(*mu_);
    T::destroy(plan_);
  }
  PlannerBase(const PlannerBase &) = delete;
  PlannerBase &operator=(const PlannerBase &) = delete;

  bool create() const noexcept { return plan_ != nullptr; } // was it opened
  // up to max_cycles more cycles; true = the call ran (report() has the verdict), false = it failed or there is no planner
  bool run(int max_cycles) noexcept
  {
    return guardedCall(plan_ != nullptr, *mu_, err_, +T::kRun, [&] { return T::run(plan_, max_cycles, &report_); });
  }
  const typename T::Report &report() const noexcept { return report_; }
  int status() const noexcept { return plan_ ? report_.status : -1; }
  bool solved() const noexcept { return plan_ && report_.status == T::kSolved; }
  bool state(typename T::State *out) const noexcept
  {
    return guardedCall(plan_ != nullptr, *mu_, err_, +T::kState, [&] { return T::stateRead(plan_, out); });
  }
  int lastError() const noexcept { return err_.code(); }
  std::string lastErrorMessage() const { return err_.message(); }
  void clearError() noexcept { err_.clear(); }
  typename T::Handle *handle() const noexcept { return plan_; }

protected:
  // shared: the Projector's mutex, or nullptr for a mutex of the planner's own (a caller on the C handles)
  explicit PlannerBase(std::mutex *shared) noexcept : mu_(shared ? shared : &own_mu_) {}
  // create_call(&handle) = the planner's *_create; then a run of no cycles for the report
  template <class F> void open(F &&create_call) noexcept
  {
    std::memset(&report_, 0, sizeof report_);
    report_.status = -1;
    report_.solved_start = report_.solved_goal = -1;
    T::blank(report_);
    int rc;
    try {
      std::lock_guard<std::mutex> hold(*mu_);
      rc = create_call(&plan_); // a NULL store: the library's own answer
      if (rc == CCMP_OK) rc = T::run(plan_, 0, &report_);
    } catch (...) {
      rc = CCMP_EHIP;
    }
    if (rc != CCMP_OK) err_.record(rc, +T::kCreate);
  }

private:
  std::mutex own_mu_;
  std::mutex *mu_;
  typename T::Handle *plan_ = nullptr;
  typename T::Report report_;
  mutable ErrorLatch err_;
};

struct PlanTraits {
  using Handle = ccmp_plan;
  using Report = ccmp_plan_report;
  using State = ccmp_plan_state;
  enum { kSolved = CCMP_PLAN_SOLVED };
  static int run(ccmp_plan *h, int n, ccmp_plan_report *r) { return ccmp_plan_run(h, n, r); }
  static int stateRead(ccmp_plan *h, ccmp_plan_state *s) { return ccmp_plan_state_read(h, s); }
  static void destroy(ccmp_plan *h) { ccmp_plan_destroy(h); }
  static constexpr const char *kRun = "ccmp_plan_run", *kState = "ccmp_plan_state_read", *kCreate = "ccmp_plan_create";
  static void blank(ccmp_plan_report &r) { r.nearest = -1; }
};

struct RRTConnectTraits {
  using Handle = ccmp_rrtc;
  using Report = ccmp_rrtc_report;
  using State = ccmp_rrtc_state;
  enum { kSolved = CCMP_RRTC_SOLVED };
  static int run(ccmp_rrtc *h, int n, ccmp_rrtc_report *r) { return ccmp_rrtc_run(h, n, r); }
  static int stateRead(ccmp_rrtc *h, ccmp_rrtc_state *s) { return ccmp_rrtc_state_read(h, s); }
  static void destroy(ccmp_rrtc *h) { ccmp_rrtc_destroy(h); }
  static constexpr const char *kRun = "ccmp_rrtc_run", *kState = "ccmp_rrtc_state_read", *kCreate = "ccmp_rrtc_create";
  static void blank(ccmp_rrtc_report &r) { r.best_a = r.best_b = -1; }
};

// the tail of Roadmap::solve / solveRRTConnect: the cycles, the report, the planner's error into the store's latch, the solved pair
template <class P, class R> int solveWith(P &planner, int max_cycles, int32_t *start, int32_t *goal, R *report, ErrorLatch &err) noexcept
{
  if (planner.create() && max_cycles > 0) planner.run(max_cycles);
  if (report) *report = planner.report();
  if (planner.lastError() != CCMP_OK) {
    err.recordAs(planner.lastError(), planner.lastErrorMessage().c_str());
    return -1;
  }
  if (planner.solved()) {
    if (start) *start = planner.report().solved_start;
    if (goal) *goal = planner.report().solved_goal;
  }
  return planner.status();
}

}  // namespace detail

// stefanBiPRM::solve / constructRoadmap / checkForSolution as one resumable object: open (start and goal vertex through
// startgoalMilestone), then cycles of growth (width candidates where the reference has one), check (closestFromGoal both ways, goal and
// start IK, the nine-pose ladder as one batch) and the solution test, with the bookkeeping on the device.  A restatement of the
// reference's STRUCTURE, not of the interleaving of its two threads; an unsettled query is skipped, not continued.
struct PlanOptions : ccmp_plan_opts {
  PlanOptions() noexcept { ccmp_plan_default_opts(this); }
};

// detail::PlannerBase's verbs and contract.  The store, the object and the scene must outlive it.
class Planner : public detail::PlannerBase<detail::PlanTraits> {
public:
  Planner(Roadmap &roadmap, const ccmp_object *object, const PlanOptions &opts = PlanOptions(), const ccmp_scene *scene = nullptr, double margin = 0.0,
          const double *goal_joints14 = nullptr, uint64_t rng_seed = 0, uint64_t first_index = 0) noexcept : PlannerBase(&roadmap.projector().mutex())
  {
    open([&](ccmp_plan **out) {
      return ccmp_plan_create(roadmap.handle(), &roadmap.projector().problem(), object, scene, margin, &roadmap.projector().ikOptions(), &opts, goal_joints14,
                              rng_seed, first_index, out);
    });
  }
  // the same on the C handles (a caller without a Projector); serialised by a mutex of its own
  Planner(ccmp_roadmap *roadmap, const ccmp_problem &problem, const ccmp_object *object, const PlanOptions &opts = PlanOptions(), const ccmp_scene *scene = nullptr,
          double margin = 0.0, const double *goal_joints14 = nullptr, uint64_t rng_seed = 0, uint64_t first_index = 0) noexcept : PlannerBase(nullptr)
  {
    open([&](ccmp_plan **out) { return ccmp_plan_create(roadmap, &problem, object, scene, margin, nullptr, &opts, goal_joints14, rng_seed, first_index, out); });
  }
};

inline int Roadmap::solve(const ccmp_object *object, int max_cycles, int32_t *start, int32_t *goal, const ccmp_plan_opts *opts, const ccmp_scene *scene,
                          double margin, const double *goal_joints14, uint64_t rng_seed, ccmp_plan_report *report) noexcept
{
  PlanOptions o;
  if (opts) static_cast<ccmp_plan_opts &>(o) = *opts;
  if (start) *start = -1;
  if (goal) *goal = -1;
  Planner planner(*this, object, o, scene, margin, goal_joints14, rng_seed);
  return detail::solveWith(planner, max_cycles, start, goal, report, err_);
}

// The reference's other planner (ConstrainedProblem::setPlanner(RRTConnect)) as one resumable object: two trees in joint space over the
// store's component labels, width samples per cycle, one traversal per extension clipped at `range`, one traversal per connection.  NOT
// OMPL's RRTConnect step for step: include/ccmp.h lists the stated differences (one clipped traversal, a one-traversal connect phase,
// unsettled extensions skipped, both trees extend from the tree vertex, counter-based draws, the proxy scene's validity).
struct RRTConnectOptions : ccmp_rrtc_opts {
  RRTConnectOptions() noexcept { ccmp_rrtc_default_opts(this); }
};

// detail::PlannerBase's verbs and contract.  The store and the scene must outlive it.
class RRTConnectPlanner : public detail::PlannerBase<detail::RRTConnectTraits> {
public:
  RRTConnectPlanner(Roadmap &roadmap, const int32_t *starts, int n_starts, const int32_t *goals, int n_goals, const RRTConnectOptions &opts = RRTConnectOptions(),
                    const ccmp_scene *scene = nullptr, double margin = 0.0, uint64_t rng_seed = 0, uint64_t first_index = 0) noexcept
      : PlannerBase(&roadmap.projector().mutex())
  {
    open([&](ccmp_rrtc **out) {
      return ccmp_rrtc_create(roadmap.handle(), &roadmap.projector().problem(), scene, margin, &opts, starts, n_starts, goals, n_goals, rng_seed, first_index, out);
    });
  }
  // the same on the C handles (a caller without a Projector); serialised by a mutex of its own
  RRTConnectPlanner(ccmp_roadmap *roadmap, const ccmp_problem &problem, const int32_t *starts, int n_starts, const int32_t *goals, int n_goals,
                    const RRTConnectOptions &opts = RRTConnectOptions(), const ccmp_scene *scene = nullptr, double margin = 0.0, uint64_t rng_seed = 0,
                    uint64_t first_index = 0) noexcept
      : PlannerBase(nullptr)
  {
    open([&](ccmp_rrtc **out) { return ccmp_rrtc_create(roadmap, &problem, scene, margin, &opts, starts, n_starts, goals, n_goals, rng_seed, first_index, out); });
  }
};

inline int Roadmap::solveRRTConnect(const int32_t *starts, int n_starts, const int32_t *goals, int n_goals, int max_cycles, int32_t *start, int32_t *goal,
                                    const ccmp_rrtc_opts *opts, const ccmp_scene *scene, double margin, uint64_t rng_seed, ccmp_rrtc_report *report) noexcept
{
  RRTConnectOptions o;
  if (opts) static_cast<ccmp_rrtc_opts &>(o) = *opts;
  if (start) *start = -1;
  if (goal) *goal = -1;
  RRTConnectPlanner planner(*this, starts, n_starts, goals, n_goals, o, scene, margin, rng_seed);
  return detail::solveWith(planner, max_cycles, start, goal, report, err_);
}

inline bool Projector::sampleCalibGoal(const double *pose8, const double *seeds, int S, double *result14, int *which, const ProxyScene &scene, double margin,
                                       double *clearance) const noexcept
{
  uint8_t ok = 0;
  int32_t slot = -1;
  double clr = std::numeric_limits<double>::quiet_NaN();
  const bool ran = detail::guardedCall(true, mu_, err_, "ccmp_pose_ik_vetted_host", [&] {
    const int rc = ccmp_pose_ik_vetted_host(ctx_, &problem_, &ik_opts_, pose8, seeds, 1, S, ikSeed(), ik_index_, scene.handle(), margin, result14, &ok, &slot,
                                            nullptr, nullptr, nullptr, nullptr, &clr);
    if (rc == CCMP_OK) ik_index_++;
    return rc;
  });
  if (!ran) {
    ok = 0;
    slot = -1;
    clr = std::numeric_limits<double>::quiet_NaN();
    detail::fillNaN(result14);
  }
  if (which) *which = slot;
  if (clearance) *clearance = clr;
  return ok != 0;
}

// discreteGeodesicBatch with the proxy pre-filter ON THE DEVICE (ccmp_geodesic_scene_host): with interpolate == false the
// traversal itself refuses a state whose clearance in `scene` does not exceed `margin` — before the step test, where the
// reference's loop asks its StateValidityChecker — and `exact` (the checker behind the proxies: MoveIt in the reference) is then
// asked only about the listed states, in order, an edge stopping at its first refusal as above.  (*blocked)[e] (nullable) = 1:
// the edge ended at a state the proxies refused (the exact checker had accepted everything before it).  scene == nullptr or
// interpolate: the overload above with `exact` as the checker.  The scene must belong to proj's context.
template <class ValidFn>
inline void discreteGeodesicBatch(const Projector &proj, const double *from, const double *to, size_t E, bool interpolate, ValidFn exact,
                                  std::vector<std::vector<std::vector<double>>> *geodesics, std::vector<char> *reached, int max_states,
                                  bool check_target, double delta, double lambda, const ProxyScene *scene, double margin,
                                  std::vector<char> *blocked = nullptr)
{
  detail::traverseBatch(proj, from, to, E, interpolate, exact, geodesics, reached, max_states, check_target, delta, lambda,
                        scene && !interpolate ? scene->handle() : nullptr, margin, blocked);
}

// ---- dump formats of the reference's planner run ----------------------------------------------------------------------
// PathGeometric::printAsMatrix as ConstrainedProblem::solveOnce writes `<obj>_path.txt`
// (src/base/constraints/ConstrainedPlanningCommon.cpp:219-222) and scripts/execute_path.py:65-87 / visualize_path.py
// parse it: the reals of one state per line in default stream format, each followed by a space, and one empty line
// after the last state.
inline void printAsMatrix(std::ostream &out, const double *states, size_t n_states, size_t dim = 14)
{
  for (size_t i = 0; i < n_states; ++i) {
    for (size_t j = 0; j < dim; ++j) out << states[i * dim + j] << ' ';
    out << '\n';
  }
  out << '\n';
  out.flush();
}

// A time-stamped path: printAsMatrix's row — the reals of one state, each followed by a space — with the row's time as one more column,
// and the empty line after the last row.  The first `dim` columns of every line are printAsMatrix's, character for character.
inline void printTrajectory(std::ostream &out, const double *states, const double *times, size_t n_states, size_t dim = 14)
{
  for (size_t i = 0; i < n_states; ++i) {
    for (size_t j = 0; j < dim; ++j) out << states[i * dim + j] << ' ';
    out << times[i] << ' ';
    out << '\n';
  }
  out << '\n';
  out.flush();
}

// The setpoints of a path (ccmp::Setpoints): one controller tick per line — tau, the positions, the velocities, each followed by a space —
// and the empty line after the last tick.
inline void printSetpoints(std::ostream &out, const double *tau, const double *q, const double *qd, size_t n_ticks, size_t dim = 14)
{
  for (size_t i = 0; i < n_ticks; ++i) {
    out << tau[i] << ' ';
    for (size_t j = 0; j < dim; ++j) out << q[i * dim + j] << ' ';
    for (size_t j = 0; j < dim; ++j) out << qd[i * dim + j] << ' ';
    out << '\n';
  }
  out << '\n';
  out.flush();
}
inline void printSetpoints(std::ostream &out, const Setpoints &s)
{
  printSetpoints(out, s.tau.data(), s.q.empty() ? nullptr : s.q[0].data(), s.qd.empty() ? nullptr : s.qd[0].data(), s.tau.size());
}
inline void printSetpoints(std::ostream &out, const JerkSetpoints &s)
{
  printSetpoints(out, s.tau.data(), s.q.empty() ? nullptr : s.q[0].data(), s.qd.empty() ? nullptr : s.qd[0].data(), s.tau.size());
}

// PlannerData::printGraphML as ConstrainedProblem::dumpGraph writes `<obj>_node_info.graphml`
// (include/closed_chain_motion_planner/base/constraints/ConstrainedPlanningCommon.h:73-87): node data = the reals of
// the milestone joined by commas, directed edges in insertion order with their weight (nullptr = 1 each).
inline void printGraphML(std::ostream &out, const double *nodes, size_t n_nodes, const std::pair<unsigned, unsigned> *edges,
                         size_t n_edges, const double *weights = nullptr, size_t dim = 14)
{
  out << "<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n"
         "<graphml xmlns=\"http://graphml.graphdrawing.org/xmlns\" xmlns:xsi=\"http://www.w3.org/2001/XMLSchema-instance\" "
         "xsi:schemaLocation=\"http://graphml.graphdrawing.org/xmlns http://graphml.graphdrawing.org/xmlns/1.0/graphml.xsd\">\n"
         "  <key id=\"key0\" for=\"node\" attr.name=\"coords\" attr.type=\"string\" />\n"
         "  <key id=\"key1\" for=\"edge\" attr.name=\"weight\" attr.type=\"double\" />\n"
         "  <graph id=\"G\" edgedefault=\"directed\" parse.nodeids=\"free\" parse.edgeids=\"canonical\" parse.order=\"nodesfirst\">\n";
  for (size_t i = 0; i < n_nodes; ++i) {
    out << "    <node id=\"n" << i << "\">\n      <data key=\"key0\">";
    for (size_t j = 0; j < dim; ++j) out << (j ? "," : "") << nodes[i * dim + j];
    out << "</data>\n    </node>\n";
  }
  for (size_t k = 0; k < n_edges; ++k)
    out << "    <edge id=\"e" << k << "\" source=\"n" << edges[k].first << "\" target=\"n" << edges[k].second
        << "\">\n      <data key=\"key1\">" << (weights ? weights[k] : 1.0) << "</data>\n    </edge>\n";
  out << "  </graph>\n</graphml>\n";
  out.flush();
}

// PlannerData::printGraphviz as dumpGraph writes `<obj>_graph_info.dot`
inline void printGraphviz(std::ostream &out, size_t n_nodes, const std::pair<unsigned, unsigned> *edges, size_t n_edges)
{
  out << "digraph G {\n";
  for (size_t i = 0; i < n_nodes; ++i) out << i << ";\n";
  for (size_t k = 0; k < n_edges; ++k) out << edges[k].first << "->" << edges[k].second << " ;\n";
  out << "}\n";
  out.flush();
}

}  // namespace ccmp

#ifdef CCMP_WITH_OMPL
// ---------------------------------------------------------------------------------------------------
// Part 2: the reference's classes, same names and signatures, backed by ccmp::Projector.
// ---------------------------------------------------------------------------------------------------
#include <Eigen/Dense>
#include <ompl/base/Constraint.h>
#include <ompl/base/StateSampler.h>
#include <ompl/base/spaces/constraint/ConstrainedStateSpace.h>
#include <ompl/util/Exception.h>

#include <closed_chain_motion_planner/kinematics/panda_model.h>  // ArmModelPtr {name, index, ...}

class KinematicChainConstraint : public ompl::base::Constraint {
public:
  explicit KinematicChainConstraint(unsigned int links, int device = 0) : ompl::base::Constraint(links, 2), impl_(new ccmp::Projector(device)) {}
  // the State* overloads of the base class stay visible next to the overrides below (the samplers and
  // discreteGeodesic call project(State*) / isSatisfied(const State*), src/base/jy_ProjectedStateSpace.cpp:13,20,27,65)
  using ompl::base::Constraint::project;
  using ompl::base::Constraint::isSatisfied;

  // ConstraintFunction.h:122-126: the two ArmModels in the order given; the base frame of each is the t_wb the ArmModel
  // carries (panda_model.h:15, filled from config->t_wb[index] at ConstrainedPlanningCommon.cpp:98) — not a table of this
  // library's — so function() multiplies with the very frame the reference's does (ConstraintFunction.h:89-90)
  void setArmModels(const ArmModelPtr &arm1, const ArmModelPtr &arm2)
  {
    impl_->setArmModels(arm1->name, arm1->index, arm2->name, arm2->index);
    const ArmModelPtr arms[2] = {arm1, arm2};
    for (int a = 0; a < 2; ++a) {
      const Eigen::Isometry3d &t_wb = arms[a]->t_wb;
      double R[9], p[3];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = t_wb.linear()(r, c);
        p[r] = t_wb.translation()(r);
      }
      impl_->setBaseFrame(a, R, p);
    }
  }
  void setInitialPosition(const Eigen::Ref<const Eigen::VectorXd> init_joint)
  {
    Eigen::VectorXd q = init_joint;  // contiguous copy
    impl_->setInitialPosition(q.data());
  }
  // opt-in (not part of the reference's class): the context's resident service kernel for the one-state-at-a-time calls below
  // and, in analytic mode, for discreteGeodesics of up to eight edges and their continuations — same results, ~10 us less per call;
  // see ccmp::Projector::setResident for what it asks of the application
  void setResident(bool on) { impl_->setResident(on); }
  void setTolerance(const double tolerance1, const double tolerance2)
  {
    try { impl_->setTolerance(tolerance1, tolerance2); }
    catch (const ccmp::Error &) {
      throw ompl::Exception("ompl::base::Constraint::setProjectionTolerance(): tolerance must be positive.");
    }
  }
  // The reference's overrides return plain bool / void and are called from the planner's main thread AND its solution-checker
  // thread (src/planner/stefanBiPRM.cpp:848-849): nothing may be thrown out of them — a transient HIP error would otherwise
  // std::terminate the planner.  A failed call keeps the reference's contract for "no": project / isSatisfied / jointValid return
  // false and leave the state as it was, function writes NaN (so that isSatisfied(f) is false); the error stays readable through
  // lastError() / lastErrorMessage() until clearError().  setTolerance above remains the only thrower, as in the reference
  // (ConstraintFunction.h:104-108).
  bool project(Eigen::Ref<Eigen::VectorXd> x) const override
  {
    double buf[14];
    ccmp::detail::load14(buf, x);
    bool ok = false;
    if (!guarded([&] { ok = impl_->project(buf); })) return false;  // x untouched
    ccmp::detail::store14(x, buf);
    return ok;
  }
  void function(const Eigen::Ref<const Eigen::VectorXd> &x, Eigen::Ref<Eigen::VectorXd> out) const override
  {
    double buf[14], f[2];
    ccmp::detail::fillNaN(f, 2);
    ccmp::detail::load14(buf, x);
    guarded([&] { impl_->function(buf, f); });
    out[0] = f[0];
    out[1] = f[1];
  }
  bool isSatisfied(const Eigen::Ref<const Eigen::VectorXd> &x) const override
  {
    double buf[14];
    ccmp::detail::load14(buf, x);
    bool ok = false;
    return guarded([&] { ok = impl_->isSatisfied(buf); }) && ok;
  }
  bool jointValid(const Eigen::Ref<const Eigen::VectorXd> &q) const
  {
    double buf[14];
    ccmp::detail::load14(buf, q);
    bool ok = false;
    return guarded([&] { ok = impl_->jointValid(buf); }) && ok;
  }
  // 0 (CCMP_OK) or the code of the first error since the last clearError() (CCMP_EHIP, CCMP_ENODEV, ...) — sticky, thread-safe
  int lastError() const
  {
    std::lock_guard<std::mutex> hold(err_mu_);
    return err_.code();
  }
  std::string lastErrorMessage() const
  {
    std::lock_guard<std::mutex> hold(err_mu_);
    return err_.message();
  }
  void clearError() const
  {
    std::lock_guard<std::mutex> hold(err_mu_);
    err_.clear();
  }
  // runs `body`; an exception of the library (or any other) is recorded, never passed on: false = it failed.  Used by the space and
  // the samplers below for their own GPU calls too.
  template <class F>
  bool guarded(F &&body) const noexcept
  {
    try {
      body();
      return true;
    } catch (const ccmp::Error &e) {
      record(e.code, e.what());
    } catch (const std::exception &e) {
      record(CCMP_EHIP, e.what());
    } catch (...) {
      record(CCMP_EHIP, "unknown exception");
    }
    return false;
  }
  ccmp::Projector &impl() const { return *impl_; }

private:
  void record(int code, const char *what) const noexcept
  {
    try {
      std::lock_guard<std::mutex> hold(err_mu_);
      err_.recordAs(code, what);  // the exception's own text
    } catch (...) {
    }
  }
  std::shared_ptr<ccmp::Projector> impl_;
  mutable std::mutex err_mu_;
  mutable ccmp::detail::ErrorLatch err_;
};
typedef std::shared_ptr<KinematicChainConstraint> ChainConstraintPtr;

// A StateValidityChecker that asks the proxy scene first and the exact checker (the reference's
// KinematicChainValidityChecker, i.e. MoveIt) only for states the proxies do not already refuse:
//   si->setStateValidityChecker(std::make_shared<PrefilteredValidityChecker>(si, scene, valid_checker_));
// `reject_below` = 0 with inscribed proxies; the answer for every state MoveIt is asked about is MoveIt's.
class PrefilteredValidityChecker : public ompl::base::StateValidityChecker {
public:
  PrefilteredValidityChecker(const ompl::base::SpaceInformationPtr &si, std::shared_ptr<ccmp::ProxyScene> scene,
                             ompl::base::StateValidityCheckerPtr exact, double reject_below = 0.0)
    : ompl::base::StateValidityChecker(si), scene_(std::move(scene)), exact_(std::move(exact)), reject_below_(reject_below)
  {
  }
  bool isValid(const ompl::base::State *state) const override
  {
    const auto &q = *state->as<ompl::base::ConstrainedStateSpace::StateType>();  // an Eigen::Map over the 14 joints, as in
    const double clr = scene_->clearance(&q[0]);                                 // KinematicChain.cpp:94-99
    if (!(clr > reject_below_)) { rejected_++; return false; }
    asked_++;
    return exact_ ? exact_->isValid(state) : true;
  }
  uint64_t rejectedByProxies() const { return rejected_.load(); }
  uint64_t askedExact() const { return asked_.load(); }
  // what jy_ProjectedStateSpace's device path uses (the proxies then run inside the traversal, ccmp_geodesic_scene_host):
  // the scene, the threshold, the exact checker alone — counted as isValid counts a state the proxies passed — and the count
  // of a state the proxies refused
  const std::shared_ptr<ccmp::ProxyScene> &scene() const { return scene_; }
  double rejectBelow() const { return reject_below_; }
  bool isValidExact(const ompl::base::State *state) const
  {
    asked_++;
    return exact_ ? exact_->isValid(state) : true;
  }
  void countRejected() const { rejected_++; }

private:
  std::shared_ptr<ccmp::ProxyScene> scene_;
  ompl::base::StateValidityCheckerPtr exact_;
  double reject_below_;
  mutable std::atomic<uint64_t> rejected_{0}, asked_{0};
};
// jy_ProjectedStateSampler (include/closed_chain_motion_planner/base/jy_ProjectedStateSpace.h:18-29): same
// name, same overrides; all three draw from the GPU's counter-based samplers through refill-on-empty buffers
// (sampleUniform: `batch` samples per launch; Near / Gaussian: a look-ahead around the current reference state).
// Every sampler has its own stream: the space hands out seed = splitmix64(space seed + running sampler number),
// as every OMPL sampler owns an independently seeded ompl::RNG.
class jy_ProjectedStateSpace;
typedef std::shared_ptr<jy_ProjectedStateSpace> jy_ProjectedStateSpacePtr;

class jy_ProjectedStateSampler : public ompl::base::WrapperStateSampler {
public:
  jy_ProjectedStateSampler(const jy_ProjectedStateSpace *space, ompl::base::StateSamplerPtr sampler);
  jy_ProjectedStateSampler(const jy_ProjectedStateSpace *space, ompl::base::StateSamplerPtr sampler, uint64_t seed);
  void sampleUniform(ompl::base::State *state) override
  {
    auto &&x = *state->as<ompl::base::ConstrainedStateSpace::StateType>();
    double buf[14];
    if (!constraint_->guarded([&] { buffer_.next(buf); })) return;  // already projected and wrapped by enforceBounds on the GPU; a failed refill leaves the state as it was (lastError() of the constraint)
    ccmp::detail::store14(x, buf);
  }
  void sampleUniformNear(ompl::base::State *state, const ompl::base::State *near, const double distance) override
  {
    sampleAround(near_, state, near, distance);
  }
  void sampleGaussian(ompl::base::State *state, const ompl::base::State *mean, const double stdDev) override
  {
    sampleAround(gauss_, state, mean, stdDev);
  }

protected:
  void sampleAround(ccmp::RefSampleBuffer &buf, ompl::base::State *state, const ompl::base::State *ref, double param)
  {
    const auto &r = *ref->as<ompl::base::ConstrainedStateSpace::StateType>();
    auto &&x = *state->as<ompl::base::ConstrainedStateSpace::StateType>();
    double rb[14], out[14];
    ccmp::detail::load14(rb, r);
    if (!constraint_->guarded([&] { buf.next(out, rb, param); })) return;  // ambient draw, project (result ignored, as the reference does) and enforceBounds on the GPU
    ccmp::detail::store14(x, out);
  }
  const std::shared_ptr<KinematicChainConstraint> constraint_;
  ccmp::SampleBuffer buffer_;
  ccmp::RefSampleBuffer near_, gauss_;
};

// jy_ProjectedStateSpace (include/closed_chain_motion_planner/base/jy_ProjectedStateSpace.h:31-54): same name,
// same overrides.  discreteGeodesic runs the traversal on the GPU and applies the space information's
// StateValidityChecker on the host exactly where the reference consults it (src/base/jy_ProjectedStateSpace.cpp:
// 65-68); checkMotion of OMPL's ConstrainedMotionValidator (isSatisfied(s2) && discreteGeodesic(s1, s2),
// src/planner/stefanBiPRM.cpp:397-398,463-464) therefore needs no change.
class jy_ProjectedStateSpace : public ompl::base::ConstrainedStateSpace {
public:
  jy_ProjectedStateSpace(const ompl::base::StateSpacePtr &ambientSpace, const ompl::base::ConstraintPtr &constraint)
    : ompl::base::ConstrainedStateSpace(ambientSpace, constraint), chain_(std::dynamic_pointer_cast<KinematicChainConstraint>(constraint)),
      seed_(ccmp::next_sampler_seed())
  {
    setName("Projected" + space_->getName());
  }
  // the seed of the next sampler of this space: splitmix64(space seed + n++)
  uint64_t nextSamplerSeed() const { return ccmp::splitmix64(seed_ + samplers_.fetch_add(1, std::memory_order_relaxed)); }
  ~jy_ProjectedStateSpace() override = default;
  ompl::base::StateSamplerPtr allocDefaultStateSampler() const override
  {
    return std::make_shared<jy_ProjectedStateSampler>(this, space_->allocDefaultStateSampler(), nextSamplerSeed());
  }
  ompl::base::StateSamplerPtr allocStateSampler() const override
  {
    return std::make_shared<jy_ProjectedStateSampler>(this, space_->allocStateSampler(), nextSamplerSeed());
  }
  bool discreteGeodesic(const ompl::base::State *from, const ompl::base::State *to, bool interpolate = false,
                        std::vector<ompl::base::State *> *geodesic = nullptr) const override
  {
    return traverse(from, to, interpolate, geodesic, false);
  }
  // checkMotion's two tests — isSatisfied(s2) && discreteGeodesic(s1, s2, false) — in one GPU launch
  bool checkMotion(const ompl::base::State *s1, const ompl::base::State *s2) const { return traverse(s1, s2, false, nullptr, true); }

  // growTree's neighbour loop (src/planner/stefanBiPRM.cpp:307-351) in one launch: discreteGeodesic(from[e], to, interpolate,
  // &(*geodesics)[e]) for every e; reached[e] is the bool the reference's call returns.  The StateValidityChecker is asked
  // about the same states in the same order as by that loop.
  void discreteGeodesics(const std::vector<const ompl::base::State *> &from, const ompl::base::State *to, bool interpolate,
                         std::vector<std::vector<ompl::base::State *>> *geodesics, std::vector<char> *reached) const
  {
    traverse(from, to, interpolate, geodesics, reached, false);
  }

  // connectionStrategy_(m) of the reference's planner (a KStrategy over tree_, src/planner/stefanBiPRM.cpp:292,390,457) on the joint
  // distance: the indices into `nodes` of the k nearest to s, nearest first, ties to the lower index; fewer when there are fewer
  // nodes.  (The reference's own metric, the object's SE3 distance: the ccmp::Roadmap overloads below.)  false (and *out empty) when the GPU call
  // failed: KinematicChainConstraint::lastError().
  bool nearestK(const std::vector<const ompl::base::State *> &nodes, const ompl::base::State *s, unsigned k, std::vector<unsigned> *out) const
  {
    out->clear();
    if (k == 0 || nodes.empty()) return true;
    std::vector<double> a(nodes.size() * 14);
    double b[14];
    for (size_t j = 0; j < nodes.size(); ++j) ccmp::detail::load14(&a[14 * j], *nodes[j]->as<StateType>());
    ccmp::detail::load14(b, *s->as<StateType>());
    std::vector<int32_t> idx;
    if (!chain_->guarded([&] { ccmp::nearestK(chain_->impl(), a.data(), nodes.size(), b, k, &idx); })) return false;
    for (int32_t j : idx)
      if (j >= 0) out->push_back((unsigned)j);
    return true;
  }

  // addMilestone's neighbour loop (src/planner/stefanBiPRM.cpp:390-409) in two calls: nearestK, then checkMotion(nodes[n], s) for
  // every neighbour n in one launch — (*reached)[r] is the bool of the reference's call for (*neighbours)[r], (*geodesics)[r]
  // (nullable) its list.  The StateValidityChecker is asked about the same states in the same order as by that loop.
  void connectMilestone(const std::vector<const ompl::base::State *> &nodes, const ompl::base::State *s, unsigned k, std::vector<unsigned> *neighbours,
                        std::vector<char> *reached, std::vector<std::vector<ompl::base::State *>> *geodesics) const
  {
    if (reached) reached->clear();
    if (geodesics) geodesics->clear();
    if (!nearestK(nodes, s, k, neighbours)) return;
    std::vector<const ompl::base::State *> from;
    for (unsigned j : *neighbours) from.push_back(nodes[j]);
    traverse(from, s, false, geodesics, reached, true);
  }

  // The same two on a device-resident ccmp::Roadmap instead of a node vector: only `s` goes up.  pose8 != nullptr ranks on the reference's
  // own tree metric, the SE3 distance between object poses (ccmp::poseOf of components[1]); pose8 == nullptr on the joint distance of s.
  // *out = indices into the roadmap.  false when the call failed: Roadmap::lastError().  The reference's order is query, then add
  // (stefanBiPRM.cpp:390-410): with s already appended at index i pass mode = CCMP_KNN_NOT_SELF, self_base = i, or s is its own neighbour.
  bool nearestK(ccmp::Roadmap &rm, const ompl::base::State *s, const double *pose8, unsigned k, std::vector<unsigned> *out, int mode = CCMP_KNN_ALL,
                size_t self_base = 0) const
  {
    out->clear();
    if (k == 0 || rm.size() == 0) return true;
    double b[14];
    ccmp::detail::load14(b, *s->as<StateType>());
    std::vector<int32_t> idx;
    if (!rm.nearestK(pose8 ? CCMP_METRIC_OBJECT : CCMP_METRIC_JOINT, pose8 ? pose8 : b, k, &idx, nullptr, mode, self_base)) return false;
    for (int32_t j : idx)
      if (j >= 0) out->push_back((unsigned)j);
    return true;
  }
  // One k-NN call, then the neighbours' joints come back from the store (k one-row reads), then the traversals and the checker's questions
  // of connectMilestone above (all neighbours in one launch).  Neighbours and raw traversals in ONE call: ccmp::Roadmap::connect.
  void connectMilestone(ccmp::Roadmap &rm, const ompl::base::State *s, const double *pose8, unsigned k, std::vector<unsigned> *neighbours,
                        std::vector<char> *reached, std::vector<std::vector<ompl::base::State *>> *geodesics, int mode = CCMP_KNN_ALL,
                        size_t self_base = 0) const
  {
    if (reached) reached->clear();
    if (geodesics) geodesics->clear();
    if (!nearestK(rm, s, pose8, k, neighbours, mode, self_base)) return;
    std::vector<ompl::base::State *> own;
    std::vector<const ompl::base::State *> from;
    bool ok = true;
    for (unsigned j : *neighbours) {
      double row[14];
      if (!(ok = rm.read(j, 1, row, nullptr))) break;
      ompl::base::State *n = allocState();
      ccmp::detail::store14(*n->as<StateType>(), row);
      own.push_back(n);
      from.push_back(n);
    }
    if (ok) traverse(from, s, false, geodesics, reached, true);
    else neighbours->clear();
    for (ompl::base::State *n : own) freeState(n);
  }

  // PathGeometric::interpolate for the solution path of ConstrainedProblem::solveOnce (ConstrainedPlanningCommon.cpp:217), in one call:
  // `states` = the solution's waypoints on entry, the dense path on return (ccmp::densifyPathLocked: the layout ccmp::printAsMatrix writes
  // as <obj>_path.txt, or `distinct` for executing it), under this space's delta and lambda.  false = the call failed: `states` is as it
  // was and the first error stays in KinematicChainConstraint::lastError().  A segment that stops short of its target is not a failure:
  // seg_ok tells.
  bool interpolatePath(std::vector<std::array<double, 14>> &states, bool distinct = false, std::vector<uint8_t> *seg_ok = nullptr) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      ccmp::check(ccmp::densifyPathLocked(proj, states, distinct, seg_ok, delta_, lambda_), "ccmp_path_densify_host");
    });
  }

  // The removal of interior vertices from a solution path (ccmp::shortcutPathLocked: every pair of waypoints put to this space's
  // checkMotion in one batch, then the cheapest path over the pairs that passed), under this space's delta and lambda: `states` = the
  // waypoints on entry, the kept ones on return; kept (nullable) = their indices in the path as it came in.  On a library error the answer
  // is the unchanged path: false, `states` as it was, the first error in KinematicChainConstraint::lastError().  Follow it with
  // interpolatePath and the host's isValid over the dense rows: a shortcut leaves the edges the host validated.
  bool shortcutPath(std::vector<std::array<double, 14>> &states, int max_span = 0, std::vector<int32_t> *kept = nullptr) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      ccmp::check(ccmp::shortcutPathLocked(proj, states, max_span, kept, nullptr, nullptr, delta_, lambda_), "ccmp_path_shortcut_host");
    });
  }

  // B-spline smoothing passes on the manifold (ccmp::smoothPathLocked: PathSimplifier::smoothBSpline's structure with the library's
  // midpoint), under this space's delta and lambda: `states` = the waypoints on entry, the smoothed path on return (up to
  // 2^max_steps (L - 1) + 1 states).  On a library error the answer is the unchanged path: false, `states` as it was, the first error in
  // KinematicChainConstraint::lastError().  Use it behind shortcutPath and follow it with interpolatePath and the host's isValid.
  bool smoothPath(std::vector<std::array<double, 14>> &states, int max_steps = 5, double min_change = 0.005, int *passes = nullptr,
                  int *moved = nullptr) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      ccmp::check(ccmp::smoothPathLocked(proj, states, max_steps, min_change, passes, moved, nullptr, nullptr, nullptr, delta_, lambda_), "ccmp_path_smooth_host");
    });
  }

  // The path resampled at even arc for execution (ccmp::resamplePathLocked: PathGeometric::interpolate(count) with the library's blend),
  // under this space's delta and lambda: `states` = the waypoints on entry (behind smoothPath), count rows on return, or with
  // count_or_0 == 0 one every `spacing` of arc (spacing <= 0: this space's delta).  On a library error, or for a path that cannot be
  // resampled (a segment that stops short, a non-finite row), the answer is the unchanged path: false, `states` as it was, an error in
  // KinematicChainConstraint::lastError().  The rows between the first and the last are new states: the host's isValid comes next.
  bool resamplePath(std::vector<std::array<double, 14>> &states, int count_or_0 = 0, double spacing = 0.0, std::vector<uint8_t> *kinds = nullptr) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      int status = CCMP_RETIME_EMPTY;
      ccmp::check(ccmp::resamplePathLocked(proj, states, count_or_0, spacing, &status, kinds, delta_, lambda_), "ccmp_path_resample");
      if (status != CCMP_RETIME_OK && status != CCMP_RETIME_POINT && !states.empty()) ccmp::check(CCMP_EINVAL, "ccmp_path_resample: the path cannot be resampled");
    });
  }

  // Time stamps for the rows of a path (ccmp::timestampPath): vmax / amax = 14 joint velocity and acceleration limits, the path starting
  // and ending at rest.  false with `times` untouched when the call failed (KinematicChainConstraint::lastError()).
  bool timePath(const std::vector<std::array<double, 14>> &states, const double *vmax, const double *amax, std::vector<double> *times, double beta = 0.5,
                double *duration = nullptr) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      ccmp::check(ccmp::timestampPath(proj, states, vmax, amax, beta, times, duration), "ccmp_path_timestamps_host");
    });
  }

  // What a controller is commanded at every tick of `period` along the timed path, and the audit of that motion (ccmp::setpointPath):
  // states and times as timePath leaves them; scene (nullable) and margin for the ticks' clearance.  The setpoints are not projected; the
  // audit's peaks say how far the motion between the rows leaves the manifold and how it stands against the limits at the controller's
  // rate.  false with *out untouched when the call failed (KinematicChainConstraint::lastError()); a path the rule gives no ticks for
  // (out of order, not finite, over max_ticks) is true with its status in out->status.
  bool setpointPath(const std::vector<std::array<double, 14>> &states, const std::vector<double> &times, const double *vmax, const double *amax,
                    ccmp::Setpoints *out, double period = 0.001, int max_ticks = 65536, const ccmp_scene *scene = nullptr, double margin = 0.0) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      ccmp::check(ccmp::setpointPath(proj, states, times, vmax, amax, out, period, max_ticks, scene, margin), "ccmp_path_setpoints_host");
    });
  }

  // Time stamps fitted to the limits at the controller's rate (ccmp::fitPath), between timePath and setpointPath: only the row intervals in
  // which the commanded motion exceeds a limit are dilated, until the audit of setpointPath passes at the ticks of opts.period or
  // opts.max_passes dilations are spent (out->status).  false with *out untouched when the call failed
  // (KinematicChainConstraint::lastError()).
  bool fitPath(const std::vector<std::array<double, 14>> &states, const std::vector<double> &times, const double *vmax, const double *amax,
               ccmp::FittedTimes *out, const ccmp::FitOptions &opts = ccmp::FitOptions()) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      ccmp::check(ccmp::fitPath(proj, states, times, vmax, amax, out, opts), "ccmp_path_fit_timestamps_host");
    });
  }

  // Jerk-bounded setpoints (ccmp::jerkSetpointPath), beside setpointPath for a controller that limits jerk: a moving average of the
  // interpolant's ticks whose window is chosen until the jerk ratio at the ticks of opts.period is within 1 (out->status, out->window).
  // false with *out untouched when the call failed (KinematicChainConstraint::lastError()).
  bool jerkSetpointPath(const std::vector<std::array<double, 14>> &states, const std::vector<double> &times, const double *vmax, const double *amax,
                        const double *jmax, ccmp::JerkSetpoints *out, const ccmp::JerkOptions &opts = ccmp::JerkOptions(), const ccmp_scene *scene = nullptr,
                        double margin = 0.0) const noexcept
  {
    return chain_->guarded([&] {
      const ccmp::Projector &proj = chain_->impl();
      std::lock_guard<std::mutex> hold(proj.mutex());
      ccmp::check(ccmp::jerkSetpointPath(proj, states, times, vmax, amax, jmax, out, opts, scene, margin), "ccmp_path_jerk_setpoints_host");
    });
  }

private:
  // every traversal of this space: edges from[e] -> to, in one call of ccmp::discreteGeodesicBatch
  void traverse(const std::vector<const ompl::base::State *> &from, const ompl::base::State *to, bool interpolate,
                std::vector<std::vector<ompl::base::State *>> *geodesics, std::vector<char> *reached, bool check_target) const
  {
    const size_t E = from.size();
    std::vector<double> a(E * 14), b(E * 14);
    for (size_t e = 0; e < E; ++e) {
      ccmp::detail::load14(&a[14 * e], *from[e]->as<StateType>());
      ccmp::detail::load14(&b[14 * e], *to->as<StateType>());
    }
    ccmp::Projector &proj = chain_->impl();
    auto &&svc = si_->getStateValidityChecker();
    std::vector<std::vector<std::vector<double>>> lists;
    ompl::base::State *scratch = allocState();
    // with a device prefilter: the proxies inside the traversal, the exact checker alone on the listed states
    const PrefilteredValidityChecker *pre = devicePrefilter(svc.get(), interpolate);
    std::vector<char> blocked;
    const auto valid = [&](const double *q) {
      ccmp::detail::store14(*scratch->as<StateType>(), q);
      return pre ? pre->isValidExact(scratch) : svc->isValid(scratch);
    };
    const bool done = chain_->guarded([&] {  // delta_ / lambda_: setDelta / setLambda of the base class stay the source of truth
      ccmp::discreteGeodesicBatch(proj, a.data(), b.data(), E, interpolate, valid, geodesics ? &lists : nullptr, reached, 64, check_target, delta_, lambda_,
                                  pre ? pre->scene().get() : nullptr, pre ? pre->rejectBelow() : 0.0, pre ? &blocked : nullptr);
    });
    freeState(scratch);
    if (pre && done)
      for (size_t e = 0; e < E; ++e)
        if (blocked[e]) pre->countRejected();
    if (!done) {  // the GPU call failed (KinematicChainConstraint::lastError()): no edge was extended
      if (geodesics) geodesics->assign(E, {});
      if (reached) reached->assign(E, 0);
      return;
    }
    if (geodesics) {
      geodesics->assign(E, {});
      for (size_t e = 0; e < E; ++e)
        for (const auto &st : lists[e]) {
          ompl::base::State *s = allocState();
          ccmp::detail::store14(*s->as<StateType>(), st.data());
          (*geodesics)[e].push_back(s);
        }
    }
  }

  // the same for one edge: a failed GPU call is "not reached", no states
  bool traverse(const ompl::base::State *from, const ompl::base::State *to, bool interpolate, std::vector<ompl::base::State *> *geodesic,
                bool check_target) const
  {
    std::vector<std::vector<ompl::base::State *>> lists;
    std::vector<char> reached;
    traverse({from}, to, interpolate, geodesic ? &lists : nullptr, &reached, check_target);
    if (geodesic) *geodesic = std::move(lists[0]);
    return reached[0] != 0;
  }

  // the space information's checker when the extend step can run its proxies on the device: a PrefilteredValidityChecker whose
  // scene lives on this space's context, and interpolate == false (the checker is asked at all).  Its counters then count what
  // the reference's order counts: per listed state one exact question, one proxy refusal for an edge that ended at one.
  const PrefilteredValidityChecker *devicePrefilter(const ompl::base::StateValidityChecker *svc, bool interpolate) const
  {
    if (interpolate) return nullptr;
    const auto *pre = dynamic_cast<const PrefilteredValidityChecker *>(svc);
    if (!pre || !pre->scene() || pre->scene()->projector().ctx() != chain_->impl().ctx()) return nullptr;
    return pre;
  }

  std::shared_ptr<KinematicChainConstraint> chain_;
  uint64_t seed_;
  mutable std::atomic<uint64_t> samplers_{0};
};

// jy_MotionValidator (include/closed_chain_motion_planner/base/jy_ProjectedStateSpace.h:57-69): the same result —
// isSatisfied(s2) && discreteGeodesic(s1, s2, false) — from one launch (jy_ProjectedStateSpace::checkMotion above); a
// space of another type falls back to the reference's two calls.
class jy_MotionValidator : public ompl::base::ConstrainedMotionValidator {
public:
  jy_MotionValidator(const ompl::base::SpaceInformationPtr &si) : ompl::base::ConstrainedMotionValidator(si) {}
  bool checkMotion(const ompl::base::State *s1, const ompl::base::State *s2) const override
  {
    if (const auto *space = dynamic_cast<const jy_ProjectedStateSpace *>(&ss_)) return space->checkMotion(s1, s2);
    return ss_.getConstraint()->isSatisfied(s2) && ss_.discreteGeodesic(s1, s2, false);
  }
};

inline jy_ProjectedStateSampler::jy_ProjectedStateSampler(const jy_ProjectedStateSpace *space, ompl::base::StateSamplerPtr sampler, uint64_t seed)
  : ompl::base::WrapperStateSampler(space, std::move(sampler)),
    constraint_(std::dynamic_pointer_cast<KinematicChainConstraint>(space->getConstraint())),
    buffer_(constraint_->impl(), seed),
    near_(constraint_->impl(), seed, ccmp::RefSampleBuffer::Near),
    gauss_(constraint_->impl(), seed, ccmp::RefSampleBuffer::Gaussian)
{
}
// the reference's two-argument constructor (jy_ProjectedStateSpace.h:21): its own stream, like every other sampler
inline jy_ProjectedStateSampler::jy_ProjectedStateSampler(const jy_ProjectedStateSpace *space, ompl::base::StateSamplerPtr sampler)
  : jy_ProjectedStateSampler(space, std::move(sampler), space->nextSamplerSeed())
{
}

#endif  // CCMP_WITH_OMPL

#endif  // CCMP_OMPL_ADAPTER_HPP
