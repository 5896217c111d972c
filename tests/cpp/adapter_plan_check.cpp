// ccmp::PlanOptions / ccmp::Planner (include/ccmp_ompl_adapter.hpp) against the interface mock: the planner's verbs compile as C++14,
// and a planner that could not be opened (no store here: no context, no device) answers "no" to every verb, throws nothing and keeps
// the library's own first error (CCMP_ENODEV on a machine without a device, CCMP_EINVAL with one) until clearError().
#include <cstdio>
#include <cstring>

#include "ccmp_ompl_adapter.hpp"

int main()
{
  ccmp::PlanOptions o;
  std::printf("defaults width %d k %d attempts %d max_states %d t %.1f sigma %.1f max_vertices %llu\n", o.width, o.k, o.attempts, o.max_states, o.t, o.sigma,
              (unsigned long long)o.max_vertices);
  ccmp_problem p;
  std::memset(&p, 0, sizeof p);
  ccmp::Planner none(nullptr, p, nullptr, o);
  const bool ran = none.run(4);
  ccmp_plan_state s;
  const bool read = none.state(&s);
  std::printf("none create %d run %d state %d solved %d status %d first %d message %d\n", none.create() ? 1 : 0, ran ? 1 : 0, read ? 1 : 0, none.solved() ? 1 : 0,
              none.status(), none.lastError(), none.lastErrorMessage().empty() ? 0 : 1);
  const int first = none.lastError();
  none.run(1);
  std::printf("none kept %d\n", none.lastError() == first ? 1 : 0);
  none.clearError();
  const int cleared = none.lastError();
  none.run(1);
  std::printf("none cleared %d then %d\n", cleared, none.lastError());
  // the one-call form exists on ccmp::Roadmap with this signature
  int (ccmp::Roadmap::*solve)(const ccmp_object *, int, int32_t *, int32_t *, const ccmp_plan_opts *, const ccmp_scene *, double, const double *, uint64_t,
                              ccmp_plan_report *) noexcept = &ccmp::Roadmap::solve;
  std::printf("solve %d\n", solve != nullptr ? 1 : 0);
  return 0;
}
