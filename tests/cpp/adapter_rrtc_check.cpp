// ccmp::RRTConnectOptions / ccmp::RRTConnectPlanner (include/ccmp_ompl_adapter.hpp) against the interface mock: the planner's verbs
// compile as C++14, and a planner that could not be opened (no store here: no context, no device) answers "no" to every verb, throws
// nothing and keeps the library's own first error (CCMP_ENODEV on a machine without a device, CCMP_EINVAL with one) until clearError().
#include <cstdio>
#include <cstring>

#include "ccmp_ompl_adapter.hpp"

int main()
{
  ccmp::RRTConnectOptions o;
  std::printf("defaults width %d max_states %d round_budget %d range %.1f max_vertices %llu\n", o.width, o.max_states, o.round_budget, o.range,
              (unsigned long long)o.max_vertices);
  ccmp_problem p;
  std::memset(&p, 0, sizeof p);
  const int32_t s[1] = {0}, g[1] = {1};
  ccmp::RRTConnectPlanner none(nullptr, p, s, 1, g, 1, o);
  const bool ran = none.run(4);
  ccmp_rrtc_state st;
  const bool read = none.state(&st);
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
  int (ccmp::Roadmap::*solve)(const int32_t *, int, const int32_t *, int, int, int32_t *, int32_t *, const ccmp_rrtc_opts *, const ccmp_scene *, double, uint64_t,
                              ccmp_rrtc_report *) noexcept = &ccmp::Roadmap::solveRRTConnect;
  std::printf("solve %d\n", solve != nullptr ? 1 : 0);
  return 0;
}
