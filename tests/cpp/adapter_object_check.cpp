// ccmp::ObjectChecker (include/ccmp_ompl_adapter.hpp) against the interface mock: every question of stefanFCL compiles — on an
// Eigen::Isometry3d, on an SE3 state pointer, on (pos, quat) — and on a checker that could not be created (no context here) every one
// answers "no", throws nothing and keeps the first error.  With a configuration file as argument (a device is then needed) the same
// questions are asked of a working checker and compared with ccmp_object_valid_ref / ccmp_object_propose_ref.
#include <Eigen/Dense>
#include <cstdio>
#include <cstring>

#include "ccmp_ompl_adapter.hpp"

namespace {

// what ompl::base::SE3StateSpace::StateType offers, as far as ccmp::poseOf reads it
struct Se3 {
  double p[3], q[4];
  struct Rot { double x, y, z, w; };
  double getX() const { return p[0]; }
  double getY() const { return p[1]; }
  double getZ() const { return p[2]; }
  Rot rotation() const { return Rot{q[0], q[1], q[2], q[3]}; }
};

void cube(double h, double *tri /* [12][9] */)
{
  static const int quad[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
  double c[8][3];
  for (int i = 0; i < 8; i++) { c[i][0] = (i & 4) ? h : -h; c[i][1] = (i & 2) ? h : -h; c[i][2] = (i & 1) ? h : -h; }
  int t = 0;
  for (const auto &q : quad)
    for (int half = 0; half < 2; half++, t++) {
      const int v[3] = {q[0], q[half ? 2 : 1], q[half ? 3 : 2]};
      for (int k = 0; k < 3; k++) memcpy(tri + t * 9 + k * 3, c[v[k]], sizeof c[0]);
    }
}

void workspace(ccmp_box *b /* [6] */)
{
  static const double c[6][3] = {{0.65, 0, 1.1}, {-0.05, 0, 1.0}, {1.35, 0, 1.0}, {0.75, -0.6, 1.0}, {0.75, 0.6, 1.0}, {0.95, 0, 1.9}};
  static const double h[6][3] = {{0.325, 0.5, 0.1}, {0.05, 0.5, 0.5}, {0.05, 0.5, 0.5}, {0.5, 0.05, 1.0}, {0.5, 0.05, 1.0}, {0.5, 0.3, 0.05}};
  memset(b, 0, 6 * sizeof *b);
  for (int i = 0; i < 6; i++) {
    memcpy(b[i].c, c[i], sizeof c[i]);
    memcpy(b[i].half, h[i], sizeof h[i]);
    b[i].R[0] = b[i].R[4] = b[i].R[8] = 1.0;
  }
}

}  // namespace

int main(int argc, char **argv)
{
  double tri[12 * 9];
  ccmp_box boxes[6];
  cube(0.02, tri);
  workspace(boxes);
  const double free_pose[8] = {0.65, 0.0, 1.5, 0, 0, 0, 1, 0}, goal[8] = {0.75, 0.1, 1.6, 0, 0, 0, 1, 0};
  Eigen::Isometry3d T;
  T.setIdentity();
  for (int i = 0; i < 3; i++) T.translation()(i) = free_pose[i];
  Se3 s{{0.65, 0.0, 1.5}, {0, 0, 0, 1}};
  {
    // no context: the checker cannot exist, and says so through every question
    ccmp::ObjectChecker none(static_cast<ccmp_ctx *>(nullptr), tri, 12, boxes, 6);
    const int first = none.lastError();
    double out[8];
    int which = 7;
    std::vector<double> rows;
    const bool a = none.isValid(T), b = none.isValid(&s), c = none.is_Valid(free_pose, free_pose + 3), d = none.isValidPose(free_pose);
    const bool e = none.propose(free_pose, goal, out, &which);
    const int n = none.ladder(free_pose, goal, &rows);
    printf("none answers %d%d%d%d%d ladder %d which %d nan %d rows %zu triangles %d first %d kept %d message %d\n", a, b, c, d, e, n, which, out[0] != out[0],
           rows.size(), none.numTriangles(), first, none.lastError() == first, !none.lastErrorMessage().empty());
    none.clearError();
    const int cleared = none.lastError();
    (void)none.isValidPose(free_pose);
    printf("none cleared %d then %d\n", cleared, none.lastError());
    // bad arguments are an argument error whatever the machine
    ccmp::ObjectChecker bad(static_cast<ccmp_ctx *>(nullptr), tri, 0, boxes, 6);
    const int bad_first = bad.lastError();
    printf("bad first %d answers %d\n", bad_first, bad.isValid(T));
  }
  if (argc < 2) return 0;
  ccmp::Projector proj(argv[1]);
  ccmp::ObjectChecker chk(proj, tri, 12, boxes, 6);
  int mismatches = chk.lastError() != 0;
  const double in_table[8] = {0.65, 0.0, 1.1, 0, 0, 0, 1, 0};
  Se3 st{{0.65, 0.0, 1.1}, {0, 0, 0, 1}};
  printf("device free %d%d%d table %d%d triangles %d\n", chk.isValid(T), chk.isValid(&s), chk.is_Valid(free_pose, free_pose + 3), chk.isValidPose(in_table),
         chk.isValid(&st), chk.numTriangles());
  const double lo[3] = {0.1, -0.5, 1.15}, hi[3] = {1.2, 0.5, 1.8};
  chk.setBounds(lo, hi);
  chk.setStream(0xC0FFEE, 100);
  int found = 0;
  for (int n = 0; n < 12; n++) {
    const double from[8] = {0.45 + 0.02 * n, 0.0, 1.25, 0, 0, 0, 1, 0};
    double out[8], ref[8];
    int which = -2;
    int32_t ref_which = -2;
    const bool ok = chk.propose(from, goal, out, &which);
    const int rc = ccmp_object_propose_ref(tri, 12, boxes, 6, from, goal, 0, 1, 0.3, 0.2, lo, hi, 2, 0xC0FFEE, 100 + (uint64_t)n, 0.0, ref, &ref_which, nullptr, nullptr);
    const bool same = rc == 0 && which == ref_which && ok == (ref_which >= 0) && (ok ? memcmp(out, ref, sizeof out) == 0 : out[0] != out[0]);
    mismatches += !same;
    found += ok;
    printf("propose n=%d ok=%d which=%d agree=%d\n", n, ok, which, same);
  }
  std::vector<double> rows;
  const int n = chk.ladder(free_pose, in_table, &rows);
  uint8_t ref_valid[9];
  mismatches += ccmp_object_valid_ref(tri, 12, boxes, 6, rows.data(), 9, 0.0, 1, ref_valid, nullptr) != 0;
  int ref_n = 0;
  while (ref_n < 9 && ref_valid[ref_n]) ref_n++;
  printf("ladder %d ref %d next %llu\n", n, ref_n, (unsigned long long)chk.nextIndex());
  // a failing call: "no", NaN, the first error kept
  double out[8];
  const bool failed = chk.propose(free_pose, goal, out, nullptr, 0.3, 0.2, 17);
  printf("summary found %d mismatches %d failed %d nan %d sticky %d\n", found, mismatches + (n != ref_n), failed, out[0] != out[0], chk.lastError());
  return 0;
}
