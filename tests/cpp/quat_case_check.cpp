// quat_case_check.cpp — host check of the quaternion's case bodies (ccmp_kin.h: quat_case, quat_of_t), in the det oracle's rounding
// model (-ffp-contract=off -DCCMP_USE_FMA):
//   1. quat_case<k> — the ONE branch the STOCK throughput kernels enter behind a scalar branch when a whole wavefront agrees on
//      the case — gives quat_of's four doubles bit for bit, and so does quat_of_t<true> (on the host: the branch-free text
//      with the lean root and quotient), over
//        a. random rotations of every case,
//        b. matrices at and beside each case boundary: tr = 0 and its neighbours by 1..3 ulp of an entry, two and three equal
//           largest diagonal entries (with tr on either side of 0),
//        c. the relative rotation init_chain_ of the fixture at its initial pose,
//        d. relative rotations R2^T R1 produced by the two chains at random states: inside the joint limits, and anywhere in the
//           in-range round's |x_j| <= 512;
//   2. the radicand lemma on the same matrices: the radicand quat_of selects is >= 1 - 2^-40 (ccmp_kin.h states why), and the root
//      lies in [1 - 2^-40, 2 + 2^-40]: the operands of the lean root and quotient are plain.
// usage: quat_case_check <config.yaml> <random rotations> <chain states>; prints one line of counts, exit status 0 iff nothing
// differed.  (tests/test_quat_case_host.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ccmp_host.h"

using namespace ccmp;

namespace {

uint64_t g_state = 0x0C0A7CA5Eull;
uint64_t next_u64() { return g_state = splitmix64(g_state); }
double uniform(double lo, double hi) { return lo + (hi - lo) * ((double)(next_u64() >> 11) * 0x1p-53); }

void rotation_of_quat(double x, double y, double z, double w, double *R)
{
  const double n = std::sqrt(x * x + y * y + z * z + w * w);
  x /= n; y /= n; z /= n; w /= n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}
void random_rotation(double *R)
{
  double q[4], n;
  do {
    n = 0.0;
    for (int k = 0; k < 4; k++) { q[k] = uniform(-1.0, 1.0); n += q[k] * q[k]; }
  } while (n < 1e-3 || n > 1.0);
  rotation_of_quat(q[0], q[1], q[2], q[3], R);
}

struct Counts {
  long cases[4] = {0, 0, 0, 0}, checked = 0, differ = 0, form_differ = 0, radicand_low = 0, root_out = 0;
  double radicand_min = 1e300, radicand_max = -1e300;
};

void check(const double *m, Counts &n, const char *what)
{
  const double tr = (m[0] + m[4]) + m[8];
  const int kase = quat_kase(m, tr);
  double qa[4], qb[4], qc[4];
  quat_of(m, qa);
  quat_case_rt(kase, m, qb);
  quat_of_t<true>(m, qc);
  n.checked++;
  n.cases[kase]++;
  if (memcmp(qa, qb, sizeof qa) != 0) {
    if (n.differ++ < 5) fprintf(stderr, "quat_case<%d> differs from quat_of (%s): m = %a %a %a / %a %a %a / %a %a %a\n", kase, what, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]);
  }
  if (memcmp(qa, qc, sizeof qa) != 0) {
    if (n.form_differ++ < 5) fprintf(stderr, "quat_of_t<true> differs from quat_of (%s), case %d\n", what, kase);
  }
  const double rad = quat_radicand(m);
  if (rad < n.radicand_min) n.radicand_min = rad;
  if (rad > n.radicand_max) n.radicand_max = rad;
  if (!(rad >= 1.0 - 0x1p-40)) {
    if (n.radicand_low++ < 5) fprintf(stderr, "radicand %a below 1 - 2^-40 (%s), case %d\n", rad, what, kase);
  }
  const double t = std::sqrt(rad);
  if (!(t >= 1.0 - 0x1p-40 && t <= 2.0 + 0x1p-40)) n.root_out++;
}

// m and its neighbours: entry e moved by 1..3 ulp either way
void check_around(const double *m, int e, Counts &n, const char *what)
{
  check(m, n, what);
  for (int step = 1; step <= 3; step++)
    for (int side = 0; side < 2; side++) {
      double b[9];
      memcpy(b, m, sizeof b);
      for (int t = 0; t < step; t++) b[e] = std::nextafter(b[e], side ? INFINITY : -INFINITY);
      check(b, n, what);
    }
}

} // namespace

int main(int argc, char **argv)
{
  if (argc < 4) return 2;
  ccmp_problem P;
  if (ccmp_problem_from_yaml(argv[1], &P) != CCMP_OK) return 3;
  const long n_rot = atol(argv[2]), n_chain = atol(argv[3]);
  ccmp_consts K;
  ccmp_host::make_consts(P, K);

  // ---- a. random rotations: every case occurs -------------------------------------------------------------------------------
  Counts ra;
  for (long k = 0; k < n_rot; k++) {
    double R[9];
    random_rotation(R);
    check(R, ra, "random rotation");
  }
  // rotations by pi about axes near the coordinate axes and near the diagonals: trace -1, the cases 0, 1, 2 and their borders
  for (long k = 0; k < n_rot / 8; k++) {
    double R[9];
    const int ax = (int)(next_u64() % 7);
    double a[3] = {ax == 0 || ax == 3 || ax == 4 || ax == 6 ? 1.0 : 0.0, ax == 1 || ax == 3 || ax == 5 || ax == 6 ? 1.0 : 0.0,
                   ax == 2 || ax == 4 || ax == 5 || ax == 6 ? 1.0 : 0.0};
    for (int c = 0; c < 3; c++) a[c] += uniform(-1e-3, 1e-3);
    rotation_of_quat(a[0], a[1], a[2], uniform(-1e-3, 1e-3), R);
    check(R, ra, "half turn");
  }

  // ---- b. the boundaries ------------------------------------------------------------------------------------------------------
  Counts rb;
  long tr_zero = 0, tr_pos = 0, tr_neg = 0, ties2 = 0, ties3 = 0;
  for (long k = 0; k < n_rot / 8; k++) {
    // angle 2 pi / 3 about a random axis has trace 0 up to rounding; the last diagonal entry then makes it 0 exactly
    double a[3], R[9];
    for (int c = 0; c < 3; c++) a[c] = uniform(-1.0, 1.0);
    const double an = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (an < 1e-3) continue;
    const double sh = std::sin(M_PI / 3.0) / an;
    rotation_of_quat(a[0] * sh, a[1] * sh, a[2] * sh, std::cos(M_PI / 3.0), R);
    const int e = 4 * (int)(next_u64() % 3);
    double others = 0.0;
    if (e == 8) { R[8] = -(R[0] + R[4]); }
    else if (e == 4) { R[4] = -R[8] - R[0]; others = (R[0] + R[4]) + R[8]; if (others != 0.0) R[4] = std::nextafter(R[4], others > 0 ? -INFINITY : INFINITY); }
    else { R[0] = -R[8] - R[4]; others = (R[0] + R[4]) + R[8]; if (others != 0.0) R[0] = std::nextafter(R[0], others > 0 ? -INFINITY : INFINITY); }
    const double tr = (R[0] + R[4]) + R[8];
    if (tr == 0.0) tr_zero++;
    check_around(R, e, rb, "trace zero");
    for (int side = 0; side < 2; side++) { // the neighbours by one ulp OF THE TRACE: the smallest entry's ulp moves it
      double b[9];
      memcpy(b, R, sizeof b);
      b[8] = std::nextafter(b[8], side ? INFINITY : -INFINITY);
      const double t2 = (b[0] + b[4]) + b[8];
      if (t2 > 0.0) tr_pos++;
      if (t2 < 0.0) tr_neg++;
      check(b, rb, "trace beside zero");
    }
  }
  for (long k = 0; k < n_rot / 8; k++) {
    double R[9];
    random_rotation(R);
    // two equal largest diagonal entries (each pair), then all three; the trace falls where it falls, and is pushed below zero
    // for half of them by a half turn's diagonal
    if (k & 1) {
      const double x = uniform(-1.0, 1.0), y = uniform(-1.0, 1.0), z = uniform(-1.0, 1.0);
      rotation_of_quat(x, y, z, uniform(-1e-2, 1e-2), R);
    }
    const int pair = (int)(next_u64() % 3);
    const int i0 = pair == 0 ? 0 : (pair == 1 ? 4 : 0), i1 = pair == 0 ? 4 : 8, i2 = 12 - i0 - i1;
    const double big = R[i0] > R[i1] ? R[i0] : R[i1];
    R[i0] = big;
    R[i1] = big;
    if (R[i2] < big) ties2++;
    check_around(R, i0, rb, "two equal diagonal entries");
    check_around(R, i1, rb, "two equal diagonal entries");
    R[i2] = big;
    ties3++;
    check_around(R, i2, rb, "three equal diagonal entries");
  }

  // ---- c. the fixture's relative rotation at its initial pose ----------------------------------------------------------------
  Counts rc;
  check_around(P.init_R, 0, rc, "init_chain_");
  check_around(P.init_R, 4, rc, "init_chain_");
  check_around(P.init_R, 8, rc, "init_chain_");
  const double init_tr = (P.init_R[0] + P.init_R[4]) + P.init_R[8];
  const int init_case = quat_kase(P.init_R, init_tr);

  // ---- d. relative rotations of the two chains at random states --------------------------------------------------------------
  Counts rd;
  for (long k = 0; k < n_chain; k++) {
    double q[14], R1[9], p1[3], R2[9], p2[3], Rc[9];
    for (int j = 0; j < 14; j++) q[j] = (k & 1) ? uniform(-512.0, 512.0) : uniform(K.lb[j % 7], K.ub[j % 7]);
    fk_arm(K, 0, q, R1, p1);
    fk_arm(K, 1, q + 7, R2, p2);
    mulT33(R2, R1, Rc);
    check(Rc, rd, "chain");
  }

  const Counts *all[4] = {&ra, &rb, &rc, &rd};
  long differ = 0, form_differ = 0, radicand_low = 0, root_out = 0, checked = 0;
  double rmin = 1e300, rmax = -1e300;
  for (const Counts *c : all) {
    differ += c->differ; form_differ += c->form_differ; radicand_low += c->radicand_low; root_out += c->root_out; checked += c->checked;
    if (c->radicand_min < rmin) rmin = c->radicand_min;
    if (c->radicand_max > rmax) rmax = c->radicand_max;
  }
  printf("{\"checked\": %ld, \"differ\": %ld, \"form_differ\": %ld, \"radicand_low\": %ld, \"root_out\": %ld, \"radicand_min_minus_1\": %.3e, "
         "\"radicand_max\": %.17g, \"random_cases\": [%ld, %ld, %ld, %ld], \"boundary_cases\": [%ld, %ld, %ld, %ld], \"tr_zero\": %ld, \"tr_pos\": %ld, "
         "\"tr_neg\": %ld, \"ties2\": %ld, \"ties3\": %ld, \"init_case\": %d, \"init_trace\": %.17g, \"chain_cases\": [%ld, %ld, %ld, %ld], \"chain\": %ld}\n",
         checked, differ, form_differ, radicand_low, root_out, rmin - 1.0, rmax, ra.cases[0], ra.cases[1], ra.cases[2], ra.cases[3], rb.cases[0],
         rb.cases[1], rb.cases[2], rb.cases[3], tr_zero, tr_pos, tr_neg, ties2, ties3, init_case, init_tr, rd.cases[0], rd.cases[1], rd.cases[2],
         rd.cases[3], rd.checked);
  return (differ || form_differ || radicand_low || root_out) ? 1 : 0;
}
