// rot_x0_check.cpp — host check of the two cuts of the throughput kernel's STOCK instantiations (ccmp_kin.h), in the det oracle's
// rounding model (-ffp-contract=off -DCCMP_USE_FMA):
//   1. rot_sc_x0 == rot_sc in all 72 bytes wherever rot_x0_admits holds, for the stock constants' four general joints, and the
//      guard turns away nothing but angles within 2^-26 of zero (and NaN); an iterate that passes the kernels' once-per-round test
//      rot_x0_round_ok has all six stencil points of its column inside that guard;
//   2. chain_residual on (tool_pose_fold, fold_other_pose) == chain_residual on tool_pose_t<true>, both components, both
//      orientations, all eight sign patterns of the diag(+-1) base frame, random frames;
//   3. the set-up raises ccmp_consts::rot_x0 for the stock constants and for nothing else.
// usage: rot_x0_check <config.yaml> <angles per joint> <frames per sign pattern and orientation>; prints one line of counts,
// exit status 0 iff nothing differed.  (tests/test_rot_x0_host.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ccmp_host.h"

using namespace ccmp;

namespace {

uint64_t g_state = 0x5EEDC0DEull;
uint64_t next_u64() { return g_state = splitmix64(g_state); }
double uniform(double lo, double hi) { return lo + (hi - lo) * ((double)(next_u64() >> 11) * 0x1p-53); }

void random_rotation(double *R)
{
  double q[4], n = 0.0;
  do {
    n = 0.0;
    for (int k = 0; k < 4; k++) { q[k] = uniform(-1.0, 1.0); n += q[k] * q[k]; }
  } while (n < 1e-3 || n > 1.0);
  n = std::sqrt(n);
  const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}

struct RotCounts { long admitted = 0, refused = 0, differ = 0, refused_far = 0; };

void check_angle(const ccmp_consts &K, int arm, int joint, double q, RotCounts &n)
{
  double s, c, A[9], B[9];
  ccmp_sincos(q, &s, &c);
  if (!rot_x0_admits(c)) {
    n.refused++;
    if (c == c && std::fabs(q) > 0x1p-26) n.refused_far++; // (beyond CCMP_SINCOS_MAX sincos gives NaN: refused, rightly)
    return;
  }
  n.admitted++;
  rot_sc(K.axis[arm][joint], K.aprod[arm][joint], s, c, A);
  rot_sc_x0(K.axis[arm][joint], K.aprod[arm][joint], s, c, B);
  if (memcmp(A, B, sizeof A) != 0) {
    if (n.differ++ < 5) fprintf(stderr, "rot_sc_x0 differs: arm %d joint %d angle %a\n", arm, joint, q);
  }
}

} // namespace

int main(int argc, char **argv)
{
  if (argc < 4) return 2;
  ccmp_problem P;
  if (ccmp_problem_from_yaml(argv[1], &P) != CCMP_OK) return 3;
  const long n_angles = atol(argv[2]), n_frames = atol(argv[3]);
  ccmp_consts K;
  ccmp_host::make_consts(P, K);
  if (!(K.stock && K.twin_arms && K.rot_x0)) { fprintf(stderr, "stock constants without rot_x0\n"); return 4; }
  for (int a = 0; a < 2; a++)
    for (int i = 0; i < 7; i++)
      if (!(K.axis[a][i][0] == 0.0)) return 4;

  // ---- 1. the short rotation ------------------------------------------------------------------------------------------
  const double pi = 3.14159265358979323846;
  std::vector<double> special = {0.0, pi / 2, pi, pi / 4, 3 * pi / 4, 5e-324, 1e-310, 0x1p-1022, 1e-300, 1e-200, 1e-100, 1e-30, 1e-20,
                                 1e-12, 1e-9, 1e-8, 1.0536712127723509e-08 /* 2^-26.5 */, 0x1p-27, 0x1p-26, 0x1p-25, 2e-8, 1e-7, 1e-4,
                                 2.8973, 1.7628, 3.0718, 0.0698, 3.7525, 0.0175, CCMP_SINCOS_MAX, 2.0 * CCMP_SINCOS_MAX, 1e300};
  for (size_t k = 0, m = special.size(); k < m; k++)
    for (int step = 1; step <= 3; step++) { // neighbours: the guard's edge sits between two of them
      double up = special[k], dn = special[k];
      for (int t = 0; t < step; t++) { up = std::nextafter(up, INFINITY); dn = std::nextafter(dn, -INFINITY); }
      special.push_back(up);
      special.push_back(dn);
    }
  special.push_back(INFINITY);
  special.push_back(NAN);
  RotCounts rc;
  const int general[4] = {1, 3, 5, 6};
  for (int arm = 0; arm < 2; arm++)
    for (int g = 0; g < 4; g++) {
      const int j = general[g];
      for (double v : special) { check_angle(K, arm, j, v, rc); check_angle(K, arm, j, -v, rc); }
      for (long k = 0; k < n_angles; k++) {
        double q;
        switch (k & 7) {
        case 0: q = std::ldexp(uniform(1.0, 2.0), (int)(next_u64() % 1080) - 1076); break;   // every magnitude down to the subnormals
        case 1: q = std::ldexp(uniform(1.0, 2.0), (int)(next_u64() % 12) - 32); break;       // around the guard's edge, 2^-32 .. 2^-20
        case 2: q = uniform(K.lb[j], K.ub[j]); break;                                         // the joint's range
        case 3: q = pi * (double)((long)(next_u64() % 5) - 2) / 2.0 + uniform(-1e-7, 1e-7); break; // beside multiples of pi/2
        default: q = uniform(-pi, pi); break;
        }
        if ((k & 7) < 2 && (next_u64() & 1)) q = -q;
        check_angle(K, arm, j, q, rc);
      }
    }

  // ---- 1b. the round's test (rot_x0_round_ok on the iterate) admits all six stencil points of the column, formed as the kernel
  // forms them (ccmp_kernels_fd.hip: jacobian_columns)
  long round_ok = 0, round_refused = 0, stencil_refused = 0;
  for (long k = 0; k < 2 * n_angles; k++) {
    double x;
    const double turns = 2.0 * pi * (double)((long)(next_u64() % 163) - 81); // multiples of 2 pi up to +-509
    switch (k & 3) {
    case 0: x = turns + std::ldexp(uniform(1.0, 2.0), -(int)(next_u64() % 34)) * ((next_u64() & 1) ? 1.0 : -1.0); break; // 2^-33 .. 2 beside one
    case 1: x = turns + uniform(-2e-4, 2e-4); break;                                                                    // around the test's edge
    case 2: x = uniform(-520.0, 520.0); break;
    default: x = uniform(-pi, pi); break;
    }
    double s, c;
    ccmp_sincos(x, &s, &c);
    if (!rot_x0_round_ok(x, c)) { round_refused++; continue; }
    round_ok++;
    const double ax = std::fabs(x);
    const double h = 1.4901161193847656e-08 * (ax >= 1 ? ax : 1);
    for (int side = 0; side < 2; side++) {
      const double hh = side ? -h : h;
      double y = x;
      for (int step = 0; step < 3; step++) {
        y = y + hh;
        double sy, cy;
        ccmp_sincos(y, &sy, &cy);
        if (!rot_x0_admits(cy)) stencil_refused++;
      }
    }
  }

  // ---- 2. the folded base frame ---------------------------------------------------------------------------------------
  long fold_cases = 0, fold_differ = 0;
  for (int arm = 0; arm < 2; arm++)
    for (int pat = 0; pat < 8; pat++) {
      ccmp_consts K2 = K;
      for (int r = 0; r < 3; r++) K2.base_R[arm][4 * r] = ((pat >> r) & 1) ? -1.0 : 1.0;
      for (long n = 0; n < n_frames; n++) {
        double R[9], o[3], To[12];
        random_rotation(R);
        random_rotation(To);
        for (int k = 0; k < 3; k++) {
          o[k] = uniform(-1.0, 1.0);
          To[9 + k] = uniform(-1.5, 1.5);
          K2.base_p[arm][k] = (n % 4 == 3) ? 0.0 : ((n % 4 == 2) ? K.base_p[arm][k] : uniform(-1.5, 1.5));
          K2.base_dp[arm][k] = K2.base_R[arm][4 * k] * K2.base_p[arm][k];
        }
        if (n % 64 == 63) { // the chain's frame at the origin: zeros everywhere
          for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
          o[0] = o[1] = o[2] = 0.0;
        }
        double Rw[9], pw[3], Rf[9], pl[3], f[2], fti[2], g[2], gti[2], Tf[12], ti[3];
        tool_pose_t<true>(K2, arm, R, o, Rw, pw);
        tool_pose_fold<true>(K2, arm, R, o, Rf, pl);
        memcpy(Tf, To, sizeof Tf);
        if (arm == 0) {
          mulTvec(&To[0], &To[9], ti);
          chain_residual(K2, Rw, pw, &To[0], &To[9], f, nullptr, nullptr);
          chain_residual_ti(K2, Rw, pw, &To[0], ti, fti, nullptr, nullptr);
          fold_other_pose<true>(K2, 0, Tf);
          chain_residual(K2, Rf, pl, &Tf[0], &Tf[9], g, nullptr, nullptr);       // without the hoisted ti: translation scaled too
          chain_residual_ti(K2, Rf, pl, &Tf[0], ti, gti, nullptr, nullptr);      // the shipped form: ti from the unscaled pose
        } else {
          chain_residual(K2, &To[0], &To[9], Rw, pw, f, nullptr, nullptr);
          fold_other_pose<true>(K2, 1, Tf);
          chain_residual(K2, &Tf[0], &Tf[9], Rf, pl, g, nullptr, nullptr);
          memcpy(fti, f, sizeof f);
          memcpy(gti, g, sizeof g);
        }
        fold_cases++;
        if (memcmp(f, g, sizeof f) != 0 || memcmp(fti, gti, sizeof f) != 0 || memcmp(f, fti, sizeof f) != 0) {
          if (fold_differ++ < 5) fprintf(stderr, "folded residual differs: arm %d pattern %d case %ld\n", arm, pat, n);
        }
      }
    }

  // ---- 3. the flag: raised for the stock constants (above), not for calibrated arms, nor for an x component that is not zero
  int flag_calibrated, flag_tilted;
  {
    ccmp_problem Q = P;
    double dh[7][4] = {};
    dh[2][3] = 1e-3; // alpha of joint 2: tilts every axis behind it
    if (ccmp_set_calibration(&Q, 0, dh) != CCMP_OK || ccmp_set_calibration(&Q, 1, dh) != CCMP_OK) return 5;
    ccmp_consts KQ;
    ccmp_host::make_consts(Q, KQ);
    flag_calibrated = KQ.rot_x0;
    Q = P;
    Q.axis[0][3][0] = Q.axis[1][3][0] = 1e-300; // still the stock structure (twin arms), but rot_sc's a0 terms are no zeros
    ccmp_host::make_consts(Q, KQ);
    flag_tilted = KQ.twin_arms ? KQ.rot_x0 : -1;
  }

  printf("{\"round_ok\": %ld, \"round_refused\": %ld, \"stencil_refused\": %ld, \"flag_calibrated\": %d, \"flag_tilted\": %d, \"admitted\": %ld, \"refused\": %ld, \"refused_far\": %ld, \"rot_differ\": %ld, \"fold_cases\": %ld, \"fold_differ\": %ld}\n",
         round_ok, round_refused, stencil_refused, flag_calibrated, flag_tilted, rc.admitted, rc.refused, rc.refused_far, rc.differ, fold_cases, fold_differ);
  return (rc.differ || rc.refused_far || stencil_refused || fold_differ || flag_calibrated != 0 || flag_tilted != 0) ? 1 : 0;
}
