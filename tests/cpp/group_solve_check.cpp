// group_solve_check.cpp — host check of the throughput layout's minimum-norm solve (ccmp_fd_newton_phase2.inc):
// the pieces of ccmp_solve.h (minnorm_sum_step, minnorm_sweep_coeffs, minnorm_rotate, minnorm_final_coeffs,
// minnorm_dx, minnorm_group_slot) composed as the kernels compose them — six virtual lanes on one group record, lane r owning
// columns r, r + 6, r + 12, lanes 0..2 (and again 3..5) forming one serial sum each from the record, the sums published in the
// record, every lane running the scalar part, the rotated columns written back in place — against the one-lane solve_minnorm, in
// the det oracle's rounding model (-ffp-contract=off -DCCMP_USE_FMA).  The statements between two barriers of the kernel text are
// one loop over the lanes here.
// usage: group_solve_check <cases.bin> <out.bin>.  cases: records of 30 doubles (J[28] as row 0 | row 1, f[2]); out: records of 30
// doubles (dx[14] of solve_minnorm, dx[14] of the six lanes, 1.0 where the first / the second sweep found b == 0 exactly).
// (tests/test_group_solve_host.py compares both with the oracle's orc_solve_minnorm.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ccmp_solve.h"

using namespace ccmp;

namespace {

// the record's layout (ccmp_kernels_fd.hip): arm 0's columns at kJ0, arm 1's in arm 0's sin/cos slots, the sums in the prefix region
constexpr int kX = 0, kSC = 14, kPre = 42, kJ0 = 150, kRec = 165, kGroup = 6;

void group_solve(const double *J, double f0, double f1, double step, double *x /* 14, updated */, double *dx_out, double *bzero)
{
  double rec[kRec];
  for (int k = 0; k < kRec; k++) rec[k] = -12345.0;
  for (int e = 0; e < 14; e++) {
    rec[kX + e] = x[e];
    const int slot = minnorm_group_slot(e, kJ0, kSC); // where stencil_combine<0> / <1> leave column e
    rec[slot] = J[e];
    rec[slot + 1] = J[14 + e];
  }
  constexpr int kSums = kPre;
  struct Lane { int kind, e0, e1, e2; bool own2; double v0[3], v1[3], g0, g1; } L[kGroup];
  for (int r = 0; r < kGroup; r++) {
    Lane &l = L[r];
    l.kind = r < 3 ? r : r - 3;
    l.e0 = kJ0 + 2 * r;
    l.e1 = r == 0 ? kJ0 + 12 : kSC + 2 * (r - 1);
    l.e2 = kSC + (r == 0 ? 10 : 12);
    l.own2 = r < 2;
    l.v0[0] = rec[l.e0]; l.v1[0] = rec[l.e0 + 1];
    l.v0[1] = rec[l.e1]; l.v1[1] = rec[l.e1 + 1];
    l.v0[2] = rec[l.e2]; l.v1[2] = rec[l.e2 + 1];
    l.g0 = f0; l.g1 = f1;
  }
  for (int pass = 0; pass < 3; pass++) {
    for (int r = 0; r < kGroup; r++) { // up to the first barrier of the pass
      const double *px = rec + (L[r].kind == 1 ? 1 : 0), *py = rec + (L[r].kind != 0 ? 1 : 0);
      double acc = 0.0;
      for (int j = 0; j < 14; j++) acc = minnorm_sum_step(px[minnorm_group_slot(j, kJ0, kSC)], py[minnorm_group_slot(j, kJ0, kSC)], acc);
      if (r < 3) rec[kSums + 3 * pass + L[r].kind] = acc;
      else if (memcmp(&acc, &rec[kSums + 3 * pass + L[r].kind], 8) != 0) { fprintf(stderr, "lanes 3..5 disagree with lanes 0..2\n"); exit(3); }
    }
    for (int r = 0; r < kGroup; r++) { // behind it
      Lane &l = L[r];
      const double a = rec[kSums + 3 * pass], d = rec[kSums + 3 * pass + 1];
      if (pass < 2) {
        const double b = rec[kSums + 3 * pass + 2];
        if (r == 0) bzero[pass] = (b == 0.0) ? 1.0 : 0.0;
        if (b != 0.0) {
          double c, s;
          minnorm_sweep_coeffs(a, d, b, c, s);
          for (int n = 0; n < 3; n++) minnorm_rotate(c, s, l.v0[n], l.v1[n]);
          minnorm_rotate(c, s, l.g0, l.g1);
          rec[l.e0] = l.v0[0]; rec[l.e0 + 1] = l.v1[0];
          rec[l.e1] = l.v0[1]; rec[l.e1 + 1] = l.v1[1];
          if (l.own2) { rec[l.e2] = l.v0[2]; rec[l.e2 + 1] = l.v1[2]; }
        }
      } else {
        double k0, k1;
        minnorm_final_coeffs(a, d, l.g0, l.g1, k0, k1);
        double *xr = rec + kX + r;
        const double d0 = minnorm_dx(k0, k1, l.v0[0], l.v1[0]), d1 = minnorm_dx(k0, k1, l.v0[1], l.v1[1]), d2 = minnorm_dx(k0, k1, l.v0[2], l.v1[2]);
        dx_out[r] = d0;
        dx_out[r + 6] = d1;
        xr[0] = CCMP_FMA(-step, d0, xr[0]);
        xr[6] = CCMP_FMA(-step, d1, xr[6]);
        if (l.own2) { dx_out[r + 12] = d2; xr[12] = CCMP_FMA(-step, d2, xr[12]); }
      }
    }
  }
  for (int e = 0; e < 14; e++) x[e] = rec[kX + e];
}

bool same(double a, double b) { return (a != a && b != b) || memcmp(&a, &b, 8) == 0; }

} // namespace

int main(int argc, char **argv)
{
  if (argc < 3) return 2;
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  double c[30], out[30];
  long n = 0, update_differ = 0;
  while (fread(c, sizeof(double), 30, fi) == 30) {
    solve_minnorm(c, c[28], c[29], &out[0]);
    double x[14], xr[14];
    for (int e = 0; e < 14; e++) x[e] = xr[e] = 0.25 * (e - 6.5); // the update of the iterate, as the kernels' two texts apply it
    group_solve(c, c[28], c[29], 0.30, x, &out[14], &out[28]);
    for (int e = 0; e < 14; e++) {
      xr[e] = CCMP_FMA(-0.30, out[e], xr[e]);
      if (!same(xr[e], x[e])) update_differ++;
    }
    fwrite(out, sizeof(double), 30, fo);
    n++;
  }
  fclose(fi);
  fclose(fo);
  printf("{\"cases\": %ld, \"update_differ\": %ld}\n", n, update_differ);
  return update_differ ? 1 : 0;
}
