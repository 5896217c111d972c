// Exercises ccmp::discreteGeodesicBatch (include/ccmp_ompl_adapter.hpp part 1) in the analytic-Jacobian mode from plain C++:
// growTree-shaped edges with interpolate == true, every edge's reached flag and its whole list as hex doubles, so that the Python
// test compares them bit for bit with the oracle's uninterrupted traversal in the same mode.
// usage: adapter_analytic_check <config.yaml> <edges.txt> <max_states>   (edges.txt: E `from` rows, then E `to` rows, 14 numbers each)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ccmp_ompl_adapter.hpp"

static void print_hex(const double *v, int n)
{
  for (int i = 0; i < n; i++) {
    uint64_t u;
    std::memcpy(&u, &v[i], 8);
    std::printf("%016" PRIx64 "%c", u, i + 1 == n ? '\n' : ' ');
  }
}

int main(int argc, char **argv)
{
  if (argc < 4) return 2;
  std::FILE *fp = std::fopen(argv[2], "r");
  if (!fp) return 3;
  std::vector<double> q;
  double v;
  while (std::fscanf(fp, "%lf", &v) == 1) q.push_back(v);
  std::fclose(fp);
  const size_t E = q.size() / 28;
  const int max_states = std::atoi(argv[3]);
  try {
    ccmp::Projector P(argv[1], 0);
    P.setJacobianMode(CCMP_JAC_ANALYTIC);
    std::vector<std::vector<std::vector<double>>> lists;
    std::vector<char> reached;
    ccmp::discreteGeodesicBatch(P, q.data(), q.data() + 14 * E, E, true, [](const double *) { return true; }, &lists, &reached, max_states);
    std::printf("error 0\n");
    for (size_t e = 0; e < E; e++) {
      std::printf("edge %zu reached %d n %zu\n", e, reached[e] ? 1 : 0, lists[e].size());
      for (const auto &row : lists[e]) print_hex(row.data(), 14);
    }
  } catch (const ccmp::Error &err) {
    std::printf("error %d\n", err.code);
    return 1;
  }
  return 0;
}
