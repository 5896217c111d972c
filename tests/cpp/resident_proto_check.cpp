// resident_proto_check.cpp — the resident service's several-edge request on the host alone (tests/test_resident_analytic_host.py):
// requests for E = 1, 5, 8 are packed and posted with the code the library's host side uses (csrc/ccmp_resident_proto.h) and judged
// by the rule the analytic service kernel applies to what it read (line_ok / multi_unpack: multi_accept).  An accepted request
// gives back every word; a request with any ONE line left from the previous sequence number, or with any ONE payload word changed
// behind its tag, is refused.  Prints one JSON line of counts; exit status 0 when nothing went wrong.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ccmp_resident_proto.h"

using namespace ccmp_res;

int main()
{
  std::mt19937_64 rng(0x5EED);
  std::uniform_real_distribution<double> u(-3.0, 3.0);
  long accepted = 0, words_back = 0, stale_refused = 0, stale_cases = 0, flip_refused = 0, flip_cases = 0, failures = 0;
  const int Es[3] = {1, 5, 8};
  for (int ei = 0; ei < 3; ei++) {
    for (int with_carry = 0; with_carry < 2; with_carry++) {
      const int E = Es[ei];
      std::vector<double> from(14 * E), to(14 * E), carry(2 * E);
      for (auto &v : from) v = u(rng);
      for (auto &v : to) v = u(rng);
      for (auto &v : carry) v = u(rng);
      from[0] = 0.0;  // an all-zero word and a NaN among the payloads
      to[13] = double_of(0x7ff8000000000001ull);
      MultiParams m;
      m.E = E; m.has_carry = with_carry; m.max_states = 64 - ei; m.round_budget = 8 * ei; m.check_target = ei & 1;
      m.delta_bits = bits_of(0.2); m.lambda_bits = bits_of(2.0);
      // the request before it, sequence number seq - 1, with other payloads: what a line that was not yet rewritten still holds
      const unsigned int seq = 0x10u + 7u * ei + with_carry;
      std::vector<word_t> prev(kMultiMaxWords, 0), area(kMultiMaxWords, 0);
      {
        std::vector<double> f2(14 * 8), t2(14 * 8), c2(16);
        for (auto &v : f2) v = u(rng);
        for (auto &v : t2) v = u(rng);
        for (auto &v : c2) v = u(rng);
        MultiParams mp = m;
        mp.E = 8;
        mp.max_states = m.max_states - 1; // (every line of it differs from the new request's)
        multi_pack(prev.data(), mp, f2.data(), t2.data(), c2.data());
        post(prev.data(), multi_lines(8), seq - 1);
      }
      area = prev;
      multi_pack(area.data(), m, from.data(), to.data(), with_carry ? carry.data() : nullptr);
      post(area.data(), multi_lines(E), seq);
      // ---- accepted, and every word comes back ----
      MultiParams got;
      if (!multi_accept(seq, area.data(), &got)) { failures++; continue; }
      accepted++;
      bool same = got.E == E && got.has_carry == with_carry && got.max_states == m.max_states && got.round_budget == m.round_budget &&
                  got.check_target == m.check_target && got.delta_bits == m.delta_bits && got.lambda_bits == m.lambda_bits;
      words_back += 7;
      for (int e = 0; e < E; e++) {
        for (int i = 0; i < 14; i++) {
          same = same && area[multi_from_word(e, i)] == bits_of(from[14 * e + i]) && area[multi_to_word(e, i)] == bits_of(to[14 * e + i]);
          words_back += 2;
        }
        for (int k = 0; k < 2; k++) {
          same = same && area[multi_carry_word(e, k)] == (with_carry ? bits_of(carry[2 * e + k]) : 0ull);
          words_back++;
        }
      }
      if (!same) failures++;
      // the previous request's sequence number does not pass for this one, nor this one's for the next
      if (multi_accept(seq - 1, area.data(), &got) || multi_accept(seq + 1, area.data(), &got)) failures++;
      // ---- any single line still the previous request's: refused ----
      for (int line = 0; line < multi_lines(E); line++) {
        std::vector<word_t> torn = area;
        memcpy(&torn[8 * line], &prev[8 * line], 64);
        stale_cases++;
        if (!multi_accept(seq, torn.data(), &got)) stale_refused++;
        // ... and a line whose payload is already the new one while its tag is still the old one, and the other way round
        torn = area;
        torn[8 * line + 7] = prev[8 * line + 7];
        stale_cases++;
        if (!multi_accept(seq, torn.data(), &got)) stale_refused++;
        torn = area;
        memcpy(&torn[8 * line], &prev[8 * line], 56);
        stale_cases++;
        if (!multi_accept(seq, torn.data(), &got)) stale_refused++;
      }
      // ---- any single payload word changed behind its tag: refused (one bit, low / middle / high, and the word replaced) ----
      for (int line = 0; line < multi_lines(E); line++)
        for (int w = 0; w < 7; w++) {
          const word_t changes[4] = {1ull, 1ull << 31, 1ull << 63, rng() | 1ull};
          for (int k = 0; k < 4; k++) {
            std::vector<word_t> bad = area;
            bad[8 * line + w] ^= changes[k];
            flip_cases++;
            if (!multi_accept(seq, bad.data(), &got)) flip_refused++;
          }
        }
    }
  }
  printf("{\"accepted\": %ld, \"words_back\": %ld, \"stale_cases\": %ld, \"stale_refused\": %ld, \"flip_cases\": %ld, \"flip_refused\": %ld, \"failures\": %ld}\n",
         accepted, words_back, stale_cases, stale_refused, flip_cases, flip_refused, failures);
  return (failures == 0 && stale_refused == stale_cases && flip_refused == flip_cases && accepted == 6) ? 0 : 1;
}
