/* ccmp_resident_proto.h — the arithmetic of the resident service's mailbox protocol (ccmp_resident.h: the layout), as plain
 * functions that the host side (ccmp_resident.cpp), the analytic service kernel (ccmp_kernels_fast.hip) and a host-only test
 * (tests/cpp/resident_proto_check.cpp) include: one text for the line tag, for posting a request and for the rule by which the
 * device accepts one.  No HIP, no library header: it compiles with a plain C++ compiler.
 *
 * A request line is 64 bytes: seven payload words and, LAST, its tag = the request's sequence number (low half) | a checksum of
 * ITS seven payload words (high half).  The host fills the payloads, then the tags; the device acts on a request only when every
 * line carries the request's sequence number and the checksum of the payload it read. */
#ifndef CCMP_RESIDENT_PROTO_H
#define CCMP_RESIDENT_PROTO_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CCMP_RES_HD __host__ __device__ inline
#else
#define CCMP_RES_HD inline
#endif

namespace ccmp_res {

typedef unsigned long long word_t;

/* ---- the several-edge request (command kResGeodesicMulti; analytic service only) ------------------------------------------------
 * line 0           parameters: (E | has_carry << 32), (max_states | round_budget << 32), check_target, delta, lambda, 2 spare | tag
 * lines 1+5e..5+5e edge e: from[0..6] | tag, from[7..13] | tag, to[0..6] | tag, to[7..13] | tag, carry_in[0..1] + 5 spare | tag
 * Only the 1 + 5 E lines of the request's edges are written and read. */
constexpr int kMultiMaxEdges = 8;
constexpr int kMultiLinesPerEdge = 5;
constexpr int kMultiMaxLines = 1 + kMultiLinesPerEdge * kMultiMaxEdges;
constexpr int kMultiMaxWords = 8 * kMultiMaxLines;
CCMP_RES_HD int multi_lines(int E) { return 1 + kMultiLinesPerEdge * E; }

/* a line's tag */
template <class W>
CCMP_RES_HD word_t line_tag(unsigned int seq, const W *w7)
{
  word_t h = 0;
  for (int i = 0; i < 7; i++) {
    const word_t v = w7[i];
    const int r = 7 * i + 1;
    h ^= (v << r) | (v >> (64 - r));
  }
  return (word_t)seq | ((word_t)(unsigned int)(h ^ (h >> 32)) << 32);
}
/* the device's rule for ONE line (eight words as it read them): the tag is the one of request `seq` over this very payload */
template <class W>
CCMP_RES_HD bool line_ok(unsigned int seq, const W *line8)
{
  const word_t tag = line8[7];
  return tag == line_tag(seq, line8);
}

struct MultiParams {
  int E, has_carry, max_states, round_budget, check_target;
  word_t delta_bits, lambda_bits;
};

CCMP_RES_HD word_t bits_of(double v)
{
  union { double d; word_t w; } u;
  u.d = v;
  return u.w;
}
CCMP_RES_HD double double_of(word_t w)
{
  union { double d; word_t w; } u;
  u.w = w;
  return u.d;
}

/* Host: the payload words of a several-edge request into `area` (kMultiMaxWords words of mailbox, or of anything else), tags NOT
 * yet written.  carry_in may be null. */
inline void multi_pack(volatile word_t *area, const MultiParams &m, const double *from, const double *to, const double *carry_in)
{
  area[0] = (word_t)(unsigned int)m.E | ((word_t)(carry_in ? 1u : 0u) << 32);
  area[1] = (word_t)(unsigned int)m.max_states | ((word_t)(unsigned int)m.round_budget << 32);
  area[2] = (word_t)(unsigned int)m.check_target;
  area[3] = m.delta_bits;
  area[4] = m.lambda_bits;
  area[5] = 0;
  area[6] = 0;
  for (int e = 0; e < m.E; e++) {
    volatile word_t *ln = area + 8 * (1 + kMultiLinesPerEdge * e);
    for (int i = 0; i < 7; i++) {
      ln[i] = bits_of(from[14 * e + i]);
      ln[8 + i] = bits_of(from[14 * e + 7 + i]);
      ln[16 + i] = bits_of(to[14 * e + i]);
      ln[24 + i] = bits_of(to[14 * e + 7 + i]);
      ln[32 + i] = 0;
    }
    if (carry_in) {
      ln[32] = bits_of(carry_in[2 * e]);
      ln[33] = bits_of(carry_in[2 * e + 1]);
    }
  }
}
/* Host: payloads are in place — the tags of `lines` lines, each stored with release order behind its payload */
inline void post(volatile word_t *area, int lines, unsigned int seq)
{
  for (int line = 0; line < lines; line++) {
#if defined(__GNUC__) || defined(__clang__)
    __atomic_store_n(&area[8 * line + 7], line_tag(seq, area + 8 * line), __ATOMIC_RELEASE);
#else
    area[8 * line + 7] = line_tag(seq, area + 8 * line);
#endif
  }
}

/* The device's acceptance rule for a several-edge request, given the words as it staged them: the parameter line names 1..8 edges
 * (multi_unpack) and it and every line of those edges is of request `seq` over the payload read (line_ok).  The kernel evaluates
 * exactly these two functions, line_ok on one thread per line; multi_accept is their conjunction in one place. */
template <class W>
CCMP_RES_HD bool multi_unpack(const W *area, MultiParams *m)
{
  const word_t w0 = area[0], w1 = area[1];
  m->E = (int)(unsigned int)(w0 & 0xffffffffull);
  m->has_carry = (int)(unsigned int)(w0 >> 32);
  m->max_states = (int)(unsigned int)(w1 & 0xffffffffull);
  m->round_budget = (int)(unsigned int)(w1 >> 32);
  m->check_target = (int)(unsigned int)(area[2] & 0xffffffffull);
  m->delta_bits = area[3];
  m->lambda_bits = area[4];
  return m->E >= 1 && m->E <= kMultiMaxEdges;
}
template <class W>
CCMP_RES_HD bool multi_accept(unsigned int seq, const W *area, MultiParams *m)
{
  if (!line_ok(seq, area) || !multi_unpack(area, m)) return false;
  const int lines = multi_lines(m->E);
  for (int line = 1; line < lines; line++)
    if (!line_ok(seq, area + 8 * line)) return false;
  return true;
}
/* where an accepted request keeps joint i of edge e's `from` / `to`, and its carry_in[k] */
CCMP_RES_HD int multi_from_word(int e, int i) { return 8 * (1 + kMultiLinesPerEdge * e + (i >= 7 ? 1 : 0)) + (i >= 7 ? i - 7 : i); }
CCMP_RES_HD int multi_to_word(int e, int i) { return 8 * (3 + kMultiLinesPerEdge * e + (i >= 7 ? 1 : 0)) + (i >= 7 ? i - 7 : i); }
CCMP_RES_HD int multi_carry_word(int e, int k) { return 8 * (5 + kMultiLinesPerEdge * e) + k; }

}  // namespace ccmp_res
#endif /* CCMP_RESIDENT_PROTO_H */
