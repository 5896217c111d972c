// The two-pass block layout of the planner handles (csrc/ccmp_stage.h: ResultBlock::piece; csrc/ccmp_planner.h: the handles'
// pieces()): the offsets of every array of ccmp_plan and ccmp_rrtc at three (width, k, max_states) against the offsets of the explicit
// take() sequence these lists replaced — literals, computed once from that sequence.  Host arithmetic only: no device, no library; the
// block is plain host memory that nothing writes.  Prints one line per case and "ok" at the end; exit status 1 on a difference.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../closed_chain_motion_planner_amd/csrc/ccmp_planner.h"

namespace {

// ResultBlock's own arithmetic, with a note of where every piece landed
struct Recorder {
  ccmp_host::ResultBlock rb;
  std::vector<size_t> off, bytes;
  template <class T> void piece(T *&p, size_t n)
  {
    rb.piece(p, n);
    if (!rb.base) return;
    off.push_back((size_t)((char *)p - rb.base));
    bytes.push_back(n * sizeof(T));
  }
};

void set_k(ccmp_plan *h, int k) { h->o.k = k; }
void set_k(ccmp_rrtc *, int) {} // RRT-Connect has no k

template <class H> bool same(const char *name, int width, int k, int max_states, const std::vector<size_t> &want, size_t want_total)
{
  H *h = new H();
  h->o.width = width;
  h->o.max_states = max_states;
  set_k(h, k);
  Recorder rec;
  h->pieces(rec); // sizes
  const size_t total = rec.rb.total;
  void *mem = malloc(total);
  rec.rb.place(mem);
  h->pieces(rec); // places
  bool ok = mem && total == want_total && rec.rb.total == total && rec.off == want;
  for (size_t i = 0; ok && i < rec.off.size(); i++) {
    const size_t end = i + 1 < rec.off.size() ? rec.off[i + 1] : total;
    ok = rec.off[i] % 256 == 0 && rec.off[i] + rec.bytes[i] <= end; // aligned, inside the block, short of the next piece
  }
  printf("%s width %d k %d max_states %d: %zu pieces, %zu bytes: %s\n", name, width, k, max_states, rec.off.size(), total, ok ? "same" : "DIFFERENT");
  free(mem);
  delete h;
  return ok;
}

}  // namespace

int main()
{
  bool ok = true;
  struct Case {
    int width, k, max_states;
    std::vector<size_t> plan, rrtc;
    size_t plan_total, rrtc_total;
  };
  const Case cases[] = {
      {1, 1, 2,
       {0, 256, 512, 768, 1024, 1280, 2048, 2816, 3072, 3328, 3584, 4864, 5120, 5376, 5632, 8192, 8448, 8704, 8960, 9216, 9472, 9728, 9984, 10240, 10496, 10752,
        11008, 11264, 11520, 11776, 12544, 13824, 14080, 14336, 14592, 14848, 16128, 16384, 16640},
       {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, 2560, 2816, 3072, 3328, 3584, 3840, 4096, 4352, 4608, 4864, 5120, 5376, 5632, 5888, 6144, 6400,
        6656, 6912, 7168, 7424, 7680},
       16896, 7936},
      {32, 5, 64,
       {0, 256, 512, 768, 1024, 1280, 3328, 5376, 5632, 6400, 7680, 11264, 11520, 11776, 12032, 1158912, 1159680, 1159936, 1160704, 1160960, 1163520, 1163776,
        1164544, 1164800, 1165056, 1165312, 1165568, 1165824, 1166080, 1166336, 1167104, 1168384, 1168640, 1168896, 1169152, 1169408, 1170688, 1170944, 1171200},
       {0, 256, 3840, 4096, 4352, 7936, 11520, 240896, 241408, 244992, 248576, 248832, 256000, 256256, 256512, 256768, 257024, 257280, 257536, 257792, 258048,
        258304, 258560, 258816, 259072, 259328, 259584, 259840, 260096, 260352, 260864},
       1171456, 261120},
      {256, 16, 64,
       {0, 256, 512, 768, 1024, 1280, 17664, 34048, 35072, 51456, 84224, 112896, 113152, 114176, 116224, 29476352, 29492736, 29496832, 29513216, 29517312,
        29582848, 29583872, 29600256, 29601280, 29601536, 29601792, 29602048, 29602304, 29602560, 29602816, 29603584, 29604864, 29605120, 29605376, 29605632,
        29605888, 29607168, 29607424, 29607680},
       {0, 256, 28928, 30976, 33024, 61696, 90368, 1925376, 1929472, 1958144, 1986816, 1988864, 2046208, 2046464, 2046720, 2046976, 2047232, 2047488, 2047744,
        2048000, 2049024, 2050048, 2051072, 2052096, 2053120, 2054144, 2055168, 2056192, 2057216, 2058240, 2062336},
       29607936, 2062592},
  };
  for (const Case &c : cases) {
    ok = same<ccmp_plan>("plan", c.width, c.k, c.max_states, c.plan, c.plan_total) && ok;
    ok = same<ccmp_rrtc>("rrtc", c.width, c.k, c.max_states, c.rrtc, c.rrtc_total) && ok;
  }
  puts(ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
