/* ccmp_stage.h — what the planner-side *_host entry points share (ccmp_roadmap.cpp, ccmp_object.cpp, ccmp_ik.cpp, ccmp_shortcut.cpp,
 * ccmp_dense.cpp, ccmp_smooth.cpp, ccmp_retime.cpp): the answer to a missing handle, two small checks, the synchronous staged call on
 * the context's stream, the device memory of one call and, for the path units, the pieces of an entry point's prologue (the read of
 * path_len, the overlap test, the row bound, the options), the plain synchronous read (read_back) and the one allocation of a result
 * handle, which the planner handles (ccmp_plan.cpp, ccmp_rrtc.cpp) state as one list of pieces.  Host only, C++ linkage, nothing
 * of the C ABI.  The projector's host path (ccmp_host_io.cpp: HostIO, the sharded calls) has other requirements and does not use
 * this.  Argument checks stay with the entry points: they run before the device guard and before anything here is constructed. */
#ifndef CCMP_STAGE_H
#define CCMP_STAGE_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ccmp_ctx.h"
#include "ccmp_resident.h"

namespace ccmp_host {

/* what an entry point answers when it is given no handle (context, store, result): a handle needs a context and a context needs a
 * device, so on a machine without one that is the reason (CCMP_ENODEV); with a device a NULL handle is an argument error */
inline int no_handle()
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CCMP_ENODEV; }
  return CCMP_EINVAL;
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

/* every path length of a [F][max_len] block is in 0 .. max_len */
inline int lens_ok(const int32_t *len, size_t F, int max_len)
{
  for (size_t f = 0; f < F; f++)
    if (len[f] < 0 || len[f] > max_len) return CCMP_EINVAL;
  return CCMP_OK;
}

/* One synchronous host call on ctx->stream: add() the pieces, alloc() the context's staging block, up(), the device-pointer form on
 * at<T>(), down(), finish().  The first failed copy (or launch given to note()) is remembered and turns every later copy into a
 * no-op; finish() waits for the stream on every path, so nothing of the call is in flight when the entry point returns.  The copies
 * also take raw device pointers (a store's rows, a call's own memory) for the forms that stage nothing or stage elsewhere. */
struct StagedCall {
  ccmp_ctx *ctx;
  const char *what; // the entry point, for ccmp_last_hip_error
  size_t total = 0;
  hipError_t err = hipSuccess;
  StagedCall(ccmp_ctx *c, const char *entry) : ctx(c), what(entry) {}
  StagedCall(const StagedCall &) = delete;
  StagedCall &operator=(const StagedCall &) = delete;

  /* the offset of a piece of `bytes`, 256-byte aligned; a piece of no bytes takes no room */
  size_t add(size_t bytes) { const size_t off = total; total = align256(total + bytes); return off; }
  int alloc() { return ensure_stage(ctx, total ? total : 256); }
  template <class T> T *at(size_t off) const { return (T *)((char *)ctx->stage + off); }
  /* the piece of an optional argument: nullptr when the caller gave none */
  template <class T> T *at(size_t off, const void *given) const { return given ? at<T>(off) : nullptr; }

  void copy(void *dst, const void *src, size_t n, hipMemcpyKind kind)
  {
    if (dst && src && n && err == hipSuccess) err = hipMemcpyAsync(dst, src, n, kind, ctx->stream);
  }
  void up(void *dev, const void *src, size_t n) { copy(dev, src, n, hipMemcpyHostToDevice); }
  void up(size_t off, const void *src, size_t n) { up(at<char>(off), src, n); }
  void down(void *dst, const void *dev, size_t n) { copy(dst, dev, n, hipMemcpyDeviceToHost); }
  void down(void *dst, size_t off, size_t n) { down(dst, at<char>(off), n); }
  void note(hipError_t e) { if (err == hipSuccess) err = e; } // a launch between the copies
  bool copy_ok() const { return err == hipSuccess; }

  /* always waits; then the device form's code, else the first copy error, else the wait's own */
  int finish(int rc)
  {
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (rc != CCMP_OK) return rc;
    if (err != hipSuccess) return hip_fail(err, what);
    if (es != hipSuccess) return hip_fail(es, what);
    return CCMP_OK;
  }
};

/* The device memory of one call: handed out in 256-byte aligned pieces of blocks of 4 MB (or the request, if larger), all of it
 * released when the call returns.  A resident service kernel is stopped before every hipMalloc and before the frees (hipFree waits for
 * the whole device).  A failed allocation leaves its text for ccmp_last_hip_error; from then on get() answers nullptr and ok() false,
 * so a call site takes all its arrays and asks once. */
class CallArena {
  static constexpr size_t kBlock = (size_t)4 << 20;
  ccmp_ctx *ctx;
  const char *what;
  std::vector<void *> blocks;
  char *cur = nullptr;
  size_t left = 0;
  bool failed = false;

 public:
  CallArena(ccmp_ctx *c, const char *what_) : ctx(c), what(what_) {}
  CallArena(const CallArena &) = delete;
  CallArena &operator=(const CallArena &) = delete;
  void *get(size_t bytes)
  {
    if (failed) return nullptr;
    bytes = align256(bytes ? bytes : 1);
    if (bytes > left) {
      const size_t sz = bytes > kBlock ? bytes : kBlock;
      void *b = nullptr;
      quiesce(ctx);
      const hipError_t e = hipMalloc(&b, sz);
      if (e != hipSuccess) { (void)hip_fail(e, what); failed = true; return nullptr; }
      blocks.push_back(b);
      cur = (char *)b;
      left = sz;
    }
    void *r = cur;
    cur += bytes;
    left -= bytes;
    return r;
  }
  template <class T> T *array(size_t n) { return (T *)get(n * sizeof(T)); }
  bool ok() const { return !failed; }
  ~CallArena()
  {
    if (blocks.empty()) return;
    quiesce(ctx);
    for (void *b : blocks) (void)hipFree(b); // waits for whatever still reads it
  }
};

/* The path units' share.  Hidden, as ccmp_pair_tests.h is: the inline functions above come out of the library as weak symbols and
 * stay so, because the list of the library's dynamic symbols is kept as it is; what is added here adds nothing to it. */
#pragma GCC visibility push(hidden)

/* a synchronous read of device memory on `st`: copied, waited for on every path, then the copy's error before the wait's */
inline int read_back(void *dst, const void *dev_src, size_t bytes, hipStream_t st)
{
  const hipError_t e = hipMemcpyAsync(dst, dev_src, bytes, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  HIP_TRY(e);
  HIP_TRY(es);
  return CCMP_OK;
}

/* the device form's one read of path_len [F] (device memory), before any launch: copied, waited for, checked */
inline int read_lens(const int32_t *path_len, size_t F, int max_len, hipStream_t st, std::vector<int32_t> *len)
{
  len->resize(F);
  if (F == 0) return CCMP_OK;
  const int rc = read_back(len->data(), path_len, F * sizeof(int32_t), st);
  return rc != CCMP_OK ? rc : lens_ok(len->data(), F, max_len);
}

constexpr size_t kMaxRows = ((size_t)1 << 31) - 1; // rows and slots are int32: a batch beyond this is an argument error

/* do two byte ranges share a byte?  (a range without a pointer or a length shares none) */
inline bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
  if (!a || !b || !na || !nb) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

/* the caller's options, or the defaults where it gave none */
template <class O> O opts_or(const O *given, void (*defaults)(O *)) { O o; defaults(&o); return given ? *given : o; }

/* The one allocation of a result handle H (ccmp_dense_paths, ccmp_sampled_paths: fields ctx, device, block): take() the pieces, then
 * alloc(), then the handle's arrays at<T>() their offsets.  result_destroy is the whole of the handle's *_destroy.
 * A handle of many arrays (ccmp_plan, ccmp_rrtc) states each ONCE instead, as piece(pointer member, element count) in a function
 * pieces(ResultBlock &) of its own: alloc_pieces() walks that list twice, to size the block and, after place(), to set the pointers.
 * The bytes of a piece follow from its pointer's type; the order of the list is the order in the block. */
struct ResultBlock {
  size_t total = 0;
  char *base = nullptr;
  size_t take(size_t bytes) { const size_t off = total; total += align256(bytes); return off; }
  template <class T> T *at(size_t off) const { return (T *)(base + off); }
  template <class T> void piece(T *&p, size_t n) { const size_t off = take(n * sizeof(T)); if (base) p = at<T>(off); }
  void place(void *block) { base = (char *)block; total = 0; } // the second walk starts here
  template <class H> int alloc_pieces(H *h, ccmp_ctx *ctx, const char *what)
  {
    h->pieces(*this);
    const int rc = alloc(h, ctx, what);
    if (rc != CCMP_OK) return rc;
    place(h->block);
    h->pieces(*this);
    return CCMP_OK;
  }
  template <class H> int alloc(H *h, ccmp_ctx *ctx, const char *what)
  {
    h->ctx = ctx;
    h->device = ctx->device;
    quiesce(ctx);
    const hipError_t e = hipMalloc(&h->block, total);
    base = (char *)h->block;
    return e == hipSuccess ? CCMP_OK : hip_fail(e, what);
  }
};

template <class H> void result_destroy(H *h)
{
  if (!h) return;
  {
    DeviceGuard guard(h->device);
    if (h->ctx && context_alive(h->ctx)) quiesce(h->ctx);
    if (h->block) (void)hipFree(h->block);
  }
  delete h;
}

#pragma GCC visibility pop

}  // namespace ccmp_host

#endif /* CCMP_STAGE_H */
