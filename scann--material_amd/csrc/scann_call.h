// What one analysis call shares on the host (header only): its device workspace, planned region by region and then allocated as one
// block of the cache (CallWs); the staging of query rows at an index's padded width (RowStage); and the checks that open the entry
// points (check_pool, check_pool_rows, level_dim, check_level).  Of the library it calls only what scann_runtime.h declares
// (cached_malloc, cached_free, fail), so a host file that includes it still links into a stand-alone program that stubs those; from
// scann_knn.h, which is self-contained, it takes the definition of scann_index (rows_of, ids_of) and nothing that needs linking.
//
// The rule of a call: one CallWs.  The regions the call's one memset clears are taken first and `zeroed = ws.bytes()` is read behind
// them; the chunk table's host copy belongs to the workspace (upload_rows), so it outlives the asynchronous copy that reads it.  The
// order of a call stays explicit: enqueue, hipStreamSynchronize, ws.release(), then HIPCHK(h, e); HIPCHK(h, e_sync).
#pragma once
#include "scann_knn.h"
#include "scann_runtime.h"

namespace scann {

// A call's device workspace.  take() declares a region by the pointer it fills, so every region is named once; alloc() takes one block
// of bytes() from the cache and points every declared pointer into it.  Between take() and alloc() a declared pointer must stay where it
// is (a local, or a field of the argument struct on the call's stack): alloc() writes through its address.  The destructor gives the
// block back without waiting for any stream: it only keeps an early return from leaking.  A call site that returns early AFTER work
// on the block has been enqueued must wait for the stream first, as every call does before its release().
class CallWs {
 public:
  CallWs() { slots_.reserve(24); }  // (one host allocation for the slots of any call here; the largest plan has 22 regions)
  CallWs(const CallWs&) = delete;
  CallWs& operator=(const CallWs&) = delete;
  ~CallWs() { release(); }

  // `count` elements of T, rounded up to 256 bytes, behind the regions taken so far; count 0 takes nothing.  Returns the region's offset
  template <class T>
  size_t take(T*& slot, size_t count) {
    slot = nullptr;
    slots_.push_back({&slot, at_});
    const size_t o = at_;
    at_ += align_up(count * sizeof(T));
    return o;
  }
  size_t bytes() const { return at_; }
  char* base() const { return base_; }

  // one cached_malloc (none for an empty plan); on success every declared pointer is base() + its offset
  hipError_t alloc() {
    if (!at_) return hipSuccess;
    const hipError_t e = cached_malloc(reinterpret_cast<void**>(&base_), at_);
    if (e != hipSuccess) {
      base_ = nullptr;
      return e;
    }
    for (const Slot& s : slots_) {
      char* p = base_ + s.off;
      std::memcpy(s.where, &p, sizeof p);  // (every T* has the representation of a char*)
    }
    return hipSuccess;
  }
  // the block back to the cache, once: after the call's wait, before its HIPCHKs
  void release() {
    cached_free(base_);
    base_ = nullptr;
    tabs_.clear();
  }

  // Enqueued on s: the table of ix's first n_chunk chunks into the region `rows` (taken, n_chunk entries) and, ids non-null, the table of
  // their ids into the region `ids`.  The host copy is the workspace's own and lives until release(), i.e. past the call's wait
  template <class F>
  hipError_t upload_rows(const scann_index* ix, int n_chunk, F* const* rows, const int64_t* const* ids, hipStream_t s) {
    if (n_chunk <= 0) return hipSuccess;
    const void* const* tab = host_table(ix, n_chunk, ids != nullptr);
    hipError_t e = hipMemcpyAsync(const_cast<F**>(rows), tab, (size_t)n_chunk * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && ids) e = hipMemcpyAsync(const_cast<const int64_t**>(ids), tab + n_chunk, (size_t)n_chunk * 8, hipMemcpyHostToDevice, s);
    return e;
  }
  // upload_rows' host copy: the rows of ix's first n_chunk chunks, then (with_ids) their ids; the workspace keeps it until release().
  // Public only so that scann_call_check.cpp can look at the table without a HIP call: a call site uses upload_rows
  const void* const* host_table(const scann_index* ix, int n_chunk, bool with_ids) {
    tabs_.reserve(2);  // (no call of the library uploads more tables)
    tabs_.emplace_back((size_t)(with_ids ? 2 : 1) * n_chunk);
    const void** tab = tabs_.back().data();
    for (int c = 0; c < n_chunk; ++c) {
      tab[c] = ix->rows_of((size_t)c);
      if (with_ids) tab[n_chunk + c] = ix->ids_of((size_t)c);
    }
    return tab;
  }

 private:
  struct Slot {
    void* where;
    size_t off;
  };
  std::vector<Slot> slots_;
  std::vector<std::vector<const void*>> tabs_;  // (a move keeps a table's storage where it is)
  size_t at_ = 0;
  char* base_ = nullptr;
};

// The kernels' argument structs declare most regions as pointers to const: the address to fill such a region through
template <class T>
inline T* writable(const T* region) { return const_cast<T*>(region); }

// nq rows of `dim` floats, `pitch` floats apart at src -- host rows (kind = hipMemcpyHostToDevice) or device rows -- as the kernels read
// an index's rows: `stride` floats apart, the padding columns zero.  Device rows that lie so already are used where they lie; any others
// are copied into a region of the call's workspace.
struct RowStage {
  float* buf = nullptr;  // the region, if one was taken
  int64_t nq = 0;
  int dim = 0, pitch = 0, stride = 0;
  hipMemcpyKind kind = hipMemcpyDeviceToDevice;
  bool copy = false;
  // declares the region in ws, if the rows need one (this object must stay where it is until ws.alloc())
  void take(CallWs& ws, int64_t nq_, int dim_, int pitch_, int stride_, hipMemcpyKind kind_) {
    nq = nq_, dim = dim_, pitch = pitch_, stride = stride_, kind = kind_;
    copy = stride != pitch || kind == hipMemcpyHostToDevice;
    if (copy) ws.take(buf, (size_t)nq * stride);
  }
  // enqueued on s, after ws.alloc(): the region cleared if it has padding columns (clear = false: it lies within what the call's own
  // memset clears), then the rows copied into it
  hipError_t stage_rows(const float* src, hipStream_t s, bool clear = true) const {
    hipError_t e = copy && clear && stride != dim ? hipMemsetAsync(buf, 0, (size_t)nq * stride * 4, s) : hipSuccess;
    if (e == hipSuccess && copy) e = hipMemcpy2DAsync(buf, (size_t)stride * 4, src, (size_t)pitch * 4, (size_t)dim * 4, (size_t)nq, kind, s);
    return e;
  }
  const float* rows(const float* src) const { return copy ? buf : src; }  // where the kernels read them
};

// ---- the checks that open an entry point; `who`: its name, the messages are "<who>: ..." ----

inline int check_pool(scann_handle* h, const scann_index* pool, const char* who) {
  if (!h || !pool) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": null handle or pool");
  if (pool->h != h) return fail(h, SCANN_ERR_INVALID, std::string(who) + ": the pool belongs to another handle");
  return SCANN_OK;
}
// (a check of its own: where it stands among an entry point's other checks decides which error a caller with two wrong arguments sees)
inline int check_pool_rows(scann_handle* h, const scann_index* pool, const char* who, int64_t max_rows) {
  if (pool->n > max_rows) return fail(h, SCANN_ERR_UNSUPPORTED, std::string(who) + ": the pool has too many rows");
  return SCANN_OK;
}

// the level's width in this model, or 0 for an unknown level
inline int level_dim(const scann_handle* h, int32_t level) {
  return level == SCANN_OUT_BF_PROPERTY ? h->cfg.dense_out : level == SCANN_OUT_AFTER_LC ? h->cfg.global_dim : 0;
}
inline int bad_level(scann_handle* h, int32_t level, const char* who) {
  return fail(h, SCANN_ERR_INVALID, std::string(who) + ": level must be SCANN_OUT_BF_PROPERTY or SCANN_OUT_AFTER_LC, got " + std::to_string(level));
}
inline int check_level(scann_handle* h, const scann_index* ix, int32_t level, const char* who) {
  const int d = level_dim(h, level);
  if (!d) return bad_level(h, level, who);
  if (d != ix->dim)
    return fail(h, SCANN_ERR_INVALID, std::string(who) + ": the index holds rows of " + std::to_string(ix->dim) + " columns, the model's " +
                                          (level == SCANN_OUT_BF_PROPERTY ? "dense_out" : "global_dim") + " is " + std::to_string(d));
  return SCANN_OK;
}

}  // namespace scann
