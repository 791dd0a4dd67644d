// Stand-alone check of the call workspace planner (scann_call.h: CallWs) for the sanitizers: `make asan-call` compiles it under
// AddressSanitizer + UBSan (host code only, no device is touched) and runs it.  The device-block cache is stubbed with host malloc and a
// count of live blocks, so the program sees every offset, every pointer alloc() fills in, and how often a block is freed.  No HIP call is
// made: of the chunk table it checks the host copy (host_table), which is what the workspace has to keep alive.
#include <cstdlib>

#define SCANN_CHECK_OWN_CACHE
#include "scann_check.h"

namespace {
int g_live = 0, g_allocs = 0, g_frees = 0;
bool g_fail_next = false;
}  // namespace

namespace scann {
hipError_t cached_malloc(void** p, size_t bytes) {
  if (g_fail_next) {
    g_fail_next = false;
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes ? bytes : 1);
  ++g_live, ++g_allocs;
  return hipSuccess;
}
void cached_free(void* p) {
  if (!p) return;
  std::free(p);
  --g_live, ++g_frees;
}
}  // namespace scann

namespace {

#define CHECK(cond) EXPECT(cond)

struct Args {
  const float* const* rows;
  unsigned long long* sums;
  const uint8_t* mask;
  float* mean;
  double* cov;
};

}  // namespace

int main() {
  {  // offsets, bytes(), a zero-count region, the pointers after alloc(), the whole block written; freed once by release() + destructor
    Args a{};
    int32_t* tail;
    CallWs ws;
    const size_t o0 = ws.take(a.sums, 3);
    const size_t zeroed = ws.bytes();
    const size_t o1 = ws.take(a.rows, 5), o2 = ws.take(a.mask, 0), o3 = ws.take(a.mean, 70), o4 = ws.take(a.cov, 33), o5 = ws.take(tail, 1);
    CHECK(o0 == 0 && o1 == 256 && o2 == 512 && o3 == 512 && o4 == 1024 && o5 == 1536);  // take order; 70 floats: 512, 33 doubles: 512
    for (size_t o : {o0, o1, o2, o3, o4, o5}) CHECK(o % 256 == 0);
    CHECK(zeroed == align_up(3 * sizeof(unsigned long long)));
    CHECK(ws.bytes() == align_up(3 * 8) + align_up(5 * sizeof(void*)) + 0 + align_up(70 * 4) + align_up(33 * 8) + align_up(4));
    CHECK(ws.base() == nullptr && g_allocs == 0);
    CHECK(ws.alloc() == hipSuccess && g_allocs == 1 && g_live == 1);
    char* base = ws.base();
    CHECK((char*)a.sums == base + o0 && (const char*)a.rows == base + o1 && (const char*)a.mask == base + o2 && (char*)a.mean == base + o3 &&
          (char*)a.cov == base + o4 && (char*)tail == base + o5);
    CHECK((const void*)a.mask == (const void*)a.mean);  // the zero-count region coincides with the next one
    std::memset(base, 0xa5, ws.bytes());              // (a block too small is a sanitizer report)
    a.sums[2] = 1, a.mean[69] = 1.f, a.cov[32] = 1.0, *tail = 1;
    ws.release();
    CHECK(g_live == 0 && g_frees == 1 && ws.base() == nullptr);
  }
  CHECK(g_live == 0 && g_frees == 1);  // (not a second time by the destructor)
  {  // the destructor alone
    float* f;
    CallWs ws;
    ws.take(f, 4);
    CHECK(ws.alloc() == hipSuccess && g_live == 1);
    f[3] = 1.f;
  }
  CHECK(g_live == 0 && g_frees == 2);
  {  // alloc() never called: nothing to free
    float* f;
    CallWs ws;
    ws.take(f, 4);
    CHECK(f == nullptr);
  }
  CHECK(g_frees == 2 && g_allocs == 2);
  {  // alloc() failed: the pointers stay null, nothing is freed
    float* f;
    CallWs ws;
    ws.take(f, 4);
    g_fail_next = true;
    CHECK(ws.alloc() == hipErrorOutOfMemory && f == nullptr && ws.base() == nullptr);
    ws.release();
  }
  CHECK(g_frees == 2 && g_allocs == 2 && g_live == 0);
  {  // an empty plan takes no block
    CallWs ws;
    CHECK(ws.alloc() == hipSuccess && ws.base() == nullptr && g_allocs == 2);
  }
  {  // the staging plan: device rows at the stride take nothing, any others a region of nq * stride floats
    CallWs ws;
    RowStage in_place, padded, host;
    in_place.take(ws, 10, 8, 8, 8, hipMemcpyDeviceToDevice);
    CHECK(!in_place.copy && ws.bytes() == 0);
    const float q[1] = {0.f};
    CHECK(in_place.rows(q) == q && in_place.stage_rows(q, nullptr) == hipSuccess);  // (nothing is enqueued)
    padded.take(ws, 10, 6, 6, 8, hipMemcpyDeviceToDevice);
    CHECK(padded.copy && ws.bytes() == align_up(10 * 8 * 4));
    host.take(ws, 3, 8, 8, 8, hipMemcpyHostToDevice);
    CHECK(host.copy && ws.bytes() == align_up(10 * 8 * 4) + align_up(3 * 8 * 4));
    CHECK(ws.alloc() == hipSuccess && (char*)padded.buf == ws.base() && (char*)host.buf == ws.base() + align_up(10 * 8 * 4));
    CHECK(padded.rows(q) == padded.buf);
  }
  {  // the chunk tables: the host copies belong to the workspace and stay as they are until release()
    scann_index ix;
    ix.dim = 6, ix.stride = 8, ix.chunk_rows = 64;
    for (int c = 0; c < 3; ++c) ix.chunks.push_back(reinterpret_cast<char*>((uintptr_t)0x10000 * (c + 1)));
    const float* const* d_rows;
    const int64_t* const* d_ids;
    CallWs ws;
    ws.take(d_rows, 3); ws.take(d_ids, 3);
    CHECK(ws.alloc() == hipSuccess);
    const void* const* t0 = ws.host_table(&ix, 3, true);
    const void* const* t1 = ws.host_table(&ix, 2, false);  // a second table (scann_index_rbf_features) must not move the first
    for (int i = 0; i < 64; ++i) (void)ws.host_table(&ix, 1, false);
    for (int c = 0; c < 3; ++c) CHECK(t0[c] == ix.rows_of((size_t)c) && t0[3 + c] == ix.ids_of((size_t)c));
    for (int c = 0; c < 2; ++c) CHECK(t1[c] == ix.rows_of((size_t)c));
    CHECK(ws.upload_rows(&ix, 0, d_rows, d_ids, nullptr) == hipSuccess);  // no chunks: nothing is enqueued
    ws.release();  // (a table freed before this, or not at all, is a sanitizer report)
  }
  CHECK(g_live == 0 && g_allocs == g_frees);
  return finish("scann_call_check");
}
