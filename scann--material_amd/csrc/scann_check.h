// What the stand-alone check programs (scann_*_check.cpp; `make asan-<name>`) share: stubs of what the device halves of the host files
// under test refer to -- none of it is called, every launch answers hipErrorNotSupported -- and the harness: a count of failures,
// EXPECT, a generator each program seeds itself, and the closing line.  Included behind the host files under test; a program keeps the
// stubs that are its own.  SCANN_CHECK_OWN_CACHE: the program brings its own block cache (scann_call_check.cpp counts the blocks).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scann_call.h"
#include "scann_cells.h"
#include "scann_silhouette.h"

namespace scann {
#ifndef SCANN_CHECK_OWN_CACHE
hipError_t cached_malloc(void**, size_t) { return hipErrorNotSupported; }
void cached_free(void*) {}
#endif
int fail(scann_handle*, int code, const std::string&) { return code; }
int check_index(scann_handle*, const scann_index*, const char*) { return SCANN_ERR_INVALID; }
int check_k(scann_handle*, int32_t, const char*) { return SCANN_ERR_INVALID; }
int forward_and_download(scann_handle_t*, scann_dbatch_t*, uint64_t, int32_t, float*, float*) { return SCANN_ERR_INVALID; }
// the twins' chain: the plain loop of scann_knn.cpp
void dist2_to_rows(const float* q, const float* rows, int64_t n, int64_t d, float* out) {
  for (int64_t r = 0; r < n; ++r) {
    float acc = 0.f;
    for (int64_t j = 0; j < d; ++j) {
      const float t = q[j] - rows[r * d + j];
      acc = fmaf(t, t, acc);
    }
    out[r] = acc;
  }
}
void peaks_geometry(int64_t, int64_t, int32_t* r, int32_t* n) { *r = TILE_TR, *n = 1; }
hipError_t launch_sil_eligible(const float* const*, int32_t, int32_t, int32_t, unsigned char*, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_cells_centre(const CellSearchArgs&, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_cells_plan(const CellSearchArgs&, int, hipStream_t) { return hipErrorNotSupported; }
}  // namespace scann

namespace {

int bad = 0;
unsigned state = 0;  // main() seeds it
inline unsigned draw() { state = state * 1664525u + 1013904223u; return (state >> 8) & 0xffffff; }

#define EXPECT(c) do { if (!(c)) ++bad, std::printf("line %d: %s\n", __LINE__, #c); } while (0)

inline uint32_t bits_of(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

// the closing line and the exit status of program `name`
inline int finish(const char* name) {
  if (bad) std::printf("%s: %d FAILED\n", name, bad);
  else std::printf("%s: ok\n", name);
  return bad ? 1 : 0;
}

}  // namespace
