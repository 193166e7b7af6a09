// k_append.hip -- tsdbhip_append's device side (gfx950): the resident RowDescs merged with a
// delta's descriptors, in the series order of the batch after the append.
//
// The delta's cells sit at the blobs' tail and have been indexed in an array of their own (the
// existing k_index path over that array); no resident cell byte moves and no resident row is
// re-indexed.  The host hands one 16-byte entry a series of the NEW order (AppendParams.ent).
//   append_scan          one device-wide exclusive scan of the new per-series row counts -- the
//                        series' resident rows, minus a replaced last row, plus its delta rows:
//                        the new series_row_ptr, n + 1 entries;
//   k_append             k_regroup generalised to two sources: a series' rows are its kept
//                        resident rows followed by its delta rows.  The unit of work is one
//                        16-byte destination word, so a wave's store is one contiguous 1-KB run;
//                        the series of a destination row is found by a binary search in the new
//                        series_row_ptr.  ROW_SFIRST is set on each series' first destination row
//                        and cleared elsewhere (a replaced only-row and the first row of a series
//                        without resident rows come from the delta, which carries no such flag);
//   k_recede_touched     k_recede (k_index.hip) for the listed series: one thread walks a series'
//                        rows carrying the latest datapoint so far and flags ROW_UNSORTED on delta
//                        rows only -- resident rows precede every delta row of their series, so
//                        their flags cannot change.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "engine.h"
#include "recede.h"

namespace tsdb {

namespace {

constexpr int APPEND_BLOCK = 256;
constexpr int64_t APPEND_MAX_BLOCKS = 2048;   // grid-stride beyond (8 blocks a CU)

static_assert(sizeof(RowDesc) == 3 * sizeof(uint4), "a RowDesc is three 16-byte words");
static_assert(offsetof(RowDesc, flags) == 2 * sizeof(uint4), "flags lead the third word");

// resident rows the series at entry e keeps
__host__ __device__ inline int64_t append_kept(const int64_t* srp_old, const int4 e) {
  if (e.x < 0) return 0;
  return srp_old[e.x + 1] - srp_old[e.x] - ((e.w & APPEND_REPLACE) ? 1 : 0);
}

__global__ __launch_bounds__(APPEND_BLOCK) void k_append(AppendParams p) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < p.n_series; i += stride) p.gid_new[i] = p.ent[i].y;
  const uint4* __restrict__ src_old = reinterpret_cast<const uint4*>(p.rows_old);
  const uint4* __restrict__ src_delta = reinterpret_cast<const uint4*>(p.rows_delta);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(p.rows_new);
  const int64_t n_words = p.n_rows * 3;
  for (int64_t w = t0; w < n_words; w += stride) {
    const int64_t r = w / 3;
    const int part = (int)(w - r * 3);
    // the series of destination row r: the last i with srp_new[i] <= r (as k_regroup)
    int64_t lo = 0, hi = p.n_series;   // srp_new[lo] <= r < srp_new[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (p.srp_new[mid] <= r) lo = mid; else hi = mid;
    }
    const int4 e = p.ent[lo];
    const int64_t j = r - p.srp_new[lo];
    const int64_t kept = append_kept(p.srp_old, e);
    uint4 v = j < kept ? src_old[(p.srp_old[e.x] + j) * 3 + part] : src_delta[((int64_t)e.z + (j - kept)) * 3 + part];
    if (part == 0)   // the row's RegRow entry moves with it
      p.reg_new[r] = j < kept ? p.reg_old[p.srp_old[e.x] + j] : p.reg_delta[(int64_t)e.z + (j - kept)];
    if (part == 2) v.x = (v.x & ~(uint32_t)ROW_SFIRST) | (j == 0 ? (uint32_t)ROW_SFIRST : 0u);
    dst[w] = v;
  }
}

// entry -> rows of the series after the append (the scan's input); the entry one past the last
// adds nothing, so that the scan's n + 1 outputs end with the row total
struct AppendCount {
  const int64_t* srp_old;
  const int4* ent;
  int64_t n;
  __host__ __device__ int64_t operator()(int64_t i) const {
    if (i >= n) return 0;
    const int4 e = ent[i];
    return append_kept(srp_old, e) + (int64_t)(e.w & ~APPEND_REPLACE);
  }
};

// k_recede's walk (recede.h) over the touched series of the gathered descriptors.  A resident
// row may already carry k_recede's own ROW_UNSORTED; its latest datapoint is then taken as the
// maximum over its cells, which for a cell sorted in itself is its last one, as k_recede read it.
__global__ __launch_bounds__(256) void k_recede_touched(AppendParams p, const int32_t* __restrict__ touched, int64_t n,
                                                        const uint8_t* __restrict__ qual) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t s = touched[t];
  const int64_t r0 = p.srp_new[s], r1 = p.srp_new[s + 1];
  const int64_t first_delta = r1 - (int64_t)(p.ent[s].w & ~APPEND_REPLACE);
  recede_series(p.rows_new, p.reg_new, r0, r1, first_delta, qual);
}

}  // namespace

hipError_t append_scan(const AppendParams& p, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<int64_t, AppendCount, hipcub::CountingInputIterator<int64_t>> in(
      idx, AppendCount{p.srp_old, p.ent, p.n_series});
  const int n1 = (int)(p.n_series + 1);
  size_t need = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, p.srp_new, n1, s);
  if (e != hipSuccess) return e;
  if (need > *tmp_bytes) {
    if (*tmp) (void)hipFree(*tmp);
    *tmp = nullptr;
    *tmp_bytes = 0;
    e = hipMalloc(tmp, need);
    if (e != hipSuccess) return e;
    *tmp_bytes = need;
  }
  size_t t = *tmp_bytes;
  return hipcub::DeviceScan::ExclusiveSum(*tmp, t, in, p.srp_new, n1, s);
}

hipError_t launch_append(const AppendParams& p, hipStream_t s) {
  const int64_t work = std::max<int64_t>(p.n_rows * 3, p.n_series);
  if (work <= 0) return hipSuccess;
  const int64_t b = std::min<int64_t>((work + APPEND_BLOCK - 1) / APPEND_BLOCK, APPEND_MAX_BLOCKS);
  hipLaunchKernelGGL(k_append, dim3((unsigned)b), dim3(APPEND_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_append_recede(const AppendParams& p, const int32_t* touched, int64_t n, const uint8_t* qual,
                                hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_recede_touched, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, touched, n, qual);
  return hipGetLastError();
}

}  // namespace tsdb
