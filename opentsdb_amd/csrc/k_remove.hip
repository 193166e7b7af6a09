// k_remove.hip -- tsdbhip_remove's device side (gfx950): rows leave the resident batch by
// (series, base-time range) from anywhere in a series.
//
//   k_remove_mark        one thread a range: two lower-bound searches of from_s / to_s over the
//                        series' resident RowDesc.base (k_upsert_rank's search) give the rows
//                        [lo, hi) the range covers, written back for the host (16 B a range) and
//                        recorded in a difference array: +1 at lo, -1 at hi, so that overlapping
//                        and repeated ranges cost O(1) each;
//   remove_scan          two device-wide scans over the rows: the inclusive sum of the difference
//                        array is the number of ranges covering each row, the exclusive sum of
//                        "covered by none" is pos[r], the kept rows before row r;
//   k_remove_gather      k_trim_gather with pos in place of the per-series skip.  The unit of work
//                        is one 16-byte destination word of a RowDesc, so a wave's store is one
//                        contiguous 1-KB run; the source of destination row d is the last r with
//                        pos[r] <= d (removed rows behind it have pos == d + 1, those before it
//                        are smaller r), found by a binary search in pos; its series by one in
//                        the new series_row_ptr; the row's RegRow moves with it; ROW_SFIRST is
//                        set on each series' first kept row and cleared elsewhere.
// Every offset is 64-bit; the only atomics are the mark's two global adds a range.  The suspects'
// re-index, the ROW_UNSORTED walk and the pack are tsdbhip_trim's kernels (k_trim.hip).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "engine.h"

namespace tsdb {

namespace {

constexpr int REMOVE_BLOCK = 256;
constexpr int64_t REMOVE_MAX_BLOCKS = 1024;   // grid-stride beyond (4 blocks a CU: the searches are latency-bound, not wide)

static_assert(sizeof(RowDesc) == 3 * sizeof(uint4), "a RowDesc is three 16-byte words");
static_assert(offsetof(RowDesc, flags) == 2 * sizeof(uint4), "flags lead the third word");
static_assert(sizeof(RemoveRange) == 24, "a range is uploaded as 24 bytes");

// the first row of [r0, r1) with base >= t
__device__ __forceinline__ int64_t remove_lower_bound(const RowDesc* __restrict__ rows, int64_t r0, int64_t r1, int64_t t) {
  int64_t lo = r0, hi = r1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rows[mid].base < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(REMOVE_BLOCK) void k_remove_mark(RemoveMarkParams p) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.n_ranges) return;
  const RemoveRange g = p.ranges[k];
  const int64_t r0 = p.srp_old[g.series], r1 = p.srp_old[g.series + 1];
  const int64_t lo = remove_lower_bound(p.rows_old, r0, r1, g.from_s);
  const int64_t hi = remove_lower_bound(p.rows_old, lo, r1, g.to_s);   // (from_s <= to_s: not before lo)
  p.lohi[2 * k] = lo;
  p.lohi[2 * k + 1] = hi;
  if (hi > lo) {
    atomicAdd(&p.diff[lo], 1);
    atomicAdd(&p.diff[hi], -1);
  }
}

// row -> 1 when no range covers it (the scan's input); the entry one past the last adds nothing,
// so that the scan's n + 1 outputs end with the kept total
struct RemoveKeep {
  const int32_t* cov;
  int64_t n;
  __host__ __device__ int32_t operator()(int64_t r) const { return r < n && cov[r] == 0 ? 1 : 0; }
};

__global__ __launch_bounds__(REMOVE_BLOCK) void k_remove_gather(RemoveParams p) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.rows_old);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(p.rows_new);
  const int64_t n_words = p.n_rows * 3;
  for (int64_t w = t0; w < n_words; w += stride) {
    const int64_t r = w / 3;
    const int part = (int)(w - r * 3);
    // the source of destination row r: the last sr with pos[sr] <= r (pos[0] = 0, pos[n_rows_old] = n_rows > r)
    int64_t lo = 0, hi = p.n_rows_old;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)p.pos[mid] <= r) lo = mid; else hi = mid;
    }
    const int64_t sr = lo;
    // its series: the last i with srp_new[i] <= r (as k_trim_gather; of row-less series that repeat an
    // offset the search takes the last, which has the row)
    lo = 0, hi = p.n_series;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (p.srp_new[mid] <= r) lo = mid; else hi = mid;
    }
    const bool first = r == p.srp_new[lo];
    uint4 v = src[sr * 3 + part];
    if (part == 0) p.reg_new[r] = p.reg_old[sr];   // the row's RegRow entry moves with it
    if (part == 2) v.x = (v.x & ~(uint32_t)ROW_SFIRST) | (first ? (uint32_t)ROW_SFIRST : 0u);
    dst[w] = v;
  }
}

template <class In, class Out>
hipError_t remove_scan_into(bool inclusive, In in, Out* out, int64_t n1, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  size_t need = 0;
  hipError_t e = inclusive ? hipcub::DeviceScan::InclusiveSum(nullptr, need, in, out, (int)n1, s)
                           : hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)n1, s);
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
  return inclusive ? hipcub::DeviceScan::InclusiveSum(*tmp, t, in, out, (int)n1, s)
                   : hipcub::DeviceScan::ExclusiveSum(*tmp, t, in, out, (int)n1, s);
}

}  // namespace

hipError_t launch_remove_mark(const RemoveMarkParams& p, hipStream_t s) {
  if (p.n_ranges <= 0) return hipSuccess;
  const int64_t b = (p.n_ranges + REMOVE_BLOCK - 1) / REMOVE_BLOCK;
  if (b > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_remove_mark, dim3((unsigned)b), dim3(REMOVE_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t remove_scan(int32_t* diff, int32_t* pos, int64_t n_rows_old, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  hipError_t e = remove_scan_into(true, diff, diff, n_rows_old + 1, tmp, tmp_bytes, s);
  if (e != hipSuccess) return e;
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<int32_t, RemoveKeep, hipcub::CountingInputIterator<int64_t>> in(
      idx, RemoveKeep{diff, n_rows_old});
  return remove_scan_into(false, in, pos, n_rows_old + 1, tmp, tmp_bytes, s);
}

hipError_t launch_remove_gather(const RemoveParams& p, hipStream_t s) {
  const int64_t work = p.n_rows * 3;
  if (work <= 0) return hipSuccess;
  const int64_t b = std::min<int64_t>((work + REMOVE_BLOCK - 1) / REMOVE_BLOCK, REMOVE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_remove_gather, dim3((unsigned)b), dim3(REMOVE_BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace tsdb
