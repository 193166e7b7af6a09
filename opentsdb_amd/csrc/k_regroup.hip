// k_regroup.hip -- tsdbhip_regroup's device side (gfx950): the resident RowDescs in a new series
// order, without touching a cell byte.
//
// The host hands one 8-byte entry a series of the NEW order: the series' CURRENT resident
// position and its new group word.  From them
//   regroup_scan   one device-wide exclusive scan of the permuted row counts
//                  (srp_old[src + 1] - srp_old[src], read through a transform iterator): the new
//                  series_row_ptr, n + 1 entries;
//   k_regroup      the RowDescs gathered into the second descriptor buffer, and the new gid.
// A RowDesc is three 16-byte words.  k_regroup's unit of work is one destination word: lane l of
// a wave writes word w0 + l, so a wave's store is one contiguous 1-KB run whatever the
// permutation; the three lanes of a row read its 48 source bytes, the only scattered access.  The
// source row of a destination row is found on the device by a binary search of the row in the
// new series_row_ptr (20 probes of an L2-resident array for a million series; no per-row map
// crosses PCIe).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "engine.h"

namespace tsdb {

namespace {

constexpr int REGROUP_BLOCK = 256;
constexpr int64_t REGROUP_MAX_BLOCKS = 2048;   // grid-stride beyond (8 blocks a CU)

static_assert(sizeof(RowDesc) == 3 * sizeof(uint4), "a RowDesc is three 16-byte words");

__global__ __launch_bounds__(REGROUP_BLOCK) void k_regroup(RegroupParams p) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < p.n_series; i += stride) p.gid_new[i] = p.ent[i].y;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.rows_old);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(p.rows_new);
  const int64_t n_words = p.n_rows * 3;
  for (int64_t w = t0; w < n_words; w += stride) {
    const int64_t r = w / 3;
    const int part = (int)(w - r * 3);
    // the series of destination row r: the last i with srp_new[i] <= r (series without rows
    // repeat a value; the last of them is followed by a larger one, as srp_new[n_series] > r)
    int64_t lo = 0, hi = p.n_series;   // srp_new[lo] <= r < srp_new[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (p.srp_new[mid] <= r) lo = mid; else hi = mid;
    }
    const int64_t sr = p.srp_old[p.ent[lo].x] + (r - p.srp_new[lo]);
    dst[w] = src[sr * 3 + part];
    if (part == 0) p.reg_new[r] = p.reg_old[sr];   // the row's RegRow entry moves with it
  }
}

// entry -> rows of the series (the scan's input); the entry one past the last adds nothing, so
// that the scan's n + 1 outputs end with the row total
struct RegroupCount {
  const int64_t* srp_old;
  const int2* ent;
  int64_t n;
  __host__ __device__ int64_t operator()(int64_t i) const {
    if (i >= n) return 0;
    const int64_t s = ent[i].x;
    return srp_old[s + 1] - srp_old[s];
  }
};

}  // namespace

hipError_t regroup_scan(const RegroupParams& p, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<int64_t, RegroupCount, hipcub::CountingInputIterator<int64_t>> in(
      idx, RegroupCount{p.srp_old, p.ent, p.n_series});
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

hipError_t launch_regroup(const RegroupParams& p, hipStream_t s) {
  const int64_t work = std::max<int64_t>(p.n_rows * 3, p.n_series);
  if (work <= 0) return hipSuccess;
  const int64_t b = std::min<int64_t>((work + REGROUP_BLOCK - 1) / REGROUP_BLOCK, REGROUP_MAX_BLOCKS);
  hipLaunchKernelGGL(k_regroup, dim3((unsigned)b), dim3(REGROUP_BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace tsdb
