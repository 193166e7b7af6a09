// k_upsert.hip -- tsdbhip_upsert's device side (gfx950): the resident RowDescs merged with a
// delta's descriptors by (series, base time), anywhere in a series.
//
// As in tsdbhip_append the delta's cells sit at the blobs' tail and have been indexed in an array
// of their own, in staging order: series by series, each series' rows by base time (distinct
// inside a series after merge_same_base).  k_append assumes a series' rows are its kept resident
// rows followed by its delta rows; here two base-sorted lists are merged, with replacement.
//   k_upsert_rank        one thread a delta row: lb = the lower bound of the row's base among its
//                        series' resident RowDesc.base, hit = 1 when that base is resident (the
//                        delta row replaces that row);
//   upsert_scan_hits     one device-wide exclusive scan of hit over all delta rows, S.  For the
//                        series entry with delta rows [d0, d0 + dn): H(b) = S[d0 + b] - S[d0];
//   upsert_scan          the new series_row_ptr: a series keeps nres + dn - H(dn) rows;
//   k_upsert             the gather.  The unit of work is one 16-byte destination word, so a
//                        wave's store is one contiguous 1-KB run; the series of destination row r
//                        is found by a binary search in the new series_row_ptr, j is the row's
//                        index inside the series.  Delta row b lands at dest(b) = lb[b] - H(b) + b
//                        (the resident rows before it, minus those of them that were replaced,
//                        plus the delta rows before it), strictly increasing in b.  With b = the
//                        number of delta rows with dest < j (a binary search over dn): dest(b) == j
//                        -> delta row d0 + b, else resident row j - b + H(b).  The RegRow moves
//                        with its row; ROW_SFIRST is set on j == 0 and cleared elsewhere.
//                        No atomics; every offset is 64-bit.
// The ROW_UNSORTED walk over the touched series and the re-index of the suspect rows are
// tsdbhip_trim's kernels (k_trim.hip).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "engine.h"

namespace tsdb {

namespace {

constexpr int UPSERT_BLOCK = 256;
constexpr int64_t UPSERT_MAX_BLOCKS = 2048;   // grid-stride beyond (8 blocks a CU)

static_assert(sizeof(RowDesc) == 3 * sizeof(uint4), "a RowDesc is three 16-byte words");
static_assert(offsetof(RowDesc, flags) == 2 * sizeof(uint4), "flags lead the third word");

__global__ __launch_bounds__(UPSERT_BLOCK) void k_upsert_rank(UpsertRankParams p) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > p.n_delta) return;
  if (k == p.n_delta) { p.hit[k] = 0; return; }   // (the scan's n + 1 outputs end with the total)
  const int32_t s = p.dser[k];
  int32_t lb = 0, hit = 0;
  if (s >= 0) {
    const int64_t r0 = p.srp_old[s], r1 = p.srp_old[s + 1];
    const uint32_t base = p.rows_delta[k].base;
    int64_t lo = r0, hi = r1;   // the first resident row with base >= the delta row's
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (p.rows_old[mid].base < base) lo = mid + 1; else hi = mid;
    }
    lb = (int32_t)(lo - r0);
    hit = lo < r1 && p.rows_old[lo].base == base ? 1 : 0;
  }
  p.lb[k] = lb;
  p.hit[k] = hit;
}

// entry -> rows of the series after the upsert (the scan's input); the entry one past the last
// adds nothing, so that the scan's n + 1 outputs end with the row total
struct UpsertCount {
  const int64_t* srp_old;
  const int4* ent;
  const int32_t* S;
  int64_t n;
  __host__ __device__ int64_t operator()(int64_t i) const {
    if (i >= n) return 0;
    const int4 e = ent[i];
    const int64_t res = e.x < 0 ? 0 : srp_old[e.x + 1] - srp_old[e.x];
    if (e.w == 0) return res;
    return res + (int64_t)e.w - (int64_t)(S[(int64_t)e.z + e.w] - S[e.z]);
  }
};

__global__ __launch_bounds__(UPSERT_BLOCK) void k_upsert(UpsertParams p) {
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
    const int64_t d0 = e.z, dn = e.w;
    bool from_delta = false;
    int64_t sr;   // the source row, in rows_delta or rows_old
    if (dn == 0) {
      sr = p.srp_old[e.x] + j;
    } else {
      const int32_t s0 = p.S[d0];
      // b: the delta rows with dest < j (dest is strictly increasing)
      int64_t bl = 0, bh = dn;
      while (bl < bh) {
        const int64_t mid = (bl + bh) >> 1;
        const int64_t dest = (int64_t)p.lb[d0 + mid] - (int64_t)(p.S[d0 + mid] - s0) + mid;
        if (dest < j) bl = mid + 1; else bh = mid;
      }
      const int64_t b = bl;
      if (b < dn && (int64_t)p.lb[d0 + b] - (int64_t)(p.S[d0 + b] - s0) + b == j) {
        from_delta = true;
        sr = d0 + b;
      } else {   // (only reached with e.x >= 0: a series without resident rows is all delta rows)
        sr = p.srp_old[e.x] + (j - b + (int64_t)(p.S[d0 + b] - s0));
      }
    }
    uint4 v = (from_delta ? src_delta : src_old)[sr * 3 + part];
    if (part == 0) p.reg_new[r] = (from_delta ? p.reg_delta : p.reg_old)[sr];   // the row's RegRow entry moves with it
    if (part == 2) v.x = (v.x & ~(uint32_t)ROW_SFIRST) | (j == 0 ? (uint32_t)ROW_SFIRST : 0u);
    dst[w] = v;
  }
}

template <typename In, typename Out>
hipError_t exclusive_sum(In in, Out out, int n, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  size_t need = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, n, s);
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
  return hipcub::DeviceScan::ExclusiveSum(*tmp, t, in, out, n, s);
}

}  // namespace

hipError_t launch_upsert_rank(const UpsertRankParams& p, hipStream_t s) {
  const int64_t n1 = p.n_delta + 1;
  hipLaunchKernelGGL(k_upsert_rank, dim3((unsigned)((n1 + UPSERT_BLOCK - 1) / UPSERT_BLOCK)), dim3(UPSERT_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t upsert_scan_hits(const int32_t* hit, int32_t* S, int64_t n_delta, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  return exclusive_sum(hit, S, (int)(n_delta + 1), tmp, tmp_bytes, s);
}

hipError_t upsert_scan(const UpsertParams& p, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<int64_t, UpsertCount, hipcub::CountingInputIterator<int64_t>> in(
      idx, UpsertCount{p.srp_old, p.ent, p.S, p.n_series});
  return exclusive_sum(in, p.srp_new, (int)(p.n_series + 1), tmp, tmp_bytes, s);
}

hipError_t launch_upsert(const UpsertParams& p, hipStream_t s) {
  const int64_t work = std::max<int64_t>(p.n_rows * 3, p.n_series);
  if (work <= 0) return hipSuccess;
  const int64_t b = std::min<int64_t>((work + UPSERT_BLOCK - 1) / UPSERT_BLOCK, UPSERT_MAX_BLOCKS);
  hipLaunchKernelGGL(k_upsert, dim3((unsigned)b), dim3(UPSERT_BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace tsdb
