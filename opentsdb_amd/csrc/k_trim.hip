// k_trim.hip -- tsdbhip_trim's device side (gfx950): old rows evicted from the resident batch and
// the blobs re-laid without their dead bytes.
//
//   trim_scan            one device-wide exclusive scan of the kept row counts (the series' rows
//                        minus the skip[i] it loses at its front): the new series_row_ptr;
//   k_trim_gather        k_regroup with a per-series skip.  The unit of work is one 16-byte
//                        destination word of a RowDesc, so a wave's store is one contiguous 1-KB
//                        run; the series of a destination row is found by a binary search in the
//                        new series_row_ptr; the row's RegRow moves with it; ROW_SFIRST is set on
//                        each series' first kept row and cleared elsewhere;
//   k_trim_stage         the suspect rows (ROW_UNSORTED that an evicted row may have caused) as
//   k_trim_unstage       unindexed descriptors in an array of their own, for the existing index
//                        path, and back;
//   k_trim_recede        k_recede (recede.h) for the listed series: any kept row may be flagged;
//   k_trim_pack<KIND>    the copy of every row's cells into the fresh blobs.  A wave owns
//                        PACK_SPAN contiguous destination bytes and lane l of it the 16-byte
//                        words l, l + 64, ..., so each of its stores is one contiguous 1-KB run
//                        whatever the order of the source rows.  Two wave-uniform binary searches
//                        in the destination offsets give the rows [r_lo, r_hi] the span touches; a
//                        lane searches only inside them (no probe when the span lies in one row).
//                        Source and destination row starts are 16-byte aligned, so the traffic is
//                        uint4 only; a row's last word is masked to its length, which makes the
//                        packed padding zero whatever the source padding held.  KIND 0 / 1: the
//                        qualifier / value blob; KIND 2: the int16 value copy (val2), which lives
//                        at qualifier offsets and exists only for the rows whose flags say so --
//                        other rows' words are written as zeros;
//   k_trim_offsets       qoff / voff of the gathered descriptors rewritten to the packed layout.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "engine.h"
#include "recede.h"

namespace tsdb {

namespace {

constexpr int TRIM_BLOCK = 256;
constexpr int64_t TRIM_MAX_BLOCKS = 2048;   // grid-stride beyond (8 blocks a CU)

static_assert(sizeof(RowDesc) == 3 * sizeof(uint4), "a RowDesc is three 16-byte words");
static_assert(offsetof(RowDesc, flags) == 2 * sizeof(uint4), "flags lead the third word");

__global__ __launch_bounds__(TRIM_BLOCK) void k_trim_gather(TrimParams p) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.rows_old);
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
    const int64_t j = r - p.srp_new[lo];
    const int64_t sr = p.srp_old[lo] + p.skip[lo] + j;
    uint4 v = src[sr * 3 + part];
    if (part == 0) p.reg_new[r] = p.reg_old[sr];   // the row's RegRow entry moves with it
    if (part == 2) v.x = (v.x & ~(uint32_t)ROW_SFIRST) | (j == 0 ? (uint32_t)ROW_SFIRST : 0u);
    dst[w] = v;
  }
}

// series -> rows it keeps (the scan's input); the entry one past the last adds nothing, so that
// the scan's n + 1 outputs end with the row total
struct TrimCount {
  const int64_t* srp_old;
  const int64_t* skip;
  int64_t n;
  __host__ __device__ int64_t operator()(int64_t i) const {
    if (i >= n) return 0;
    return srp_old[i + 1] - srp_old[i] - skip[i];
  }
};

__global__ __launch_bounds__(256) void k_trim_stage(const RowDesc* __restrict__ rows, const int64_t* __restrict__ list,
                                                    int64_t n, RowDesc* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const RowDesc s = rows[list[t]];
  RowDesc d{};   // what a load hands the index: where the cells are, nothing derived
  d.qoff = s.qoff;
  d.voff = s.voff;
  d.base = s.base;
  d.qlen = s.qlen;
  d.vlen = s.vlen;
  out[t] = d;
}

__global__ __launch_bounds__(256) void k_trim_unstage(const RowDesc* __restrict__ in, const RegRow* __restrict__ reg_in,
                                                      const int64_t* __restrict__ list, int64_t n,
                                                      RowDesc* __restrict__ rows, RegRow* __restrict__ reg) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t r = list[t];
  RowDesc d = in[t];
  d.flags = (d.flags & ~(uint32_t)ROW_SFIRST) | (rows[r].flags & (uint32_t)ROW_SFIRST);   // (the gather placed it)
  rows[r] = d;
  reg[r] = reg_in[t];
}

__global__ __launch_bounds__(256) void k_trim_recede(RowDesc* __restrict__ rows, RegRow* __restrict__ reg,
                                                     const int64_t* __restrict__ srp, const int32_t* __restrict__ series,
                                                     int64_t n, const uint8_t* __restrict__ qual) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t s = series[t];
  recede_series(rows, reg, srp[s], srp[s + 1], srp[s], qual);
}

// ---- the pack ------------------------------------------------------------------------------------
constexpr int PACK_WPL = 4;                          // 16-byte words a lane copies
constexpr int PACK_SPAN_WORDS = 64 * PACK_WPL;       // a wave's span: 4 KB of destination
constexpr int PACK_BLOCK = 256;                      // four spans a block

// row -> its aligned length (the scan's input); the entry one past the last adds nothing
template <int KIND>
struct PackLen {
  const RowDesc* rows;
  int64_t n;
  __host__ __device__ uint64_t operator()(int64_t i) const {
    if (i >= n) return 0;
    const uint64_t len = KIND == 1 ? rows[i].vlen : rows[i].qlen;
    return (len + 15) & ~(uint64_t)15;
  }
};

// the last r in [lo, hi) with dst[r] <= b, given dst[lo] <= b < dst[hi]
__device__ __forceinline__ int64_t pack_row_of(const uint64_t* __restrict__ dst, int64_t lo, int64_t hi, uint64_t b) {
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (dst[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

template <int KIND>
__global__ __launch_bounds__(PACK_BLOCK) void k_trim_pack(TrimPackParams p) {
  const uint64_t* __restrict__ dof = KIND == 1 ? p.vdst : p.qdst;
  const uint8_t* __restrict__ src = KIND == 0 ? p.qual : KIND == 1 ? p.val : p.val2;
  uint8_t* __restrict__ out = KIND == 0 ? p.qual_new : KIND == 1 ? p.val_new : p.val2_new;
  const int64_t total_w = (int64_t)((KIND == 1 ? p.v_total : p.q_total) >> 4);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int64_t w0 = ((int64_t)blockIdx.x * (PACK_BLOCK / 64) + wave) * PACK_SPAN_WORDS;   // wave-uniform
  if (w0 >= total_w) return;
  const int64_t w_last = min(w0 + PACK_SPAN_WORDS, total_w) - 1;
  // the rows the span touches: dof[n_rows] = total > every word of it, and rows without bytes
  // repeat an offset, of which the search takes the last
  const int64_t r_lo = pack_row_of(dof, 0, p.n_rows, (uint64_t)w0 << 4);
  const int64_t r_hi = pack_row_of(dof, r_lo, p.n_rows, (uint64_t)w_last << 4);
  uint4 v[PACK_WPL];
  int64_t wd[PACK_WPL];
  uint32_t keep[PACK_WPL];   // bytes of the word inside its row (0: none is written as data)
#pragma unroll
  for (int k = 0; k < PACK_WPL; k++) {
    const int64_t w = w0 + lane + 64 * k;
    wd[k] = w;
    const int64_t wc = min(w, w_last);   // (the loads are unconditional in count)
    const uint64_t b = (uint64_t)wc << 4;
    const int64_t r = pack_row_of(dof, r_lo, r_hi + 1, b);
    const RowDesc d = p.rows[r];
    const uint64_t o = b - dof[r];
    const uint64_t len = KIND == 1 ? d.vlen : d.qlen;
    const uint64_t so = (KIND == 1 ? d.voff : d.qoff) + o;
    v[k] = *reinterpret_cast<const uint4*>(src + so);
    uint32_t kp = (uint32_t)min<uint64_t>(16, len - o);
    if (KIND == 2 && (d.flags & (ROW_QW_MASK | ROW_ALLI | ROW_VLE2 | ROW_ERR)) != (2u | ROW_ALLI | ROW_VLE2)) kp = 0;
    keep[k] = kp;
  }
#pragma unroll
  for (int k = 0; k < PACK_WPL; k++) {
    if (wd[k] > w_last) continue;
    uint4 x = v[k];
    const uint32_t kp = keep[k];
    if (kp < 16) {   // a row's last word, or a row without an int16 copy: the rest is zero
      uint32_t c[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t lo = 4u * i;
        c[i] = kp >= lo + 4 ? c[i] : kp <= lo ? 0u : (c[i] & (0xFFFFFFFFu >> (8u * (lo + 4 - kp))));
      }
      x = make_uint4(c[0], c[1], c[2], c[3]);
    }
    *reinterpret_cast<uint4*>(out + ((uint64_t)wd[k] << 4)) = x;
  }
}

__global__ __launch_bounds__(256) void k_trim_offsets(RowDesc* __restrict__ rows, const uint64_t* __restrict__ qdst,
                                                      const uint64_t* __restrict__ vdst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
    rows[r].qoff = qdst[r];
    rows[r].voff = vdst[r];
  }
}

template <class In, class Out>
hipError_t scan_into(In in, Out* out, int64_t n1, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  size_t need = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)n1, s);
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
  return hipcub::DeviceScan::ExclusiveSum(*tmp, t, in, out, (int)n1, s);
}

template <int KIND>
hipError_t launch_pack_kind(const TrimPackParams& p, hipStream_t s) {
  const int64_t total_w = (int64_t)((KIND == 1 ? p.v_total : p.q_total) >> 4);
  if (total_w <= 0 || p.n_rows <= 0) return hipSuccess;
  const int64_t spans = (total_w + PACK_SPAN_WORDS - 1) / PACK_SPAN_WORDS;
  const int64_t blocks = (spans + PACK_BLOCK / 64 - 1) / (PACK_BLOCK / 64);
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_trim_pack<KIND>, dim3((unsigned)blocks), dim3(PACK_BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace

hipError_t trim_scan(const TrimParams& p, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<int64_t, TrimCount, hipcub::CountingInputIterator<int64_t>> in(
      idx, TrimCount{p.srp_old, p.skip, p.n_series});
  return scan_into(in, p.srp_new, p.n_series + 1, tmp, tmp_bytes, s);
}

hipError_t launch_trim_gather(const TrimParams& p, hipStream_t s) {
  const int64_t work = p.n_rows * 3;
  if (work <= 0) return hipSuccess;
  const int64_t b = std::min<int64_t>((work + TRIM_BLOCK - 1) / TRIM_BLOCK, TRIM_MAX_BLOCKS);
  hipLaunchKernelGGL(k_trim_gather, dim3((unsigned)b), dim3(TRIM_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_trim_stage(const RowDesc* rows, const int64_t* list, int64_t n, RowDesc* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_trim_stage, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, list, n, out);
  return hipGetLastError();
}

hipError_t launch_trim_unstage(const RowDesc* in, const RegRow* reg_in, const int64_t* list, int64_t n, RowDesc* rows,
                               RegRow* reg, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_trim_unstage, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, reg_in, list, n, rows, reg);
  return hipGetLastError();
}

hipError_t launch_trim_recede(RowDesc* rows, RegRow* reg, const int64_t* srp, const int32_t* series, int64_t n,
                              const uint8_t* qual, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_trim_recede, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, reg, srp, series, n, qual);
  return hipGetLastError();
}

hipError_t trim_pack_scan(const RowDesc* rows, int64_t n_rows, uint64_t* qdst, uint64_t* vdst, void** tmp,
                          size_t* tmp_bytes, hipStream_t s) {
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<uint64_t, PackLen<0>, hipcub::CountingInputIterator<int64_t>> qin(idx, PackLen<0>{rows, n_rows});
  hipcub::TransformInputIterator<uint64_t, PackLen<1>, hipcub::CountingInputIterator<int64_t>> vin(idx, PackLen<1>{rows, n_rows});
  hipError_t e = scan_into(qin, qdst, n_rows + 1, tmp, tmp_bytes, s);
  if (e != hipSuccess) return e;
  return scan_into(vin, vdst, n_rows + 1, tmp, tmp_bytes, s);
}

hipError_t launch_trim_pack(const TrimPackParams& p, hipStream_t s) {
  hipError_t e = launch_pack_kind<0>(p, s);
  if (e != hipSuccess) return e;
  e = launch_pack_kind<1>(p, s);
  if (e != hipSuccess) return e;
  return p.val2 && p.val2_new ? launch_pack_kind<2>(p, s) : hipSuccess;
}

hipError_t launch_trim_offsets(RowDesc* rows, const uint64_t* qdst, const uint64_t* vdst, int64_t n_rows, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  const int64_t b = std::min<int64_t>((n_rows + 255) / 256, TRIM_MAX_BLOCKS);
  hipLaunchKernelGGL(k_trim_offsets, dim3((unsigned)b), dim3(256), 0, s, rows, qdst, vdst, n_rows);
  return hipGetLastError();
}

}  // namespace tsdb
