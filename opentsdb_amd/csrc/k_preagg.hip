// k_preagg.hip -- pre-aggregate generation (the group-by half of the 2.4 rollup storage model,
// TSDB.addAggregatePointInternal with is_groupby, src/core/TSDB.java:1441-1588): the dense
// [function][group][slot] results of n_funcs downsampled group-by queries (engine.cpp
// tsdbhip_preagg_run gathers them into one slab on the device) -> the cells a TSD would write
// with addAggregatePoint(metric, ts, value, tags, true, interval, rollup_agg, groupby_agg).
//
// One pass each over all n_funcs * G * K entries, whatever the number of functions:
//   k_preagg_size   a code per entry: 0 = no cell (slot not emitted, or the group has no span in
//                   the scan range), else the value length -- 4 when (float) v == v, else 8
//                   (Tags.fitsInFloat; downsampled group results are always doubles, so no integer
//                   cell is written); NaN / +-Inf raise the error word (addAggregatePoint rejects
//                   them);
//   preagg_scan     one device-wide exclusive scan of a packed key (cells in the low half, float64
//                   cells in the high half): cell c of an entry, its value offset 4 * (c + c64);
//                   the qualifier length is the same for every cell, so its offset is c * qlen;
//   k_preagg_write  function index, group, row base time, qualifier and big-endian value bytes of
//                   every cell at its offsets; the sentinel entry n writes the totals.
// Entries are 1-8 bytes read and <= 31 bytes written each: the kernels are a thread per entry over
// a grid-stride loop, consecutive lanes on consecutive entries (cells of a wave land in one
// contiguous run of each output array).
#include <hipcub/hipcub.hpp>

#include "engine.h"
#include "rollup_codec.h"
#include "../../include/tsdbhip.h"

namespace tsdb {

namespace {

constexpr int PREAGG_BLOCK = 256;
constexpr int64_t PREAGG_MAX_BLOCKS = 2048;

__device__ __forceinline__ bool preagg_live(const PreaggParams& p, int64_t idx) {
  if (!p.flag[idx]) return false;
  return p.act[idx / p.K] != 0;   // idx / K = f * G + g
}

// value length of the cell (0: addAggregatePoint rejects the value)
__device__ __forceinline__ int preagg_vlen(double v) {
  if (v != v || v == INFINITY || v == -INFINITY) return 0;
  return (double)(float)v == v ? 4 : 8;
}

// Row base time and qualifier of the cell at `ts` seconds.  Form A: getRollupBasetime /
// buildRollupQualifier of the interval; form B: the hour row and Internal.buildQualifier of a
// second timestamp (src/core/Internal.java:848-862).  False: IllegalArgumentException.
__device__ __forceinline__ bool preagg_key(const PreaggParams& p, int64_t ts, int16_t flags, int32_t agg_id,
                                           int32_t& base, uint8_t q[3]) {
  if (p.form_b) {
    if (ts < 0 || (ts & RC_SECOND_MASK) != 0) return false;
    base = jint(ts - ts % 3600);
    const uint32_t w = ((uint32_t)(ts - (ts - ts % 3600)) << 4) | (uint32_t)flags;
    q[0] = (uint8_t)(w >> 8);
    q[1] = (uint8_t)w;
    q[2] = 0;
    return true;
  }
  return rc_basetime(ts, p.iv, base) && rc_qualifier(ts, base, flags, agg_id, p.iv, q);
}

__global__ __launch_bounds__(PREAGG_BLOCK) void k_preagg_size(PreaggParams p) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx <= p.n; idx += stride) {
    uint8_t code = 0;
    if (idx < p.n && preagg_live(p, idx)) {
      const int len = preagg_vlen(p.val[idx]);
      const int64_t f = idx / (p.G * p.K);
      const int64_t k = idx % p.K;
      int32_t base;
      uint8_t q[3];
      if (len == 0 || !preagg_key(p, (p.B0 + k * p.I) / 1000, len == 4 ? 0xB : 0xF, p.agg_id[f], base, q))
        atomicCAS(p.err, 0, (int32_t)TSDB_E_ILLEGAL_ARGUMENT);
      else
        code = (uint8_t)len;
    }
    p.code[idx] = code;   // (entry n: the sentinel, no cell)
  }
}

__global__ __launch_bounds__(PREAGG_BLOCK) void k_preagg_write(PreaggParams p) {
  const int qlen = p.form_b ? 2 : 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx <= p.n; idx += stride) {
    const uint64_t o = p.off[idx];
    const int64_t c = (int64_t)(o & 0xFFFFFFFFu);
    const uint64_t vo = 4 * ((uint64_t)c + (o >> 32));
    if (idx == p.n) {   // the sentinel: totals, the closing value offset, the first error raised
      int32_t e = 0;
      for (int f = 0; f < p.n_funcs; f++)
        if (!e) e = p.qerr[f];
      if (!e) e = *p.err;
      p.o_voff[c] = vo;
      p.totals->cells = c;
      p.totals->qual_bytes = (uint64_t)c * qlen;
      p.totals->value_bytes = vo;
      p.totals->err = e;
      p.totals->pad = 0;
      continue;
    }
    const int len = p.code[idx];
    if (!len) continue;
    const double v = p.val[idx];
    const int64_t f = idx / (p.G * p.K);
    const int64_t g = idx / p.K - f * p.G;
    const int64_t k = idx % p.K;
    int32_t base;
    uint8_t q[3];
    preagg_key(p, (p.B0 + k * p.I) / 1000, len == 4 ? 0xB : 0xF, p.agg_id[f], base, q);
    p.o_func[c] = (int32_t)f;
    p.o_group[c] = (int32_t)g;
    p.o_base[c] = (uint32_t)base;
    for (int b = 0; b < qlen; b++) p.o_qual[c * qlen + b] = q[b];
    p.o_voff[c] = vo;
    // value bytes big-endian; every length is a multiple of 4, so is every offset
    uint32_t* w = reinterpret_cast<uint32_t*>(p.o_val + vo);
    if (len == 4) {
      w[0] = __builtin_bswap32(__float_as_uint((float)v));
    } else {
      const uint64_t u = (uint64_t)__double_as_longlong(v);
      w[0] = __builtin_bswap32((uint32_t)(u >> 32));
      w[1] = __builtin_bswap32((uint32_t)u);
    }
  }
}

unsigned preagg_blocks(int64_t n1) {
  const int64_t b = (n1 + PREAGG_BLOCK - 1) / PREAGG_BLOCK;
  return (unsigned)(b < 1 ? 1 : b > PREAGG_MAX_BLOCKS ? PREAGG_MAX_BLOCKS : b);
}

// code -> packed scan key: one cell in the low 32 bits, one float64 cell in the high 32 bits
struct PreaggKey {
  __host__ __device__ uint64_t operator()(uint8_t code) const {
    return code == 0 ? 0ull : code == 8 ? (1ull | (1ull << 32)) : 1ull;
  }
};

}  // namespace

hipError_t launch_preagg_size(const PreaggParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_preagg_size, dim3(preagg_blocks(p.n + 1)), dim3(PREAGG_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_preagg_write(const PreaggParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_preagg_write, dim3(preagg_blocks(p.n + 1)), dim3(PREAGG_BLOCK), 0, s, p);
  return hipGetLastError();
}

// exclusive prefix sum of the packed keys of n1 = n + 1 codes (temp storage grown on demand);
// n1 < 2^31, so neither half of the key overflows into the other
hipError_t preagg_scan(const uint8_t* code, uint64_t* off, int64_t n1, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  hipcub::TransformInputIterator<uint64_t, PreaggKey, const uint8_t*> in(code, PreaggKey());
  size_t need = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, off, (int)n1, s);
  if (e != hipSuccess) return e;
  if (need > *tmp_bytes) {
    if (*tmp) (void)hipFree(*tmp);
    *tmp = nullptr;
    e = hipMalloc(tmp, need);
    if (e != hipSuccess) { *tmp_bytes = 0; return e; }
    *tmp_bytes = need;
  }
  size_t t = *tmp_bytes;
  return hipcub::DeviceScan::ExclusiveSum(*tmp, t, in, off, (int)n1, s);
}

}  // namespace tsdb
