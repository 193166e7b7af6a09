// k_tags.hip -- tsdbhip_regroup_tags' device side (gfx950): a query's tag filters, its group keys
// and their dense numbering over the resident tag table.
//
// The table is the loaded series' tags in batch order: tag_ptr[n + 1] and one 8-byte (tagk, tagv)
// pair a tag, tagk ascending inside a series -- the row key's own order.
//   k_tags_match    one thread a series: every filter against the series' short sorted tag list
//                   (the sets by binary search, unsigned), the verdict, and the group-by tagvs as
//                   key words, column-major.  The only pass that reads the table.
// The numbering, ids in the lexicographic order of the unsigned key words, has two routes:
//   rank            per column a presence bit a UID (one OR a word, skipped when a plain load
//                   already shows the bit), a scan of the words' population counts, hence an
//                   order-preserving dense rank a column; the mixed-radix composite of the ranks
//                   has the keys' order, and a presence word a composite plus one scan give the
//                   id.  No sort over the series.
//   sort            any UIDs, any number of distinct keys: an LSD radix sort of the series' order,
//                   one stable 32-bit pass a column from the last to the first (hipCUB), head
//                   flags, one scan.  A key never has to fit 64 bits.
// Both write the distinct keys in id order.  Nothing synchronises: the host waits once, for the
// ids' download.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "engine.h"
#include "../../include/tsdbhip.h"

namespace tsdb {

namespace {

constexpr int TAGS_BLOCK = 256;
constexpr int64_t TAGS_MAX_BLOCKS = 2048;   // grid-stride beyond (8 blocks a CU)
// Presence bits of UIDs below 32 * TAGS_LDS_WORDS are gathered in LDS, a block's series together,
// and reach the global map as one OR a non-zero word at the block's end: a column of few distinct
// values is a handful of words that every series would otherwise hit (16 KB of LDS for 8 columns).
constexpr int TAGS_LDS_WORDS = 512;

// the tagv of tagk k among the series' tags [a, b)
__device__ __forceinline__ bool tag_find(const uint2* __restrict__ pairs, int64_t a, int64_t b, uint32_t k, uint32_t& v) {
  for (int64_t e = a; e < b; e++) {
    const uint2 t = pairs[e];
    if (t.x == k) {
      v = t.y;
      return true;
    }
    if (t.x > k) break;
  }
  return false;
}

// v in the ascending set s[lo, hi)
__device__ __forceinline__ bool set_has(const uint32_t* __restrict__ s, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint32_t x = s[mid];
    if (x == v) return true;
    if (x < v) lo = mid + 1; else hi = mid;
  }
  return false;
}

__global__ __launch_bounds__(TAGS_BLOCK) void k_tags_match(TagsParams p) {
  __shared__ uint32_t lpres[TAGS_MAX_GROUP_BY * TAGS_LDS_WORDS];
  const int lw = (int)(p.W < TAGS_LDS_WORDS ? p.W : TAGS_LDS_WORDS);   // words a column held in LDS
  if (p.pres) {
    for (int x = threadIdx.x; x < p.n_group_by * TAGS_LDS_WORDS; x += TAGS_BLOCK) lpres[x] = 0u;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_series; i += stride) {
    const int64_t a = p.tag_ptr[i], b = p.tag_ptr[i + 1];
    bool vis = true;
    for (int f = 0; f < p.n_filters && vis; f++) {
      const TagFilterDev t = p.filters[f];
      uint32_t v = 0;
      const bool has = tag_find(p.pairs, a, b, t.tagk, v);
      switch (t.kind) {
        case TSDB_TF_ANY: vis = has; break;
        case TSDB_TF_IN: vis = has && set_has(p.sets, t.set_begin, t.set_end, v); break;
        case TSDB_TF_NOT_IN: vis = !has || !set_has(p.sets, t.set_begin, t.set_end, v); break;
        default: vis = !has; break;   // TSDB_TF_NOT_KEY
      }
    }
    if (vis && p.explicit_tags) {   // exactly the filters' tagks: two ascending lists, equal
      vis = b - a == p.n_etagk;
      for (int e = 0; e < p.n_etagk && vis; e++) vis = p.pairs[a + e].x == p.etagk[e];
    }
    uint32_t key[TAGS_MAX_GROUP_BY];
    bool complete = vis;
#pragma unroll
    for (int j = 0; j < TAGS_MAX_GROUP_BY; j++) {
      key[j] = 0;
      if (j < p.n_group_by && complete) complete = tag_find(p.pairs, a, b, p.group_by[j], key[j]);
    }
    p.ids[i] = !vis ? TSDB_GROUP_EXCLUDED : complete ? 0 : TSDB_GROUP_NONE;
#pragma unroll
    for (int j = 0; j < TAGS_MAX_GROUP_BY; j++) {
      if (j >= p.n_group_by) break;
      const uint32_t v = complete ? key[j] : 0u;
      p.kw[(int64_t)j * p.n_series + i] = v;
      if (complete && p.pres) {   // (v is at most the table's largest tagv: below 32 * W)
        const uint32_t bit = 1u << (v & 31);
        if ((v >> 5) < (uint32_t)lw) {
          uint32_t* const w = lpres + j * TAGS_LDS_WORDS + (v >> 5);
          if (!(*w & bit)) atomicOr(w, bit);
        } else {
          uint32_t* const w = p.pres + (int64_t)j * p.W + (v >> 5);
          if (!(*w & bit)) atomicOr(w, bit);
        }
      }
    }
  }
  if (p.pres) {
    __syncthreads();
    for (int x = threadIdx.x; x < p.n_group_by * lw; x += TAGS_BLOCK) {
      const int j = x / lw, wi = x - j * lw;
      const uint32_t bits = lpres[j * TAGS_LDS_WORDS + wi];
      uint32_t* const w = p.pres + (int64_t)j * p.W + wi;   // (wi < lw <= W)
      if (bits && (*w & bits) != bits) atomicOr(w, bits);
    }
  }
}

// ---- the rank route -------------------------------------------------------------------------
struct PopcIn {
  const uint32_t* w;
  int64_t n;
  __host__ __device__ uint32_t operator()(int64_t i) const { return i < n ? (uint32_t)__popc(w[i]) : 0u; }
};

// the columns' cardinalities into mixed-radix weights (one thread: at most 8 columns)
__global__ void k_tags_radix(TagsParams p) {
  if (blockIdx.x || threadIdx.x) return;
  unsigned long long prod = 1;
  bool ok = true;
  for (int j = p.n_group_by - 1; j >= 0; j--) {
    const unsigned long long card = p.wrank[(int64_t)(j + 1) * p.W] - p.wrank[(int64_t)j * p.W];
    p.meta->mult[j] = ok ? (uint32_t)prod : 0u;
    prod *= card;   // (below 2^22 * 2^24 while ok)
    if (prod > (unsigned long long)TAGS_RANK_MAX_KEYS) {
      ok = false;
      prod = 1;
    }
  }
  p.meta->rank_ok = ok ? 1u : 0u;
}

__global__ __launch_bounds__(TAGS_BLOCK) void k_tags_compose(TagsParams p) {
  if (!p.meta->rank_ok) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_series; i += stride) {
    if (p.ids[i] != 0) continue;
    uint32_t comp = 0;
    for (int j = 0; j < p.n_group_by; j++) {
      const uint32_t v = p.kw[(int64_t)j * p.n_series + i];
      const int64_t w = (int64_t)j * p.W + (v >> 5);
      const uint32_t r = p.wrank[w] - p.wrank[(int64_t)j * p.W] + (uint32_t)__popc(p.pres[w] & ((1u << (v & 31)) - 1u));
      comp += r * p.meta->mult[j];
    }
    p.comp[i] = comp;     // below the cardinalities' product, at most TAGS_RANK_MAX_KEYS
    if (!p.cpres[comp]) p.cpres[comp] = 1u;   // (idempotent; the load spares most stores of a large group)
  }
}

__global__ __launch_bounds__(TAGS_BLOCK) void k_tags_rank_assign(TagsParams p) {
  if (!p.meta->rank_ok) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 == 0) p.meta->n_groups = p.crank[TAGS_RANK_MAX_KEYS];
  for (int64_t i = t0; i < p.n_series; i += stride) {
    if (p.ids[i] != 0) continue;
    const uint32_t id = p.crank[p.comp[i]];
    p.ids[i] = (int32_t)id;
    for (int j = 0; j < p.n_group_by; j++)   // (every series of a group stores the same words)
      p.keys[(int64_t)id * p.n_group_by + j] = p.kw[(int64_t)j * p.n_series + i];
  }
}

// ---- the sort route -------------------------------------------------------------------------
__global__ __launch_bounds__(TAGS_BLOCK) void k_tags_iota(uint32_t* pa, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) pa[i] = (uint32_t)i;
}

// column `col` in the present order; col < 0: 0 for a series with a complete key, 1 for the others
__global__ __launch_bounds__(TAGS_BLOCK) void k_tags_gather(TagsParams p, const uint32_t* pa, uint32_t* ka, int col) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_series; i += stride) {
    const uint32_t s = pa[i];
    ka[i] = col < 0 ? (p.ids[s] != 0 ? 1u : 0u) : p.kw[(int64_t)col * p.n_series + s];
  }
}

__global__ __launch_bounds__(TAGS_BLOCK) void k_tags_heads(TagsParams p, const uint32_t* pa) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_series; i += stride) {
    const uint32_t s = pa[i];
    uint32_t h = 0;
    if (p.ids[s] == 0) {   // (the series with a complete key come first: so is pa[i - 1])
      h = i == 0 ? 1u : 0u;
      const uint32_t q = i ? pa[i - 1] : s;
      for (int j = 0; j < p.n_group_by && !h; j++)
        h = p.kw[(int64_t)j * p.n_series + s] != p.kw[(int64_t)j * p.n_series + q] ? 1u : 0u;
    }
    p.head[i] = h;
  }
}

__global__ __launch_bounds__(TAGS_BLOCK) void k_tags_sort_assign(TagsParams p, const uint32_t* pa) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n_series; i += stride) {
    if (i == p.n_series - 1) p.meta->n_groups = p.hsum[i];
    const uint32_t s = pa[i];
    if (p.ids[s] != 0) continue;
    const uint32_t id = p.hsum[i] - 1u;
    p.ids[s] = (int32_t)id;
    if (p.head[i])
      for (int j = 0; j < p.n_group_by; j++) p.keys[(int64_t)id * p.n_group_by + j] = p.kw[(int64_t)j * p.n_series + s];
  }
}

unsigned blocks_for(int64_t n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + TAGS_BLOCK - 1) / TAGS_BLOCK, TAGS_MAX_BLOCKS));
}

hipError_t grow_tmp(void** tmp, size_t* tmp_bytes, size_t need) {
  if (need <= *tmp_bytes && *tmp) return hipSuccess;
  if (*tmp) (void)hipFree(*tmp);
  *tmp = nullptr;
  *tmp_bytes = 0;
  const hipError_t e = hipMalloc(tmp, std::max<size_t>(need, 16));
  if (e == hipSuccess) *tmp_bytes = std::max<size_t>(need, 16);
  return e;
}

}  // namespace

hipError_t launch_tags_match(const TagsParams& p, hipStream_t s) {
  if (p.n_series <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_tags_match, dim3(blocks_for(p.n_series)), dim3(TAGS_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t tags_number_rank(const TagsParams& p, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  if (p.n_series <= 0) return hipSuccess;
  const int64_t words = (int64_t)p.n_group_by * p.W;   // at most 8 * 2^19
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<uint32_t, PopcIn, hipcub::CountingInputIterator<int64_t>> in(idx, PopcIn{p.pres, words});
  const int n1 = (int)(words + 1), nk = (int)(TAGS_RANK_MAX_KEYS + 1);
  size_t need1 = 0, need2 = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need1, in, p.wrank, n1, s);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, need2, p.cpres, p.crank, nk, s);
  if (e != hipSuccess) return e;
  e = grow_tmp(tmp, tmp_bytes, std::max(need1, need2));
  if (e != hipSuccess) return e;
  size_t t = *tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(*tmp, t, in, p.wrank, n1, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_tags_radix, dim3(1), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_tags_compose, dim3(blocks_for(p.n_series)), dim3(TAGS_BLOCK), 0, s, p);
  t = *tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(*tmp, t, p.cpres, p.crank, nk, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_tags_rank_assign, dim3(blocks_for(p.n_series)), dim3(TAGS_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t tags_number_sort(const TagsParams& p, void** tmp, size_t* tmp_bytes, hipStream_t s) {
  if (p.n_series <= 0) return hipSuccess;
  const int n = (int)p.n_series;
  size_t need1 = 0, need2 = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, need1, p.ka, p.kb, p.pa, p.pb, n, 0, 32, s);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::InclusiveSum(nullptr, need2, p.head, p.hsum, n, s);
  if (e != hipSuccess) return e;
  e = grow_tmp(tmp, tmp_bytes, std::max(need1, need2));
  if (e != hipSuccess) return e;
  const dim3 grid(blocks_for(p.n_series)), block(TAGS_BLOCK);
  uint32_t* pa = p.pa;
  uint32_t* pb = p.pb;
  hipLaunchKernelGGL(k_tags_iota, grid, block, 0, s, pa, p.n_series);
  // least significant first: the last column ... the first, then complete keys before the others
  for (int col = p.n_group_by - 1; col >= -1; col--) {
    hipLaunchKernelGGL(k_tags_gather, grid, block, 0, s, p, pa, p.ka, col);
    size_t t = *tmp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(*tmp, t, p.ka, p.kb, pa, pb, n, 0, col < 0 ? 1 : 32, s);
    if (e != hipSuccess) return e;
    std::swap(pa, pb);
  }
  hipLaunchKernelGGL(k_tags_heads, grid, block, 0, s, p, pa);
  size_t t = *tmp_bytes;
  e = hipcub::DeviceScan::InclusiveSum(*tmp, t, p.head, p.hsum, n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_tags_sort_assign, grid, block, 0, s, p, pa);
  return hipGetLastError();
}

}  // namespace tsdb
