// k_last.hip -- tsdbhip_last's device side (gfx950): the newest datapoint of each selected series
// at or before its anchor hour (TSUIDQuery.getLastPoint, src/meta/TSUIDQuery.java:161-217,
// over Internal.extractDataPoints, src/core/Internal.java:237-326).  Nothing streams: a series is a
// chain of small dependent reads -- its position, two series_row_ptr entries, a binary search over
// RowDesc.base, the 48-byte RowDesc, then 2-4 B of qualifier and 1-8 B of value -- so the kernels
// keep many chains in flight and make each as short as the descriptor allows.
//
//   k_last_pick   one lane a selected series.  The answer row is the series' latest row with
//                 lo <= base <= h (row bases are unique multiples of 3600 s, so the reference's walk
//                 back hour by hour is one upper-bound search and one comparison).  By the row's
//                 flags the lane then takes one of three routes:
//                   direct  not ROW_UNSORTED, one qualifier width QW, a uniform value length VL: the
//                           last datapoint's qualifier is at qoff + (ndp - 1) QW, its value at
//                           voff + (ndp - 1) VL (never taken from the cell's end: the index accepts
//                           vlen >= the lengths' sum, so a meta byte is no fact of the descriptor);
//                   copied  not ROW_UNSORTED, 2-byte qualifiers, 1-2-byte integers of varying
//                           length and the context's int16 copy: the value is val2[qoff + 2 (ndp - 1)];
//                   walked  everything else (mixed qualifier widths, varying lengths without the
//                           copy, every ROW_UNSORTED row): (output slot, row) goes to a device list
//                           through a wave-aggregated cursor.
//                 On the first two routes a regular row (RegRow.step != 0) that is ROW_ALLF or
//                 ROW_ALLI needs no qualifier at all: the offset is first + (ndp - 1) step and the
//                 type is the flag's.  "No answer" is written as kind 0 by the lane itself.
//   k_last_walk   one wave a listed row, grid-stride over the device-side count (no host
//                 synchronisation in between): the forward pass of index_row_generic (k_index.hip),
//                 64 datapoints a step -- qualifier widths, a wave prefix sum of the value lengths
//                 for the value offsets -- with a running arg-max of the offset in ms, ties to the
//                 later position (the last element of extractDataPoints' stable sort).  Lane 0
//                 decodes the winner.
// Cells are big-endian at unaligned addresses: qualifier and value are assembled from byte loads,
// one datapoint a series.  The only floating-point operation is the float32 -> double widening.
// An answer row flagged ROW_ERR sets the call's error word; no other row's flags are looked at.
#include <algorithm>

#include "kcommon.h"

namespace tsdb {

namespace {

constexpr int LAST_BLOCK = 256;
constexpr int LAST_WAVES = LAST_BLOCK / 64;
constexpr int64_t LAST_WALK_MAX_BLOCKS = 1024;   // k_last_walk's grid cap (4 waves a block); grid-stride beyond

enum : int { LR_OFF = -1, LR_NONE = 0, LR_DIRECT = 1, LR_COPIED = 2, LR_WALK = 3, LR_ERR = 4 };

// len big-endian bytes at p, in the low bits
__device__ __forceinline__ uint64_t last_be(const uint8_t* __restrict__ p, int len) {
  uint64_t b = 0;
  for (int k = 0; k < len; k++) b = (b << 8) | p[k];
  return b;
}

// Cell.parseValue: a long sign-extended from 1 / 2 / 4 / 8 bytes (kind 1), or a double, a float32
// widened (kind 2); 0: a length the flags cannot carry
__device__ __forceinline__ int last_decode(uint64_t be, int len, bool fl, uint64_t& bits) {
  if (fl) {
    if (len == 4) { bits = (uint64_t)__double_as_longlong((double)__uint_as_float((uint32_t)be)); return 2; }
    if (len == 8) { bits = be; return 2; }
    return 0;
  }
  switch (len) {
    case 1: bits = (uint64_t)(int64_t)(int8_t)(uint8_t)be; return 1;
    case 2: bits = (uint64_t)(int64_t)(int16_t)(uint16_t)be; return 1;
    case 4: bits = (uint64_t)(int64_t)(int32_t)(uint32_t)be; return 1;
    case 8: bits = be; return 1;
  }
  return 0;
}

// the offset in ms and the flag nibble of the w-byte qualifier at q (Internal.getOffsetFromQualifier)
__device__ __forceinline__ uint32_t last_qual(const uint8_t* __restrict__ q, int w, uint32_t& fb) {
  if (w == 4) {
    const uint32_t x = (uint32_t)last_be(q, 4);
    fb = x & 0xF;
    return (x & 0x0FFFFFC0u) >> 6;
  }
  const uint32_t x = (uint32_t)last_be(q, 2);
  fb = x & 0xF;
  return (x >> 4) * 1000u;
}

__global__ __launch_bounds__(LAST_BLOCK) void k_last_pick(LastParams p) {
  __shared__ uint32_t h[4];
  if (threadIdx.x < 4) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int route = LR_OFF;
  int64_t row = -1;
  if (i < p.n_sel) {
    route = LR_NONE;
    const int64_t s = p.pos[i];
    const int64_t r0 = p.srp[s], r1 = p.srp[s + 1];
    const int64_t t = p.anchor_each ? p.anchor_each[i] : p.anchor_s;
    const int64_t hh = t - t % 3600;                    // Internal.baseTime
    const int64_t lo_t = hh > p.back_s ? hh - p.back_s : 0;
    // the first row of [r0, r1) with base > hh; the one before it is the latest at or before the anchor hour
    int64_t lo = r0, hi = r1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)p.rows[mid].base <= hh) lo = mid + 1; else hi = mid;
    }
    int kind = 0;
    int64_t ts = 0;
    uint64_t bits = 0;
    if (lo > r0) {
      const RowDesc d = p.rows[lo - 1];
      if ((int64_t)d.base >= lo_t) {
        row = lo - 1;
        const uint32_t f = d.flags;
        const int qw = (int)(f & ROW_QW_MASK), vl = (int)((f & ROW_VL_MASK) >> ROW_VL_SHIFT);
        const bool plain = !(f & ROW_UNSORTED) && (qw == 2 || qw == 4) && d.ndp > 0;
        if (f & ROW_ERR) {
          route = LR_ERR;
        } else if (p.walk_all) {
          route = LR_WALK;
        } else if (plain && vl != 0) {
          route = LR_DIRECT;
        } else if (plain && qw == 2 && p.val2 && (f & (ROW_VLE2 | ROW_ALLI)) == (ROW_VLE2 | ROW_ALLI)) {
          route = LR_COPIED;
        } else {
          route = LR_WALK;
        }
        // (what the index guarantees of a row without ROW_ERR, checked where the addresses are formed)
        if ((route == LR_DIRECT || route == LR_COPIED) &&
            ((uint64_t)d.ndp * (uint64_t)qw > d.qlen || (uint64_t)d.ndp * (uint64_t)vl > d.vlen))
          route = LR_ERR;
        if (route == LR_DIRECT || route == LR_COPIED) {
          const uint64_t last = (uint64_t)d.ndp - 1;
          const RegRow g = p.reg[row];
          uint32_t off_ms, fb = 0;
          bool fl;
          if (g.step != 0 && (f & (ROW_ALLF | ROW_ALLI))) {   // regular and of one type: no qualifier read
            off_ms = (g.first + (uint32_t)last * g.step) * 1000u;
            fl = (f & ROW_ALLF) != 0;
          } else {
            off_ms = last_qual(p.qual + d.qoff + last * (uint64_t)qw, qw, fb);
            fl = (fb & 8) != 0;
          }
          ts = (int64_t)d.base * 1000 + (int64_t)off_ms;
          if (route == LR_DIRECT) {
            kind = last_decode(last_be(p.val + d.voff + last * (uint64_t)vl, vl), vl, fl, bits);
          } else {
            bits = (uint64_t)(int64_t)reinterpret_cast<const int16_t*>(p.val2 + d.qoff)[last];
            kind = 1;
          }
          if (kind == 0) route = LR_ERR;   // (an indexed row without ROW_ERR has legal lengths)
        }
      }
    }
    if (route == LR_ERR) {
      set_err(p.err, TSDB_E_ILLEGAL_DATA);
      kind = 0;
    }
    if (route != LR_WALK) {
      p.ts_ms[i] = kind ? ts : 0;
      p.bits[i] = kind ? bits : 0;
      p.kind[i] = (uint8_t)kind;
    }
  }
  // the walk list: one cursor add a wave (the list's order does not matter, an entry owns its slot)
  const int lane = lane_id();
  const uint64_t mw = __ballot(route == LR_WALK);
  if (mw) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&p.cnt[LC_WALKED], (unsigned long long)__popcll(mw));
    const uint32_t blo = __shfl((uint32_t)base, 0, 64), bhi = __shfl((uint32_t)(base >> 32), 0, 64);
    if (route == LR_WALK) {
      const int64_t at = (int64_t)(((uint64_t)bhi << 32) | blo) + lanes_below(mw);
      p.list[2 * at] = i;
      p.list[2 * at + 1] = row;
    }
  }
  // the route counts: a ballot a route, one LDS add a wave, one global add a block
  for (int c = 0; c < 3; c++) {
    const uint64_t m = __ballot(route == c);   // LR_NONE, LR_DIRECT, LR_COPIED = LC_NONE, LC_DIRECT, LC_COPIED
    if (m && lane == 0) atomicAdd(&h[c], (uint32_t)__popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < 3 && h[threadIdx.x]) atomicAdd(&p.cnt[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}
static_assert(LR_NONE == LC_NONE && LR_DIRECT == LC_DIRECT && LR_COPIED == LC_COPIED && LR_WALK == LC_WALKED,
              "k_last_pick counts a route in the slot of its number");

__global__ __launch_bounds__(LAST_BLOCK) void k_last_walk(LastParams p) {
  const int lane = lane_id();
  const int64_t n = (int64_t)p.cnt[LC_WALKED];
  const int64_t stride = (int64_t)gridDim.x * LAST_WAVES;
  for (int64_t e = (int64_t)blockIdx.x * LAST_WAVES + (threadIdx.x >> 6); e < n; e += stride) {
    const int64_t slot = p.list[2 * e], r = p.list[2 * e + 1];
    const RowDesc d = p.rows[r];
    const uint8_t* __restrict__ q = p.qual + d.qoff;
    const uint32_t ndp = d.ndp, qwf = d.flags & ROW_QW_MASK;
    // per lane: the best datapoint among those it has seen -- offset (ms) << 32 | position, so that
    // the maximum is the largest offset and, among equal offsets, the later position
    uint64_t best = 0;
    bool any = false;
    uint32_t b_vo = 0, b_fb = 0;
    long long vcarry = 0;
    uint32_t qcarry = 0;
    for (uint32_t i0 = 0; i0 < ndp; i0 += 64) {
      const uint32_t i = i0 + lane;
      const bool in = i < ndp;
      uint32_t qpos = 0, w = 2;
      if (qwf) {
        w = qwf;
        qpos = i * w;
      } else {
        // mixed second / millisecond qualifiers: the widths are found sequentially, every lane the same walk
        uint32_t pos = qcarry;
        for (int t = 0; t < 64 && i0 + t < ndp; t++) {
          const uint32_t ww = ((q[pos] & 0xF0) == 0xF0) ? 4 : 2;
          if (t == lane) { qpos = pos; w = ww; }
          pos += ww;
        }
        qcarry = pos;
      }
      uint32_t fb = 0, off = 0;
      if (in) off = last_qual(q + qpos, (int)w, fb);
      const int len = in ? (int)(fb & 7) + 1 : 0;
      const int incl = wave_incl_sum(len);
      const long long vo = vcarry + incl - len;
      vcarry += __shfl(incl, 63, 64);
      const uint64_t key = ((uint64_t)off << 32) | i;
      if (in && (!any || key > best)) {   // (a lane's positions ascend: an equal offset later replaces)
        best = key;
        any = true;
        b_vo = (uint32_t)vo;
        b_fb = fb;
      }
    }
    uint64_t top = any ? best : 0;
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)top, dd, 64), hi = __shfl_xor((uint32_t)(top >> 32), dd, 64);
      const uint64_t o = ((uint64_t)hi << 32) | lo;
      top = o > top ? o : top;
    }
    const uint64_t mwin = __ballot(any && best == top);   // positions are unique: one lane
    const int wl = mwin ? (int)__builtin_ctzll(mwin) : 0;
    const uint32_t w_vo = __shfl(b_vo, wl, 64), w_fb = __shfl(b_fb, wl, 64);
    if (lane == 0) {
      const int len = (int)(w_fb & 7) + 1;
      uint64_t bits = 0;
      int kind = 0;
      if (mwin && (uint64_t)w_vo + (uint64_t)len <= (uint64_t)d.vlen)
        kind = last_decode(last_be(p.val + d.voff + w_vo, len), len, (w_fb & 8) != 0, bits);
      if (kind == 0) set_err(p.err, TSDB_E_ILLEGAL_DATA);
      p.ts_ms[slot] = kind ? (int64_t)d.base * 1000 + (int64_t)(top >> 32) : 0;
      p.bits[slot] = kind ? bits : 0;
      p.kind[slot] = (uint8_t)kind;
    }
  }
}

}  // namespace

hipError_t launch_last(const LastParams& p, hipStream_t s) {
  if (p.n_sel <= 0) return hipSuccess;
  const int64_t b = (p.n_sel + LAST_BLOCK - 1) / LAST_BLOCK;
  if (b > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_last_pick, dim3((unsigned)b), dim3(LAST_BLOCK), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the list holds at most n_sel rows: a small selection launches a small grid
  const int64_t wb = std::min<int64_t>((p.n_sel + LAST_WAVES - 1) / LAST_WAVES, LAST_WALK_MAX_BLOCKS);
  hipLaunchKernelGGL(k_last_walk, dim3((unsigned)wb), dim3(LAST_BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace tsdb
