// k_put.hip -- tsdbhip_put's device side (gfx950): the merged cells of a call's touched rows, built
// at the blobs' tail (TSDB.addPointInternal / storeIntoDB, src/core/TSDB.java:1012-1262,
// read back through CompactionQueue.Compaction.compact, src/core/CompactionQueue.java:330-616, with
// the resident cell as one column older than every put, ColumnDatapointIterator's single-datapoint
// fixups included).
//
// The host has validated the points, dropped those a later point of the call shadows or beats at
// its offset, and sorted each delta row's survivors by offset: a row's puts arrive with strictly
// increasing offsets, each with the running sums of the qualifier and value bytes of the puts
// before it.  The values are encoded here.  One wave a delta row, grid-stride, three routes:
//   added   no resident row: every lane encodes its puts at their running sums.
//   tail    the resident row is not ROW_ERR / ROW_UNSORTED, has one qualifier width and a uniform
//           value length, its blobs sit 16-byte aligned, it needs no single-datapoint fixup, and the
//           first put lies strictly after its last offset (from the last qualifier, or from RegRow
//           when the row is regular and of one type, as k_last_pick's direct route).  The resident
//           ndp * QW qualifier and ndp * VL value bytes are copied in 16-byte words, the remainder
//           in bytes, without decoding; the puts are encoded behind them.
//   walked  everything else, and every resident row under option PUT_WALK: the forward pass of
//           index_row_generic / k_last_walk, 64 datapoints a step -- qualifier widths, a wave prefix
//           sum of the value lengths -- merged with the puts.  A lane finds its datapoint's place
//           among the puts by binary search; a put of the same offset wins (the value bytes are
//           compared), so the datapoint's output position is the surviving resident bytes before it
//           plus the bytes of the puts before it, and the lane also writes the puts that fall
//           between the datapoint before its own and its own.  The puts past the last datapoint
//           are written by all lanes at the end.
// The meta byte follows a row of two or more datapoints and is MS_MIXED_COMPACT when qualifier
// widths mix; the resident cell's own meta byte is never looked at.  Lane 0 writes the row's exact
// qlen / vlen into its RowDesc.  A malformed cell, an offset inside the cell that does not
// increase, and a datapoint that loses to a put with other value bytes (without the fix flag) each
// leave their smallest (delta row << 32 | ms offset) in the call's report; the host refuses.
// Cells are big-endian at unaligned addresses: assembled from byte loads and stores.
#include <algorithm>

#include "kcommon.h"

namespace tsdb {

namespace {

constexpr int PUT_BLOCK = 256;
constexpr int PUT_WAVES = PUT_BLOCK / 64;
constexpr int64_t PUT_MAX_BLOCKS = 2048;   // grid cap; grid-stride beyond

__device__ __forceinline__ uint64_t put_be(const uint8_t* __restrict__ p, int len) {
  uint64_t b = 0;
  for (int k = 0; k < len; k++) b = (b << 8) | p[k];
  return b;
}

// the offset in ms and the flag nibble of the w-byte qualifier at q (Internal.getOffsetFromQualifier)
__device__ __forceinline__ uint32_t put_qual(const uint8_t* __restrict__ q, int w, uint32_t& fb) {
  if (w == 4) {
    const uint32_t x = (uint32_t)put_be(q, 4);
    fb = x & 0xF;
    return (x & 0x0FFFFFC0u) >> 6;
  }
  const uint32_t x = (uint32_t)put_be(q, 2);
  fb = x & 0xF;
  return (x >> 4) * 1000u;
}

__device__ __forceinline__ int put_len(const PutPoint& t) { return (int)(t.meta & 0xFF); }
__device__ __forceinline__ int put_width(const PutPoint& t) { return (int)(t.meta >> 16); }

// Internal.buildQualifier and the value bytes of one put, at oq / ov
__device__ __forceinline__ void put_encode(const PutPoint& t, uint8_t* __restrict__ oq, uint8_t* __restrict__ ov) {
  const uint32_t fl = (t.meta >> 8) & 0xF;
  if (put_width(t) == 4) {
    const uint32_t x = 0xF0000000u | (t.off_ms << 6) | fl;
    oq[0] = (uint8_t)(x >> 24);
    oq[1] = (uint8_t)(x >> 16);
    oq[2] = (uint8_t)(x >> 8);
    oq[3] = (uint8_t)x;
  } else {
    const uint32_t x = ((t.off_ms / 1000u) << 4) | fl;
    oq[0] = (uint8_t)(x >> 8);
    oq[1] = (uint8_t)x;
  }
  const int len = put_len(t);
  for (int k = 0; k < len; k++) ov[k] = (uint8_t)(t.bits >> (8 * (len - 1 - k)));
}

// the first put of [0, n) whose offset is not below off
__device__ __forceinline__ int put_lower_bound(const PutPoint* __restrict__ pts, int n, uint32_t off) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pts[mid].off_ms < off) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void put_report(unsigned long long* slot, int64_t k, uint32_t off) {
  atomicMin(slot, ((unsigned long long)k << 32) | off);
}

__global__ __launch_bounds__(PUT_BLOCK) void k_put(PutParams p) {
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * PUT_WAVES;
  uint32_t n_tail = 0, n_walk = 0;
  for (int64_t k = (int64_t)blockIdx.x * PUT_WAVES + (threadIdx.x >> 6); k < p.n_rows; k += stride) {
    const PutRow R = p.prow[k];
    const RowDesc slot = p.drows[k];
    uint8_t* __restrict__ oq = p.qual + slot.qoff;
    uint8_t* __restrict__ ov = p.val + slot.voff;
    const PutPoint* __restrict__ pts = p.pts + R.p0;
    const int np = R.np;
    uint32_t rq = 0, rv = 0;       // the surviving resident bytes, qualifiers and values
    uint32_t segs = (uint32_t)np;  // datapoints of the merged row
    uint32_t widths = R.widths;    // bit 0: a 2-byte qualifier, bit 1: a 4-byte one
    int tail_from = 0;             // the puts not yet written
    bool bad = false;
    if (R.res >= 0) {
      const RowDesc d = p.rows[R.res];
      const uint8_t* __restrict__ q = p.qual + d.qoff;
      const uint8_t* __restrict__ v = p.val + d.voff;
      const uint32_t f = d.flags, ndp = d.ndp;
      const uint32_t qwf = f & ROW_QW_MASK, vl = (f & ROW_VL_MASK) >> ROW_VL_SHIFT;
      bool tail = false;
      if (f & ROW_ERR) {
        if (lane == 0) put_report(&p.rep[PR_MALFORMED], k, 0);
        bad = true;
      } else if (!p.walk_all && !(f & ROW_UNSORTED) && (qwf == 2 || qwf == 4) && vl != 0 && ndp > 0 &&
                 !(ndp == 1 && qwf == 2) && ((d.qoff | d.voff) & 15) == 0 && (uint64_t)ndp * qwf <= d.qlen &&
                 (uint64_t)ndp * vl <= d.vlen) {
        const RegRow g = p.reg[R.res];
        uint32_t last_ms, fb;
        if (g.step != 0 && (f & (ROW_ALLF | ROW_ALLI)))
          last_ms = (g.first + (ndp - 1) * g.step) * 1000u;
        else
          last_ms = put_qual(q + (uint64_t)(ndp - 1) * qwf, (int)qwf, fb);
        tail = pts[0].off_ms > last_ms;
      }
      if (tail) {
        n_tail++;
        rq = ndp * qwf;
        rv = ndp * vl;
        const uint4* __restrict__ sq = reinterpret_cast<const uint4*>(q);
        const uint4* __restrict__ sv = reinterpret_cast<const uint4*>(v);
        uint4* __restrict__ dq = reinterpret_cast<uint4*>(oq);
        uint4* __restrict__ dv = reinterpret_cast<uint4*>(ov);
        for (uint32_t w = lane; w < (rq >> 4); w += 64) dq[w] = sq[w];
        for (uint32_t w = lane; w < (rv >> 4); w += 64) dv[w] = sv[w];
        if ((uint32_t)lane < (rq & 15)) oq[(rq & ~15u) + lane] = q[(rq & ~15u) + lane];
        if ((uint32_t)lane < (rv & 15)) ov[(rv & ~15u) + lane] = v[(rv & ~15u) + lane];
        segs += ndp;
        widths |= qwf == 2 ? 1u : 2u;
      } else if (!bad) {
        n_walk++;
        // ColumnDatapointIterator's fixups of a single-datapoint column (2-byte qualifier): an 8-byte
        // float under the 4-byte flags loses its four leading zero bytes; the length bits follow the value
        int fix_len = 0, fix_skip = 0;
        if (d.qlen == 2) {
          const uint32_t q1 = q[1];
          if ((q1 & 8) && (q1 & 7) == 3 && d.vlen == 8) {
            if (v[0] | v[1] | v[2] | v[3]) bad = true;
            fix_len = 4;
            fix_skip = 4;
          } else if (d.vlen >= 1 && d.vlen <= 8) {
            fix_len = (int)d.vlen;
          } else {
            bad = true;
          }
          if (bad && lane == 0) put_report(&p.rep[PR_MALFORMED], k, 0);
        }
        long long vcarry = 0;
        uint32_t qcarry = 0;
        uint32_t prev_off = 0;
        bool have_prev = false;
        int prev_end = 0;   // the puts before and at the datapoint before this step's first
        const uint32_t n = d.qlen == 2 ? 1u : ndp;   // (a 2-byte qualifier is one datapoint whatever the index made of it)
        for (uint32_t i0 = 0; i0 < n && !bad; i0 += 64) {
          const uint32_t i = i0 + lane;
          const bool in = i < n;
          uint64_t qpos = 0;
          uint32_t w = 2;
          bool found = qwf != 0;
          if (qwf) {
            w = qwf;
            qpos = (uint64_t)i * w;
          } else {
            // mixed second / millisecond qualifiers: the widths are found sequentially, every lane the same walk
            uint32_t pos = qcarry;
            for (int t = 0; t < 64 && i0 + t < n && pos < d.qlen; t++) {
              const uint32_t ww = ((q[pos] & 0xF0) == 0xF0) ? 4 : 2;
              if (t == lane) { qpos = pos; w = ww; found = true; }
              pos += ww;
            }
            qcarry = pos;
          }
          const bool q_ok = found && qpos + w <= d.qlen;
          uint32_t fb = 0, off = 0;
          if (in && q_ok) off = put_qual(q + qpos, (int)w, fb);
          if (fix_len) fb = (fb & 8) | (uint32_t)(fix_len - 1);
          const int len = in && q_ok ? (int)(fb & 7) + 1 : 0;
          const int incl = wave_incl_sum(len);
          const long long vo = vcarry + incl - len + fix_skip;
          vcarry += __shfl(incl, 63, 64);
          const bool v_ok = (uint64_t)vo + (uint64_t)len <= (uint64_t)d.vlen;
          const uint64_t m_mal = __ballot(in && !(q_ok && v_ok));
          const uint32_t up_off = __shfl_up(off, 1, 64);
          const bool has_before = lane > 0 || have_prev;
          const uint32_t before = lane > 0 ? up_off : prev_off;
          const uint64_t m_uns = __ballot(in && has_before && off <= before);
          if (m_mal | m_uns) {   // (uniform) nothing of the row is written from here on
            if (in && !(q_ok && v_ok)) put_report(&p.rep[PR_MALFORMED], k, 0);
            else if (in && has_before && off <= before) put_report(&p.rep[PR_UNSORTED], k, off);
            bad = true;
            break;
          }
          const int a = in ? put_lower_bound(pts, np, off) : np;
          const bool eq = in && a < np && pts[a].off_ms == off;
          const bool surv = in && !eq;
          if (eq) {   // the put wins; Compaction compares the discarded value's bytes with the kept one's
            const PutPoint t = pts[a];
            const int tl = put_len(t);
            const uint64_t mask = tl == 8 ? ~0ull : ((1ull << (8 * tl)) - 1);
            if (!p.fix && (tl != len || (t.bits & mask) != put_be(v + vo, len))) put_report(&p.rep[PR_CONFLICT], k, off);
          }
          const int sq_ = surv ? (int)w : 0, sv_ = surv ? len : 0;
          const int iq = wave_incl_sum(sq_), iv = wave_incl_sum(sv_);
          const uint32_t eq_ = rq + (uint32_t)(iq - sq_), ev_ = rv + (uint32_t)(iv - sv_);
          const int end = a + (eq ? 1 : 0);
          const int up_end = __shfl_up(end, 1, 64);
          const int g0 = lane > 0 ? up_end : prev_end;
          if (in) {
            // the puts between the datapoint before and this one, and the one that takes this one's place
            for (int j = g0; j < end; j++) {
              const PutPoint t = pts[j];
              put_encode(t, oq + eq_ + t.qpre, ov + ev_ + t.vpre);
            }
            if (surv) {
              const uint32_t pq = a < np ? pts[a].qpre : R.qsum, pv = a < np ? pts[a].vpre : R.vsum;
              uint8_t* __restrict__ wq = oq + eq_ + pq;
              uint8_t* __restrict__ wv = ov + ev_ + pv;
              for (uint32_t b = 0; b < w; b++) wq[b] = q[qpos + b];
              if (fix_len) wq[w - 1] = (uint8_t)((q[qpos + w - 1] & 0xF0) | fb);
              for (int b = 0; b < len; b++) wv[b] = v[vo + b];
            }
          }
          const int last_lane = (int)min(63u, n - 1 - i0);
          rq += (uint32_t)__shfl(iq, 63, 64);
          rv += (uint32_t)__shfl(iv, 63, 64);
          prev_off = __shfl(off, last_lane, 64);
          prev_end = __shfl(end, last_lane, 64);
          have_prev = true;
          segs += (uint32_t)__popcll(__ballot(surv));
          if (__ballot(surv && w == 2)) widths |= 1u;
          if (__ballot(surv && w == 4)) widths |= 2u;
        }
        tail_from = prev_end;
      }
    }
    if (bad) continue;
    for (int j = tail_from + lane; j < np; j += 64) {
      const PutPoint t = pts[j];
      put_encode(t, oq + rq + t.qpre, ov + rv + t.vpre);
    }
    if (lane == 0) {
      const uint32_t vsum = rv + R.vsum;
      if (segs > 1) ov[vsum] = widths == 3u ? 1 : 0;   // Const.MS_MIXED_COMPACT
      p.drows[k].qlen = rq + R.qsum;
      p.drows[k].vlen = vsum + (segs > 1 ? 1u : 0u);
    }
  }
  if (lane == 0) {
    if (n_tail) atomicAdd(&p.rep[PR_TAIL], (unsigned long long)n_tail);
    if (n_walk) atomicAdd(&p.rep[PR_WALKED], (unsigned long long)n_walk);
  }
}

}  // namespace

hipError_t launch_put(const PutParams& p, hipStream_t s) {
  if (p.n_rows <= 0) return hipSuccess;
  const int64_t b = std::min<int64_t>((p.n_rows + PUT_WAVES - 1) / PUT_WAVES, PUT_MAX_BLOCKS);
  hipLaunchKernelGGL(k_put, dim3((unsigned)b), dim3(PUT_BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // namespace tsdb
