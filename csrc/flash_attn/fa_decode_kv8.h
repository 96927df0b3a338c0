// Device code shared by the FP8 KV cache kernels (fa_decode_kv8.hip, fa_decode_chunk_kv8.hip) on top
// of fa_decode_common.h: the one row quantizer every kernel that writes cache rows goes through, and
// the attention body of both attention kernels. gfx950, wave64.
//
// Format: a cached row is D OCP e4m3 bytes plus one fp32 scale, row = bytes * scale.
//
// Attention geometry: G = D/16 lanes own a row (G = 8 for D = 80, five of them active), 16 elements
// per lane, one 16-B load. The 16-bit kernels' D/8 lanes with an 8-B load were measured first: the
// arithmetic of a row and lane (conversion, DPP sum, exp2, mask, addresses) does not shrink with the
// bytes, so per byte it doubled and the kernel ran at 0.46-0.60 of the HBM rate where the 16-bit one
// reaches 0.9, slower than it at d 80 (profiles/decode_kv8.md). With 16 elements per lane a row costs
// half the lanes: the per-row work is shared by twice the bytes and the DPP sum is one step shorter.
// The products run as packed fp32 (v_pk_fma_f32) on the pairs v_cvt_pk_f32_fp8 delivers.
#pragma once

#include "fa_decode_common.h"

namespace cs336 {
namespace {

constexpr float kFp8Max = 448.f;  // largest finite e4m3 value

typedef float kv8_f2 __attribute__((ext_vector_type(2)));

template <int CTRL>
__device__ __forceinline__ float kv8_dpp_max(float v) {
  return fmaxf(v, dpp_f32<CTRL>(v));
}

// max over the G lanes of a row group (group_sum's DPP pattern); every lane gets it
template <int G>
__device__ __forceinline__ float group_max(float v) {
  v = kv8_dpp_max<0xB1>(v);
  v = kv8_dpp_max<0x4E>(v);
  if constexpr (G >= 8) v = kv8_dpp_max<0x141>(v);
  if constexpr (G >= 16) v = kv8_dpp_max<0x140>(v);
  return v;
}

// The row quantizer, on the 16-bit kernels' geometry (decode_group(D) lanes, 8 fp32 values per lane).
// Every lane of a group calls it with its 8 values of one row (`active` false for the idle lanes of
// a D = 80 group, whose values do not count and whose bytes are not stored); returns the lane's 8
// bytes and, in every lane, the row's scale. The quotient is clamped before the conversion: e4m3
// has no inf, and a quotient a hair above 448 would become the NaN byte. Division, not a reciprocal
// multiply: the eager reference divides, and the row's largest element has to land on +-448.
template <int G>
__device__ __forceinline__ uint2 kv8_quantize_row(const Chunk8& x, bool active, float& scale) {
  float amax = 0.f;
  if (active) {
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x.f[i]));
  }
  amax = group_max<G>(amax);
  scale = amax > 0.f ? amax / kFp8Max : 1.f;
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x.f[i] / scale, -kFp8Max), kFp8Max);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);  // round to nearest even
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

// ---- attention ----

// lanes per row (16 elements each)
__host__ __device__ constexpr int kv8_group(int D) { return D <= 32 ? 2 : (D <= 64 ? 4 : 8); }
// Query tiles: 1 and 4. A lane keeps 34 registers per query (16 scaled query elements, 16 output
// columns, max and sum), so the 16-bit kernel's 8-query tile does not fit; n > 4 runs ceil(n / 4)
// query tiles, each reading the (half-size) rows once.
__host__ __device__ constexpr int kv8_chunk_qt(int n) { return n <= 1 ? 1 : 4; }
// rows per lane group and tile: the 16-bit kernels' 4 rows of 16 B, so two tiles in flight hold the
// same bytes per lane; the 4-query tile halves it to fit its per-query state
__host__ __device__ constexpr int kv8_unroll(int qt) { return qt >= 4 ? 2 : 4; }
__host__ __device__ constexpr int kv8_tile(int D, int qt) { return (kDecodeThreads / kv8_group(D)) * kv8_unroll(qt); }

// sum over the G lanes of a row group; every lane of the group gets the total
template <int G>
__device__ __forceinline__ float kv8_group_sum(float v) {
  v += dpp_f32<0xB1>(v);                         // quad_perm [1,0,3,2]
  if constexpr (G >= 4) v += dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]
  if constexpr (G >= 8) v += dpp_f32<0x141>(v);  // row_half_mirror
  return v;
}

// 16 consecutive elements as fp32 pairs
struct Pairs16 {
  kv8_f2 p[8];
};

// 16 e4m3 bytes -> fp32, eight v_cvt_pk_f32_fp8; exact (every e4m3 value is an fp32 value)
__device__ __forceinline__ Pairs16 kv8_unpack(const uint4& r) {
  Pairs16 c;
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c.p[2 * i] = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    c.p[2 * i + 1] = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
  }
  return c;
}

// One key tile in registers: rows u * NG + gi (u < U) of the tile for lane group gi, as loaded.
template <int U>
struct Kv8Tile {
  uint4 k[U], v[U];
  float ks[U], vs[U];
  int last;  // (uniform) rows 0 .. last of the tile are valid; -1: none
};

// The walk of one workgroup over the rows of one (batch, head): uniform plane bases plus 32-bit lane
// offsets, so the address arithmetic of a row is a min, a 24-bit multiply-add per plane and a shift
// (the 16-bit kernels select between 64-bit pointers per load; with four loads per row that was a
// third of the loop). The masked-slot rule as a clamp: a row beyond the tile's last valid one reads
// that one (a tile wholly beyond `end` reads row end - 1), so the loads stay unconditional, the loop
// body one basic block, and nothing at or beyond `end` is touched in any of the four planes. Row
// strides are below 2^22 bytes (the binding checks), so a tile's offsets fit 32 bits.
template <int U, int NG>
struct Kv8Rows {
  const uint8_t* k;  // (uniform) row 0, column 0 of the (b, h) planes
  const uint8_t* v;
  const float* ks;
  const float* vs;
  uint32_t k_sn, v_sn;  // (uniform) row strides in bytes
  uint32_t col;         // this lane's first column
  int gi;               // this lane's group

  __device__ __forceinline__ void issue(Kv8Tile<U>& t, int64_t j0, int64_t end) const {
    constexpr int KT = NG * U;
    const int64_t left = end - 1 - j0;
    t.last = left < 0 ? -1 : (left < KT - 1 ? (int)left : KT - 1);
    const int64_t jb = left < 0 ? end - 1 : j0;  // the first row this tile's loads may touch
    const uint32_t e = t.last < 0 ? 0u : (uint32_t)t.last;
    const uint8_t* kt = k + jb * k_sn;
    const uint8_t* vt = v + jb * v_sn;
    const uint8_t* kst = (const uint8_t*)(ks + jb);
    const uint8_t* vst = (const uint8_t*)(vs + jb);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t r = (uint32_t)(gi + u * NG);
      const uint32_t rel = r < e ? r : e;
      t.k[u] = *reinterpret_cast<const uint4*>(kt + ((uint32_t)__umul24(rel, k_sn) + col));
      t.v[u] = *reinterpret_cast<const uint4*>(vt + ((uint32_t)__umul24(rel, v_sn) + col));
      t.ks[u] = *reinterpret_cast<const float*>(kst + rel * 4u);
      t.vs[u] = *reinterpret_cast<const float*>(vst + rel * 4u);
    }
  }
  // whether row u of the tile (for this lane's group) is one of [begin, end)
  __device__ __forceinline__ bool valid(const Kv8Tile<U>& t, int u) const { return gi + u * NG <= t.last; }
};

// running softmax state of one lane for one query: max and sum of its group's rows (exp2 domain), 16
// output columns
struct Online16 {
  float m, l;
  kv8_f2 acc[8];
};

// The body of fa_decode_kv8_kernel (QT = 1, called with n = 1: q (B, 1, H, D) is (B, H, D)) and
// fa_decode_chunk_kv8_kernel (QT = 4): fa_decode_chunk_kernel's algorithm on this format. A workgroup
// owns QT consecutive queries of one (b, h, split); split over keys with fp32 partials; two register
// buffers with the next tile's loads issued before this tile's arithmetic, in one basic block;
// per-query masks; fixed-order combines, no atomics. k_scale[row] multiplies the group-summed dot
// product once per query and v_scale[row] is folded into the probability (acc += (p * vs) * v, l += p
// unscaled).
template <typename T, int D, int QT>
__device__ __forceinline__ void kv8_attention(const DecodeChunkParams& p, const Kv8Scales& sc, const int qtiles) {
  typedef typename Elem<T>::storage S;
  constexpr int G = kv8_group(D);
  constexpr int NG = kDecodeThreads / G;  // lane groups (rows per load step) of the workgroup
  constexpr int U = kv8_unroll(QT);
  constexpr int KT = NG * U;  // keys per tile
  constexpr int C = D / 16;   // active lanes of a group

  __shared__ float sm_m[kDecodeWaves][QT];
  __shared__ float sm_l[kDecodeWaves][QT];
  __shared__ float sm_acc[kDecodeWaves][QT][D];

  const int tid = threadIdx.x;
  const int split = blockIdx.x % p.splits;
  const int rest = blockIdx.x / p.splits;
  const int qt = rest % qtiles;
  const int row = rest / qtiles;  // b * H + h
  const int b = row / p.H, h = row - b * p.H;
  const int gi = tid / G, c = tid % G;
  const bool active = c < C;
  const int i0 = qt * QT;  // first query of the tile

  // per-query key bounds; a query at or beyond n (the tail of the last tile) has none
  const int64_t kvl = p.kv_len[b];
  int lim[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    int64_t bound = kvl - (int64_t)(p.n - 1 - (i0 + qi));
    bound = bound < 0 ? 0 : (bound > p.max_len ? p.max_len : bound);
    lim[qi] = i0 + qi < p.n ? (int)bound : 0;
  }
  // the tile's range is its last real query's (the bounds do not decrease with i)
  int n = 0;
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) n = lim[qi] > n ? lim[qi] : n;
  const int tiles = (n + KT - 1) / KT;
  const int per = (tiles + p.splits - 1) / p.splits;
  const int64_t begin = (int64_t)split * per * KT;
  const int64_t end = begin + (int64_t)per * KT < n ? begin + (int64_t)per * KT : n;

  // (the idle lanes of a D = 80 group load column 0 again; their q is 0 and their acc is not stored)
  Kv8Rows<U, NG> kvr;
  kvr.k = (const uint8_t*)p.k + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
  kvr.v = (const uint8_t*)p.v + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh;
  kvr.ks = sc.k + (int64_t)b * sc.k_sb + (int64_t)h * sc.k_sh;
  kvr.vs = sc.v + (int64_t)b * sc.v_sb + (int64_t)h * sc.v_sh;
  kvr.k_sn = (uint32_t)p.k_sn;
  kvr.v_sn = (uint32_t)p.v_sn;
  kvr.col = active ? 16 * c : 0;
  kvr.gi = gi;

  // this lane's 16 elements of every query, with scale * log2(e) folded in (exp2-domain scores)
  kv8_f2 q[QT][8];
  Online16 st[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
#pragma unroll
    for (int i = 0; i < 8; ++i) q[qi][i] = kv8_f2{0.f, 0.f};
    if (active && i0 + qi < p.n) {
      const S* qp = (const S*)p.q + (((int64_t)b * p.n + i0 + qi) * p.H + h) * D + 16 * c;
      const Chunk8 lo = load8<T>(qp), hi = load8<T>(qp + 8);
      const float f = p.scale * kLog2e;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        q[qi][i] = kv8_f2{lo.f[2 * i] * f, lo.f[2 * i + 1] * f};
        q[qi][4 + i] = kv8_f2{hi.f[2 * i] * f, hi.f[2 * i + 1] * f};
      }
    }
    st[qi].m = -INFINITY;
    st[qi].l = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) st[qi].acc[i] = kv8_f2{0.f, 0.f};
  }

  typedef Kv8Tile<U> Tile;
  auto compute = [&](const Tile& t, int64_t j0) __attribute__((always_inline)) {
    float s[QT][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const Pairs16 kk = kv8_unpack(t.k[u]);
      const bool ok = kvr.valid(t, u);
      const int jr = ok ? (int)(j0 + u * NG + gi) : 0x7fffffff;  // (end <= max_len < 2^31)
#pragma unroll
      for (int qi = 0; qi < QT; ++qi) {
        kv8_f2 d2 = q[qi][0] * kk.p[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) d2 = __builtin_elementwise_fma(q[qi][i], kk.p[i], d2);
        const float d = kv8_group_sum<G>(d2.x + d2.y) * t.ks[u];
        if constexpr (QT == 1) {
          s[qi][u] = ok ? d : -INFINITY;
        } else {
          // per-query mask (the split's end and the query's bound) as a bit select on the sign of
          // jr - lim: QT * U compare masks in SGPR pairs spill the SGPR file (fa_decode_chunk_kernel)
          int diff = jr - lim[qi];  // < 0 iff jr < lim (both >= 0)
          asm("" : "+v"(diff));     // (opaque, or the compiler turns the bit select back into compare masks)
          const uint32_t keep = (uint32_t)(diff >> 31);
          s[qi][u] = __uint_as_float((__float_as_uint(d) & keep) | (0xff800000u & ~keep));
        }
      }
    }
    float msub[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
      float tmax = st[qi].m;
#pragma unroll
      for (int u = 0; u < U; ++u) tmax = fmaxf(tmax, s[qi][u]);
      // a group that has seen no valid key yet keeps m = -inf; subtract 0 there so nothing is inf - inf
      msub[qi] = tmax == -INFINITY ? 0.f : tmax;
      const float alpha = __builtin_amdgcn_exp2f(st[qi].m - msub[qi]);
      st[qi].m = tmax;
      st[qi].l *= alpha;
#pragma unroll
      for (int i = 0; i < 8; ++i) st[qi].acc[i] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const Pairs16 vv = kv8_unpack(t.v[u]);
#pragma unroll
      for (int qi = 0; qi < QT; ++qi) {
        const float pu = __builtin_amdgcn_exp2f(s[qi][u] - msub[qi]);
        st[qi].l += pu;
        const float pv = pu * t.vs[u];
        const kv8_f2 pv2 = kv8_f2{pv, pv};
#pragma unroll
        for (int i = 0; i < 8; ++i) st[qi].acc[i] = __builtin_elementwise_fma(pv2, vv.p[i], st[qi].acc[i]);
      }
    }
  };

  if (begin < end) {  // (uniform over the workgroup)
    // Two tiles per iteration in two register buffers, with no exit between them: the body is one
    // basic block in which each tile's loads are issued one tile ahead of their use (fa_decode_kernel).
    // A tile wholly beyond `end` computes a no-op: every score is -inf, every weight 0.
    // The scheduling barriers keep each tile's loads where they are written: left alone, the
    // scheduler sinks them to their uses to save registers (load, wait, load, wait), which serializes
    // the loop on the memory latency -- measured at 4 us per 128-row tile, d 80.
    Tile ta, tb;
    kvr.issue(ta, begin, end);
    for (int64_t j0 = begin; j0 < end; j0 += 2 * KT) {
      kvr.issue(tb, j0 + KT, end);
      __builtin_amdgcn_sched_barrier(0);
      compute(ta, j0);
      __builtin_amdgcn_sched_barrier(0);
      kvr.issue(ta, j0 + 2 * KT, end);
      __builtin_amdgcn_sched_barrier(0);
      compute(tb, j0 + KT);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // combine the lane groups of each wave (butterfly over the lanes that hold the same columns), then
  // the 4 waves through LDS, in wave order
  const int wave = tid / kWave, lane = tid % kWave;
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    Online16& o = st[qi];
#pragma unroll
    for (int off = G; off < kWave; off *= 2) {
      const float m2 = __shfl_xor(o.m, off, kWave), l2 = __shfl_xor(o.l, off, kWave);
      const float M = fmaxf(o.m, m2);
      const float sub = M == -INFINITY ? 0.f : M;  // both empty: nothing is inf - inf
      const float wa = __builtin_amdgcn_exp2f(o.m - sub), wb = __builtin_amdgcn_exp2f(m2 - sub);
      o.l = o.l * wa + l2 * wb;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o.acc[i].x = o.acc[i].x * wa + __shfl_xor(o.acc[i].x, off, kWave) * wb;
        o.acc[i].y = o.acc[i].y * wa + __shfl_xor(o.acc[i].y, off, kWave) * wb;
      }
      o.m = M;
    }
    if (lane == 0) {
      sm_m[wave][qi] = o.m;
      sm_l[wave][qi] = o.l;
    }
    if (lane < G && active) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        sm_acc[wave][qi][16 * c + 2 * i] = o.acc[i].x;
        sm_acc[wave][qi][16 * c + 2 * i + 1] = o.acc[i].y;
      }
    }
  }
  __syncthreads();
  const int64_t orows = (int64_t)p.B * p.n * p.H;
  for (int idx = tid; idx < QT * D; idx += kDecodeThreads) {
    const int qi = idx / D, cc = idx - qi * D;
    if (i0 + qi >= p.n) break;  // (qi does not decrease with idx)
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < kDecodeWaves; ++w) M = fmaxf(M, sm_m[w][qi]);
    float L = 0.f, o = 0.f;
    if (M != -INFINITY) {
#pragma unroll
      for (int w = 0; w < kDecodeWaves; ++w) {
        const float wt = __builtin_amdgcn_exp2f(sm_m[w][qi] - M);  // 0 for a wave with m = -inf
        L = fmaf(sm_l[w][qi], wt, L);
        o = fmaf(sm_acc[w][qi][cc], wt, o);
      }
      o = o / L;  // L >= 1: the row holding the maximum contributes exp2(0)
    }
    const float lse = M == -INFINITY ? -INFINITY : (M + __builtin_amdgcn_logf(L)) * kLn2;
    const int64_t orow = ((int64_t)b * p.n + i0 + qi) * p.H + h;
    if (p.splits == 1) {
      ((S*)p.o)[orow * D + cc] = Elem<T>::from_f(o);
      if (cc == 0) p.lse[orow] = lse;
    } else {
      const int64_t pr = (int64_t)split * orows + orow;
      p.opart[pr * D + cc] = o;
      if (cc == 0) p.lpart[pr] = lse;
    }
  }
}

}  // namespace
}  // namespace cs336
