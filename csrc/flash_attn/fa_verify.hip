// Verify attention for MI355X (gfx950 / CDNA4): up to 16 new query rows per (batch, head) against a KV
// cache, streaming K / V once at MFMA rate, on the dense and on the paged cache layout. The small-n
// sibling of fa_extend.hip (128-row query tile, everything through LDS) and the MFMA sibling of
// fa_decode_chunk.hip (VALU, 8-row tile) for the verify step of speculative decoding.
// cs336-build: no-packed-f32 (the rescale and merge loops stay single v_mul_f32 / v_fma_f32)
//
// Semantics are fa_decode_chunk's: q (B, n, H, D) contiguous; kv_len[b] counts the keys AFTER the
// chunk's own rows were appended; query i sees keys [0, kv_len[b] - (n - 1 - i)), clamped to
// [0, max_len]; a bound <= 0 gives o = 0, lse = -inf. Outputs o (B, n, H, D) in q's dtype and the
// natural-log lse (B, n, H) fp32. bf16 / fp16, D in {32, 64, 80, 128}, any n >= 1 (ceil(n / 16) query
// tiles, each streaming its own key range: the kernel is built for n <= 16).
//
// Design: the skinny-M GEMM's operand scheme (gemm_skinny.h) with the helpers of fa_common.h.
//   * Work split: 1-D grid of (query tile of 16, batch*head, key split), key splits of one tile
//     adjacent, the last query tiles first. A workgroup is 4 waves. Inside the workgroup's range the
//     waves take alternating 32-key sub-tiles (wave w: sub-tiles w, w + 4, ... of the range, i.e. one
//     of each 128 keys), each with its own online-softmax state (m, l, O); the four states are merged
//     once at the end through LDS in wave order. The main loop has no workgroup barrier.
//   * S^T = K Q^T on v_mfma_f32_16x16x32_{bf16,f16}: K is the A operand, lane l holding 16 B of key
//     row l & 15 at d = 32 ks + 8 (l >> 4), loaded from global memory straight into VGPRs (the
//     row-major cache is already that layout: no LDS for K). Q is the B operand, resident (D/32 x 4
//     VGPRs). The accumulator holds keys 4 (l >> 4) .. +3 of query l & 15: the query is on the lane, its
//     running max is combined over the four lane groups by one v_permlane16_swap and one
//     v_permlane32_swap per sub-tile, and the row sum stays lane-partial until the end.
//     scale * log2(e) is applied in the exp2 FMA in fp32. d 80 is 2.5 k-steps: lane groups 2 and 3
//     of the third step hold zeros and load nothing.
//   * O^T = V^T P^T: the two 16-key accumulators of a sub-tile are packed straight into the B operand,
//     k index 8g + r = key 4g + r of the first (r < 4) and key 16 + 4g + r - 4 of the second; V^T (the
//     A operand) is read in the same key order with two ds_read_b64_tr_b16 per 16 d. Each wave stages
//     its own 32 V rows global -> registers -> a wave-private swizzled LDS image. K has two register
//     sets and V one (free again once written to the image): V of sub-tile j + 1 and then K of j + 2
//     are issued around sub-tile j's MFMAs, so a wave waits for its rows with half a sub-tile still
//     in flight. LDS operations of one wave execute in order, so a wavefront-scope fence (no
//     instruction) between the writes and the transposed reads is all the ordering the image needs. O^T is D/16 accumulators of
//     4 fp32 (d 80: 5, no pad; its LDS rows are 192 B because the swizzle is defined for that length).
//   * Rows that must not be seen: addresses of rows at or beyond the tile's key range are clamped to
//     its last row, so such a row is never loaded; in the one sub-tile that straddles the range their V
//     staging is zeroed (P = 0 times a NaN would be NaN under MFMA) and their scores are replaced by a
//     select. Rows in a query's future inside the range are this chunk's rows, finite, and get weight 0
//     by the per-query mask; only sub-tiles that straddle some query's bound pay the mask. Queries at
//     and beyond n have a zero Q fragment and are not stored.
//   * Split over keys: split s of S takes sub-tiles [T*s/S, T*(s+1)/S) of the range's T sub-tiles, a
//     function of the tile's bound and S alone: any page placement, and the dense and paged kernels on
//     the same rows, give the same bits. S == 1 writes o / lse; otherwise each split writes normalised
//     fp32 partials in fa_decode_chunk's layout (an empty split: lse = -inf) and fa_decode_chunk_merge
//     combines them. No atomics, no scratch.
//   * Row address policy (template parameter): dense strides, or pool + clamp(table[b, j >> lg], 0,
//     num_pages - 1) * s_page + h * s_h + (j & (P - 1)) * s_n in 64-bit element offsets. Pages hold at
//     least 16 rows and a sub-tile starts at a multiple of 32, so a sub-tile touches two table entries
//     (rows 0-15, rows 16-31): both are wave-uniform, requested for the NEXT sub-tile before this
//     sub-tile's row loads are issued, with the row index clamped to the range's last row (the table is
//     never read beyond entry (kv_len[b] - 1) >> lg).
//   * Deviations from the plan. One V image per wave, not two: with in-order LDS and no workgroup
//     barrier a second image buys a single wave nothing, and two full K + V register sets spilled at
//     d 128 (256 VGPRs + scratch), so V keeps one set. Out-of-range rows are not branched around:
//     clamped addresses plus the zeroing in the straddling sub-tile give the same image.
#include "fa_verify.h"

#include <algorithm>

namespace cs336 {
namespace fa {

// (Mma32, xrow_max / xrow_sum and the row address policies VerifyRows<P>: fa_verify.h)
template <typename T, int D, typename P>
__global__ __launch_bounds__(256, 2) void fa_verify_kernel(const P p, const int nqt) {
  typedef typename Elem<T>::storage S;
  typedef VerifyRows<P> Rows;
  static_assert(sizeof(S) == 2, "fa_verify: 16-bit types only");
  constexpr int DP = PadD<D>::value;  // width of S^T's k loop and of an LDS row (80 -> 96)
  constexpr int RB = DP * 2;          // bytes per LDS row of V
  constexpr int CREAL = D / 8;        // 16-byte chunks of a cached row
  constexpr int NKS = DP / 32;        // k-steps of S^T
  constexpr int NDT = D / 16;         // 16-row blocks of O^T
  constexpr int BQ = 16, BK = 32;     // queries per workgroup, keys per sub-tile
  constexpr int LPT = BK * CREAL / 64;  // 16-B V staging loads per lane per sub-tile
  static_assert(BK * CREAL % 64 == 0, "staging rounds must be whole");
  constexpr int VBUF = BK * RB;  // one V image
  static_assert(NDT * 1024 <= VBUF, "a wave's O state must fit its V image");

  __shared__ __attribute__((aligned(1024))) char smem[4 * VBUF];
  __shared__ float sm_m[4][BQ], sm_l[4][BQ];

  const int lane = threadIdx.x & 63, wave = wave_id();
  const int r = lane & 15, g = lane >> 4;

  // block -> (query tile, batch*head, split): splits adjacent, last query tiles first
  const int nsplit = p.splits, sp = (int)(blockIdx.x % (unsigned)nsplit);
  const int rest = (int)(blockIdx.x / (unsigned)nsplit);
  const int nbh = p.B * p.H;
  const int qb = nqt - 1 - rest / nbh, bh = rest % nbh;
  const int b = bh / p.H, h = bh % p.H;
  const int q0 = qb * BQ;

  // ---- key bounds: of this lane's query, of the tile (its last real query) and its first query ----
  const int64_t kvl = p.kv_len[b];
  auto bound = [&](int i) {  // keys query i sees (0 <= i < n)
    const int64_t v = kvl - (int64_t)(p.n - 1 - i);
    return (int)(v < 0 ? 0 : (v > p.max_len ? p.max_len : v));
  };
  const int nkeys = bound(min(q0 + BQ, p.n) - 1);
  const int wmin = bound(q0);
  const int qrow = q0 + r;
  const bool valid_q = qrow < p.n;
  const int lim_q = valid_q ? bound(qrow) : 0;

  const S* Kg = (const S*)p.k;
  const S* Vg = (const S*)p.v;
  const Rows rows(p, b, h);

  // ---- Q fragments (B operand), resident: query r, d = 32 ks + 8 g .. +7 -------------------------
  const int64_t orow = ((int64_t)b * p.n + qrow) * p.H + h;  // row of q, o and lse
  uint4 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int e = 32 * ks + 8 * g;
    qf[ks] = (valid_q && e < D) ? *reinterpret_cast<const uint4*>((const S*)p.q + orow * D + e) : make_uint4(0, 0, 0, 0);
  }

  // this workgroup's sub-tiles [T0, T1) of the range; this wave's are T0 + wave + 4 j, j < cnt
  const int NT = (nkeys + BK - 1) / BK;
  const int T0 = (int)((int64_t)NT * sp / nsplit), T1 = (int)((int64_t)NT * (sp + 1) / nsplit);
  const int mine = T1 - T0 - wave;
  const int cnt = mine > 0 ? (mine + 3) >> 2 : 0;
  const int last_key = nkeys - 1;

  // K has two register sets (sub-tile j + 1's, and later j + 2's, loads are in flight under sub-tile
  // j's MFMAs), V one: it is free again once it is written to the wave's image. K and V are two load
  // streams, each one sub-tile per step and each with the table entries of its next sub-tile
  // (rows 0-15 / 16-31) requested a step ahead.
  struct KSet {
    uint4 k[2][NKS];
  };
  struct Pages {
    int p0, p1;
  };
  auto fetch = [&](int j) {
    const int key0 = (T0 + wave + 4 * j) * BK;
    Pages g2;
    g2.p0 = Rows::kPaged ? rows.page(min(key0, last_key)) : 0;
    g2.p1 = Rows::kPaged ? rows.page(min(key0 + 16, last_key)) : 0;
    return g2;
  };
  Pages pgk = {0, 0}, pgv = {0, 0};
  auto kload = [&](KSet& f, int j) __attribute__((always_inline)) {
    const int key0 = (T0 + wave + 4 * j) * BK;
    const Pages cur = pgk;
    if (Rows::kPaged) pgk = fetch(j + 1);  // in flight under this sub-tile's row loads
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = min(key0 + 16 * t + r, last_key);
      const S* src = Kg + rows.k(key, t ? cur.p1 : cur.p0) + 8 * g;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        if (32 * ks + 32 <= D || 32 * ks + 8 * g < D)
          f.k[t][ks] = *reinterpret_cast<const uint4*>(src + 32 * ks);
        else
          f.k[t][ks] = make_uint4(0, 0, 0, 0);
      }
    }
  };
  uint4 vst[LPT];
  auto vload = [&](int j) __attribute__((always_inline)) {
    const int key0 = (T0 + wave + 4 * j) * BK;
    const Pages cur = pgv;
    if (Rows::kPaged) pgv = fetch(j + 1);
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = lane + 64 * i;
      const int rr = c / CREAL, ch = c % CREAL;
      const int key = min(key0 + rr, last_key);
      vst[i] = *reinterpret_cast<const uint4*>(Vg + rows.v(key, rr >= 16 ? cur.p1 : cur.p0) + ch * 8);
    }
  };

  float m = kNegBig, l = 0.f;
  f32x4 o[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float c2 = p.scale * kLog2e;

  // transposed-read offsets in a V image: 16-lane group g reads rows 4g .. 4g+3 (and + 16), lane
  // r gets column r of the 16-wide d block: the key order of the packed P operand
  uint32_t tra[NDT], trb[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    const int ra = 4 * g + (r >> 2), chunk = 2 * dt + ((r & 3) >> 1), within = (r & 1) * 8;
    tra[dt] = (uint32_t)(lds_off<RB>(ra, chunk) + within);
    trb[dt] = (uint32_t)(lds_off<RB>(ra + 16, chunk) + within);
  }

  char* const Vs = smem + wave * VBUF;  // this wave's image

  auto tile = [&](KSet& f, int j) __attribute__((always_inline)) {
    const int key0 = (T0 + wave + 4 * j) * BK;
    // ---- V: registers -> this wave's image (rows beyond the range: zeros) ----
    if (key0 + BK > nkeys) {  // (wave-uniform) the range's last, partial sub-tile
#pragma unroll
      for (int i = 0; i < LPT; ++i)
        if (key0 + (lane + 64 * i) / CREAL >= nkeys) vst[i] = make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = lane + 64 * i;
      *reinterpret_cast<uint4*>(Vs + lds_off<RB>(c / CREAL, c % CREAL)) = vst[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    vload(j + 1);  // (the staging registers are free again)
    // ---- S^T = K Q^T: s[t][i] is key key0 + 16 t + 4 g + i of query r ----
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) s[t] = Mma32<T>::mma(as_frag<T>(f.k[t][ks]), as_frag<T>(qf[ks]), s[t]);
    }
    kload(f, j + 2);  // (this set's MFMAs are issued)
    if (key0 + BK > wmin) {  // (wave-uniform) some query's bound falls inside this sub-tile
      const int lim = lim_q - key0 - 4 * g;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (16 * t + i >= lim) s[t][i] = -INFINITY;
    }
    // ---- online softmax (query on the lane), deferred rescale ----
    float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])),
                     fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
    mx = xhalf_max(xrow_max(mx));
    const float mt = mx * c2;
    if (__ballot(mt > m + kRescaleThr) != 0) {  // wave-uniform
      const float m_new = fmaxf(m, mt);
      const float alpha = fexp2(m - m_new);
      l *= alpha;
      m = m_new;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[dt][i] *= alpha;
    }
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = fexp2(fmaf(s[t][i], c2, -m));  // (a masked score: exp2(-inf) = 0)
        s[t][i] = pv;
        rs += pv;
      }
    l += rs;
    // ---- O^T += V^T P^T ----
    const typename Mma16<T>::frag pf = Mma16<T>::pack(s[0][0], s[0][1], s[0][2], s[0][3], s[1][0], s[1][1], s[1][2], s[1][3]);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = Mma32<T>::mma(lds_tr_read<T>(Vs, tra[dt], trb[dt]), pf, o[dt]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // this image's reads stay before its next writes
  };

  // V(j + 1) is issued before K(j + 2), so sub-tile j + 1 waits for its own rows with K(j + 2) in flight.
  // The loads past the wave's last sub-tile are issued too (a branch around them would make every wait
  // in the loop a full drain): their rows are clamped to the range's last row and nobody reads them.
  KSet ka, kb;
  if (cnt > 0) {
    pgk = pgv = fetch(0);
    kload(ka, 0);
    vload(0);
    kload(kb, 1);
  }
  int j = 0;
  for (; j + 2 <= cnt; j += 2) {
    tile(ka, j);
    tile(kb, j + 1);
  }
  if (j < cnt) tile(ka, j);

  // ---- merge the four waves' states in wave order ----
  l = xhalf_sum(xrow_sum(l));
  {
    f32x4* Ow = reinterpret_cast<f32x4*>(Vs);  // (after this wave's own image reads: LDS is in order)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) Ow[dt * 64 + lane] = o[dt];
    if (g == 0) {
      sm_m[wave][r] = m;
      sm_l[wave][r] = l;
    }
  }
  __syncthreads();
  float M = sm_m[0][r];
#pragma unroll
  for (int w = 1; w < 4; ++w) M = fmaxf(M, sm_m[w][r]);
  float a[4], L = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    a[w] = fexp2(sm_m[w][r] - M);
    L = fmaf(a[w], sm_l[w][r], L);
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  const float lse = L > 0.f ? (M + __log2f(L)) * kLn2 : -INFINITY;
  const int64_t prow = (int64_t)sp * p.B * p.n * p.H + orow;
  // wave w finishes d blocks w, w + 4, ...: lane (r, g) holds d = 16 dt + 4 g .. +3 of query r
  for (int dt = wave; dt < NDT; dt += 4) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const f32x4 ow = reinterpret_cast<const f32x4*>(smem + w * VBUF)[dt * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(a[w], ow[i], acc[i]);
    }
    if (!valid_q) continue;
    const int d = 16 * dt + 4 * g;
    if (nsplit > 1) {
      *reinterpret_cast<float4*>(p.opart + prow * D + d) = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
    } else {
      const uint32_t lo = (uint32_t)Elem<T>::from_f(acc[0] * inv) | ((uint32_t)Elem<T>::from_f(acc[1] * inv) << 16);
      const uint32_t hi = (uint32_t)Elem<T>::from_f(acc[2] * inv) | ((uint32_t)Elem<T>::from_f(acc[3] * inv) << 16);
      *reinterpret_cast<uint2*>((S*)p.o + orow * D + d) = make_uint2(lo, hi);
    }
  }
  if (wave == 0 && g == 0 && valid_q) {
    if (nsplit > 1)
      p.lpart[prow] = lse;
    else
      p.lse[orow] = lse;
  }
}

template <typename T, int D, typename P>
void launch_verify(const P& p, hipStream_t s) {
  const int nqt = fa_verify_query_tiles(p.n);
  const dim3 grid((unsigned)((int64_t)nqt * p.B * p.H * p.splits)), block(256);
  hipLaunchKernelGGL((fa_verify_kernel<T, D, P>), grid, block, 0, s, p, nqt);
}

template <typename T, typename P>
void launch_verify_d(const P& p, hipStream_t s) {
  switch (p.D) {
    case 32: launch_verify<T, 32, P>(p, s); break;
    case 64: launch_verify<T, 64, P>(p, s); break;
    case 80: launch_verify<T, 80, P>(p, s); break;
    case 128: launch_verify<T, 128, P>(p, s); break;
    default: abort();  // the binding checks the head dim
  }
}

// kernel, then fa_decode_chunk's merge launch over the partials (same layout)
template <typename P>
void verify(const P& p, DType t, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0 || p.n <= 0) return;
  switch (t) {
    case DType::BF16: launch_verify_d<BF16, P>(p, s); break;
    case DType::F16: launch_verify_d<F16, P>(p, s); break;
    default: abort();  // the binding checks the dtype
  }
  if (p.splits > 1) {
    DecodeChunkParams m;
    m.q = p.q; m.k = p.k; m.v = p.v;
    m.o = p.o;
    m.lse = p.lse;
    m.kv_len = p.kv_len;
    m.k_sb = m.k_sh = m.k_sn = m.v_sb = m.v_sh = m.v_sn = 0;
    m.B = p.B; m.n = p.n; m.H = p.H; m.D = p.D; m.max_len = p.max_len;
    m.scale = p.scale;
    m.splits = p.splits;
    m.opart = p.opart;
    m.lpart = p.lpart;
    fa_decode_chunk_merge(m, t, s);
  }
}

}  // namespace fa

int fa_verify_query_tiles(int n) { return (n + 15) / 16; }

int fa_verify_splits(int B, int H, int n, int max_kv_len) {
  // two workgroups per CU keep enough row loads in flight (a wave has one sub-tile's K and V ahead of
  // its MFMAs): 512 workgroups for the 256 CUs, never more splits than 128-key tiles (so never more
  // than sub-tiles), at most 64 partials to merge
  const int64_t wgs = (int64_t)B * H * fa_verify_query_tiles(n);
  if (wgs <= 0) return 1;
  const int64_t tiles = ((int64_t)max_kv_len + 127) / 128;
  int64_t want = (512 + wgs - 1) / wgs;
  want = std::min<int64_t>(want, tiles);
  want = std::min<int64_t>(want, 64);
  return (int)std::max<int64_t>(want, 1);
}

void fa_verify(const VerifyParams& p, DType t, hipStream_t s) { fa::verify(p, t, s); }
void fa_verify_paged(const VerifyPagedParams& p, DType t, hipStream_t s) { fa::verify(p, t, s); }

}  // namespace cs336
