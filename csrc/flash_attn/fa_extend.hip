// Extend attention for MI355X (gfx950 / CDNA4): n new query rows per (batch, head) against a KV cache
// that already holds keys, at MFMA rate, on the dense and on the paged cache layout. The MFMA sibling
// of fa_decode_chunk.hip (whose VALU query tile is 8 rows) for chunked prefill, a follow-up prompt and
// different suffixes on a forked prefix.
// cs336-build: no-packed-f32 (the rescale and normalise loops stay single v_mul_f32 beside the MFMAs)
//
// Semantics are fa_decode_chunk's: q (B, n, H, D) contiguous; kv_len[b] counts the keys AFTER the
// chunk's own rows were appended; query i sees keys [0, kv_len[b] - (n - 1 - i)), clamped to
// [0, max_len] (bottom-right-aligned causality); a bound <= 0 gives o = 0, lse = -inf. Outputs
// o (B, n, H, D) in q's dtype and the natural-log lse (B, n, H) fp32. bf16 / fp16, D in {32, 64, 80, 128}.
//
// Design: the VGPR-staged form of fa_fwd.hip with the helpers of fa_common.h.
//   * Work split: 1-D grid of (query tile, batch*head, key split), key splits of one tile adjacent,
//     the last (heaviest) query tiles dispatched first. A workgroup is 4 waves and owns 128 query
//     rows, 32 per wave on v_mfma_f32_32x32x16_{bf16,f16}. The 32x32x16 shape was kept over a 64-row
//     tile on 16x16x32 because every fragment layout here (row fragments, the accumulator-to-operand
//     packing, the transposed V reads) is the forward's, checked on the host by host_checks.cpp; with
//     n < 128 the waves past the last query row only help staging, and the key split, not the query
//     tile, supplies the workgroups (profiles/decode_extend.md has the small-n rows).
//   * S^T = K Q^T, so a lane owns one query column and its running max / sum are lane-local. Q
//     fragments stay resident in registers. scale * log2(e) is applied in the exp2 FMA in fp32, not
//     folded into the 16-bit Q (which would round the scaled query a second time).
//   * K / V tiles of 64 keys go global -> registers -> swizzled LDS, double buffered: the next tile's
//     global loads are issued before this tile's MFMAs and written to the other buffer after them. P
//     is packed from the accumulator straight into the PV operand; V^T comes from ds_read_b64_tr_b16.
//     d 80 is computed as 96 (the pad chunks are zeros in LDS, never loaded or stored).
//   * Row address policy (template parameter): DenseRows k + b*s_b + h*s_h + j*s_n; PagedRows
//     pool + clamp(table[b, j >> lg], 0, num_pages - 1)*s_page + h*s_h + (j & (P - 1))*s_n, all in
//     64-bit element offsets. A staging lane loads 16 B of one row, so each lane looks up the page of
//     its own row; the ids of tile j + 1 are requested before tile j's row loads are issued (and are
//     older than them on the memory counter), so the table's round trip never sits between row loads
//     (the scheme of fa_decode_paged.hip). The index is clamped to the tile's last valid row: the
//     table is never read beyond entry (kv_len[b] - 1) >> lg.
//   * Rows that must not be seen: a staged row at or beyond the query tile's key range (which ends
//     at or below kv_len[b]) is written to LDS as zeros and never loaded. Masking the score is not
//     enough with MFMA: P = 0 times a NaN of an uninitialised row is NaN. Rows in a query's future
//     but inside the range are rows of this chunk, finite, and get weight 0 by the mask.
//   * Causality: a query tile's key range is [0, bound of its last real query); tiles beyond it are
//     never loaded, a wave skips tiles wholly beyond all of its rows, and only tiles that straddle
//     some query's bound pay the mask. Queries at and beyond n are masked and not stored.
//   * Split over keys: split s of S takes key tiles [T*s/S, T*(s+1)/S) of the range's T tiles, a
//     function of the tile's bound and S alone, so the result depends on the logical rows only: any
//     page placement, and the dense and paged kernels on the same rows, give the same bits. S == 1
//     writes o / lse; otherwise each split writes a normalised fp32 partial and its LSE in
//     fa_decode_chunk's layout (opart (S, B*n*H, D), lpart (S, B*n*H); an empty split lse = -inf) and
//     fa_decode_chunk_merge combines them. No atomics, no scratch.
#include "fa_common.h"

#include <algorithm>

namespace cs336 {
namespace fa {

// ---- row address policies: element offset of cached row `key` (K and V planes) -------------------
template <typename P>
struct ExtendRows;

template <>
struct ExtendRows<ExtendParams> {
  static constexpr bool kPaged = false;
  int64_t k0, v0, k_sn, v_sn;
  __device__ __forceinline__ ExtendRows(const ExtendParams& p, int b, int h)
      : k0((int64_t)b * p.k_sb + (int64_t)h * p.k_sh), v0((int64_t)b * p.v_sb + (int64_t)h * p.v_sh), k_sn(p.k_sn),
        v_sn(p.v_sn) {}
  __device__ __forceinline__ int page(int) const { return 0; }
  __device__ __forceinline__ int64_t k(int key, int) const { return k0 + (int64_t)key * k_sn; }
  __device__ __forceinline__ int64_t v(int key, int) const { return v0 + (int64_t)key * v_sn; }
};

template <>
struct ExtendRows<ExtendPagedParams> {
  static constexpr bool kPaged = true;
  const int* tbl;
  int64_t k0, v0, k_sp, v_sp, k_sn, v_sn;
  int lg, pmask, last_page;
  __device__ __forceinline__ ExtendRows(const ExtendPagedParams& p, int b, int h)
      : tbl(p.table + (int64_t)b * p.table_sb), k0((int64_t)h * p.k_sh), v0((int64_t)h * p.v_sh), k_sp(p.k_sp),
        v_sp(p.v_sp), k_sn(p.k_sn), v_sn(p.v_sn), lg(p.lg_page), pmask((1 << p.lg_page) - 1),
        last_page(p.num_pages - 1) {}
  // the raw table entry of `key`'s page (clamped at its use: nothing here waits for the load)
  __device__ __forceinline__ int page(int key) const { return tbl[key >> lg]; }
  __device__ __forceinline__ int64_t k(int key, int pg) const {
    const int id = pg < 0 ? 0 : (pg > last_page ? last_page : pg);
    return k0 + (int64_t)id * k_sp + (int64_t)(key & pmask) * k_sn;
  }
  __device__ __forceinline__ int64_t v(int key, int pg) const {
    const int id = pg < 0 ? 0 : (pg > last_page ? last_page : pg);
    return v0 + (int64_t)id * v_sp + (int64_t)(key & pmask) * v_sn;
  }
};

template <typename T, int D, typename P>
__global__ __launch_bounds__(256, 2) void fa_extend_kernel(const P p, const int nqt) {
  typedef typename Elem<T>::storage S;
  typedef ExtendRows<P> Rows;
  constexpr int ES = sizeof(S);
  static_assert(ES == 2, "fa_extend: 16-bit types only");
  constexpr int DP = PadD<D>::value;  // compute width (80 -> 96)
  constexpr int RB = DP * ES;         // bytes per LDS row
  constexpr int CPR = RB / 16;        // 16-byte chunks per row
  constexpr int CREAL = D * ES / 16;  // chunks that hold real data
  constexpr int EPC = 16 / ES;        // elements per chunk
  constexpr int BM = 128, BN = 64;
  constexpr int TILE = BN * RB;
  constexpr int LPT = BN * CPR / 256;  // 16-B staging loads per thread per tile
  static_assert(BN * CPR % 256 == 0, "staging rounds must be whole");
  constexpr int NDT = DP / 32;         // 32-wide d tiles of O^T
  constexpr int NQF = DP / 16;         // resident Q fragments per lane
  constexpr int NKR = (D + 15) / 16;   // k-steps of S^T over the real d

  __shared__ __attribute__((aligned(1024))) char smem[2 * 2 * TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int l32 = lane & 31, hh = lane >> 5;

  // block -> (query tile, batch*head, split): splits adjacent, last query tiles first
  const int nsplit = p.splits, sp = (int)(blockIdx.x % (unsigned)nsplit);
  const int rest = (int)(blockIdx.x / (unsigned)nsplit);
  const int nbh = p.B * p.H;
  const int qb = nqt - 1 - rest / nbh, bh = rest % nbh;
  const int b = bh / p.H, h = bh % p.H;
  const int q0 = qb * BM;

  // ---- key bounds: of a query, of the tile (its last real query) and of this wave's rows ---------
  const int64_t kvl = p.kv_len[b];
  auto bound = [&](int i) {  // keys query i sees (0 <= i < n)
    const int64_t v = kvl - (int64_t)(p.n - 1 - i);
    return (int)(v < 0 ? 0 : (v > p.max_len ? p.max_len : v));
  };
  const int nkeys = bound(min(q0 + BM, p.n) - 1);
  const int qw0 = q0 + wave * 32;
  const int qrow = qw0 + l32;
  const bool valid_q = qrow < p.n;
  const int lim_q = valid_q ? bound(qrow) : 0;
  // (wave-uniform) the largest and the smallest bound among the wave's real rows
  const int wmax = qw0 < p.n ? bound(min(qw0 + 32, p.n) - 1) : 0;
  const int wmin = qw0 < p.n ? bound(qw0) : 0;

  const S* Kg = (const S*)p.k;
  const S* Vg = (const S*)p.v;
  const Rows rows(p, b, h);

  // ---- Q fragments (B operand), resident for the whole kernel ---------------------------------
  const int64_t orow = ((int64_t)b * p.n + qrow) * p.H + h;  // row of q, o and lse
  uint4 qf[NQF];
#pragma unroll
  for (int i = 0; i < NQF; ++i) {
    const int e = 16 * i + 8 * hh;
    qf[i] = (valid_q && e < D) ? *reinterpret_cast<const uint4*>((const S*)p.q + orow * D + e) : make_uint4(0, 0, 0, 0);
  }

  // this block's key tiles: [jt0, jt0 + ntiles) of the tile's range; j below is relative to jt0
  const int ntiles_all = (nkeys + BN - 1) / BN;
  const int jt0 = (int)((int64_t)ntiles_all * sp / nsplit);
  const int ntiles = (int)((int64_t)ntiles_all * (sp + 1) / nsplit) - jt0;

  // ---- staging: chunk c = tid + 256 i of a tile is 16 B of row c / CPR ----------------------------
  uint4 kst[LPT], vst[LPT];
  int pg[LPT];  // paged: table entries of the rows of the NEXT tile to be loaded
  auto fetch = [&](int j) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int key = (jt0 + j) * BN + (tid + 256 * i) / CPR;
      pg[i] = Rows::kPaged ? rows.page(min(key, nkeys - 1)) : 0;
    }
  };
  auto gload = [&](int j) {
    int cur[LPT];
#pragma unroll
    for (int i = 0; i < LPT; ++i) cur[i] = pg[i];
    if (Rows::kPaged) fetch(j + 1);  // in flight under this tile's row loads and MFMAs
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = tid + 256 * i;
      const int r = c / CPR, ch = c % CPR;
      const int key = (jt0 + j) * BN + r;
      if (key < nkeys && (CREAL == CPR || ch < CREAL)) {
        kst[i] = *reinterpret_cast<const uint4*>(Kg + rows.k(key, cur[i]) + ch * EPC);
        vst[i] = *reinterpret_cast<const uint4*>(Vg + rows.v(key, cur[i]) + ch * EPC);
      } else {  // beyond the range (or the d pad): zeros, so 0 * P is 0 whatever the cache holds there
        kst[i] = make_uint4(0, 0, 0, 0);
        vst[i] = make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto swrite = [&](int buf) {
    char* Ks = smem + buf * 2 * TILE;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = tid + 256 * i;
      const int off = lds_off<RB>(c / CPR, c % CPR);
      *reinterpret_cast<uint4*>(Ks + off) = kst[i];
      *reinterpret_cast<uint4*>(Ks + TILE + off) = vst[i];
    }
  };

  float m = kNegBig, l = 0.f;
  f32x16 o[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) o[i] = zero16();
  const float c2 = p.scale * kLog2e;

  auto tile = [&](int j, const char* Ks) __attribute__((always_inline)) {
    const int kt0 = (jt0 + j) * BN;
    if (kt0 >= wmax) return;  // wholly beyond every row of this wave (wave-uniform)
    const char* Vs = Ks + TILE;
    // ---- S^T = K Q^T ----
    f32x16 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = zero16();
#pragma unroll
      for (int ks = 0; ks < NKR; ++ks)
        s[t] = Mma16<T>::mma(lds_row_frag<T, RB>(Ks, 32 * t, ks, lane), as_frag<T>(qf[ks]), s[t]);
    }
    // ---- mask: key kt0 + 32t + acc_row(r, hh) counts for this lane's query iff it is < lim_q ----
    if (kt0 + BN > wmin) {
      const int lim = lim_q - 1 - kt0 - 4 * hh;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (32 * t + acc_row(r, 0) > lim) s[t][r] = -INFINITY;
    }
    // ---- online softmax (query on the lane), deferred rescale ----
    float mx = s[0][0];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
    mx = xhalf_max(mx);
    const float mt = mx * c2;
    if (__ballot(mt > m + kRescaleThr) != 0) {  // wave-uniform
      const float m_new = fmaxf(m, mt);
      const float alpha = fexp2(m - m_new);
      l *= alpha;
      m = m_new;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
    }
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = fexp2(fmaf(s[t][r], c2, -m));  // (a masked score: exp2(-inf) = 0)
        s[t][r] = pv;
        rs += pv;
      }
    l += rs;
    // ---- O^T += V^T P^T ----
    typename Mma16<T>::frag pf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      pf[t][0] = pack_acc<T>(s[t], 0);
      pf[t][1] = pack_acc<T>(s[t], 1);
    }
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          o[dt] = Mma16<T>::mma(lds_tr_frag<T, RB>(Vs, 32 * t, s2, dt, lane), pf[t][s2], o[dt]);
  };

  if (ntiles > 0) {  // (uniform over the workgroup)
    fetch(0);
    gload(0);
    swrite(0);
  }
  __syncthreads();
  for (int j = 0; j < ntiles; ++j) {
    const int buf = j & 1;
    if (j + 1 < ntiles) gload(j + 1);
    tile(j, smem + buf * 2 * TILE);
    if (j + 1 < ntiles) swrite(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue ----
  l = xhalf_sum(l);
  if (!valid_q) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  const float lse = l > 0.f ? (m + __log2f(l)) * kLn2 : -INFINITY;
  if (nsplit > 1) {
    // normalised fp32 partial of this key range and its LSE, in fa_decode_chunk's layout
    const int64_t prow = (int64_t)sp * p.B * p.n * p.H + orow;
    float* dst = p.opart + prow * D;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = dt * 32 + 8 * g + 4 * hh;
        if (DP == D || d < D)
          *reinterpret_cast<float4*>(dst + d) =
              make_float4(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
      }
    if (hh == 0) p.lpart[prow] = lse;
    return;
  }
  // lane half hh holds d 8g + 4hh .. +3 of its row per register group g; one v_permlane32_swap per
  // dword pairs groups (g, g + 1), so each half stores 16 B (o is contiguous with 16-B rows). Both
  // halves of a query are here or neither (valid_q depends on lane & 31 only).
  S* dst = (S*)p.o + orow * D;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      uint32_t c[4];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r0 = 4 * g + 2 * k;
        const uint32_t lo = (uint32_t)Elem<T>::from_f(o[dt][r0] * inv) | ((uint32_t)Elem<T>::from_f(o[dt][r0 + 1] * inv) << 16);
        const uint32_t hi = (uint32_t)Elem<T>::from_f(o[dt][r0 + 4] * inv) | ((uint32_t)Elem<T>::from_f(o[dt][r0 + 5] * inv) << 16);
        const auto sw = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
        c[k] = sw[0];
        c[2 + k] = sw[1];
      }
      const int d = dt * 32 + 8 * g + 8 * hh;
      if (DP == D || d < D) *reinterpret_cast<uint4*>(dst + d) = make_uint4(c[0], c[1], c[2], c[3]);
    }
  if (hh == 0) p.lse[orow] = lse;
}

template <typename T, int D, typename P>
void launch_extend(const P& p, hipStream_t s) {
  const int nqt = fa_extend_query_tiles(p.n);
  const dim3 grid((unsigned)((int64_t)nqt * p.B * p.H * p.splits)), block(256);
  hipLaunchKernelGGL((fa_extend_kernel<T, D, P>), grid, block, 0, s, p, nqt);
}

template <typename T, typename P>
void launch_extend_d(const P& p, hipStream_t s) {
  switch (p.D) {
    case 32: launch_extend<T, 32, P>(p, s); break;
    case 64: launch_extend<T, 64, P>(p, s); break;
    case 80: launch_extend<T, 80, P>(p, s); break;
    case 128: launch_extend<T, 128, P>(p, s); break;
    default: abort();  // the binding checks the head dim
  }
}

// kernel, then fa_decode_chunk's merge launch over the partials (same layout)
template <typename P>
void extend(const P& p, DType t, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0 || p.n <= 0) return;
  switch (t) {
    case DType::BF16: launch_extend_d<BF16, P>(p, s); break;
    case DType::F16: launch_extend_d<F16, P>(p, s); break;
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

int fa_extend_query_tiles(int n) { return (n + 127) / 128; }

int fa_extend_splits(int B, int H, int n, int max_kv_len) {
  // fa_decode_splits' rule on this kernel's tiles: enough workgroups to cover the 256 CUs, never more
  // splits than 64-key tiles, at most 64 partials to merge
  const int64_t wgs = (int64_t)B * H * fa_extend_query_tiles(n);
  if (wgs <= 0) return 1;
  const int64_t tiles = ((int64_t)max_kv_len + 63) / 64;
  int64_t want = (256 + wgs - 1) / wgs;
  want = std::min<int64_t>(want, tiles);
  want = std::min<int64_t>(want, 64);
  return (int)std::max<int64_t>(want, 1);
}

void fa_extend(const ExtendParams& p, DType t, hipStream_t s) { fa::extend(p, t, s); }
void fa_extend_paged(const ExtendPagedParams& p, DType t, hipStream_t s) { fa::extend(p, t, s); }

}  // namespace cs336
