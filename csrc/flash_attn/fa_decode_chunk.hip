// Multi-token (chunk) attention against a KV cache, split over the keys, and the kernel that appends
// a chunk's rotated K / V rows to the cache. gfx950, wave64. The n-token sibling of fa_decode.hip:
// a chunked prefill or the verify step of speculative decoding scores n query rows per (batch, head)
// against one cache.
//
// fa_decode_chunk: q (B, n, H, D) -- the layout the fused QKV row gives -- against keys of a
// (B, H, max_len, D) cache view. kv_len[b] counts the keys AFTER the chunk's own rows were appended;
// query i sees keys [0, kv_len[b] - (n - 1 - i)), clamped to [0, max_len] (bottom-right-aligned
// causality). A query whose bound is <= 0 gives o = 0, lse = -inf.
//
// Form: fa_decode's VALU form, not MFMA. A verify step has n <= 16 rows per head, at most one MFMA
// tile, and the kernel is bound by streaming K and V once; the row-per-lane-group layout of
// fa_decode (D/8 lanes own a row, 16-B loads straight to VGPRs, two register buffers so the next key
// tile's loads are in flight under this tile's arithmetic, DPP sum over the lane group) already
// streams at the HBM rate and needs no LDS staging or operand transposes. Large prefill chunks,
// where an MFMA form would pay, are out of scope (README).
//
// Query tile: a workgroup owns QT consecutive queries of one (b, h, split) and applies every loaded
// K / V row to all of them, so a row is read from memory once per query tile. Every lane keeps, per
// query, the running max / sum and an 8-wide fp32 output slice (10 VGPRs) plus the query's 8 scaled
// elements: 144 VGPRs at QT = 8, beside the two row buffers. The kernel is instantiated for QT in
// {1, 4, 8}; the host picks the smallest that holds n (8 for n > 8, with ceil(n / 8) query tiles as a
// further grid dimension), so n = 1 does fa_decode's work and a short chunk does not pay for eight
// queries. Queries of a tile at and beyond n are masked (bound 0) and not stored. The VALU work per
// loaded byte is QT times fa_decode's: QT = 4 still streams at the n = 1 rate, QT = 8 is VALU-bound at
// about half of it (profiles/decode_chunk.md). There is no QT = 2: as compiled it was slower than
// QT = 4 at every measured shape, so n = 2 runs the QT = 4 kernel with two masked queries.
//
// Split over keys: the grid is B*H*qtiles*splits. A tile's key range is [0, bound of its last query)
// (the largest of the tile); split s takes an equal share of it, rounded up to the key tile. The mask
// is per query: row j counts for query i only if j < bound_i, so a row of the chunk that lies in a
// query's future is loaded but has weight 0. splits == 1 writes o / lse directly; otherwise each
// split writes a normalized fp32 partial O and its natural-log LSE (opart (splits, B*n*H, D), lpart
// (splits, B*n*H)) and fa_decode_chunk_merge_kernel combines them. An empty split writes lse = -inf.
// No atomics: bitwise reproducible for a given (n, splits). Nothing synchronizes the host.
//
// Rows at and beyond kv_len[b] are never loaded (a masked slot of the last tile re-reads the split's
// last valid row). All cache addressing is in 64-bit element offsets.
#include "fa_decode_common.h"

namespace cs336 {
namespace {

template <typename T, int D, int QT>
__global__ __launch_bounds__(kDecodeThreads) void fa_decode_chunk_kernel(const DecodeChunkParams p, const int qtiles) {
  typedef typename Elem<T>::storage S;
  constexpr int G = decode_group(D);
  constexpr int NG = kDecodeThreads / G;  // lane groups (rows per load step) of the workgroup
  // rows per lane group and tile: fa_decode's, halved for 16-bit types at QT = 8, where the scores of
  // a tile (QT * U) and the row buffers (8U) no longer fit beside the per-query state
  constexpr int U = QT >= 8 && sizeof(S) == 2 ? 2 : decode_unroll(sizeof(S));
  constexpr int KT = NG * U;  // keys per tile
  constexpr int C = D / 8;    // active lanes of a group

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
  const int col = active ? 8 * c : 0;
  const S* __restrict__ kbase = (const S*)p.k + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh + col;
  const S* __restrict__ vbase = (const S*)p.v + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh + col;

  // this lane's 8 elements of every query, with scale * log2(e) folded in (exp2-domain scores)
  Chunk8 q[QT];
  Online st[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
#pragma unroll
    for (int i = 0; i < 8; ++i) q[qi].f[i] = 0.f;
    if (active && i0 + qi < p.n) {
      q[qi] = load8<T>((const S*)p.q + (((int64_t)b * p.n + i0 + qi) * p.H + h) * D + 8 * c);
      const float sc = p.scale * kLog2e;
#pragma unroll
      for (int i = 0; i < 8; ++i) q[qi].f[i] *= sc;
    }
    st[qi].m = -INFINITY;
    st[qi].l = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) st[qi].acc[i] = 0.f;
  }

  // Row addressing and the unconditional loads are fa_decode's: rows j0 + u * NG + gi of a tile by
  // pointers that advance one tile per call; a row at or beyond `end` re-reads row end - 1 (a valid
  // row of this split; its score is masked below). Rows beyond kv_len are never touched.
  const int64_t first = begin + gi;
  const S* kptr = kbase + first * p.k_sn;
  const S* vptr = vbase + first * p.v_sn;
  const S* const klast = kbase + (end - 1) * p.k_sn;
  const S* const vlast = vbase + (end - 1) * p.v_sn;
  const int64_t k_ustep = (int64_t)NG * p.k_sn, v_ustep = (int64_t)NG * p.v_sn;
  auto issue = [&](Raw8<T>(&kr)[U], Raw8<T>(&vr)[U], int64_t j0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = j0 + u * NG + gi < end;
      kr[u] = load_raw<T>(ok ? kptr + u * k_ustep : klast);
      vr[u] = load_raw<T>(ok ? vptr + u * v_ustep : vlast);
    }
    kptr += U * k_ustep;
    vptr += U * v_ustep;
  };
  auto compute = [&](const Raw8<T>(&kr)[U], const Raw8<T>(&vr)[U], int64_t j0) __attribute__((always_inline)) {
    float s[QT][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const Chunk8 kk = unpack<T>(kr[u]);
      const int64_t j = j0 + u * NG + gi;
      const int jr = j < end ? (int)j : 0x7fffffff;  // (end <= max_len < 2^31)
#pragma unroll
      for (int qi = 0; qi < QT; ++qi) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = fmaf(q[qi].f[i], kk.f[i], d);
        d = group_sum<G>(d);
        // per-query mask (the split's end and the query's bound): s = jr < lim ? d : -inf, as a bit
        // select on the sign of jr - lim. QT * U compare masks held in SGPR pairs spill the SGPR file.
        int diff = jr - lim[qi];  // < 0 iff jr < lim (both >= 0)
        asm("" : "+v"(diff));     // (opaque, or the compiler turns the bit select back into compare masks)
        const uint32_t keep = (uint32_t)(diff >> 31);
        s[qi][u] = __uint_as_float((__float_as_uint(d) & keep) | (0xff800000u & ~keep));
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
      const Chunk8 vv = unpack<T>(vr[u]);
#pragma unroll
      for (int qi = 0; qi < QT; ++qi) {
        const float pu = __builtin_amdgcn_exp2f(s[qi][u] - msub[qi]);
        st[qi].l += pu;
#pragma unroll
        for (int i = 0; i < 8; ++i) st[qi].acc[i] = fmaf(pu, vv.f[i], st[qi].acc[i]);
      }
    }
  };

  if (begin < end) {  // (uniform over the workgroup)
    // two tiles per iteration in two register buffers, one basic block (see fa_decode_kernel)
    Raw8<T> ka[U], va[U], kb[U], vb[U];
    issue(ka, va, begin);
    for (int64_t j0 = begin; j0 < end; j0 += 2 * KT) {
      issue(kb, vb, j0 + KT);
      compute(ka, va, j0);
      issue(ka, va, j0 + 2 * KT);
      compute(kb, vb, j0 + KT);
    }
  }

  // combine the lane groups of each wave (butterfly over the lanes that hold the same columns), then
  // the 4 waves through LDS, in wave order
  const int wave = tid / kWave, lane = tid % kWave;
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
#pragma unroll
    for (int off = G; off < kWave; off *= 2) {
      const float m2 = __shfl_xor(st[qi].m, off, kWave), l2 = __shfl_xor(st[qi].l, off, kWave);
      float acc2[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc2[i] = __shfl_xor(st[qi].acc[i], off, kWave);
      online_merge(st[qi], m2, l2, acc2);
    }
    if (lane == 0) {
      sm_m[wave][qi] = st[qi].m;
      sm_l[wave][qi] = st[qi].l;
    }
    if (lane < G && active) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_acc[wave][qi][8 * c + i] = st[qi].acc[i];
    }
  }
  __syncthreads();
  const int64_t rows = (int64_t)p.B * p.n * p.H;
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
      const int64_t pr = (int64_t)split * rows + orow;
      p.opart[pr * D + cc] = o;
      if (cc == 0) p.lpart[pr] = lse;
    }
  }
}

// o = sum_s w_s opart[s] / sum_s w_s, w_s = exp(lpart[s] - max lpart); lse = max + log(sum w)
template <typename T, int D>
__global__ __launch_bounds__(128) void fa_decode_chunk_merge_kernel(const DecodeChunkParams p) {
  typedef typename Elem<T>::storage S;
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid >= D) return;
  const int64_t rows = (int64_t)p.B * p.n * p.H;
  float M = -INFINITY;
  for (int s = 0; s < p.splits; ++s) M = fmaxf(M, p.lpart[s * rows + row]);
  float W = 0.f, o = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < p.splits; ++s) {
      const float w = __builtin_amdgcn_exp2f((p.lpart[s * rows + row] - M) * kLog2e);  // empty split: 0
      W += w;
      o = fmaf(w, p.opart[(s * rows + row) * D + tid], o);
    }
    o = o / W;
  }
  ((S*)p.o)[row * D + tid] = Elem<T>::from_f(o);
  if (tid == 0) p.lse[row] = M == -INFINITY ? -INFINITY : M + __builtin_amdgcn_logf(W) * kLn2;
}

// One thread per (batch, token, q|k|v part, head, 8-element chunk) of the chunk's fused projection rows.
template <typename T>
__global__ __launch_bounds__(256) void kv_append_rope_chunk_kernel(const AppendChunkParams p, int total) {
  typedef typename Elem<T>::storage S;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int D8 = p.D / 8, HD8 = p.H * D8;
  const int bt = idx / (3 * HD8), r = idx - bt * 3 * HD8;  // bt = b * n + token
  const int b = bt / p.n, t = bt - b * p.n;
  const int part = r / HD8, hc = r - part * HD8;
  const int h = hc / D8, c = hc - h * D8;
  const int64_t pos = (int64_t)p.pos[b] + t;
  const bool in_range = pos >= 0 && pos < p.max_len && pos < p.ctx;
  S* qout = (S*)p.q_out + ((int64_t)bt * p.H + h) * p.D + 8 * c;
  if (!in_range) {  // no slot for this token: nothing is stored to the cache
    if (part == 0) {
      Chunk8 z;
#pragma unroll
      for (int e = 0; e < 8; ++e) z.f[e] = 0.f;
      store8<T>(qout, z);
    }
    return;
  }
  Chunk8 x = load8<T>((const S*)p.qkv + (int64_t)b * p.qkv_sb + (int64_t)t * p.qkv_sn + (int64_t)part * p.H * p.D +
                      h * p.D + 8 * c);
  if (part < 2) {
    const int half = p.D / 2;
    const float4 cs = *reinterpret_cast<const float4*>(p.cos + pos * half + 4 * c);
    const float4 sn = *reinterpret_cast<const float4*>(p.sin + pos * half + 4 * c);
    const float cv[4] = {cs.x, cs.y, cs.z, cs.w}, sv[4] = {sn.x, sn.y, sn.z, sn.w};
    Chunk8 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      y.f[2 * e] = cv[e] * x.f[2 * e] - sv[e] * x.f[2 * e + 1];
      y.f[2 * e + 1] = sv[e] * x.f[2 * e] + cv[e] * x.f[2 * e + 1];
    }
    x = y;
  }
  if (part == 0) {
    store8<T>(qout, x);
  } else {
    S* cache = (S*)(part == 1 ? p.k : p.v);
    const int64_t sb = part == 1 ? p.k_sb : p.v_sb, sh = part == 1 ? p.k_sh : p.v_sh;
    const int64_t sn_ = part == 1 ? p.k_sn : p.v_sn;
    store8<T>(cache + (int64_t)b * sb + (int64_t)h * sh + pos * sn_ + 8 * c, x);
  }
}

template <typename T, int D, int QT>
void launch_chunk_qt(const DecodeChunkParams& p, hipStream_t s) {
  const int qtiles = (p.n + QT - 1) / QT;
  const dim3 grid((unsigned)((int64_t)p.B * p.H * qtiles * p.splits));
  hipLaunchKernelGGL((fa_decode_chunk_kernel<T, D, QT>), grid, dim3(kDecodeThreads), 0, s, p, qtiles);
}

template <typename T, int D>
void launch_chunk_merge(const DecodeChunkParams& p, hipStream_t s) {
  hipLaunchKernelGGL((fa_decode_chunk_merge_kernel<T, D>), dim3((unsigned)((int64_t)p.B * p.n * p.H)), dim3(128), 0, s,
                     p);
}

template <typename T>
void launch_chunk_merge_d(const DecodeChunkParams& p, hipStream_t s) {
  switch (p.D) {
    case 32: launch_chunk_merge<T, 32>(p, s); break;
    case 64: launch_chunk_merge<T, 64>(p, s); break;
    case 80: launch_chunk_merge<T, 80>(p, s); break;
    case 128: launch_chunk_merge<T, 128>(p, s); break;
    default: abort();
  }
}

template <typename T, int D>
void launch_chunk(const DecodeChunkParams& p, hipStream_t s) {
  switch (fa_decode_chunk_qt(p.n)) {
    case 1: launch_chunk_qt<T, D, 1>(p, s); break;
    case 4: launch_chunk_qt<T, D, 4>(p, s); break;
    default: launch_chunk_qt<T, D, kDecodeChunkQT>(p, s); break;
  }
  if (p.splits > 1) launch_chunk_merge<T, D>(p, s);
}

template <typename T>
void launch_chunk_d(const DecodeChunkParams& p, hipStream_t s) {
  switch (p.D) {
    case 32: launch_chunk<T, 32>(p, s); break;
    case 64: launch_chunk<T, 64>(p, s); break;
    case 80: launch_chunk<T, 80>(p, s); break;
    case 128: launch_chunk<T, 128>(p, s); break;
    default: abort();  // the binding checks the head dim
  }
}

}  // namespace

int fa_decode_chunk_qt(int n) { return n <= 1 ? 1 : (n <= 4 ? 4 : kDecodeChunkQT); }

void fa_decode_chunk(const DecodeChunkParams& p, DType t, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0 || p.n <= 0) return;
  switch (t) {
    case DType::F32: launch_chunk_d<float>(p, s); break;
    case DType::BF16: launch_chunk_d<BF16>(p, s); break;
    case DType::F16: launch_chunk_d<F16>(p, s); break;
  }
}

void fa_decode_chunk_merge(const DecodeChunkParams& p, DType t, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0 || p.n <= 0) return;
  switch (t) {
    case DType::F32: launch_chunk_merge_d<float>(p, s); break;
    case DType::BF16: launch_chunk_merge_d<BF16>(p, s); break;
    case DType::F16: launch_chunk_merge_d<F16>(p, s); break;
  }
}

void kv_append_rope_chunk(const AppendChunkParams& p, DType t, hipStream_t s) {
  const int64_t total64 = (int64_t)p.B * p.n * 3 * p.H * (p.D / 8);
  if (total64 <= 0) return;
  const int total = (int)total64;  // (the binding checks that it fits)
  const dim3 grid((unsigned)((total64 + 255) / 256)), block(256);
  switch (t) {
    case DType::F32: hipLaunchKernelGGL(kv_append_rope_chunk_kernel<float>, grid, block, 0, s, p, total); break;
    case DType::BF16: hipLaunchKernelGGL(kv_append_rope_chunk_kernel<BF16>, grid, block, 0, s, p, total); break;
    case DType::F16: hipLaunchKernelGGL(kv_append_rope_chunk_kernel<F16>, grid, block, 0, s, p, total); break;
  }
}

}  // namespace cs336
