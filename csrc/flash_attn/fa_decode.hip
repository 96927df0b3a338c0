// Single-token (decode) attention against a KV cache, split over the keys, and the kernel that
// appends the new token's rotated K / V row to the cache. gfx950, wave64.
//
// fa_decode: one query row per (batch, head) against keys [0, kv_len[b]) of a (B, H, max_len, D)
// cache view. 1 FLOP per byte read, so there is no MFMA and no LDS staging: K and V rows go from
// global memory straight to VGPRs with 16-B loads and the dot product / P.V run on the VALU in fp32.
//
// Layout (row per lane group): a row of D elements is owned by G = D/8 lanes (G = 16 for D = 80, ten
// of them active), 8 elements per lane -- one 16-B load for 16-bit types, two for fp32 -- so one load
// instruction of a wave covers 64/G consecutive rows, fully coalesced. The G partial dot products
// are summed with DPP (quad_perm, row_half_mirror, row_mirror: no LDS, no bpermute); every lane of
// the group then holds the score and keeps its own running max / sum and an 8-wide fp32 slice of the
// output, so P.V needs no cross-lane traffic at all. A workgroup (4 waves = 256/G lane groups) walks
// its key range in tiles of U rows per group. The rows stay packed as loaded (converted to fp32 at
// their use) in two register buffers: the next tile's 2U loads are issued before the current tile is
// computed, so every wave always has loads in flight. The lane groups' (max, sum, acc) are combined
// once at the end, inside each wave by a shuffle butterfly and across the 4 waves through LDS, in a
// fixed order.
//
// Split over keys: the grid is B*H*splits; split s of sequence b takes an equal share (rounded up to
// the key tile) of kv_len[b], which is read in the kernel -- nothing here synchronizes the host.
// splits == 1 writes o / lse directly; otherwise each split writes a normalized fp32 partial O and
// its natural-log LSE (opart (splits, B*H, D), lpart (splits, B*H)) and fa_decode_merge_kernel
// combines them. An empty split writes lse = -inf (and zeros), which the merge gives weight 0. No
// atomics anywhere: the result is bitwise reproducible for a given split count.
//
// Rows at and beyond kv_len[b] are never loaded (a masked slot of the last tile re-reads the split's
// last valid row), so they may hold anything.
// All cache addressing is in 64-bit element offsets.
#include "fa_decode_common.h"

namespace cs336 {
namespace {

template <typename T, int D>
__global__ __launch_bounds__(kDecodeThreads) void fa_decode_kernel(const DecodeParams p) {
  typedef typename Elem<T>::storage S;
  constexpr int G = decode_group(D);
  constexpr int NG = kDecodeThreads / G;  // lane groups (rows per load step) of the workgroup
  constexpr int U = decode_unroll(sizeof(S));
  constexpr int KT = NG * U;  // keys per tile
  constexpr int C = D / 8;    // active lanes of a group

  __shared__ float sm_m[kDecodeWaves];
  __shared__ float sm_l[kDecodeWaves];
  __shared__ float sm_acc[kDecodeWaves][D];

  const int tid = threadIdx.x;
  const int split = blockIdx.x % p.splits;
  const int row = blockIdx.x / p.splits;  // b * H + h
  const int b = row / p.H, h = row - b * p.H;
  const int gi = tid / G, c = tid % G;
  const bool active = c < C;

  int n = p.kv_len[b];
  n = n < 0 ? 0 : (n > p.max_len ? p.max_len : n);
  const int tiles = (n + KT - 1) / KT;
  const int per = (tiles + p.splits - 1) / p.splits;
  const int64_t begin = (int64_t)split * per * KT;
  const int64_t end = begin + (int64_t)per * KT < n ? begin + (int64_t)per * KT : n;

  // (the idle lanes of a D = 80 group load column 0 again; their q is 0 and their acc is not stored)
  const int col = active ? 8 * c : 0;
  const S* __restrict__ kbase = (const S*)p.k + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh + col;
  const S* __restrict__ vbase = (const S*)p.v + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh + col;

  // this lane's 8 query elements, with scale * log2(e) folded in (scores live in the exp2 domain)
  Chunk8 q;
#pragma unroll
  for (int i = 0; i < 8; ++i) q.f[i] = 0.f;
  if (active) {
    q = load8<T>((const S*)p.q + (int64_t)row * D + 8 * c);
    const float sc = p.scale * kLog2e;
#pragma unroll
    for (int i = 0; i < 8; ++i) q.f[i] *= sc;
  }

  Online st;
  st.m = -INFINITY;
  st.l = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) st.acc[i] = 0.f;

  // rows j0 + u * NG + gi of a tile, by pointers that advance one tile per call (no 64-bit multiply
  // per row). A row at or beyond `end` re-reads row end - 1 instead (a valid row of this split; its
  // score is masked to -inf below): the loads stay unconditional, so the loop body is one basic block
  // and the wait counts let the next tile's loads stay in flight under this tile's arithmetic. Rows
  // beyond kv_len are never touched.
  const int64_t first = begin + gi;
  const S* kptr = kbase + first * p.k_sn;
  const S* vptr = vbase + first * p.v_sn;
  const S* const klast = kbase + (end - 1) * p.k_sn;
  const S* const vlast = vbase + (end - 1) * p.v_sn;
  const int64_t k_ustep = (int64_t)NG * p.k_sn, v_ustep = (int64_t)NG * p.v_sn;
  auto issue = [&](Raw8<T>(&kr)[U], Raw8<T>(&vr)[U], int64_t j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = j0 + u * NG + gi < end;
      kr[u] = load_raw<T>(ok ? kptr + u * k_ustep : klast);
      vr[u] = load_raw<T>(ok ? vptr + u * v_ustep : vlast);
    }
    kptr += U * k_ustep;
    vptr += U * v_ustep;
  };
  auto compute = [&](const Raw8<T>(&kr)[U], const Raw8<T>(&vr)[U], int64_t j0) {
    float s[U];
    float tmax = st.m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const Chunk8 kk = unpack<T>(kr[u]);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = fmaf(q.f[i], kk.f[i], d);
      d = group_sum<G>(d);
      s[u] = j0 + u * NG + gi < end ? d : -INFINITY;
      tmax = fmaxf(tmax, s[u]);
    }
    // a group that has seen no valid key yet keeps m = -inf; subtract 0 there so nothing is inf - inf
    const float msub = tmax == -INFINITY ? 0.f : tmax;
    const float alpha = __builtin_amdgcn_exp2f(st.m - msub);
    st.m = tmax;
    st.l *= alpha;
#pragma unroll
    for (int i = 0; i < 8; ++i) st.acc[i] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const Chunk8 vv = unpack<T>(vr[u]);
      const float pu = __builtin_amdgcn_exp2f(s[u] - msub);
      st.l += pu;
#pragma unroll
      for (int i = 0; i < 8; ++i) st.acc[i] = fmaf(pu, vv.f[i], st.acc[i]);
    }
  };

  if (begin < end) {  // (uniform over the workgroup)
    // Two tiles per iteration in two register buffers, with no exit between them: the body is one
    // basic block in which each tile's loads are issued one tile ahead of their use (an exit between
    // the halves lets the compiler sink the loads down to their use, and a single buffer copied at
    // the end of the iteration has to wait for them there). A tile wholly beyond `end` computes a
    // no-op: every score is -inf, every weight 0.
    Raw8<T> ka[U], va[U], kb[U], vb[U];
    issue(ka, va, begin);
    for (int64_t j0 = begin; j0 < end; j0 += 2 * KT) {
      issue(kb, vb, j0 + KT);
      compute(ka, va, j0);
      issue(ka, va, j0 + 2 * KT);
      compute(kb, vb, j0 + KT);
    }
  }

  // combine the lane groups of each wave: butterfly over the lanes that hold the same columns
#pragma unroll
  for (int off = G; off < kWave; off *= 2) {
    const float m2 = __shfl_xor(st.m, off, kWave), l2 = __shfl_xor(st.l, off, kWave);
    float acc2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc2[i] = __shfl_xor(st.acc[i], off, kWave);
    online_merge(st, m2, l2, acc2);
  }
  // ... and the 4 waves through LDS, in wave order
  const int wave = tid / kWave, lane = tid % kWave;
  if (lane == 0) {
    sm_m[wave] = st.m;
    sm_l[wave] = st.l;
  }
  if (lane < G && active) {
#pragma unroll
    for (int i = 0; i < 8; ++i) sm_acc[wave][8 * c + i] = st.acc[i];
  }
  __syncthreads();
  if (tid < D) {
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < kDecodeWaves; ++w) M = fmaxf(M, sm_m[w]);
    float L = 0.f, o = 0.f;
    if (M != -INFINITY) {
#pragma unroll
      for (int w = 0; w < kDecodeWaves; ++w) {
        const float wt = __builtin_amdgcn_exp2f(sm_m[w] - M);  // 0 for a wave with m = -inf
        L = fmaf(sm_l[w], wt, L);
        o = fmaf(sm_acc[w][tid], wt, o);
      }
      o = o / L;  // L >= 1: the row holding the maximum contributes exp2(0)
    }
    const float lse = M == -INFINITY ? -INFINITY : (M + __builtin_amdgcn_logf(L)) * kLn2;
    if (p.splits == 1) {
      ((S*)p.o)[(int64_t)row * D + tid] = Elem<T>::from_f(o);
      if (tid == 0) p.lse[row] = lse;
    } else {
      const int64_t pr = (int64_t)split * p.B * p.H + row;
      p.opart[pr * D + tid] = o;
      if (tid == 0) p.lpart[pr] = lse;
    }
  }
}

// o = sum_s w_s opart[s] / sum_s w_s, w_s = exp(lpart[s] - max lpart); lse = max + log(sum w)
template <typename T, int D>
__global__ __launch_bounds__(128) void fa_decode_merge_kernel(const DecodeParams p) {
  typedef typename Elem<T>::storage S;
  const int row = blockIdx.x, tid = threadIdx.x;
  if (tid >= D) return;
  const int64_t rows = (int64_t)p.B * p.H;
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
  ((S*)p.o)[(int64_t)row * D + tid] = Elem<T>::from_f(o);
  if (tid == 0) p.lse[row] = M == -INFINITY ? -INFINITY : M + __builtin_amdgcn_logf(W) * kLn2;
}

// One thread per (batch, q|k|v part, head, 8-element chunk) of the new token's fused projection row.
template <typename T>
__global__ __launch_bounds__(256) void kv_append_rope_kernel(const AppendParams p, int total) {
  typedef typename Elem<T>::storage S;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int D8 = p.D / 8, HD8 = p.H * D8;
  const int b = i / (3 * HD8), r = i - b * 3 * HD8;
  const int part = r / HD8, hc = r - part * HD8;
  const int h = hc / D8, c = hc - h * D8;
  const int pos = p.pos[b];
  const bool in_range = pos >= 0 && pos < p.max_len && pos < p.ctx;
  S* qout = (S*)p.q_out + ((int64_t)b * p.H + h) * p.D + 8 * c;
  if (!in_range) {  // no slot for this token: nothing is stored to the cache
    if (part == 0) {
      Chunk8 z;
#pragma unroll
      for (int e = 0; e < 8; ++e) z.f[e] = 0.f;
      store8<T>(qout, z);
    }
    return;
  }
  Chunk8 x = load8<T>((const S*)p.qkv + (int64_t)b * p.qkv_sb + (int64_t)part * p.H * p.D + h * p.D + 8 * c);
  if (part < 2) {
    const int half = p.D / 2;
    const float4 cs = *reinterpret_cast<const float4*>(p.cos + (int64_t)pos * half + 4 * c);
    const float4 sn = *reinterpret_cast<const float4*>(p.sin + (int64_t)pos * half + 4 * c);
    const float cc[4] = {cs.x, cs.y, cs.z, cs.w}, ss[4] = {sn.x, sn.y, sn.z, sn.w};
    Chunk8 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      y.f[2 * e] = cc[e] * x.f[2 * e] - ss[e] * x.f[2 * e + 1];
      y.f[2 * e + 1] = ss[e] * x.f[2 * e] + cc[e] * x.f[2 * e + 1];
    }
    x = y;
  }
  if (part == 0) {
    store8<T>(qout, x);
  } else {
    S* cache = (S*)(part == 1 ? p.k : p.v);
    const int64_t sb = part == 1 ? p.k_sb : p.v_sb, sh = part == 1 ? p.k_sh : p.v_sh;
    const int64_t sn_ = part == 1 ? p.k_sn : p.v_sn;
    store8<T>(cache + (int64_t)b * sb + (int64_t)h * sh + (int64_t)pos * sn_ + 8 * c, x);
  }
}

template <typename T, int D>
void launch_merge(const DecodeParams& p, hipStream_t s) {
  hipLaunchKernelGGL((fa_decode_merge_kernel<T, D>), dim3((unsigned)(p.B * p.H)), dim3(128), 0, s, p);
}

template <typename T, int D>
void launch_decode(const DecodeParams& p, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)p.B * p.H * p.splits));
  hipLaunchKernelGGL((fa_decode_kernel<T, D>), grid, dim3(kDecodeThreads), 0, s, p);
  if (p.splits > 1) launch_merge<T, D>(p, s);
}

template <typename T>
void launch_decode_d(const DecodeParams& p, hipStream_t s) {
  switch (p.D) {
    case 32: launch_decode<T, 32>(p, s); break;
    case 64: launch_decode<T, 64>(p, s); break;
    case 80: launch_decode<T, 80>(p, s); break;
    case 128: launch_decode<T, 128>(p, s); break;
    default: abort();  // the binding checks the head dim
  }
}

template <typename T>
void launch_merge_d(const DecodeParams& p, hipStream_t s) {
  switch (p.D) {
    case 32: launch_merge<T, 32>(p, s); break;
    case 64: launch_merge<T, 64>(p, s); break;
    case 80: launch_merge<T, 80>(p, s); break;
    case 128: launch_merge<T, 128>(p, s); break;
    default: abort();
  }
}

}  // namespace

int fa_decode_key_tile(int D, DType t) { return decode_tile(D, t == DType::F32 ? 4 : 2); }

int fa_decode_splits(int B, int H, int D, DType t, int max_kv_len) {
  // One workgroup per CU of the MI355X (256): with its loads pipelined one tile ahead a 4-wave
  // workgroup streams at its CU's share of the HBM rate, so more splits than that only add partials
  // for the merge to read (25 rows x 16384 keys: 109 us unsplit, 48 us at 8 splits, 57 us at 32). A
  // split keeps at least four key tiles, so that the per-workgroup prologue and combine stay small
  // next to the streaming loop (25 rows x 512 keys: 1 split 10 us, 4 splits 12 us), and at most 64
  // partials are merged. Sweep of forced split counts: profiles/decode_attention.md.
  const int64_t rows = (int64_t)B * H;
  if (rows <= 0) return 1;
  const int KT = fa_decode_key_tile(D, t);
  const int64_t tiles = ((int64_t)max_kv_len + KT - 1) / KT;
  int64_t want = (256 + rows - 1) / rows;
  if (want > tiles / 4) want = tiles / 4;
  if (want > 64) want = 64;
  if (want < 1) want = 1;
  return (int)want;
}

void fa_decode(const DecodeParams& p, DType t, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0) return;
  switch (t) {
    case DType::F32: launch_decode_d<float>(p, s); break;
    case DType::BF16: launch_decode_d<BF16>(p, s); break;
    case DType::F16: launch_decode_d<F16>(p, s); break;
  }
}

void fa_decode_merge(const DecodeParams& p, DType t, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0) return;
  switch (t) {
    case DType::F32: launch_merge_d<float>(p, s); break;
    case DType::BF16: launch_merge_d<BF16>(p, s); break;
    case DType::F16: launch_merge_d<F16>(p, s); break;
  }
}

void kv_append_rope(const AppendParams& p, DType t, hipStream_t s) {
  const int64_t total64 = (int64_t)p.B * 3 * p.H * (p.D / 8);
  if (total64 <= 0) return;
  const int total = (int)total64;  // one token per sequence: far below 2^31 (the binding checks it)
  const dim3 grid((unsigned)((total64 + 255) / 256)), block(256);
  switch (t) {
    case DType::F32: hipLaunchKernelGGL(kv_append_rope_kernel<float>, grid, block, 0, s, p, total); break;
    case DType::BF16: hipLaunchKernelGGL(kv_append_rope_kernel<BF16>, grid, block, 0, s, p, total); break;
    case DType::F16: hipLaunchKernelGGL(kv_append_rope_kernel<F16>, grid, block, 0, s, p, total); break;
  }
}

}  // namespace cs336
