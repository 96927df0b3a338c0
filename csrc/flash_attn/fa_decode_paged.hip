// Decode attention and K / V append on a PAGED cache: fa_decode.hip's two kernels with one
// indirection in the address. gfx950, wave64.
//
// The pool is (num_pages, H, P, D) (a page takes the place of a batch row whose max_len is the page
// size P, a power of two >= 16) and row j of sequence b lives at
//   pool + table[b, j >> lg] * s_page + h * s_h + (j & (P - 1)) * s_n        (lg = log2 P)
// in 64-bit element offsets, the three strides taken from the view (a layer slice of a larger pool
// is read in place).
//
// fa_decode_paged is the algorithm of fa_decode_kernel unchanged: a row per lane group, 16-B loads
// straight to VGPRs, two register buffers a tile ahead, the DPP group sum, the in-workgroup combine,
// the grid B*H*splits and fp32 partials in fa_decode_merge's layout (the merge launch is the
// existing one). What is new is the dependent load: the table entry, then the row.
//
// Where the page ids come from -- registers, a tile ahead. Every `issue` of a tile's row loads is
// preceded by the load of the page ids of the tile AFTER the one being issued (U ids per lane: one
// per row the lane group owns); the ids an `issue` consumes were therefore requested one whole
// issue + compute earlier, and, being older than every row load in flight, have arrived by the time
// the older tile's rows have (the memory counter retires loads in order). The table's L2 round trip
// thus never sits between two row loads. The alternative, staging the split's slice of the table
// in LDS before the loop, was not taken: the slice has no bound (max_len / P entries), so it needs a
// second code path for a slice that does not fit, and a barrier in front of the first load; the
// register scheme costs 2U VGPRs, has one path and keeps the loop body one basic block with
// unconditional loads. A wave's load covers 64/G <= 16 consecutive rows, which P >= 16 keeps inside
// one page: the ids of a wave's lanes differ at most between its load steps, not within one.
//
// Rows: the slot of row j is computed from min(j, end - 1), so a masked slot of the last tile
// re-reads the split's last valid row (as in fa_decode_kernel) and the table is never read beyond
// entry (kv_len[b] - 1) >> lg: entries past a sequence's pages may hold -1 or stale ids, and rows at
// or beyond kv_len[b] may hold anything. An id that is read is clamped to [0, num_pages): a table
// the host corrupted reads a wrong page, never memory outside the pool.
//
// Split boundaries are those of fa_decode_kernel: a function of kv_len[b] and splits alone. The
// result therefore depends on the logical rows only -- any placement of the pages gives the same
// bits -- and is bitwise reproducible (no atomics).
//
// kv_append_rope_paged: token i of sequence b is rotated at pos[b] + i and written to that slot
// through the table; nothing is stored (and the token's q row is zeroed) when the slot is outside
// [0, min(max_len, ctx)) or its table entry is outside [0, num_pages).
#include "fa_decode_common.h"

namespace cs336 {
namespace {

template <typename T, int D>
__global__ __launch_bounds__(kDecodeThreads) void fa_decode_paged_kernel(const DecodePagedParams p) {
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

  // (max_len = table columns * P < 2^30, checked by the binding: row indices stay in 32 bits)
  int n = p.kv_len[b];
  n = n < 0 ? 0 : (n > p.max_len ? p.max_len : n);
  const int tiles = (n + KT - 1) / KT;
  const int per = (tiles + p.splits - 1) / p.splits;
  const int begin = split * per * KT;
  const int end = begin + per * KT < n ? begin + per * KT : n;

  // (the idle lanes of a D = 80 group load column 0 again; their q is 0 and their acc is not stored)
  const int col = active ? 8 * c : 0;
  const S* __restrict__ kbase = (const S*)p.k + (int64_t)h * p.k_sh + col;
  const S* __restrict__ vbase = (const S*)p.v + (int64_t)h * p.v_sh + col;
  const int* __restrict__ tbl = p.table + (int64_t)b * p.table_sb;
  const int lg = p.lg_page, pmask = (1 << p.lg_page) - 1, last_page = p.num_pages - 1;

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

  // Row j0 + u * NG + gi of a tile, clamped to the split's last valid row (whose score is masked to
  // -inf in compute): `fetch` loads the page ids of the tile's rows, `issue` the rows of a tile whose
  // ids were fetched a tile earlier. Both are unconditional loads.
  const int lastrow = end - 1;
  auto fetch = [&](int(&pg)[U], int j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * NG + gi;
      pg[u] = tbl[(j < lastrow ? j : lastrow) >> lg];  // (clamped at its use: nothing here waits for it)
    }
  };
  auto issue = [&](Raw8<T>(&kr)[U], Raw8<T>(&vr)[U], const int(&pg)[U], int j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * NG + gi;
      const int r = (j < lastrow ? j : lastrow) & pmask;
      const int id = pg[u] < 0 ? 0 : (pg[u] > last_page ? last_page : pg[u]);
      kr[u] = load_raw<T>(kbase + ((int64_t)id * p.k_sp + (int64_t)r * p.k_sn));
      vr[u] = load_raw<T>(vbase + ((int64_t)id * p.v_sp + (int64_t)r * p.v_sn));
    }
  };
  auto compute = [&](const Raw8<T>(&kr)[U], const Raw8<T>(&vr)[U], int j0) {
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
    // fa_decode_kernel's loop -- two tiles per iteration in two register buffers, no exit between
    // them -- with the page ids of the tile after next fetched in front of every issue.
    Raw8<T> ka[U], va[U], kb[U], vb[U];
    int pa[U], pb[U];
    fetch(pa, begin);
    fetch(pb, begin + KT);
    issue(ka, va, pa, begin);
    for (int j0 = begin; j0 < end; j0 += 2 * KT) {
      fetch(pa, j0 + 2 * KT);
      issue(kb, vb, pb, j0 + KT);
      compute(ka, va, j0);
      fetch(pb, j0 + 3 * KT);
      issue(ka, va, pa, j0 + 2 * KT);
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

// One thread per (batch, token, q|k|v part, head, 8-element chunk) of the fused projection rows.
template <typename T>
__global__ __launch_bounds__(256) void kv_append_rope_paged_kernel(const AppendPagedParams p, int total) {
  typedef typename Elem<T>::storage S;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int D8 = p.D / 8, HD8 = p.H * D8;
  const int bt = idx / (3 * HD8), r = idx - bt * 3 * HD8;  // bt = b * n + token
  const int b = bt / p.n, t = bt - b * p.n;
  const int part = r / HD8, hc = r - part * HD8;
  const int h = hc / D8, c = hc - h * D8;
  const int64_t pos = (int64_t)p.pos[b] + t;
  // the table is read only for a slot it has an entry for; an entry that names no page stores nothing
  bool in_range = pos >= 0 && pos < p.max_len && pos < p.ctx;
  int page = -1;
  if (in_range) {
    page = p.table[(int64_t)b * p.table_sb + (pos >> p.lg_page)];
    in_range = page >= 0 && page < p.num_pages;
  }
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
    S* pool = (S*)(part == 1 ? p.k : p.v);
    const int64_t sp = part == 1 ? p.k_sp : p.v_sp, sh = part == 1 ? p.k_sh : p.v_sh;
    const int64_t sn_ = part == 1 ? p.k_sn : p.v_sn;
    const int64_t slot = pos & ((1 << p.lg_page) - 1);
    store8<T>(pool + (int64_t)page * sp + (int64_t)h * sh + slot * sn_ + 8 * c, x);
  }
}

template <typename T, int D>
void launch_paged(const DecodePagedParams& p, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)p.B * p.H * p.splits));
  hipLaunchKernelGGL((fa_decode_paged_kernel<T, D>), grid, dim3(kDecodeThreads), 0, s, p);
}

template <typename T>
void launch_paged_d(const DecodePagedParams& p, hipStream_t s) {
  switch (p.D) {
    case 32: launch_paged<T, 32>(p, s); break;
    case 64: launch_paged<T, 64>(p, s); break;
    case 80: launch_paged<T, 80>(p, s); break;
    case 128: launch_paged<T, 128>(p, s); break;
    default: abort();  // the binding checks the head dim
  }
}

}  // namespace

void fa_decode_paged(const DecodePagedParams& p, DType t, hipStream_t s) {
  if (p.B <= 0 || p.H <= 0) return;
  switch (t) {
    case DType::F32: launch_paged_d<float>(p, s); break;
    case DType::BF16: launch_paged_d<BF16>(p, s); break;
    case DType::F16: launch_paged_d<F16>(p, s); break;
  }
  if (p.splits > 1) {  // the partials have fa_decode's layout: its merge launch combines them
    DecodeParams m;
    m.q = p.q; m.k = p.k; m.v = p.v;
    m.o = p.o;
    m.lse = p.lse;
    m.kv_len = p.kv_len;
    m.k_sb = m.k_sh = m.k_sn = m.v_sb = m.v_sh = m.v_sn = 0;
    m.B = p.B; m.H = p.H; m.D = p.D; m.max_len = p.max_len;
    m.scale = p.scale;
    m.splits = p.splits;
    m.opart = p.opart;
    m.lpart = p.lpart;
    fa_decode_merge(m, t, s);
  }
}

void kv_append_rope_paged(const AppendPagedParams& p, DType t, hipStream_t s) {
  const int64_t total64 = (int64_t)p.B * p.n * 3 * p.H * (p.D / 8);
  if (total64 <= 0) return;
  const int total = (int)total64;  // (the binding checks that it fits)
  const dim3 grid((unsigned)((total64 + 255) / 256)), block(256);
  switch (t) {
    case DType::F32: hipLaunchKernelGGL(kv_append_rope_paged_kernel<float>, grid, block, 0, s, p, total); break;
    case DType::BF16: hipLaunchKernelGGL(kv_append_rope_paged_kernel<BF16>, grid, block, 0, s, p, total); break;
    case DType::F16: hipLaunchKernelGGL(kv_append_rope_paged_kernel<F16>, grid, block, 0, s, p, total); break;
  }
}

}  // namespace cs336
