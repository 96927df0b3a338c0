// Verify attention on the FP8 KV cache for MI355X (gfx950 / CDNA4): up to 16 new query rows per
// (batch, head) against e4m3 K / V rows with one fp32 scale per row (the format of fa_decode_kv8.h),
// streaming the half-size rows once at MFMA rate. The FP8 sibling of fa_verify.hip, and the MFMA
// sibling of fa_decode_chunk_kv8.hip (VALU, 4-query tiles that each re-read the cache).
// cs336-build: no-packed-f32 (the rescale, scale and merge loops stay single v_mul_f32 / v_fma_f32)
//
// Semantics, grid, split rule, partials and merge are fa_verify.hip's: q (B, n, H, D) bf16 / fp16,
// kv_len[b] counts the keys after the chunk's own rows were appended, query i sees keys
// [0, kv_len[b] - (n - 1 - i)) clamped to [0, max_len]; a 16-query tile per workgroup, 4 waves on
// alternating 32-key sub-tiles, split s of S takes sub-tiles [T s / S, T (s + 1) / S); S > 1 writes
// fa_decode_chunk's fp32 partials. D in {32, 64, 80, 128}. No atomics, no scratch.
//
// What the byte rows change (a row of D bytes is half a 16-bit row, so the load shapes differ):
//   * K operand. Lane (r, g) loads 16 consecutive BYTES of key row r, d = 64 i + 16 g .. + 15 of 64-wide
//     block i, straight from global memory into 4 VGPRs, and uses them for two k-steps: bytes 0-7 are
//     the lane's k indices 8 g .. 8 g + 7 of step 2 i, bytes 8-15 those of step 2 i + 1. The k order of
//     an MFMA is free as long as A and B agree: the resident Q fragment of step 2 i + s is q's
//     d = 64 i + 16 g + 8 s .. + 7. d 32 is half a block (lane groups 2, 3 hold zeros and load
//     nothing), d 80 one block plus a 16-byte tail held by lane group 0, d 128 two blocks. The bytes
//     become 16-bit operands in registers by v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0 (Act<T> of
//     gemm_skinny.h, the e4m3 weight policy's conversion): exact, two values per instruction. Two K
//     register sets are 2 x (2 x D/64 x 4 + 1) VGPRs, half the 16-bit kernel's.
//   * k_scale multiplies the fp32 score after the MFMA. The accumulator of lane (r, g) holds keys
//     4 g .. 4 g + 3 of both 16-key blocks, eight scales; they are requested as ONE dword per lane (lane
//     l: key l & 31 of the sub-tile) together with the sub-tile's K rows, two sub-tiles ahead, kept in
//     the K register set, and spread through 128 B of wave-private LDS (one write, two 16-B reads) when
//     the sub-tile is computed. The index is clamped to the range's last row like the row addresses, so
//     nothing at or beyond the range -- or the plane's end, whatever max_len is -- is read; the scores
//     of such rows are replaced by the 16-bit kernel's select.
//   * V operand. A staging lane loads 16 B = 16 elements of one row and the row's v_scale, converts to
//     fp32 (v_cvt_pk_f32_fp8, exact), multiplies by the scale, rounds once to the compute type and
//     writes two 16-B chunks of the wave-private swizzled 16-bit image; transposed reads, P packing and
//     the O^T MFMAs are then the 16-bit kernel's. The scale is applied here and not folded into P:
//     p * v_scale would fall into fp16 subnormals for rows with a small amax. d 80 has 160 chunks per
//     sub-tile: the third staging round is predicated to lanes 0-31. Rows at or beyond the range are
//     staged as zeros.
//   * Row address policy: a template parameter (Kv8Rows below, the dense planes); a paged one adds the
//     page lookup of VerifyRows<VerifyPagedParams> and nothing else.
#include "fa_verify.h"

#include "../gemm/gemm_skinny.h"  // Act<T>::lo / hi: two e4m3 bytes -> a packed pair of T

namespace cs336 {
namespace fa {

// dense planes: VerifyRows' byte-plane offsets (an e4m3 element is a byte) plus the scale planes'
struct Kv8Rows : VerifyRows<VerifyParams> {
  int64_t ks0, vs0;
  __device__ __forceinline__ Kv8Rows(const VerifyKv8Params& p, int b, int h)
      : VerifyRows<VerifyParams>(p.base, b, h), ks0((int64_t)b * p.sc.k_sb + (int64_t)h * p.sc.k_sh),
        vs0((int64_t)b * p.sc.v_sb + (int64_t)h * p.sc.v_sh) {}
  __device__ __forceinline__ int64_t ks(int key, int) const { return ks0 + key; }
  __device__ __forceinline__ int64_t vs(int key, int) const { return vs0 + key; }
};

// two fp32 values -> a packed pair of T, round to nearest even
template <typename T>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  return (uint32_t)Elem<T>::from_f(a) | ((uint32_t)Elem<T>::from_f(b) << 16);
}

// 16 e4m3 bytes times `s` -> 16 values of T (lo: elements 0-7, hi: 8-15), one rounding
template <typename T>
__device__ __forceinline__ void scale16(const uint4& raw, float s, uint4& lo, uint4& hi) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    o[2 * i] = pack2<T>(a.x * s, a.y * s);
    o[2 * i + 1] = pack2<T>(c.x * s, c.y * s);
  }
  lo = make_uint4(o[0], o[1], o[2], o[3]);
  hi = make_uint4(o[4], o[5], o[6], o[7]);
}

template <typename T, int D, typename Rows>
__global__ __launch_bounds__(256, 2) void fa_verify_kv8_kernel(const VerifyKv8Params pp, const int nqt) {
  typedef typename Elem<T>::storage S;
  static_assert(sizeof(S) == 2, "fa_verify_kv8: 16-bit q / o only");
  const VerifyParams& p = pp.base;
  constexpr int RB = PadD<D>::value * 2;  // bytes per LDS row of the 16-bit V image (d 80: 192)
  constexpr int NB = (D + 63) / 64;       // 16-B K loads per lane and key row (64-wide d blocks)
  constexpr int NKS = 2 * NB;             // k-steps of S^T
  constexpr int NDT = D / 16;             // 16-row blocks of O^T
  constexpr int BQ = 16, BK = 32;         // queries per workgroup, keys per sub-tile
  constexpr int CR8 = D / 16;             // 16-byte chunks of a cached (byte) row
  constexpr int NCH = BK * CR8;           // ... of a sub-tile's V rows
  constexpr int LPT = (NCH + 63) / 64;    // V staging rounds (d 80: the third one is half a wave)
  constexpr int VBUF = BK * RB;           // one V image
  static_assert(NDT * 1024 <= VBUF, "a wave's O state must fit its V image");

  __shared__ __attribute__((aligned(1024))) char smem[4 * VBUF];
  __shared__ __attribute__((aligned(16))) float sm_ks[4][BK];
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

  const uint8_t* Kg = (const uint8_t*)p.k;
  const uint8_t* Vg = (const uint8_t*)p.v;
  const float* KSg = pp.sc.k;
  const float* VSg = pp.sc.v;
  const Rows rows(pp, b, h);

  // ---- Q fragments (B operand), resident, in K's k order: step 2 i + s is d = 64 i + 16 g + 8 s .. +7 ----
  const int64_t orow = ((int64_t)b * p.n + qrow) * p.H + h;  // row of q, o and lse
  uint4 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int e = 64 * (ks >> 1) + 16 * g;
    qf[ks] = (valid_q && e < D) ? *reinterpret_cast<const uint4*>((const S*)p.q + orow * D + e + 8 * (ks & 1))
                                : make_uint4(0, 0, 0, 0);
  }

  // this workgroup's sub-tiles [T0, T1) of the range; this wave's are T0 + wave + 4 j, j < cnt
  const int NT = (nkeys + BK - 1) / BK;
  const int T0 = (int)((int64_t)NT * sp / nsplit), T1 = (int)((int64_t)NT * (sp + 1) / nsplit);
  const int mine = T1 - T0 - wave;
  const int cnt = mine > 0 ? (mine + 3) >> 2 : 0;
  const int last_key = nkeys - 1;

  // K has two register sets (raw bytes and the lane's k_scale dword), V one set of raw bytes and row
  // scales, free again once it is converted into the wave's image: fa_verify.hip's two load streams.
  struct KSet {
    uint4 k[2][NB];
    float ks;
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
      const uint8_t* src = Kg + rows.k(key, t ? cur.p1 : cur.p0) + 16 * g;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        if (64 * i + 64 <= D || 64 * i + 16 * g < D)
          f.k[t][i] = *reinterpret_cast<const uint4*>(src + 64 * i);
        else
          f.k[t][i] = make_uint4(0, 0, 0, 0);
      }
    }
    const int skey = min(key0 + (lane & 31), last_key);
    f.ks = KSg[rows.ks(skey, (lane & 16) ? cur.p1 : cur.p0)];
  };
  uint4 vst[LPT];
  float vsc[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    vst[i] = make_uint4(0, 0, 0, 0);
    vsc[i] = 0.f;
  }
  auto vload = [&](int j) __attribute__((always_inline)) {
    const int key0 = (T0 + wave + 4 * j) * BK;
    const Pages cur = pgv;
    if (Rows::kPaged) pgv = fetch(j + 1);
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = lane + 64 * i;
      if (64 * i + 64 <= NCH || c < NCH) {
        const int rr = c / CR8, ch = c % CR8;
        const int key = min(key0 + rr, last_key);
        const int pg = rr >= 16 ? cur.p1 : cur.p0;
        vst[i] = *reinterpret_cast<const uint4*>(Vg + rows.v(key, pg) + ch * 16);
        vsc[i] = VSg[rows.vs(key, pg)];
      }
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
  float* const Ks = sm_ks[wave];        // ... and its sub-tile's 32 k_scales

  auto tile = [&](KSet& f, int j) __attribute__((always_inline)) {
    const int key0 = (T0 + wave + 4 * j) * BK;
    // ---- V: bytes * v_scale -> T -> this wave's image (rows beyond the range: zeros); k_scale -> LDS ----
    if (key0 + BK > nkeys) {  // (wave-uniform) the range's last, partial sub-tile
#pragma unroll
      for (int i = 0; i < LPT; ++i)
        if (key0 + (lane + 64 * i) / CR8 >= nkeys) {
          vst[i] = make_uint4(0, 0, 0, 0);
          vsc[i] = 0.f;
        }
    }
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int c = lane + 64 * i;
      if (64 * i + 64 <= NCH || c < NCH) {
        const int rr = c / CR8, ch = c % CR8;
        uint4 lo, hi;
        scale16<T>(vst[i], vsc[i], lo, hi);
        *reinterpret_cast<uint4*>(Vs + lds_off<RB>(rr, 2 * ch)) = lo;
        *reinterpret_cast<uint4*>(Vs + lds_off<RB>(rr, 2 * ch + 1)) = hi;
      }
    }
    if (lane < BK) Ks[lane] = f.ks;
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
      for (int i = 0; i < NB; ++i) {
        const uint4 w = f.k[t][i];
        const uint4 k0 = make_uint4(Act<T>::lo(w.x), Act<T>::hi(w.x), Act<T>::lo(w.y), Act<T>::hi(w.y));
        const uint4 k1 = make_uint4(Act<T>::lo(w.z), Act<T>::hi(w.z), Act<T>::lo(w.w), Act<T>::hi(w.w));
        s[t] = Mma32<T>::mma(as_frag<T>(k0), as_frag<T>(qf[2 * i]), s[t]);
        s[t] = Mma32<T>::mma(as_frag<T>(k1), as_frag<T>(qf[2 * i + 1]), s[t]);
      }
    }
    // the scores' k_scales: keys 4 g .. 4 g + 3 of both 16-key blocks
    const float4 sc0 = *reinterpret_cast<const float4*>(Ks + 4 * g);
    const float4 sc1 = *reinterpret_cast<const float4*>(Ks + 16 + 4 * g);
    kload(f, j + 2);  // (this set's MFMAs are issued and its k_scale is in LDS)
    s[0][0] *= sc0.x; s[0][1] *= sc0.y; s[0][2] *= sc0.z; s[0][3] *= sc0.w;
    s[1][0] *= sc1.x; s[1][1] *= sc1.y; s[1][2] *= sc1.z; s[1][3] *= sc1.w;
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
    __builtin_amdgcn_wave_barrier();  // this image's (and the scales') reads stay before their next writes
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

  // ---- merge the four waves' states in wave order (fa_verify.hip's epilogue) ----
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
      *reinterpret_cast<uint2*>((S*)p.o + orow * D + d) =
          make_uint2(pack2<T>(acc[0] * inv, acc[1] * inv), pack2<T>(acc[2] * inv, acc[3] * inv));
    }
  }
  if (wave == 0 && g == 0 && valid_q) {
    if (nsplit > 1)
      p.lpart[prow] = lse;
    else
      p.lse[orow] = lse;
  }
}

template <typename T, int D>
void launch_verify_kv8(const VerifyKv8Params& p, hipStream_t s) {
  const int nqt = fa_verify_query_tiles(p.base.n);
  const dim3 grid((unsigned)((int64_t)nqt * p.base.B * p.base.H * p.base.splits)), block(256);
  hipLaunchKernelGGL((fa_verify_kv8_kernel<T, D, Kv8Rows>), grid, block, 0, s, p, nqt);
}

template <typename T>
void launch_verify_kv8_d(const VerifyKv8Params& p, hipStream_t s) {
  switch (p.base.D) {
    case 32: launch_verify_kv8<T, 32>(p, s); break;
    case 64: launch_verify_kv8<T, 64>(p, s); break;
    case 80: launch_verify_kv8<T, 80>(p, s); break;
    case 128: launch_verify_kv8<T, 128>(p, s); break;
    default: abort();  // the binding checks the head dim
  }
}

}  // namespace fa

// kernel, then fa_decode_chunk's merge launch over the partials (same layout)
void fa_verify_kv8(const VerifyKv8Params& pp, DType t, hipStream_t s) {
  const VerifyParams& p = pp.base;
  if (p.B <= 0 || p.H <= 0 || p.n <= 0) return;
  switch (t) {
    case DType::BF16: fa::launch_verify_kv8_d<BF16>(pp, s); break;
    case DType::F16: fa::launch_verify_kv8_d<F16>(pp, s); break;
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

}  // namespace cs336
