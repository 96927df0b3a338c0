// FP8 KV cache: single-token attention over e4m3 K / V rows with per-row scales, the append of new
// rows and the prefill's row store. gfx950, wave64. The sibling of fa_decode.hip on the format of
// fa_decode_kv8.h: a cached row is D e4m3 bytes plus one fp32 scale, D + 4 bytes instead of 2 D.
//
// fa_decode_kv8: fa_decode's algorithm -- row per lane group, split over keys, two register buffers
// with the next tile's loads issued before this tile's arithmetic in one basic block, DPP group sum,
// per-lane online softmax, fixed-order combines, no atomics -- in the body it shares with the chunk
// kernel (kv8_attention, fa_decode_kv8.h), as its 1-query tile. What differs from the 16-bit kernel:
//   * D/16 lanes own a row, 16 elements per lane, one 16-B load; the bytes stay packed until their
//     use, where eight v_cvt_pk_f32_fp8 convert them exactly, and the products are packed fp32;
//   * k_scale[row] multiplies the group-summed dot product once; v_scale[row] is folded into the
//     probability (acc += (p * vs) * v, l += p unscaled): two more multiplies per row and lane;
//   * each row's two scales are 4-B loads at the same address in all lanes of the group (one wave
//     load covers 64 / G consecutive fp32). A masked slot re-reads the scales of the split's last
//     valid row, as it does the row, so scales at and beyond kv_len[b] are never touched either;
//   * addresses are a uniform 64-bit base, advanced per tile, plus a 32-bit lane offset (Kv8Rows).
// The fp32 partials of splits > 1 are merged by fa_decode.hip's merge launch (fa_decode_merge).
//
// kv_append_rope_kv8: q | k | v rows in, rotated q out, the fp32 rotated k and the plain v quantized
// once into row pos[b] + i. The 16-bit append's thread-per-8-elements map has no row reduction; here
// a lane group owns a row (of q, k or v), so the row's amax is a DPP reduction. One kernel serves the
// single-token and the chunk op. kv_quantize_rows: the same quantizer over rows of a strided
// (B, H, n, D) tensor, the prefill's store. All three write rows through kv8_quantize_row, in 64-bit
// offsets.
#include "fa_decode_kv8.h"

namespace cs336 {
namespace {

template <typename T, int D>
__global__ __launch_bounds__(kDecodeThreads) void fa_decode_kv8_kernel(const DecodeKv8Params pp) {
  // one query per (batch, head): the 1-query tile of the shared body, q (B, H, D) read as (B, 1, H, D)
  const DecodeParams& s = pp.base;
  DecodeChunkParams p;
  p.q = s.q; p.k = s.k; p.v = s.v; p.o = s.o; p.lse = s.lse; p.kv_len = s.kv_len;
  p.k_sb = s.k_sb; p.k_sh = s.k_sh; p.k_sn = s.k_sn;
  p.v_sb = s.v_sb; p.v_sh = s.v_sh; p.v_sn = s.v_sn;
  p.B = s.B; p.n = 1; p.H = s.H; p.D = s.D; p.max_len = s.max_len;
  p.scale = s.scale;
  p.splits = s.splits; p.opart = s.opart; p.lpart = s.lpart;
  kv8_attention<T, D, 1>(p, pp.sc, 1);
}

// One lane group per (batch, token, q|k|v part, head) row of the fused projection rows.
template <typename T, int D>
__global__ __launch_bounds__(kDecodeThreads) void kv_append_rope_kv8_kernel(const AppendKv8Params pp, int64_t rows) {
  typedef typename Elem<T>::storage S;
  const AppendChunkParams& p = pp.base;
  constexpr int G = decode_group(D);
  constexpr int NG = kDecodeThreads / G;
  constexpr int C = D / 8;
  const int gi = threadIdx.x / G, c = threadIdx.x % G;
  const bool active = c < C;
  int64_t r = (int64_t)blockIdx.x * NG + gi;
  // (a group past the last row repeats it: the DPP reduction wants every lane, and the repeated
  // stores write the same values)
  r = r < rows ? r : rows - 1;
  const int64_t bt = r / (3 * p.H);  // b * n + token
  const int ph = (int)(r - bt * 3 * p.H);
  const int part = ph / p.H, h = ph - part * p.H;
  const int b = (int)(bt / p.n), t = (int)(bt - (int64_t)b * p.n);
  const int64_t pos = (int64_t)p.pos[b] + t;
  const bool in_range = pos >= 0 && pos < p.max_len && pos < p.ctx;
  const int col = active ? 8 * c : 0;

  Chunk8 x;
#pragma unroll
  for (int e = 0; e < 8; ++e) x.f[e] = 0.f;
  if (in_range) {  // (uniform over the group)
    x = load8<T>((const S*)p.qkv + (int64_t)b * p.qkv_sb + (int64_t)t * p.qkv_sn + (int64_t)part * p.H * D + h * D +
                 col);
    if (part < 2) {
      const int half = D / 2;
      const float4 cs = *reinterpret_cast<const float4*>(p.cos + pos * half + col / 2);
      const float4 sn = *reinterpret_cast<const float4*>(p.sin + pos * half + col / 2);
      const float cv[4] = {cs.x, cs.y, cs.z, cs.w}, sv[4] = {sn.x, sn.y, sn.z, sn.w};
      Chunk8 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        y.f[2 * e] = cv[e] * x.f[2 * e] - sv[e] * x.f[2 * e + 1];
        y.f[2 * e + 1] = sv[e] * x.f[2 * e] + cv[e] * x.f[2 * e + 1];
      }
      x = y;
    }
  }
  // every lane of the wave takes part in the reduction; a q row's and a slotless row's result is dropped
  float scale;
  const uint2 bytes = kv8_quantize_row<G>(x, active, scale);
  if (!active) return;
  if (part == 0) {
    // (a token without a slot: x is still 0, its q row is zeroed)
    store8<T>((S*)p.q_out + (bt * p.H + h) * D + 8 * c, x);
  } else if (in_range) {
    uint8_t* plane = (uint8_t*)(part == 1 ? p.k : p.v);
    float* splane = part == 1 ? pp.sc.k : pp.sc.v;
    const int64_t sb = part == 1 ? p.k_sb : p.v_sb, sh = part == 1 ? p.k_sh : p.v_sh;
    const int64_t sn_ = part == 1 ? p.k_sn : p.v_sn;
    const int64_t ssb = part == 1 ? pp.sc.k_sb : pp.sc.v_sb, ssh = part == 1 ? pp.sc.k_sh : pp.sc.v_sh;
    *reinterpret_cast<uint2*>(plane + (int64_t)b * sb + (int64_t)h * sh + pos * sn_ + 8 * c) = bytes;
    if (c == 0) splane[(int64_t)b * ssb + (int64_t)h * ssh + pos] = scale;
  }
}

// One lane group per row of x (B, H, n, D) -> row of the byte plane and its scale.
template <typename T, int D>
__global__ __launch_bounds__(kDecodeThreads) void kv_quantize_rows_kernel(const QuantizeRowsParams p, int64_t rows) {
  typedef typename Elem<T>::storage S;
  constexpr int G = decode_group(D);
  constexpr int NG = kDecodeThreads / G;
  constexpr int C = D / 8;
  const int gi = threadIdx.x / G, c = threadIdx.x % G;
  const bool active = c < C;
  int64_t r = (int64_t)blockIdx.x * NG + gi;
  r = r < rows ? r : rows - 1;  // (as in the append kernel)
  const int64_t bh = r / p.n;
  const int64_t i = r - bh * p.n;
  const int64_t b = bh / p.H, h = bh - b * p.H;
  const Chunk8 x = load8<T>((const S*)p.x + b * p.x_sb + h * p.x_sh + i * p.x_sn + (active ? 8 * c : 0));
  float scale;
  const uint2 bytes = kv8_quantize_row<G>(x, active, scale);
  if (!active) return;
  *reinterpret_cast<uint2*>((uint8_t*)p.out + b * p.o_sb + h * p.o_sh + i * p.o_sn + 8 * c) = bytes;
  if (c == 0) p.scale[b * p.s_sb + h * p.s_sh + i] = scale;
}

template <typename T, int D>
void launch_decode(const DecodeKv8Params& p, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)p.base.B * p.base.H * p.base.splits));
  hipLaunchKernelGGL((fa_decode_kv8_kernel<T, D>), grid, dim3(kDecodeThreads), 0, s, p);
}

template <typename T, int D>
void launch_append(const AppendKv8Params& p, hipStream_t s) {
  const int64_t rows = (int64_t)p.base.B * p.base.n * 3 * p.base.H;
  constexpr int NG = kDecodeThreads / decode_group(D);
  hipLaunchKernelGGL((kv_append_rope_kv8_kernel<T, D>), dim3((unsigned)((rows + NG - 1) / NG)), dim3(kDecodeThreads), 0,
                     s, p, rows);
}

template <typename T, int D>
void launch_quantize(const QuantizeRowsParams& p, hipStream_t s) {
  const int64_t rows = (int64_t)p.B * p.H * p.n;
  constexpr int NG = kDecodeThreads / decode_group(D);
  hipLaunchKernelGGL((kv_quantize_rows_kernel<T, D>), dim3((unsigned)((rows + NG - 1) / NG)), dim3(kDecodeThreads), 0,
                     s, p, rows);
}

// (the bindings check the head dim)
#define CS336_KV8_SWITCH_D(fn, T, D, p, s)        \
  switch (D) {                                    \
    case 32: fn<T, 32>(p, s); break;              \
    case 64: fn<T, 64>(p, s); break;              \
    case 80: fn<T, 80>(p, s); break;              \
    case 128: fn<T, 128>(p, s); break;            \
    default: abort();                             \
  }
#define CS336_KV8_SWITCH(fn, t, D, p, s)                            \
  switch (t) {                                                      \
    case DType::F32: CS336_KV8_SWITCH_D(fn, float, D, p, s) break;  \
    case DType::BF16: CS336_KV8_SWITCH_D(fn, BF16, D, p, s) break;  \
    case DType::F16: CS336_KV8_SWITCH_D(fn, F16, D, p, s) break;    \
  }

}  // namespace

int fa_decode_kv8_chunk_qt(int n) { return kv8_chunk_qt(n); }

int fa_decode_kv8_key_tile(int D, int n) { return kv8_tile(D, kv8_chunk_qt(n)); }

int fa_decode_kv8_splits(int B, int H, int D, int n, int max_kv_len) {
  // fa_decode_splits' rule (one workgroup per CU, at least four key tiles per split, at most 64
  // partials) over the (batch, head, query tile) rows and this format's key tile
  const int QT = kv8_chunk_qt(n);
  const int64_t rows = (int64_t)B * H * ((n + QT - 1) / QT);
  if (rows <= 0) return 1;
  const int KT = kv8_tile(D, QT);
  const int64_t tiles = ((int64_t)max_kv_len + KT - 1) / KT;
  int64_t want = (256 + rows - 1) / rows;
  if (want > tiles / 4) want = tiles / 4;
  if (want > 64) want = 64;
  if (want < 1) want = 1;
  return (int)want;
}

void fa_decode_kv8(const DecodeKv8Params& p, DType t, hipStream_t s) {
  if (p.base.B <= 0 || p.base.H <= 0) return;
  CS336_KV8_SWITCH(launch_decode, t, p.base.D, p, s)
  if (p.base.splits > 1) fa_decode_merge(p.base, t, s);
}

void kv_append_rope_kv8(const AppendKv8Params& p, DType t, hipStream_t s) {
  if ((int64_t)p.base.B * p.base.n * p.base.H <= 0) return;
  CS336_KV8_SWITCH(launch_append, t, p.base.D, p, s)
}

void kv_quantize_rows(const QuantizeRowsParams& p, DType t, hipStream_t s) {
  if ((int64_t)p.B * p.H * p.n <= 0) return;
  CS336_KV8_SWITCH(launch_quantize, t, p.D, p, s)
}

}  // namespace cs336
