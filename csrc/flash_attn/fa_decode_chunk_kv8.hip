// FP8 KV cache: multi-token (chunk) attention over e4m3 K / V rows with per-row scales. gfx950,
// wave64. The sibling of fa_decode_chunk.hip on the format of fa_decode_kv8.h, and the n-query form
// of fa_decode_kv8.hip: q (B, n, H, D), kv_len[b] counts the keys after the chunk's own rows were
// appended, query i sees keys [0, kv_len[b] - (n - 1 - i)) clamped to [0, max_len].
//
// fa_decode_chunk's algorithm in the body shared with fa_decode_kv8 (kv8_attention, fa_decode_kv8.h):
// a workgroup owns 4 consecutive queries of one (b, h, split) and applies every loaded row to all of
// them; per-query masks as a bit select; split over keys with fp32 partials merged by
// fa_decode_chunk.hip's merge launch (fa_decode_chunk_merge). There is no 8-query tile: at 16 elements
// per lane a query costs 34 registers, so n > 4 runs ceil(n / 4) query tiles (a grid dimension), each
// reading the half-size rows once. n == 1 is fa_decode_kv8's kernel: (B, 1, H, D) is its (B, H, D).
// The chunk's rows are appended by kv_append_rope_kv8 (fa_decode_kv8.hip).
#include "fa_decode_kv8.h"

namespace cs336 {
namespace {

constexpr int kQT = 4;

template <typename T, int D>
__global__ __launch_bounds__(kDecodeThreads) void fa_decode_chunk_kv8_kernel(const DecodeChunkKv8Params pp,
                                                                             const int qtiles) {
  kv8_attention<T, D, kQT>(pp.base, pp.sc, qtiles);
}

template <typename T, int D>
void launch_chunk(const DecodeChunkKv8Params& p, hipStream_t s) {
  const int qtiles = (p.base.n + kQT - 1) / kQT;
  const dim3 grid((unsigned)((int64_t)p.base.B * p.base.H * qtiles * p.base.splits));
  hipLaunchKernelGGL((fa_decode_chunk_kv8_kernel<T, D>), grid, dim3(kDecodeThreads), 0, s, p, qtiles);
}

template <typename T>
void launch_chunk_d(const DecodeChunkKv8Params& p, hipStream_t s) {
  switch (p.base.D) {
    case 32: launch_chunk<T, 32>(p, s); break;
    case 64: launch_chunk<T, 64>(p, s); break;
    case 80: launch_chunk<T, 80>(p, s); break;
    case 128: launch_chunk<T, 128>(p, s); break;
    default: abort();  // the binding checks the head dim
  }
}

}  // namespace

void fa_decode_chunk_kv8(const DecodeChunkKv8Params& p, DType t, hipStream_t s) {
  const DecodeChunkParams& c = p.base;
  if (c.B <= 0 || c.H <= 0 || c.n <= 0) return;
  if (c.n == 1) {  // the single-query kernel: same layout, same partials
    DecodeKv8Params one;
    DecodeParams& d = one.base;
    d.q = c.q; d.k = c.k; d.v = c.v; d.o = c.o; d.lse = c.lse; d.kv_len = c.kv_len;
    d.k_sb = c.k_sb; d.k_sh = c.k_sh; d.k_sn = c.k_sn;
    d.v_sb = c.v_sb; d.v_sh = c.v_sh; d.v_sn = c.v_sn;
    d.B = c.B; d.H = c.H; d.D = c.D; d.max_len = c.max_len;
    d.scale = c.scale;
    d.splits = c.splits; d.opart = c.opart; d.lpart = c.lpart;
    one.sc = p.sc;
    fa_decode_kv8(one, t, s);
    return;
  }
  switch (t) {
    case DType::F32: launch_chunk_d<float>(p, s); break;
    case DType::BF16: launch_chunk_d<BF16>(p, s); break;
    case DType::F16: launch_chunk_d<F16>(p, s); break;
  }
  if (c.splits > 1) fa_decode_chunk_merge(c, t, s);
}

}  // namespace cs336
