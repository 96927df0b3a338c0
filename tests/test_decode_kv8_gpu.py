"""FP8 KV cache kernels on the GPU (``csrc/flash_attn/fa_decode_kv8.hip``, ``fa_decode_chunk_kv8.hip``):
attention over e4m3 K / V rows with per-row scales, the append of quantized rows and the prefill's row
store.

Attention oracle: fp64 softmax attention and LSE over ``bytes.double() * scale.double()`` of the valid
rows, from the same rounded q. The bounds are ``fa_decode``'s (``test_decode_attention_gpu.py``):
max |o - ref| < 2e-2 for 16-bit q, < 1e-4 for fp32, the same for the finite LSE entries. They carry
over because the conversion of the bytes is exact and the rest is the same fp32 arithmetic plus two
multiplies per row. Rows at and beyond ``kv_len[b]`` hold the NaN byte 0x7f and a NaN scale.

Append oracle: ``x`` is the fp64 rotation of the rounded inputs (plain V for the V part) and
``s = amax|x| / 448``. Required: ``|scale / s - 1| <= 1e-5`` and, per element,
``|byte * scale - x| <= 2^-4 |x| + 2^-10 s + 1e-4 amax`` -- three mantissa bits give half a step of
2^-4 relative, the subnormal spacing is 2^-9 in scaled units, and the last term absorbs a rounding
decision flipped by the fp32 rotation error. The row's largest element is the byte +-448, no byte is
a NaN byte, and q is within the RoPE kernel's tolerance (1e-5 fp32, 1e-2 16-bit)."""

import functools
import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"
E4M3 = torch.float8_e4m3fn
B, H, MAX_LEN = 3, 3, 320
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DIMS = [32, 64, 80, 128]
# the third at max_len 1200: the largest key tile is 512 rows (d 32), so the longest sequence spans
# more than two tiles and the two-tile steady-state loop runs at every head dim
KV_LENS = [((1, 65, 300), 320), ((64, 128, 320), 320), ((1, 1025, 1200), 1200)]
SPLITS = [0, 1, 2, 5]
NS = [1, 2, 4, 5, 8, 11]  # both query tiles (1, 4), ragged tiles, and two and three tiles of the grid dimension


def _tol(dt):
    return 2e-2 if dt != torch.float32 else 1e-4


def _u8(t):
    return t.view(torch.uint8)


def _planes(x, kv_len):
    """Reference-quantized planes of ``x`` (B, H, N, d) with NaN bytes and NaN scales from kv_len[b] on."""
    q, s = ops.kv_quantize_ref(x)
    q, s = q.clone(), s.clone()
    for b, n in enumerate(kv_len):
        _u8(q)[b, :, n:] = 0x7f
        s[b, :, n:] = float("nan")
    return q, s


def _deq64(plane, scale):
    return plane.float().double() * scale.double()[..., None]


def _oracle(q, k, v, kv_len, scale):
    """fp64 attention of each sequence over its first kv_len[b] rows only (k, v fp64)."""
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:2], float("-inf"), dtype=torch.float64, device=q.device)
    for b, n in enumerate(kv_len):
        if n == 0:
            continue
        s = torch.einsum("hd,hnd->hn", q[b].double(), k[b, :, :n]) * scale
        lse[b] = torch.logsumexp(s, -1)
        o[b] = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v[b, :, :n])
    return o, lse


def _bound(kv, n, i, max_len):
    return min(max(kv - (n - 1 - i), 0), max_len)


def _chunk_oracle(q, k, v, kv_len, scale):
    n = q.shape[1]
    o = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    lse = torch.full(q.shape[:3], float("-inf"), dtype=torch.float64, device=q.device)
    for b, kv in enumerate(kv_len):
        for i in range(n):
            L = _bound(kv, n, i, k.shape[2])
            if L == 0:
                continue
            s = torch.einsum("hd,hnd->hn", q[b, i].double(), k[b, :, :L]) * scale
            lse[b, i] = torch.logsumexp(s, -1)
            o[b, i] = torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v[b, :, :L])
    return o, lse


@functools.lru_cache(maxsize=None)
def _cache(d, kv_len, max_len, batch=B):
    """The four planes and their fp64 dequantized rows, built once per (d, lengths) and shared by every
    dtype, split count and chunk size; nothing modifies them."""
    g = torch.Generator(device=DEV).manual_seed(1234 + d)
    k8, ks = _planes(torch.randn(batch, H, max_len, d, device=DEV, generator=g), kv_len)
    v8, vs = _planes(torch.randn(batch, H, max_len, d, device=DEV, generator=g), kv_len)
    lens = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    return k8, v8, ks, vs, lens, _deq64(k8, ks), _deq64(v8, vs)


@functools.lru_cache(maxsize=None)
def _case(dt, d, kv_len, max_len, qmul=1.0, batch=B):
    k8, v8, ks, vs, lens, kd, vd = _cache(d, kv_len, max_len, batch)
    g = torch.Generator(device=DEV).manual_seed(99 + d)
    q = (torch.randn(batch, H, d, device=DEV, generator=g) * qmul).to(dt)
    ref_o, ref_l = _oracle(q, kd, vd, kv_len, 1.0 / math.sqrt(d))
    return q, k8, v8, ks, vs, lens, ref_o, ref_l


@functools.lru_cache(maxsize=None)
def _chunk_case(dt, d, n, kv_len, max_len):
    k8, v8, ks, vs, lens, kd, vd = _cache(d, kv_len, max_len)
    g = torch.Generator(device=DEV).manual_seed(77 + d + n)
    q = torch.randn(B, n, H, d, device=DEV, generator=g).to(dt)
    ref_o, ref_l = _chunk_oracle(q, kd, vd, kv_len, 1.0 / math.sqrt(d))
    return q, k8, v8, ks, vs, lens, ref_o, ref_l


def _check(o, lse, ref_o, ref_l, dt, what=""):
    assert o.dtype == dt and lse.dtype == torch.float32
    assert o.shape == ref_o.shape and lse.shape == ref_l.shape
    assert torch.isfinite(o).all(), what
    eo = (o.double() - ref_o).abs().max().item()
    fin = torch.isfinite(ref_l)
    assert torch.equal(torch.isfinite(lse), fin), what
    assert (lse[~fin] < 0).all(), what
    assert torch.equal(o[~fin], torch.zeros_like(o[~fin])), what  # no key: o = 0
    el = (lse.double()[fin] - ref_l[fin]).abs().max().item() if fin.any() else 0.0
    print(f"{what} max|o-ref| {eo:.3e} max|lse-ref| {el:.3e}")
    assert eo < _tol(dt), (what, eo)
    assert el < _tol(dt), (what, el)


def test_extension_has_kv8_ops_and_exports_its_tile():
    assert _ext.load_ext(), _ext.load_error()
    hip = torch.ops.cs336
    for name in ("fa_decode_kv8", "fa_decode_chunk_kv8", "kv_append_rope_kv8", "kv_append_rope_chunk_kv8",
                 "kv_quantize_rows"):
        assert hasattr(hip, name), name
    # 256 / (d / 16 lanes per row) groups, 4 rows per group and tile (2 at the 4-query tile of n > 1)
    assert [int(hip.fa_decode_kv8_key_tile(d, 1)) for d in DIMS] == [512, 256, 128, 128]
    assert [int(hip.fa_decode_kv8_key_tile(d, 4)) for d in DIMS] == [256, 128, 64, 64]
    assert [int(hip.fa_decode_kv8_key_tile(d, 9)) for d in DIMS] == [256, 128, 64, 64]
    assert max(int(hip.fa_decode_kv8_key_tile(d, 1)) for d in DIMS) * 2 < 1200
    # at least four key tiles per split, one workgroup per CU, at most 64 partials
    assert int(hip.fa_decode_kv8_splits(1, 25, 64, 1, 16384)) == 11
    assert int(hip.fa_decode_kv8_splits(1, 25, 64, 1, 2048)) == 2
    assert int(hip.fa_decode_kv8_splits(1, 25, 64, 1, 512)) == 1
    assert int(hip.fa_decode_kv8_splits(1, 1, 128, 1, 1 << 20)) == 64


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("kv_len,max_len", KV_LENS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_decode_attention_grid(dt, d, kv_len, max_len, splits):
    q, k8, v8, ks, vs, lens, ref_o, ref_l = _case(dt, d, kv_len, max_len)
    o, lse = ops.decode_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} {kv_len} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("dt", DTYPES)
def test_peaky(dt, splits):
    """q x 8: a softmax dominated by a few keys (scores of +-30) stays finite and within tolerance."""
    q, k8, v8, ks, vs, lens, ref_o, ref_l = _case(dt, 64, *KV_LENS[0], 8.0)
    o, lse = ops.decode_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    _check(o, lse, ref_o, ref_l, dt, f"peaky {dt} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 1, 5])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_empty_sequence(dt, splits):
    q, k8, v8, ks, vs, lens, ref_o, ref_l = _case(dt, 64, (0, 7), MAX_LEN, batch=2)
    o, lse = ops.decode_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    assert not torch.isnan(o).any() and not torch.isnan(lse).any()
    assert torch.equal(o[0], torch.zeros_like(o[0]))
    assert torch.isinf(lse[0]).all() and (lse[0] < 0).all()
    _check(o, lse, ref_o, ref_l, dt, f"empty {dt} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
@pytest.mark.parametrize("d", [64, 80])
def test_strided_cache_views_bitwise(d, splits):
    """A layer slice of (L, B, H, max_len, d) / (L, B, H, max_len) planes and a batch sub-view are read
    in place and give the bits of the contiguous call."""
    dt = torch.bfloat16
    q, k8, v8, ks, vs, lens, ref_o, ref_l = _case(dt, d, *KV_LENS[0])
    o0, l0 = ops.decode_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    big = [torch.full((2, *t.shape), 0x7f, device=DEV, dtype=torch.uint8).view(E4M3) for t in (k8, v8)]
    bigs = [torch.full((2, *t.shape), float("nan"), device=DEV) for t in (ks, vs)]
    for dst, src in zip(big + bigs, (k8, v8, ks, vs)):
        dst[1].copy_(src)
    o1, l1 = ops.decode_attention(q, big[0][1], big[1][1], lens, splits=splits, k_scale=bigs[0][1], v_scale=bigs[1][1])
    assert torch.equal(o1, o0) and torch.equal(l1, l0)
    sub = [t[1:3] for t in (q, k8, v8, lens, ks, vs)]
    assert not sub[1].is_contiguous() or sub[1].data_ptr() != k8.data_ptr()
    o2, l2 = ops.decode_attention(*sub[:4], splits=splits, k_scale=sub[4], v_scale=sub[5])
    cl = [t.clone() for t in sub]
    o3, l3 = ops.decode_attention(*cl[:4], splits=splits, k_scale=cl[4], v_scale=cl[5])
    assert torch.equal(o2, o3) and torch.equal(l2, l3)
    _check(o2, l2, ref_o[1:3], ref_l[1:3], dt, f"batch sub-view d{d} splits {splits}:")


@pytest.mark.parametrize("splits", [0, 5])
def test_run_to_run_bitwise(splits):
    q, k8, v8, ks, vs, lens, _, _ = _case(torch.bfloat16, 128, *KV_LENS[2])
    o0, l0 = ops.decode_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    o1, l1 = ops.decode_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    qc = _chunk_case(torch.bfloat16, 128, 5, *KV_LENS[2])[0]
    a = ops.decode_attention_chunk(qc, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    b = ops.decode_attention_chunk(qc, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_64bit_cache_offsets():
    """Head 1 of a (1, 2, 2^24 + 16, 128) byte plane starts beyond a 2 GiB byte offset."""
    d, n, max_len = 128, 300, 2**24 + 16
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(7)
    k8 = torch.empty(1, 2, max_len, d, device=DEV, dtype=torch.uint8).view(E4M3)
    v8 = torch.empty(1, 2, max_len, d, device=DEV, dtype=torch.uint8).view(E4M3)
    ks = torch.empty(1, 2, max_len, device=DEV)
    vs = torch.empty(1, 2, max_len, device=DEV)
    assert k8.stride(1) * k8.element_size() > 2**31
    for p8, sc in ((k8, ks), (v8, vs)):
        xq, xs = ops.kv_quantize_ref(torch.randn(1, 2, n, d, device=DEV, generator=g))
        _u8(p8)[:, :, :n] = _u8(xq)
        sc[:, :, :n] = xs
    q = torch.randn(1, 2, d, device=DEV, generator=g).to(dt)
    lens = torch.tensor([n], dtype=torch.int32, device=DEV)
    ref_o, ref_l = _oracle(q, _deq64(k8[:, :, :n], ks[:, :, :n]), _deq64(v8[:, :, :n], vs[:, :, :n]), (n,),
                           1.0 / math.sqrt(d))
    for splits in (0, 1):  # 0: the host sizes the split count from max_kv_len = max_len
        o, lse = ops.decode_attention(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
        _check(o, lse, ref_o, ref_l, dt, f"64-bit splits {splits}:")
    o, lse = ops.decode_attention(q, k8, v8, lens, max_kv_len=n, k_scale=ks, v_scale=vs)
    _check(o, lse, ref_o, ref_l, dt, "64-bit max_kv_len 300:")
    oc, lc = ops.decode_attention_chunk(q[:, None], k8, v8, lens, max_kv_len=n, k_scale=ks, v_scale=vs)
    _check(oc[:, 0], lc[:, 0], ref_o, ref_l, dt, "64-bit chunk n 1:")


def _chunk_grid():
    """Every (d, n) with the dtype, lengths and split count rotating, so that every value of every axis
    meets every head dim."""
    cases = []
    for di, d in enumerate(DIMS):
        for ni, n in enumerate(NS):
            for j in range(2):
                i = 2 * ni + j + di
                cases.append((d, DTYPES[i % 3], n, KV_LENS[(i // 2) % 3], SPLITS[(i + i // 4) % 4]))
        mine = [c for c in cases if c[0] == d]
        assert {c[1] for c in mine} == set(DTYPES) and {c[4] for c in mine} == set(SPLITS)
        assert {c[3] for c in mine} == set(KV_LENS)
    return cases


@pytest.mark.parametrize("d,dt,n,kv,splits", _chunk_grid())
def test_decode_attention_chunk_grid(d, dt, n, kv, splits):
    kv_len, max_len = kv
    q, k8, v8, ks, vs, lens, ref_o, ref_l = _chunk_case(dt, d, n, kv_len, max_len)
    o, lse = ops.decode_attention_chunk(q, k8, v8, lens, splits=splits, k_scale=ks, v_scale=vs)
    _check(o, lse, ref_o, ref_l, dt, f"{dt} d{d} n{n} {kv_len} splits {splits}:")


@pytest.mark.parametrize("n", [4, 11])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_chunk_query_matches_the_single_query_kernel(dt, n):
    """Query i of an n-chunk against ``decode_attention`` of that query over its own key count on the
    same cache: within the bound both are held to against the oracle."""
    kv_len, max_len = KV_LENS[1]
    q, k8, v8, ks, vs, lens, _, _ = _chunk_case(dt, 64, n, kv_len, max_len)
    o, lse = ops.decode_attention_chunk(q, k8, v8, lens, k_scale=ks, v_scale=vs)
    for i in range(n):
        li = torch.tensor([_bound(kv, n, i, max_len) for kv in kv_len], dtype=torch.int32, device=DEV)
        o1, l1 = ops.decode_attention(q[:, i].contiguous(), k8, v8, li, k_scale=ks, v_scale=vs)
        assert (o[:, i].double() - o1.double()).abs().max().item() < _tol(dt), i
        assert (lse[:, i].double() - l1.double()).abs().max().item() < _tol(dt), i


def test_unsupported_inputs():
    q, k8, v8, ks, vs, lens, _, _ = _case(torch.bfloat16, 64, *KV_LENS[0])
    hip = torch.ops.cs336
    with pytest.raises(RuntimeError):  # a 16-bit cache is the other op's
        hip.fa_decode_kv8(q, k8.to(torch.bfloat16), v8.to(torch.bfloat16), ks, vs, lens, 0.1, 300, 0)
    with pytest.raises(RuntimeError):  # scale planes of another shape
        hip.fa_decode_kv8(q, k8, v8, ks[:, :, :100], vs, lens, 0.1, 300, 0)
    with pytest.raises(RuntimeError):
        hip.fa_decode_kv8(q, k8, v8, ks, vs, lens, 0.1, MAX_LEN + 1, 0)
    with pytest.raises(ValueError):
        ops.decode_attention(q, k8, v8, lens)
    with pytest.raises(ValueError):
        ops.decode_attention(q, k8.to(torch.bfloat16), v8.to(torch.bfloat16), lens, k_scale=ks, v_scale=vs)
    # other head dims run the reference
    c = [t[..., :48].contiguous() for t in (q, k8, v8)]
    o, _ = ops.decode_attention(c[0], c[1], c[2], lens, k_scale=ks, v_scale=vs)
    assert o.shape == (B, H, 48) and torch.isfinite(o).all()


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert _ext.load_ext(), _ext.load_error()
    with FakeTensorMode():
        q = torch.empty(2, 5, 80, device=DEV, dtype=torch.bfloat16)
        cache = torch.empty(3, 2, 5, 40, 80, device=DEV, dtype=E4M3)
        sc = torch.empty(3, 2, 5, 40, device=DEV)
        lens = torch.empty(2, device=DEV, dtype=torch.int32)
        o, lse = torch.ops.cs336.fa_decode_kv8(q, cache[1], cache[2], sc[1], sc[2], lens, 0.1, 40, 0)
        assert o.shape == (2, 5, 80) and o.dtype == torch.bfloat16 and lse.shape == (2, 5)
        o, lse = torch.ops.cs336.fa_decode_chunk_kv8(q[:, None].expand(2, 3, 5, 80), cache[1], cache[2], sc[1], sc[2],
                                                     lens, 0.1, 40, 0)
        assert o.shape == (2, 3, 5, 80) and lse.shape == (2, 3, 5) and lse.dtype == torch.float32
        qkv = torch.empty(2, 3 * 5 * 80, device=DEV, dtype=torch.bfloat16)
        cs = torch.empty(40, 40, device=DEV, dtype=torch.float32)
        qo = torch.ops.cs336.kv_append_rope_kv8(qkv, cs, cs, lens, cache[1], cache[2], sc[1], sc[2])
        assert qo.shape == (2, 5, 80) and qo.dtype == torch.bfloat16
        qo = torch.ops.cs336.kv_append_rope_chunk_kv8(qkv[:, None].expand(2, 4, 1200), cs, cs, lens, cache[1],
                                                      cache[2], sc[1], sc[2])
        assert qo.shape == (2, 4, 5, 80)


# ---------------------------------------------------------------------------------------------
# append and quantize kernels
# ---------------------------------------------------------------------------------------------
def _sentinel_planes(d, max_len, layers=2):
    k = torch.full((layers, B, H, max_len, d), 0x7f, device=DEV, dtype=torch.uint8).view(E4M3)
    return k, k.clone(), torch.full((layers, B, H, max_len), float("nan"), device=DEV), torch.full(
        (layers, B, H, max_len), float("nan"), device=DEV)


def _rope64(x, cos, sin, pos):
    """fp64 rotation of x (B, H, n, d) at pos (B, n)."""
    return ops.rope_ref(x.double(), cos.double(), sin.double(), pos[:, None, :])


def _check_rows(bytes_, scale, x, what):
    """bytes_ (..., d) e4m3 and scale (...) of the rows whose exact values are x (..., d) fp64."""
    b8 = _u8(bytes_)
    assert not ((b8 & 0x7f) == 0x7f).any(), what
    amax = x.abs().amax(dim=-1)
    s = amax / 448.0
    assert ((scale.double() / s - 1).abs() <= 1e-5).all(), what
    val = bytes_.float().double()
    err = (val * scale.double()[..., None] - x).abs()
    bound = 2.0 ** -4 * x.abs() + (2.0 ** -10 * s + 1e-4 * amax)[..., None]
    assert (err <= bound).all(), (what, (err - bound).max().item())
    big = x.abs().argmax(dim=-1, keepdim=True)
    assert torch.equal(val.gather(-1, big), torch.sign(x.gather(-1, big)) * 448.0), what


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_append(dt, d, n):
    """The single append (n == 1) and the chunk append against the fp64 rotation; slots beyond the cache
    store nothing to any plane; the planes are layer slices of larger tensors."""
    from cs336_systems.models import RotaryEmbedding

    max_len = 16
    g = torch.Generator(device=DEV).manual_seed(d + n)
    re = RotaryEmbedding(max_len, d, 10000.0).to(DEV)
    qkv = torch.randn(B, n, 3 * H * d, device=DEV, generator=g).to(dt)
    k8, v8, ks, vs = _sentinel_planes(d, max_len)
    pos_l = [0, 7, 16 - max(n - 2, 1)]  # the last sequence: n == 1 fits, n == 5 has two tokens without a slot
    pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
    if n == 1:
        q = ops.kv_append_rope(qkv[:, 0], re.cos, re.sin, pos, k8[1], v8[1], k_scale=ks[1], v_scale=vs[1])[:, None]
    else:
        q = ops.kv_append_rope_chunk(qkv, re.cos, re.sin, pos, k8[1], v8[1], k_scale=ks[1], v_scale=vs[1])
    assert q.shape == (B, n, H, d) and q.dtype == dt and q.is_contiguous()
    q_in, k_in, v_in = (t.transpose(1, 2) for t in qkv.view(B, n, 3, H, d).unbind(2))  # (B, H, n, d)
    slot = pos.long()[:, None] + torch.arange(n, device=DEV)[None, :]
    ok = slot < max_len
    p = slot.clamp(max=max_len - 1)
    tol = 1e-5 if dt == torch.float32 else 1e-2
    q_ref = _rope64(q_in, re.cos, re.sin, p).transpose(1, 2) * ok[:, :, None, None]
    torch.testing.assert_close(q.double(), q_ref, rtol=tol, atol=tol)
    k_ref = _rope64(k_in, re.cos, re.sin, p)
    wrote = torch.zeros(2, B, H, max_len, dtype=torch.bool, device=DEV)
    for b in range(B):
        for i in range(n):
            if not ok[b, i]:
                continue
            r = int(slot[b, i])
            wrote[1, b, :, r] = True
            _check_rows(k8[1, b, :, r], ks[1, b, :, r], k_ref[b, :, i], f"k {dt} d{d} b{b} i{i}")
            _check_rows(v8[1, b, :, r], vs[1, b, :, r], v_in[b, :, i].double(), f"v {dt} d{d} b{b} i{i}")
    assert wrote[1].sum() == H * int(ok.sum()) and bool(ok.all()) == (n == 1)
    for p8, sc in ((k8, ks), (v8, vs)):
        assert (_u8(p8)[~wrote] == 0x7f).all() and sc[~wrote].isnan().all()
        assert not sc[wrote].isnan().any()


def test_append_out_of_range_writes_nothing():
    from cs336_systems.models import RotaryEmbedding

    d, max_len = 64, 16
    re = RotaryEmbedding(max_len, d, 10000.0).to(DEV)
    qkv = torch.randn(B, 2, 3 * H * d, device=DEV).to(torch.bfloat16)
    k8, v8, ks, vs = _sentinel_planes(d, max_len)
    for pos_l in ([16, -2, 1000], [-5, 17, 2**31 - 2]):  # (no token of the 2-token chunk has a slot either)
        pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
        q = ops.kv_append_rope(qkv[:, 0], re.cos, re.sin, pos, k8[1], v8[1], k_scale=ks[1], v_scale=vs[1])
        qc = ops.kv_append_rope_chunk(qkv, re.cos, re.sin, pos, k8[1], v8[1], k_scale=ks[1], v_scale=vs[1])
        assert not q.any() and not qc.any()
        assert (_u8(k8) == 0x7f).all() and (_u8(v8) == 0x7f).all() and ks.isnan().all() and vs.isnan().all()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_append_chunk_single_and_quantize_rows_agree_bitwise(dt, d):
    """One row quantizer: the chunk append against n single appends, ``kv_quantize_rows`` against the V
    part of the append on the same rows, and against itself on a transposed view."""
    from cs336_systems.models import RotaryEmbedding

    n, max_len = 5, 16
    g = torch.Generator(device=DEV).manual_seed(3 * d)
    re = RotaryEmbedding(max_len, d, 10000.0).to(DEV)
    qkv = torch.randn(B, n, 3 * H * d, device=DEV, generator=g).to(dt)
    qkv[0, 1, 2 * H * d:2 * H * d + d] = 0.0  # an all-zero V row: scale 1, zero bytes
    pos = torch.tensor([0, 7, 13], dtype=torch.int32, device=DEV)
    a, b = _sentinel_planes(d, max_len), _sentinel_planes(d, max_len)
    qa = ops.kv_append_rope_chunk(qkv, re.cos, re.sin, pos, a[0][1], a[1][1], k_scale=a[2][1], v_scale=a[3][1])
    qb = torch.stack([ops.kv_append_rope(qkv[:, i], re.cos, re.sin, pos + i, b[0][1], b[1][1], k_scale=b[2][1],
                                         v_scale=b[3][1]) for i in range(n)], dim=1)
    assert torch.equal(qa, qb)
    for x, y in zip(a, b):
        if x.dtype == E4M3:
            assert torch.equal(_u8(x), _u8(y))
        else:
            assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(0.0), y.nan_to_num(0.0))
    assert a[3][1, 0, 0, 1] == 1.0 and not _u8(a[1])[1, 0, 0, 1].any()
    # the V rows of sequence 0 and 1 (all n tokens have slots) through kv_quantize_rows
    v_view = qkv.view(B, n, 3, H, d)[:, :, 2].transpose(1, 2)  # (B, H, n, d), as the prefill passes it
    assert not v_view.is_contiguous()
    c8, _, cs, _ = _sentinel_planes(d, max_len, layers=1)
    ops.kv_quantize_rows(v_view, c8[0], cs[0])
    e8, _, es, _ = _sentinel_planes(d, max_len, layers=1)
    ops.kv_quantize_rows(v_view.contiguous(), e8[0], es[0])
    assert torch.equal(_u8(c8), _u8(e8)) and torch.equal(cs[0, :, :, :n], es[0, :, :, :n])
    assert (_u8(c8)[0, :, :, n:] == 0x7f).all() and cs[0, :, :, n:].isnan().all()
    for bi, p in ((0, 0), (1, 7)):
        assert torch.equal(_u8(c8)[0, bi, :, :n], _u8(a[1])[1, bi, :, p:p + n])
        assert torch.equal(cs[0, bi, :, :n], a[3][1, bi, :, p:p + n])


@pytest.mark.parametrize("dt", DTYPES)
def test_quantize_rows_is_the_reference_quantizer_bitwise(dt):
    """With no rotation in the way the kernel and the eager reference do the same fp32 arithmetic --
    amax, one correctly rounded division for the scale and one per element, clamp, RNE -- on the same
    values, so bytes and scales are equal bit for bit (extreme rows included)."""
    d = 80
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(B, H, 9, d, device=DEV, generator=g)
    x[0, 0, 0] = 0.0
    x[0, 0, 1, 3] *= 1e4
    x[0, 0, 2] = 1e-30 if dt != torch.float16 else 1e-7
    x[0, 0, 3] *= 1e4
    x = x.to(dt)
    p8, _, sc, _ = _sentinel_planes(d, 16, layers=1)
    ops.kv_quantize_rows(x, p8[0], sc[0])
    rq, rs = ops.kv_quantize_ref(x)
    assert torch.equal(sc[0, :, :, :9], rs) and torch.equal(_u8(p8)[0, :, :, :9], _u8(rq))
    assert not ((_u8(p8)[0, :, :, :9] & 0x7f) == 0x7f).any()
    assert sc[0, 0, 0, 0] == 1.0 and not _u8(p8)[0, 0, 0, 0].any()
