"""FP8 KV cache on the CPU (fp32 model, eager reference ops): the reference row quantizer, the four
planes of ``KVCache(fp8=True)``, the argument errors, the chunk append against single appends and the
model paths (prefill, single steps, a chunk step, ``generate``, ``DecodeGraph(capture=False)``) on the
tiny 2-layer model of ``test_decode_graph.py``.

Dequantized error bound of a row with scale ``s = amax / 448``: e4m3 has three mantissa bits, so a
normal value rounds within half a step, ``2^-4`` relative; below the smallest normal (``2^-6`` in
scaled units) the spacing is ``2^-9``, half of it ``2^-10 * s`` absolute. The fp32 division and
product add a few fp32 ulps: ``|byte * s - x| <= 2^-4 |x| + 2^-10 s + 1e-6 amax``."""

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph
from cs336_systems.models.kv_cache import KVCache

E4M3 = torch.float8_e4m3fn
CFG = dict(vocab_size=101, context_length=32, d_model=64, num_layers=2, num_heads=4, d_ff=96, rope_theta=10000.0)


def _rows():
    torch.manual_seed(0)
    x = torch.randn(40, 64)
    x[0] = 0.0  # an all-zero row
    x[1, 5] *= 1e4  # one element 1e4 times the rest
    x[2] = 1e-30
    x[3] = -1e-30
    x[4] *= 1e20
    x[5, :] = 0.0
    x[5, 7] = -3.0  # a single non-zero element
    return x


def test_reference_quantizer():
    x = _rows()
    q, s = ops.kv_quantize_ref(x)
    assert q.dtype == E4M3 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == (40,)
    b = q.view(torch.uint8)
    assert s[0] == 1.0 and not b[0].any()
    assert not ((b & 0x7f) == 0x7f).any()  # no NaN byte
    amax = x.abs().amax(dim=-1)
    assert torch.equal(s[1:], amax[1:] / 448.0)
    big = x.abs().argmax(dim=-1)
    top = q.float().gather(1, big[:, None])[:, 0]
    assert torch.equal(top[1:], torch.sign(x.gather(1, big[:, None])[:, 0])[1:] * 448.0)
    deq = ops.kv_dequantize(q, s)
    err = (deq.double() - x.double()).abs()
    bound = 2.0 ** -4 * x.double().abs() + (2.0 ** -10 * s.double() + 1e-6 * amax.double())[:, None]
    assert (err <= bound).all(), (err - bound).max()
    # bf16 and fp16 rows are quantized from their fp32 values
    for dt in (torch.bfloat16, torch.float16):
        xh = torch.randn(8, 32).to(dt)
        qh, sh = ops.kv_quantize_ref(xh)
        q32, s32 = ops.kv_quantize_ref(xh.float())
        assert torch.equal(qh.view(torch.uint8), q32.view(torch.uint8)) and torch.equal(sh, s32)


def test_kv_quantize_rows_writes_the_first_rows_only():
    torch.manual_seed(1)
    x = torch.randn(2, 3, 5, 32)
    plane = torch.full((2, 3, 9, 32), 0x7f, dtype=torch.uint8).view(E4M3)
    scale = torch.full((2, 3, 9), float("nan"))
    ops.kv_quantize_rows(x.transpose(1, 2).contiguous().transpose(1, 2), plane, scale)  # a (B, n, H, d) view
    q, s = ops.kv_quantize_ref(x)
    assert torch.equal(plane.view(torch.uint8)[:, :, :5], q.view(torch.uint8)) and torch.equal(scale[:, :, :5], s)
    assert (plane.view(torch.uint8)[:, :, 5:] == 0x7f).all() and scale[:, :, 5:].isnan().all()
    with pytest.raises(ValueError):
        ops.kv_quantize_rows(x, torch.zeros(2, 3, 9, 32), scale)
    with pytest.raises(ValueError):
        ops.kv_quantize_rows(torch.randn(2, 3, 10, 32), plane, scale)


def test_cache_planes_and_bookkeeping():
    c = KVCache((2, 4, 16), 3, max_len=32, dtype=torch.bfloat16, fp8=True)
    assert c.fp8 and c.dtype == torch.bfloat16
    assert c.k.shape == c.v.shape == (2, 3, 4, 32, 16) and c.k.dtype == c.v.dtype == E4M3
    assert c.k_scale.shape == c.v_scale.shape == (2, 3, 4, 32) and c.k_scale.dtype == c.v_scale.dtype == torch.float32
    assert c.nbytes == 2 * 3 * 4 * 32 * (16 + 4) * 2
    assert "e4m3" in repr(c) and "bfloat16" in repr(c)
    p = KVCache((2, 4, 16), 3, max_len=32, dtype=torch.bfloat16)
    assert not p.fp8 and p.k_scale is None and p.v_scale is None and p.dtype == torch.bfloat16
    assert p.nbytes == 2 * 3 * 4 * 32 * 16 * 2 * 2 and "e4m3" not in repr(p)
    # the ratio at the head dims the kernels take: (d + 4) / 2d
    for d, lo, hi in ((64, 0.52, 0.56), (128, 0.51, 0.52)):
        a, b = KVCache((1, 1, d), 1, max_len=8, dtype=torch.bfloat16, fp8=True), KVCache((1, 1, d), 1, max_len=8, dtype=torch.bfloat16)
        assert lo <= a.nbytes / b.nbytes <= hi
    c.advance(7)
    assert c.length == 7 and c.lengths.tolist() == [7, 7, 7]
    c.truncate(4)
    assert c.length == 4 and c.lengths.tolist() == [4, 4, 4]
    with pytest.raises(ValueError):
        c.truncate(5)
    c.reset()
    assert c.length == 0 and c.lengths.tolist() == [0, 0, 0]


def test_error_paths():
    torch.manual_seed(2)
    B, H, N, d = 2, 2, 8, 32
    q = torch.randn(B, H, d)
    k8 = torch.zeros(B, H, N, d, dtype=torch.uint8).view(E4M3)
    v8 = k8.clone()
    sc = torch.ones(B, H, N)
    k16, v16 = torch.zeros(B, H, N, d), torch.zeros(B, H, N, d)
    lens = torch.tensor([3, 8], dtype=torch.int32)
    pos = torch.tensor([3, 7], dtype=torch.int32)
    cos, sin = torch.ones(N, d // 2), torch.zeros(N, d // 2)
    qkv = torch.randn(B, 3 * H * d)
    calls = [
        lambda k, v, **s: ops.decode_attention(q, k, v, lens, **s),
        lambda k, v, **s: ops.decode_attention_chunk(q[:, None], k, v, lens, **s),
        lambda k, v, **s: ops.kv_append_rope(qkv, cos, sin, pos, k, v, **s),
        lambda k, v, **s: ops.kv_append_rope_chunk(qkv[:, None], cos, sin, pos, k, v, **s),
    ]
    for call in calls:
        with pytest.raises(ValueError, match="needs k_scale and v_scale"):
            call(k8, v8)
        with pytest.raises(ValueError, match="needs k_scale and v_scale"):
            call(k8, v8, k_scale=sc)
        with pytest.raises(ValueError, match="go with a float8_e4m3fn cache"):
            call(k16, v16, k_scale=sc, v_scale=sc)
        with pytest.raises(ValueError):
            call(k8, v8, k_scale=sc[:, :, :4], v_scale=sc)
        call(k8, v8, k_scale=sc, v_scale=sc.clone())  # (and the well-formed call runs)
    m = BasicsTransformerLM(**CFG).eval()
    with pytest.raises(ValueError, match="use_cache"):
        m.generate(torch.randint(0, 101, (1, 4)), 2, kv_fp8=True)
    with pytest.raises(ValueError, match="use_cache"):
        m.generate(torch.randint(0, 101, (1, 4)), 2, top_k=1, draft=m, kv_fp8=True)


def _planes(B, H, N, d):
    k = torch.full((B, H, N, d), 0x7f, dtype=torch.uint8).view(E4M3)
    return k, k.clone(), torch.full((B, H, N), float("nan")), torch.full((B, H, N), float("nan"))


def test_chunk_append_equals_single_appends_bitwise():
    torch.manual_seed(3)
    B, H, N, d, n = 3, 2, 16, 32, 5
    theta = torch.arange(N)[:, None] * (10000.0 ** (-torch.arange(0, d, 2) / d))[None, :]
    cos, sin = theta.cos(), theta.sin()
    qkv = torch.randn(B, n, 3 * H * d)
    pos = torch.tensor([0, 9, 13], dtype=torch.int32)  # the last sequence runs out of slots after 3 tokens
    a, b = _planes(B, H, N, d), _planes(B, H, N, d)
    qa = ops.kv_append_rope_chunk(qkv, cos, sin, pos, a[0], a[1], k_scale=a[2], v_scale=a[3])
    qb = torch.stack([ops.kv_append_rope(qkv[:, i], cos, sin, pos + i, b[0], b[1], k_scale=b[2], v_scale=b[3])
                      for i in range(n)], dim=1)
    assert torch.equal(qa, qb)
    for x, y in zip(a, b):
        if x.dtype == E4M3:
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        else:
            assert torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(0.0), y.nan_to_num(0.0))
    # written: rows pos .. pos + n - 1 that exist; everything else untouched
    wrote = torch.zeros(B, N, dtype=torch.bool)
    for bi, p in enumerate(pos.tolist()):
        wrote[bi, p:min(p + n, N)] = True
    assert torch.equal(~a[2].isnan(), wrote[:, None, :].expand(B, H, N))
    assert torch.equal((a[0].view(torch.uint8) != 0x7f).any(dim=-1), wrote[:, None, :].expand(B, H, N))
    # the q rows are the plain append's, and the K rows its rotated rows quantized once from fp32
    k16, v16 = torch.zeros(B, H, N, d), torch.zeros(B, H, N, d)
    q16 = ops.kv_append_rope_chunk(qkv, cos, sin, pos, k16, v16)
    assert torch.equal(qa, q16)
    kq, ks = ops.kv_quantize_ref(k16)
    sel = wrote[:, None, :].expand(B, H, N)
    assert torch.equal(a[0].view(torch.uint8)[sel], kq.view(torch.uint8)[sel]) and torch.equal(a[2][sel], ks[sel])


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return BasicsTransformerLM(**CFG).eval()


def _teacher_forced(m, seq, cache):
    """Prefill 5, single steps to 20, one chunk step of 6, single steps to the end: logits (B, 32, V)."""
    out = [m.forward_cached(seq[:, :5], cache)]
    for n in range(5, 20):
        out.append(m.forward_cached(seq[:, n:n + 1], cache))
    out.append(m.forward_cached(seq[:, 20:26], cache, chunk=True))
    for n in range(26, 32):
        out.append(m.forward_cached(seq[:, n:n + 1], cache))
    return torch.cat(out, dim=1)


def test_model_paths_with_an_fp8_cache(model):
    m = model
    torch.manual_seed(4)
    seq = torch.randint(0, 101, (3, 32))
    plain, fp8 = KVCache(m, 3), KVCache(m, 3, fp8=True)
    assert fp8.dtype == torch.float32 and fp8.nbytes * 2 < plain.nbytes  # (fp32 rows: (d + 4) / 4d)
    with torch.no_grad():
        ref = _teacher_forced(m, seq, plain)
        got = _teacher_forced(m, seq, fp8)
        full = m(seq)
    assert fp8.length == 32 and fp8.lengths.tolist() == [32] * 3
    assert got.shape == ref.shape == (3, 32, 101) and torch.isfinite(got).all()
    assert torch.allclose(ref, full, atol=1e-4)  # (the plain cache is the exact path)
    # the prefill attends to its own unquantized K / V: its logits are the plain cache's
    assert torch.equal(got[:, :5], ref[:, :5])
    e_q = (got - ref).abs().max().item()
    print(f"e_q (fp32 model, FP8 cache against plain cache, largest logit distance): {e_q:.4e}, "
          f"largest |logit| {ref.abs().max().item():.3f}")
    assert not torch.equal(got[:, 5:], ref[:, 5:]) and e_q > 0
    assert e_q < 0.25 * ref.abs().max().item()  # quantization noise, not a wrong row
    # every cached row is a quantized row: no NaN byte, and a K row's largest byte is +-448
    assert not ((fp8.k.view(torch.uint8) & 0x7f) == 0x7f).any() and not ((fp8.v.view(torch.uint8) & 0x7f) == 0x7f).any()
    assert (fp8.k.float().abs().amax(dim=-1) == 448.0).all()
    # layer 0 sees the same inputs with either cache: its rows are the plain rows, quantized
    for p8, s8, p in ((fp8.k[0], fp8.k_scale[0], plain.k[0]), (fp8.v[0], fp8.v_scale[0], plain.v[0])):
        err = (ops.kv_dequantize(p8, s8) - p).abs()
        assert (err <= 2.0 ** -4 * p.abs() + (2.0 ** -10 * s8 + 1e-5 * p.abs().amax(dim=-1))[..., None]).all()


def test_generate_and_speculative_with_an_fp8_cache(model):
    m = model
    torch.manual_seed(5)
    x = torch.randint(0, 101, (2, 6))
    out = m.generate(x, 30, top_k=1, use_cache=True, kv_fp8=True)  # 26 cached steps, then the sliding window
    assert out.shape == (2, 30) and out.dtype == torch.int64
    # the greedy loop by hand over an FP8 cache
    cache = KVCache(m, 2, fp8=True)
    with torch.no_grad():
        logits, toks = m.forward_cached(x, cache), []
        for _ in range(26):
            toks.append(logits[:, -1].argmax(dim=-1, keepdim=True))
            logits = m.forward_cached(toks[-1], cache)
    assert torch.equal(out[:, :26], torch.cat(toks, dim=1))
    # speculative decoding with the model as its own draft: exactly greedy over the FP8 cache
    spec = m.generate(x, 20, top_k=1, use_cache=True, draft=m, draft_tokens=3, kv_fp8=True)
    assert spec.shape == (2, 20)


def test_eager_graph_step_over_an_fp8_cache_equals_forward_cached(model):
    m = model
    torch.manual_seed(6)
    seq = torch.randint(0, 101, (3, 32))
    ca, cb, cc = KVCache(m, 3, fp8=True), KVCache(m, 3, fp8=True), KVCache(m, 3, fp8=True)
    dg = DecodeGraph(m, cb, capture=False)
    dg4 = DecodeGraph(m, cc, capture=False, tokens=4)
    with torch.no_grad():
        assert torch.equal(m.forward_cached(seq[:, :5], ca), m.forward_cached(seq[:, :5], cb))
        m.forward_cached(seq[:, :5], cc)
        rows = []
        for n in range(5, 29):
            want = m.forward_cached(seq[:, n:n + 1], ca)
            rows.append(want)
            assert torch.equal(dg.step(seq[:, n:n + 1]), want), n
        for n in range(5, 29, 4):  # the chunk step writes the same rows and reads them within fp32 noise
            got = dg4.step(seq[:, n:n + 4])
            assert torch.allclose(got, torch.cat(rows[n - 5:n - 1], dim=1), atol=1e-4), n
    for x, y, z in ((ca.k, cb.k, cc.k), (ca.v, cb.v, cc.v)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        # layer 0's rows depend on the tokens alone: the chunk append writes the single append's bits
        assert torch.equal(x[0].view(torch.uint8), z[0].view(torch.uint8))
    assert torch.equal(ca.k_scale, cb.k_scale) and torch.equal(ca.v_scale, cb.v_scale)
    assert torch.equal(ca.k_scale[0], cc.k_scale[0]) and torch.equal(ca.v_scale[0], cc.v_scale[0])
    assert torch.allclose(ca.k_scale, cc.k_scale, rtol=1e-4) and torch.allclose(ca.v_scale, cc.v_scale, rtol=1e-4)
