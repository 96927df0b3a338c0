"""FP8 weight-only decode on the CPU: the row quantizer (``ops.quantize_fp8_rows``), the op wrapper
(``ops.skinny_linear_fp8``), ``Fp8DecodeWeights`` and the ``weights=`` argument of ``DecodeGraph`` /
``generate``.

Quantizer bound, per element: ``|wq*scale - w| <= 2^-4 |w| + 2^-10 * scale``. The first term is half an
ulp of e4m3's 3-bit mantissa, the second half the subnormal spacing 2^-9 (in units of the row scale).

Model bound. ``test_decode_graph.py`` compares fp32 models bit for bit and holds no bound for a bf16
model against its exact counterpart; the project's one rule for that is the ``2 * e + ulp`` of
``test_generate_cache_gpu.py`` / ``test_decode_graph_gpu.py``, taken here as those files take it:
``e`` is the worst error of the bf16 model's ordinary forward against the exact model with the same
(bf16) weights, ``ulp`` one bf16 ulp of the largest reference logit. The quantized steps are compared
with the fp64 model loaded with the DEQUANTIZED weights, so the quantization error itself is not in
the comparison: what is left is bf16 activations and one rounding per projection, as in ``e``. For
the same reason the quantized arm's prompt is prefilled inside ``gemm.skinny_decode(fp8=qw)``: a
prefill on the 16-bit weights, which is what ``generate`` does, leaves K / V of the UNQUANTIZED model
in the cache and puts the quantization error back (0.090 instead of 0.018 here).
Measured on the model below: e 2.2e-02, quantized steps 1.8e-02, ulp 1.6e-02 (bound 5.9e-02)."""

import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights, softmax
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.ops import gemm

F8 = torch.float8_e4m3fn
CFG = dict(vocab_size=97, context_length=32, d_model=64, num_layers=2, num_heads=2, d_ff=128, rope_theta=10000.0)


def _rows():
    """Rows whose magnitudes span 2^-12 .. 2^12, an all-zero row, a row with one non-zero element and a
    row whose small elements fall into e4m3's subnormal range (below 2^-6 of scale, i.e. 2^-6 * amax / 448)."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(25, 96, generator=g) * (2.0 ** torch.arange(-12, 13, dtype=torch.float32))[:, None]
    zero = torch.zeros(1, 96)
    one = torch.zeros(1, 96)
    one[0, 17] = -3.7
    sub = torch.randn(1, 96, generator=g) * 2.0**-17  # |q| = 448 * |w| / 1.5 ~ 2^-9: the subnormal grid
    sub[0, 5] = 1.5
    return torch.cat([w, zero, one, sub]), 25, 26, 27


def test_quantizer_error_bound_and_bytes():
    w, iz, io, isub = _rows()
    wq, scale = ops.quantize_fp8_rows(w)
    assert wq.dtype == F8 and wq.shape == w.shape and wq.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    deq = wq.double() * scale.double()[:, None]
    err = (deq - w.double()).abs()
    bound = 2.0**-4 * w.double().abs() + 2.0**-10 * scale.double()[:, None]
    assert bool((err <= bound).all()), (err - bound).max().item()
    # the row maximum maps to +-448 exactly, with the sign of the element
    amax, arg = w.abs().max(dim=1)
    q = wq.float()
    for n in range(w.shape[0]):
        if n != iz:
            assert q[n, arg[n]].item() == math.copysign(448.0, w[n, arg[n]].item()), n
            assert scale[n].item() == (amax[n] / 448).item()
    byt = wq.view(torch.uint8)
    assert not bool(((byt == 0x7F) | (byt == 0xFF)).any())
    assert scale[iz].item() == 1.0 and not bool(byt[iz].any())
    assert int((q[io] != 0).sum()) == 1 and q[io, 17].item() == -448.0
    # the small elements of the subnormal row land on the subnormal grid k * 2^-9, some of them non-zero
    small = q[isub][torch.arange(96) != 5].abs()
    assert bool((small < 2.0**-6).all()) and bool((small > 0).any())
    # 16-bit and fp64 inputs quantize like their fp32 values
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        wd = w.to(dt)
        if not torch.isfinite(wd).all():
            continue
        a, b = ops.quantize_fp8_rows(wd)
        c, d = ops.quantize_fp8_rows(wd.float())
        assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)) and torch.equal(b, d)


def test_quantizer_clamps_a_quotient_above_448():
    # amax / (amax / 448) can round to the float above 448; whatever it does, no NaN byte comes out
    g = torch.Generator().manual_seed(1)
    w = torch.rand(4096, 16, generator=g) * 3 + 0.01
    wq, _ = ops.quantize_fp8_rows(w)
    byt = wq.view(torch.uint8)
    assert not bool(((byt == 0x7F) | (byt == 0xFF)).any())
    assert bool((wq.float().abs().amax(dim=1) == 448).all())


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_quantizer_refuses_non_finite_input(bad):
    w = torch.ones(3, 16)
    w[1, 2] = bad
    with pytest.raises(ValueError):
        ops.quantize_fp8_rows(w)
    with pytest.raises(ValueError):
        ops.quantize_fp8_rows_(w, torch.empty(3, 16, dtype=F8), torch.empty(3))
    with pytest.raises(ValueError):
        ops.quantize_fp8_rows(torch.ones(16))  # 2-D only


def test_in_place_quantizer_matches_and_does_not_reallocate():
    w, *_ = _rows()
    wq, scale = ops.quantize_fp8_rows(w)
    buf = torch.zeros(w.shape[0] + 2, w.shape[1], dtype=F8)
    sb = torch.zeros(w.shape[0] + 2)
    wq2, s2 = buf[1:-1], sb[1:-1]  # views of larger buffers, as Fp8DecodeWeights uses them
    pq, ps = wq2.data_ptr(), s2.data_ptr()
    ops.quantize_fp8_rows_(w, wq2, s2)
    assert wq2.data_ptr() == pq and s2.data_ptr() == ps
    assert torch.equal(wq2.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(s2, scale)
    assert not bool(buf.view(torch.uint8)[0].any()) and not bool(buf.view(torch.uint8)[-1].any())
    assert sb[0].item() == 0 and sb[-1].item() == 0


@pytest.mark.parametrize("rows", [(1,), (16,), (2, 3), (17,), (5, 8)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32, torch.float64])
def test_skinny_linear_fp8_cpu_is_the_reference(rows, dt):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(*rows, 32, generator=g).to(dt)
    wq, scale = ops.quantize_fp8_rows(torch.randn(13, 32, generator=g))
    got = ops.skinny_linear_fp8(x, wq, scale)
    want = ops.skinny_linear_fp8_ref(x.reshape(-1, 32), wq, scale)
    assert got.shape == (*rows, 13) and got.dtype == dt
    assert torch.equal(got.reshape(-1, 13), want)
    cdt = dt if dt in (torch.float32, torch.float64) else torch.float32
    by_hand = ((x.reshape(-1, 32).to(cdt) @ wq.to(cdt).T) * scale.to(cdt)).to(dt)
    assert torch.equal(want, by_hand)
    assert torch.equal(ops.skinny_linear_fp8(x, wq.view(torch.uint8), scale), got)  # the uint8 view


def _bf16_model(seed=0):
    torch.manual_seed(seed)
    return BasicsTransformerLM(**CFG).to(torch.bfloat16).eval()


def _ulp_bf16(x):
    return 2.0 ** (math.floor(math.log2(x)) - 7)


def test_quantized_eager_steps_against_the_exact_fp64_model():
    m = _bf16_model()
    qw = Fp8DecodeWeights(m)
    exact = BasicsTransformerLM(**CFG).double().eval()  # the dequantized weights, exactly
    exact.load_state_dict({k: v for k, v in qw.dequantized_state_dict(torch.float64).items()})
    for name, p in exact.named_parameters():
        if "proj" in name or "ffn" in name or "lm_head" in name:
            wq, scale = qw.lookup(dict(m.named_parameters())[name])
            assert torch.equal(p.detach(), wq.double() * scale.double()[:, None]), name
    m64 = BasicsTransformerLM(**CFG).double().eval()  # the bf16 model's own weights, exactly
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    seq = torch.randint(0, 97, (2, 13), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        e16 = (m(seq).double() - m64(seq)).abs().max().item()
        cq, cx = KVCache(m, 2), KVCache(exact, 2)
        with gemm.skinny_decode(fp8=qw):  # the prompt's K / V from the quantized weights too
            m.forward_cached(seq[:, :5], cq)
        exact.forward_cached(seq[:, :5], cx)
        dg = DecodeGraph(m, cq, capture=False, weights=qw)
        plain = DecodeGraph(m, KVCache(m, 2), capture=False)
        m.forward_cached(seq[:, :5], plain.cache)
        worst, top, differs = 0.0, 0.0, False
        for n in range(5, 13):  # 8 teacher-forced steps
            got = dg.step(seq[:, n:n + 1])
            ref = exact.forward_cached(seq[:, n:n + 1], cx)
            assert got.shape == (2, 1, 97) and got.dtype == torch.bfloat16
            worst = max(worst, (got.double() - ref).abs().max().item())
            top = max(top, ref.abs().max().item())
            differs |= not torch.equal(got, plain.step(seq[:, n:n + 1]))
    ulp = _ulp_bf16(top)
    print(f"e16 {e16:.3e} quantized steps {worst:.3e} ulp {ulp:.3e}")
    assert worst <= 2 * e16 + ulp, (worst, e16, ulp)
    assert differs  # the steps did read the quantized weights
    assert cq.length == 13 and gemm._FP8 is None and not gemm._SKINNY


def test_refresh_requantizes_in_place_and_nbytes():
    m = _bf16_model(1)
    qw = Fp8DecodeWeights(m)
    rows = sum(p.shape[0] for n, p in m.named_parameters() if p.dim() == 2 and "token_embeddings" not in n)
    elems = sum(p.numel() for n, p in m.named_parameters() if p.dim() == 2 and "token_embeddings" not in n)
    assert qw.nbytes == elems + 4 * rows
    at = m.layers[1].attn
    wq, scale = qw.lookup(at.k_proj.weight)
    assert wq.shape == (64, 64) and scale.shape == (64,)
    ptr, before, s_before = wq.data_ptr(), wq.clone().view(torch.uint8), scale.clone()
    with torch.no_grad():
        at.k_proj.weight[3].mul_(4.0)
    assert qw.refresh() is qw
    wq2, scale2 = qw.lookup(at.k_proj.weight)
    assert wq2.data_ptr() == ptr and wq.data_ptr() == ptr
    assert torch.equal(wq2.view(torch.uint8), before)  # a power of two moves into the scale alone
    assert torch.equal(scale2[3], s_before[3] * 4) and torch.equal(scale2[:3], s_before[:3])
    a, b = ops.quantize_fp8_rows(at.k_proj.weight.detach())
    assert torch.equal(a.view(torch.uint8), wq2.view(torch.uint8)) and torch.equal(b, scale2)
    # not this model's tensors: no entry
    assert qw.lookup(torch.zeros(64, 64, dtype=torch.bfloat16)) is None
    assert qw.lookup(m.token_embeddings.weight) is None and qw.lookup(m.ln_final.weight) is None


def test_mm_nt_takes_the_table_only_inside_the_context():
    m = _bf16_model(2)
    qw = Fp8DecodeWeights(m)
    w = m.lm_head.weight.detach()
    x = torch.randn(4, 64).bfloat16()
    plain = gemm.mm_nt(x, w)
    assert torch.equal(plain, x @ w.t())
    with gemm.skinny_decode(fp8=qw):
        assert torch.equal(gemm.mm_nt(x, w), ops.skinny_linear_fp8_ref(x, *qw.lookup(w)))
        other = w.clone()
        assert torch.equal(gemm.mm_nt(x, other), plain)  # not in the table: today's path
        with gemm.skinny_decode():  # nested without fp8: off, and restored afterwards
            assert gemm.fp8_lookup(w) is None
        assert gemm.fp8_lookup(w) is not None
    assert gemm.fp8_lookup(w) is None and torch.equal(gemm.mm_nt(x, w), plain)


def test_error_paths():
    m32 = BasicsTransformerLM(**CFG).eval()
    with pytest.raises(ValueError, match="bf16 or fp16"):
        Fp8DecodeWeights(m32)
    torch.manual_seed(0)
    odd = BasicsTransformerLM(**{**CFG, "d_model": 72, "num_heads": 2}).to(torch.bfloat16).eval()  # K = 72
    with pytest.raises(ValueError, match="qkv.*multiple of 16"):
        Fp8DecodeWeights(odd)
    m, other = _bf16_model(), _bf16_model(1)
    qw = Fp8DecodeWeights(other)
    with pytest.raises(ValueError, match="different model"):
        DecodeGraph(m, KVCache(m, 2), capture=False, weights=qw)
    x = torch.randint(0, 97, (2, 5))
    with pytest.raises(ValueError, match="graph"):
        m.generate(x, 4, top_k=1, use_cache=True, weights=Fp8DecodeWeights(m))
    m.layers[0].attn.context_parallel = (None, "ring")
    try:
        with pytest.raises(NotImplementedError):
            Fp8DecodeWeights(m)
    finally:
        m.layers[0].attn.context_parallel = None


def test_generate_with_a_caller_owned_quantized_eager_graph():
    m = _bf16_model(4)
    qw = Fp8DecodeWeights(m)
    x = torch.randint(0, 97, (2, 5), generator=torch.Generator().manual_seed(5))
    dg = DecodeGraph(m, KVCache(m, 2), capture=False, weights=qw)
    torch.manual_seed(7)
    out = m.generate(x, 12, top_k=1, use_cache=True, graph=dg)
    # the same loop by hand: a 16-bit prefill, then quantized steps
    cache = KVCache(m, 2)
    de = DecodeGraph(m, cache, capture=False, weights=qw)
    torch.manual_seed(7)
    with torch.no_grad():
        logits = m.forward_cached(x, cache)
        toks = []
        for _ in range(12):
            lg = logits[:, -1].float()
            lg = lg.masked_fill(lg < lg.max(dim=-1, keepdim=True).values, float("-inf"))
            toks.append(torch.multinomial(softmax(lg, dim=-1), 1))
            if len(toks) < 12:
                logits = de.step(toks[-1])
    assert torch.equal(out, torch.cat(toks, dim=1))
