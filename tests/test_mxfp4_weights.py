"""MXFP4 weight-only decode on the CPU: the block quantizer (``ops.quantize_mxfp4_rows``), its inverse
(``ops.dequantize_mxfp4_rows``), the op wrapper (``ops.skinny_linear_mxfp4``), ``Mxfp4DecodeWeights`` and the
``weights=`` argument of ``DecodeGraph`` with it, by the pattern of ``test_fp8_weights.py``.

The format is fixed: byte ``j`` of a row holds the code of ``k = 2j`` in bits 3:0 and of ``k = 2j+1`` in bits
7:4; a code is ``sign << 3 | m`` with ``m`` indexing {0, .5, 1, 1.5, 2, 3, 4, 6}; one e8m0 byte per 32 values,
``X = floor(log2(amax)) - 2`` clamped to [-23, 13], elements rounded to nearest with ties to the even code and
saturated at +-6.

The model comparison: the quantized eager steps against the fp64 forward of ``dequantized_state_dict()``,
with the bf16 model's own distance ``e16`` to its exact fp64 counterpart as the yardstick, ``<= 2 * e16 +
ulp`` as in ``test_fp8_weights.py``. The quantized arm's prompt is prefilled inside
``gemm.skinny_decode(weights=qw)`` so that its cached K / V come from the quantized weights too."""

import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights, Mxfp4DecodeWeights
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.ops import gemm

VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
CFG = dict(vocab_size=97, context_length=32, d_model=64, num_layers=2, num_heads=2, d_ff=96, rope_theta=10000.0)


def _codes(wq):
    """(N, K) codes of the packed bytes"""
    return torch.stack((wq & 0xF, wq >> 4), dim=2).view(wq.shape[0], -1)


def test_code_table_through_dequantize():
    wq = torch.zeros(1, 16, dtype=torch.uint8)
    wq[0, :8] = torch.tensor([c | ((c + 8) << 4) for c in range(8)], dtype=torch.uint8)  # k = 2c: +val, 2c+1: -val
    for byte, mul in ((127, 1.0), (128, 2.0), (104, 2.0 ** -23), (140, 2.0 ** 13)):
        dq = ops.dequantize_mxfp4_rows(wq, torch.tensor([[byte]], dtype=torch.uint8))
        assert dq.shape == (1, 32) and dq.dtype == torch.float32
        want = torch.tensor([s * v * mul for v in VALUES for s in (1.0, -1.0)])
        assert torch.equal(dq[0, :16], want) and not dq[0, 16:].any()
        assert torch.equal(torch.signbit(dq[0, :16]), torch.tensor([False, True] * 8))  # -0 keeps its sign
        for dt in (torch.bfloat16, torch.float16, torch.float64):  # exact in every dtype inside the clamp
            assert torch.equal(ops.dequantize_mxfp4_rows(wq, torch.tensor([[byte]], dtype=torch.uint8), dt).double(), dq.double())
    # the torch views are accepted where uint8 is
    sc = torch.full((1, 1), 127, dtype=torch.uint8)
    assert torch.equal(ops.dequantize_mxfp4_rows(wq.view(torch.float4_e2m1fn_x2), sc.view(torch.float8_e8m0fnu)),
                       ops.dequantize_mxfp4_rows(wq, sc))


def test_nibble_order_one_hot():
    for k in range(64):
        w = torch.zeros(2, 64)
        w[1, k] = -3.0
        wq, scale = ops.quantize_mxfp4_rows(w)
        assert wq.shape == (2, 32) and wq.dtype == torch.uint8 and scale.shape == (2, 2) and scale.dtype == torch.uint8
        assert wq.is_contiguous() and scale.is_contiguous()
        want = torch.zeros(2, 32, dtype=torch.uint8)
        want[1, k // 2] = (8 | 7) << (4 * (k % 2))  # -3 in a block with amax 3: X = -1, element -6, code 7 | sign
        assert torch.equal(wq, want), k
        ws = torch.full((2, 2), 127, dtype=torch.uint8)
        ws[1, k // 32] = 126
        assert torch.equal(scale, ws), k
        assert torch.equal(ops.dequantize_mxfp4_rows(wq, scale), w)


TIES = [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0), (7.9, 6.0)]


def test_ties_to_even_and_saturation():
    w = torch.zeros(1, 32)
    w[0, 0] = 4.0  # X = 0: the elements are the inputs
    for i, (v, _) in enumerate(TIES):
        w[0, 1 + i] = v
        w[0, 9 + i] = -v
    w[0, 17] = -0.0
    w[0, 18] = -0.1  # rounds to zero: the sign bit stays
    wq, scale = ops.quantize_mxfp4_rows(w)
    assert scale.tolist() == [[127]]
    dq = ops.dequantize_mxfp4_rows(wq, scale)[0]
    codes = _codes(wq)[0]
    assert dq[0] == 4.0
    for i, (v, r) in enumerate(TIES):
        assert dq[1 + i] == r, (v, dq[1 + i].item())
        assert dq[9 + i] == -r and codes[9 + i] == (codes[1 + i] | 8), v
    assert codes[17] == 8 and codes[18] == 8 and codes[19] == 0
    # just off the ties: nearest
    w2 = torch.zeros(1, 32)
    w2[0, 0] = 4.0
    off = [(0.2500001, 0.5), (0.7499999, 0.5), (1.2500001, 1.5), (1.7499999, 1.5), (2.5000002, 3.0), (3.4999998, 3.0),
           (5.0000005, 6.0), (4.9999995, 4.0)]
    for i, (v, _) in enumerate(off):
        w2[0, 1 + i] = v
    dq2 = ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(w2))[0]
    for i, (v, r) in enumerate(off):
        assert dq2[1 + i] == r, (v, dq2[1 + i].item())


def test_scale_bytes_at_and_below_powers_of_two_zero_blocks_and_the_clamp():
    exps = list(range(-30, 21))
    w = torch.zeros(len(exps), 96)
    for i, e in enumerate(exps):
        w[i, 5] = 2.0 ** e  # block 0: an exact power of two
        w[i, 40] = -torch.nextafter(torch.tensor(2.0 ** e), torch.tensor(0.0)).item()  # block 1: one ulp below it
    wq, scale = ops.quantize_mxfp4_rows(w)  # block 2 is all zero
    for i, e in enumerate(exps):
        assert scale[i, 0].item() == min(max(e - 2, -23), 13) + 127, e
        assert scale[i, 1].item() == min(max(e - 3, -23), 13) + 127, e
        assert scale[i, 2].item() == 127
    assert not wq[:, 32:].any()
    assert int(scale.min()) == 127 - 23 and int(scale.max()) == 127 + 13  # bytes 0 and 255 never come out
    dq = ops.dequantize_mxfp4_rows(wq, scale)
    in0 = [i for i, e in enumerate(exps) if -23 <= e - 2 <= 13]
    in1 = [i for i, e in enumerate(exps) if -23 <= e - 3 <= 13]
    assert torch.equal(dq[in0, 5], w[in0, 5])  # 4 * 2^X
    # one ulp below 2^e the element is 7.99.. at X = e - 3, beyond 6: it saturates at 6 * 2^X
    assert torch.equal(dq[in1, 40], torch.tensor([-6.0 * 2.0 ** (exps[i] - 3) for i in in1]))
    # below the clamp a block flushes towards zero, above it saturates at 6 * 2^13
    assert dq[0, 5] == 0.0 and dq[-1, 5] == 6.0 * 2.0 ** 13


def test_requantizing_is_the_identity_and_the_error_bound():
    g = torch.Generator().manual_seed(0)
    e = torch.randint(-12, 9, (40, 1), generator=g)
    w = torch.randn(40, 160, generator=g) * torch.exp2(e.float())
    w[3] *= 0  # zero rows and a heavy tail
    w[5, ::7] *= 50.0
    for src in (w, w.bfloat16(), w.half(), w.double()):
        wq, scale = ops.quantize_mxfp4_rows(src)
        dq = ops.dequantize_mxfp4_rows(wq, scale)
        wq2, scale2 = ops.quantize_mxfp4_rows(dq)
        assert torch.equal(wq2, wq) and torch.equal(scale2, scale)
        step = torch.exp2(scale.float() - 127).repeat_interleave(32, dim=1)  # 2^X
        wf = src.float()
        err = (wf - dq).abs()
        near = wf.abs() <= 6 * step
        assert bool((err[near] <= step[near]).all()) and bool((err[~near] <= 2 * step[~near]).all())
        assert near.float().mean() > 0.9
        assert torch.equal(torch.signbit(dq), torch.signbit(wf))  # the sign bit is the input's, zeros included
    # Gaussian weights: the relative RMS error the README quotes
    wg = torch.randn(512, 1600, generator=g) * 0.02
    rel = ((wg - ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(wg))).pow(2).mean() / wg.pow(2).mean()).sqrt().item()
    print(f"relative RMS error on N(0, 0.02^2): {rel:.4f}")
    assert 0.10 < rel < 0.13


def test_bad_inputs_raise():
    w = torch.randn(3, 64)
    for bad in (float("inf"), float("-inf"), float("nan")):
        wb = w.clone()
        wb[1, 5] = bad
        with pytest.raises(ValueError, match="inf or NaN"):
            ops.quantize_mxfp4_rows(wb)
    with pytest.raises(ValueError, match="32"):
        ops.quantize_mxfp4_rows(torch.randn(3, 48))
    with pytest.raises(ValueError):
        ops.quantize_mxfp4_rows(torch.ones(64))  # 2-D only
    with pytest.raises(ValueError):
        ops.quantize_mxfp4_rows_(w, torch.empty(3, 16, dtype=torch.uint8), torch.empty(3, 2, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.quantize_mxfp4_rows_(w, torch.empty(3, 32, dtype=torch.uint8), torch.empty(3, 2, dtype=torch.float32))
    with pytest.raises(ValueError):
        ops.dequantize_mxfp4_rows(torch.empty(3, 32, dtype=torch.uint8), torch.empty(3, 3, dtype=torch.uint8))


def test_in_place_quantizer_writes_views():
    w = torch.randn(5, 64, generator=torch.Generator().manual_seed(1))
    wq, scale = ops.quantize_mxfp4_rows(w)
    buf = torch.full((7, 32), 0xEE, dtype=torch.uint8)
    sb = torch.full((7, 4), 0xEE, dtype=torch.uint8)
    wq2, s2 = buf[1:-1], sb[1:-1, 1:3]  # views of larger buffers; the scale rows are padded
    ptr = buf.data_ptr()
    ops.quantize_mxfp4_rows_(w, wq2, s2)
    assert buf.data_ptr() == ptr and torch.equal(wq2, wq) and torch.equal(s2, scale)
    assert bool((buf[0] == 0xEE).all()) and bool((buf[-1] == 0xEE).all())
    assert bool((sb[0] == 0xEE).all()) and bool((sb[:, 0] == 0xEE).all()) and bool((sb[:, 3] == 0xEE).all())
    b4, b8 = torch.zeros(5, 32, dtype=torch.uint8), torch.zeros(5, 2, dtype=torch.uint8)
    ops.quantize_mxfp4_rows_(w, b4.view(torch.float4_e2m1fn_x2), b8.view(torch.float8_e8m0fnu))  # the torch views
    assert torch.equal(b4, wq) and torch.equal(b8, scale)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("rows", [(3,), (2, 1), (5, 4)])
def test_skinny_linear_mxfp4_cpu_is_the_reference(rows, dt):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(*rows, 64, generator=g).to(dt)
    wq, scale = ops.quantize_mxfp4_rows(torch.randn(13, 64, generator=g))
    got = ops.skinny_linear_mxfp4(x, wq, scale)
    want = ops.skinny_linear_mxfp4_ref(x.reshape(-1, 64), wq, scale)
    assert got.shape == (*rows, 13) and got.dtype == dt
    assert torch.equal(got.reshape(-1, 13), want)
    exact = x.reshape(-1, 64).double() @ ops.dequantize_mxfp4_rows(wq, scale, torch.float64).T
    tol = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -20}[dt]
    assert (want.double() - exact).abs().max() <= tol * exact.abs().max() + 1e-5
    assert torch.equal(ops.skinny_linear_mxfp4(x, wq.view(torch.float4_e2m1fn_x2), scale.view(torch.float8_e8m0fnu)), got)


def _bf16_model(seed=0, dt=torch.bfloat16):
    torch.manual_seed(seed)
    return BasicsTransformerLM(**CFG).to(dt).eval()


def _ulp_bf16(x):
    return 2.0 ** (math.floor(math.log2(x)) - 7)


def test_lookup_refresh_and_nbytes():
    m = _bf16_model(1)
    qw = Mxfp4DecodeWeights(m)
    elems = sum(p.numel() for n, p in m.named_parameters() if p.dim() == 2 and "token_embeddings" not in n)
    assert qw.nbytes * 32 == elems * 17
    at, ff = m.layers[1].attn, m.layers[0].ffn
    wq, scale = qw.lookup(at.k_proj.weight)  # a single matrix of a group: a row slice of the grouped table
    assert wq.shape == (64, 32) and scale.shape == (64, 2) and wq.dtype == scale.dtype == torch.uint8
    a, b = ops.quantize_mxfp4_rows(at.k_proj.weight.detach())
    assert torch.equal(a, wq) and torch.equal(b, scale)
    from cs336_systems.models import fused

    for params in ([at.q_proj.weight, at.k_proj.weight, at.v_proj.weight], [ff.w1.weight, ff.w3.weight]):
        gv = fused.grouped_view([p.detach() for p in params])
        if gv is not None:  # the grouped operand the decode step multiplies by
            gq, gs = qw.lookup(gv)
            rows = sum(p.shape[0] for p in params)
            assert gq.shape == (rows, 32) and gs.shape == (rows, 2)
            assert torch.equal(gq, torch.cat([qw.lookup(p)[0] for p in params]))
            assert gq.data_ptr() == qw.lookup(params[0])[0].data_ptr()
    hq, hs = qw.lookup(m.lm_head.weight)
    assert hq.shape == (97, 32) and hs.shape == (97, 2)
    # refresh: requantized in place, every address kept
    ptrs = {n: tuple(t.data_ptr() for t in qw.lookup(p)) for n, p in m.named_parameters() if qw.lookup(p) is not None}
    assert len(ptrs) == 2 * 7 + 1
    before, s_before = wq.clone(), scale.clone()
    with torch.no_grad():
        at.k_proj.weight[3].mul_(4.0)
    assert qw.refresh() is qw
    for n, p in m.named_parameters():
        if n in ptrs:
            assert tuple(t.data_ptr() for t in qw.lookup(p)) == ptrs[n], n
    wq2, scale2 = qw.lookup(at.k_proj.weight)
    assert torch.equal(wq2, before) and torch.equal(wq, before)  # a power of two moves into the scales alone
    assert torch.equal(scale2[3], s_before[3] + 2) and torch.equal(scale2[:3], s_before[:3])
    assert qw.lookup(torch.zeros(64, 64, dtype=torch.bfloat16)) is None
    assert qw.lookup(m.token_embeddings.weight) is None and qw.lookup(m.ln_final.weight) is None


def test_mm_nt_runs_the_weights_own_linear_only_inside_the_context():
    m = _bf16_model(2)
    q4, q8 = Mxfp4DecodeWeights(m), Fp8DecodeWeights(m)
    w = m.lm_head.weight.detach()
    x = torch.randn(4, 64).bfloat16()
    plain = gemm.mm_nt(x, w)
    with gemm.skinny_decode(weights=q4):
        assert torch.equal(gemm.mm_nt(x, w), ops.skinny_linear_mxfp4_ref(x, *q4.lookup(w)))
        assert torch.equal(gemm.mm_nt(x, w.clone()), plain)  # not in the table: today's path
        with gemm.skinny_decode(fp8=q8):  # nested: the inner object's format, restored afterwards
            assert torch.equal(gemm.mm_nt(x, w), ops.skinny_linear_fp8_ref(x, *q8.lookup(w)))
        assert torch.equal(gemm.mm_nt(x, w), ops.skinny_linear_mxfp4_ref(x, *q4.lookup(w)))
    with gemm.skinny_decode(fp8=q4):  # the older keyword takes either class
        assert torch.equal(gemm.mm_nt(x, w), ops.skinny_linear_mxfp4_ref(x, *q4.lookup(w)))
    with gemm.skinny_decode(weights=q8):
        assert torch.equal(gemm.mm_nt(x, w), ops.skinny_linear_fp8_ref(x, *q8.lookup(w)))
    with pytest.raises(ValueError):
        with gemm.skinny_decode(fp8=q8, weights=q4):
            pass
    assert gemm.fp8_lookup(w) is None and torch.equal(gemm.mm_nt(x, w), plain) and not gemm._SKINNY


def test_error_paths():
    with pytest.raises(ValueError, match="bf16 or fp16"):
        Mxfp4DecodeWeights(BasicsTransformerLM(**CFG).eval())  # an fp32 model
    torch.manual_seed(0)
    odd = BasicsTransformerLM(**{**CFG, "d_model": 48, "num_heads": 2}).to(torch.bfloat16).eval()  # K = 48
    with pytest.raises(ValueError, match="qkv.*multiple of 32"):
        Mxfp4DecodeWeights(odd)
    m, other = _bf16_model(), _bf16_model(1)
    with pytest.raises(ValueError, match="different model"):
        DecodeGraph(m, KVCache(m, 2), capture=False, weights=Mxfp4DecodeWeights(other))
    with pytest.raises(ValueError, match="graph"):
        m.generate(torch.randint(0, 97, (2, 5)), 4, top_k=1, use_cache=True, weights=Mxfp4DecodeWeights(m))
    m.layers[0].attn.context_parallel = (None, "ring")
    try:
        with pytest.raises(NotImplementedError):
            Mxfp4DecodeWeights(m)
    finally:
        m.layers[0].attn.context_parallel = None


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_quantized_eager_steps_against_the_exact_fp64_model(dt):
    m = _bf16_model(dt=dt)
    qw = Mxfp4DecodeWeights(m)
    exact = BasicsTransformerLM(**CFG).double().eval()  # the dequantized weights, exactly
    exact.load_state_dict(qw.dequantized_state_dict(torch.float64))
    for name, p in exact.named_parameters():
        if "proj" in name or "ffn" in name or "lm_head" in name:
            wq, scale = qw.lookup(dict(m.named_parameters())[name])
            assert torch.equal(p.detach(), ops.dequantize_mxfp4_rows(wq, scale, torch.float64)), name
    m64 = BasicsTransformerLM(**CFG).double().eval()  # the 16-bit model's own weights, exactly
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    seq = torch.randint(0, 97, (2, 13), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        e16 = (m(seq).double() - m64(seq)).abs().max().item()
        cq, cx = KVCache(m, 2), KVCache(exact, 2)
        with gemm.skinny_decode(weights=qw):  # the prompt's K / V from the quantized weights too
            m.forward_cached(seq[:, :5], cq)
        exact.forward_cached(seq[:, :5], cx)
        dg = DecodeGraph(m, cq, capture=False, weights=qw)
        plain = DecodeGraph(m, KVCache(m, 2), capture=False)
        m.forward_cached(seq[:, :5], plain.cache)
        worst, top, differs = 0.0, 0.0, False
        for n in range(5, 13):  # 8 teacher-forced steps
            got = dg.step(seq[:, n:n + 1])
            ref = exact.forward_cached(seq[:, n:n + 1], cx)
            assert got.shape == (2, 1, 97) and got.dtype == dt
            worst = max(worst, (got.double() - ref).abs().max().item())
            top = max(top, ref.abs().max().item())
            differs |= not torch.equal(got, plain.step(seq[:, n:n + 1]))
    ulp = _ulp_bf16(top) if dt == torch.bfloat16 else _ulp_bf16(top) / 8
    print(f"{dt}: e16 {e16:.3e} quantized steps {worst:.3e} ulp {ulp:.3e}")
    assert worst <= 2 * e16 + ulp, (worst, e16, ulp)
    assert differs  # the steps did read the quantized weights
    assert cq.length == 13 and gemm._FP8 is None and not gemm._SKINNY
