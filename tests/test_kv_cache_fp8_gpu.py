"""``KVCache(fp8=True)`` through the model on the GPU: the captured and replayed decode step over an FP8
cache against the same step run eagerly (``capture=False``) on a second FP8 cache, bit for bit (logits,
bytes and scales), and against the fp32 eager forward of the same weights over a plain cache.

Yardstick: ``e_hip`` and ``ulp`` are taken as ``test_decode_graph_fp8_gpu.py`` takes them (the worst
error of the bf16 model's ordinary forward against the fp32 eager forward ``ref`` of its own weights;
one bf16 ulp of the largest reference logit). ``e_q`` is what the format itself costs: the fp32 model
on the eager PyTorch backend, teacher-forced over an FP8 cache against the same steps over a plain
cache, largest logit distance. ``e_kv8`` is the distance of the replayed bf16 FP8-cache logits to
``ref``; the test asserts ``e_kv8 <= 2 * (e_q + e_hip) + ulp``. The factor 2 is a margin, not a
derivation: a bf16 row and its fp32 counterpart can round to different bytes, so the two error sources
do not simply add. ``e_ref16`` (printed, not asserted) is the same distance for the bf16 model on the
eager PyTorch backend over an FP8 cache: the reference ops alone.

Models are those of ``test_decode_graph_gpu.py`` (context 128, 2 layers, d_model 256 / 4 heads and
160 / 2 heads) in bf16.

Measured on an MI355X (e_hip / e_q / ulp / e_kv8 / e_ref16, and the bound): d_model 256: 2.03e-02 /
5.88e-02 / 1.56e-02 / 5.66e-02 / 6.64e-02, bound 1.74e-01; d_model 160: 1.58e-02 / 4.97e-02 / 1.56e-02 /
4.95e-02 / 5.37e-02, bound 1.47e-01. The replayed step is as far from the fp32 plain-cache forward as the
format itself puts the fp32 model (e_q), the reference ops alone stay within the bound too, and the
factor 2 is not used up. Speculative case: worst max(ref) - ref[token] 2.8e-02 against 2 E = 3.6e-01."""

import math

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights
from cs336_systems.models.kv_cache import KVCache
from cs336_systems.models.speculative import speculative_generate

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
MODELS = [(256, 4), (160, 2)]


def _cfg(d_model, heads):
    return dict(vocab_size=500, context_length=128, d_model=d_model, num_layers=2, num_heads=heads, d_ff=512,
                rope_theta=10000.0)


def _ulp(dt, x):
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dt]
    return 2.0 ** (math.floor(math.log2(x)) - mant)


def _model(d_model, heads, dt=BF16, seed=0):
    torch.manual_seed(seed)
    return BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(dt).eval()


def _fp32_twin(m, d_model, heads):
    m32 = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    return m32


def _same_cache(a, b, upto=None):
    """Lengths, bytes (as uint8) and scales of the rows [0, upto) (default: the cached ones)."""
    upto = a.length if upto is None else upto
    if a.length != b.length or not torch.equal(a.lengths, b.lengths):
        return False
    for x, y in ((a.k, b.k), (a.v, b.v)):
        if not torch.equal(x.view(torch.uint8)[:, :, :, :upto], y.view(torch.uint8)[:, :, :, :upto]):
            return False
    return (torch.equal(a.k_scale[:, :, :, :upto], b.k_scale[:, :, :, :upto])
            and torch.equal(a.v_scale[:, :, :, :upto], b.v_scale[:, :, :, :upto]))


def _stepwise(m, seq, cache, first=9):
    """Teacher-forced logits at positions first - 1 .. end: a prefill, then single cached steps."""
    rows = [m.forward_cached(seq[:, :first], cache)[:, -1:]]
    for n in range(first, seq.shape[1]):
        rows.append(m.forward_cached(seq[:, n:n + 1], cache))
    return torch.cat(rows, dim=1)


@pytest.mark.parametrize("d_model,heads", MODELS)
def test_replay_equals_eager_and_error_yardstick(d_model, heads):
    dt = BF16
    m = _model(d_model, heads)
    seq = torch.randint(0, 500, (2, 128), device=DEV)
    m32 = _fp32_twin(m, d_model, heads)
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()[:, 8:]  # fp32, no cache: logits at positions 8 .. 127
        plain32 = _stepwise(m32, seq, KVCache(m32, 2)).double()
        e_q = (_stepwise(m32, seq, KVCache(m32, 2, fp8=True)).double() - plain32).abs().max().item()
        e_ref16 = (_stepwise(m, seq, KVCache(m, 2, fp8=True)).double() - ref).abs().max().item()
    assert (plain32 - ref).abs().max().item() < 1e-3  # (the plain cached path is the forward)
    with torch.no_grad():
        e_hip = (m(seq).double()[:, 8:] - ref).abs().max().item()
    cg, ce, cp = KVCache(m, 2, fp8=True), KVCache(m, 2, fp8=True), KVCache(m, 2)
    assert cg.fp8 and cg.dtype == dt and 0.52 <= cg.nbytes / cp.nbytes <= 0.56
    with torch.no_grad():
        first = m.forward_cached(seq[:, :9], cg)[:, -1]
        m.forward_cached(seq[:, :9], ce)
        m.forward_cached(seq[:, :9], cp)
        assert _same_cache(cg, ce)
        dg = DecodeGraph(m, cg, capture=True, warmup=2)
        assert cg.length == 9 and cg.lengths.tolist() == [9, 9] and _same_cache(cg, ce)
        de = DecodeGraph(m, ce, capture=False)
        plain = DecodeGraph(m, cp, capture=True)
        rows, differs = [first], False
        for n in range(9, 128):  # 119 teacher-forced steps
            got = dg.step(seq[:, n:n + 1])
            want = de.step(seq[:, n:n + 1])
            assert got.shape == (2, 1, 500) and got.dtype == dt
            assert torch.equal(got, want), n
            rows.append(got[:, -1].clone())  # the static buffer is overwritten by the next step
            differs = differs or not torch.equal(got, plain.step(seq[:, n:n + 1]))
    assert cg.length == 128 and cg.lengths.tolist() == [128, 128] and _same_cache(cg, ce)
    assert not ((cg.k.view(torch.uint8) & 0x7f) == 0x7f).any() and not ((cg.v.view(torch.uint8) & 0x7f) == 0x7f).any()
    graphed = torch.stack(rows, dim=1)
    e_kv8 = (graphed.double() - ref).abs().max().item()
    ulp = _ulp(dt, ref.abs().max().item())
    print(f"d_model {d_model} heads {heads} {dt}: e_hip {e_hip:.4e} e_q {e_q:.4e} ulp {ulp:.3e} e_kv8 {e_kv8:.4e} "
          f"e_ref16 {e_ref16:.4e} bound {2 * (e_q + e_hip) + ulp:.4e}")
    assert e_kv8 <= 2 * (e_q + e_hip) + ulp, (e_kv8, e_q, e_hip, ulp)
    assert differs  # ... and it is not the plain-cache step


def test_chunk_step_replay_equals_eager():
    m = _model(256, 4, seed=4)
    seq = torch.randint(0, 500, (2, 40), device=DEV)
    cg, ce = KVCache(m, 2, fp8=True), KVCache(m, 2, fp8=True)
    with torch.no_grad():
        for c in (cg, ce):
            m.forward_cached(seq[:, :8], c)
        dg = DecodeGraph(m, cg, tokens=4)
        de = DecodeGraph(m, ce, capture=False, tokens=4)
        assert cg.length == 8 and _same_cache(cg, ce)
        for n in range(8, 40, 4):
            got, want = dg.step(seq[:, n:n + 4]), de.step(seq[:, n:n + 4])
            assert got.shape == (2, 4, 500) and torch.equal(got, want), n
        assert cg.length == 40 and _same_cache(cg, ce)
        # rejected tokens are forgotten in place; the graph goes on from the shorter cache
        for c in (cg, ce):
            c.truncate(33)
        assert torch.equal(dg.step(seq[:, 33:37]), de.step(seq[:, 33:37])) and _same_cache(cg, ce)


def test_fp8_weights_and_fp8_cache_combine_and_reuse_after_reset():
    m = _model(160, 2, seed=3)
    qw = Fp8DecodeWeights(m)
    seq = torch.randint(0, 500, (3, 40), device=DEV)
    cg, ce, cw = KVCache(m, 3, fp8=True), KVCache(m, 3, fp8=True), KVCache(m, 3, fp8=True)
    with torch.no_grad():
        for c in (cg, ce, cw):
            m.forward_cached(seq[:, :9], c)
        dg = DecodeGraph(m, cg, weights=qw)
        de = DecodeGraph(m, ce, capture=False, weights=qw)
        d16 = DecodeGraph(m, cw, capture=False)  # 16-bit weights over an FP8 cache
        moved = False
        for n in range(9, 20):
            got = dg.step(seq[:, n:n + 1])
            assert torch.equal(got, de.step(seq[:, n:n + 1])), n
            moved = moved or not torch.equal(got, d16.step(seq[:, n:n + 1]))
        assert moved and _same_cache(cg, ce)
        # the same graph after reset() and a prefill of another length
        for c in (cg, ce):
            c.reset()
            m.forward_cached(seq[:, 20:25], c)
        assert cg.length == 5
        for n in range(25, 32):
            assert torch.equal(dg.step(seq[:, n:n + 1]), de.step(seq[:, n:n + 1])), n
        assert cg.length == 12 and _same_cache(cg, ce)


def _sample_top1(logits):
    """``generate``'s own sampling at ``top_k=1`` (as in ``test_decode_graph_gpu.py``)."""
    from cs336_systems.models import softmax

    logits = logits[:, -1].float() / 1.0
    vals, _ = torch.topk(logits, 1)
    logits = logits.masked_fill(logits < vals[:, -1:], float("-inf"))
    return torch.multinomial(softmax(logits, dim=-1), 1)


def test_generate_with_graph_over_an_fp8_cache():
    m = _model(256, 4, seed=1)
    x = torch.randint(0, 500, (3, 9), device=DEV)
    torch.manual_seed(7)
    out = m.generate(x, 16, top_k=1, use_cache=True, graph=True, kv_fp8=True)
    # the same kernels in a manual loop over the eager arm
    cache = KVCache(m, 3, fp8=True)
    de = DecodeGraph(m, cache, capture=False)
    torch.manual_seed(7)
    with torch.no_grad():
        logits = m.forward_cached(x, cache)
        toks = []
        for _ in range(16):
            toks.append(_sample_top1(logits))
            if len(toks) < 16:
                logits = de.step(toks[-1])
    assert out.shape == (3, 16) and torch.equal(out, torch.cat(toks, dim=1))
    # a caller-owned graph: its own cache is used, whatever its format
    dg = DecodeGraph(m, KVCache(m, 3, fp8=True))
    torch.manual_seed(7)
    assert torch.equal(m.generate(x, 16, top_k=1, use_cache=True, graph=dg), out)
    assert m.generate(x, 16, top_k=1, use_cache=True, kv_fp8=True).shape == (3, 16)  # eager steps
    with pytest.raises(ValueError):
        m.generate(x, 4, top_k=1, kv_fp8=True)


@pytest.mark.parametrize("graph", [False, True])
def test_speculative_bf16_tokens_are_near_argmax(graph):
    """The rule of ``test_generate_chunk_gpu.py::test_speculative_bf16_tokens_are_near_argmax`` with this
    file's bound: every emitted token was the argmax of logits that lie within
    ``E = 2 * (e_q + e_hip) + ulp`` of the fp32 eager logits ``ref``, so ``max(ref) - ref[token] <= 2 E``.
    ``e_q`` is measured along the emitted sequence."""
    import copy

    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(256, 4)).eval()  # (CPU generator: the models of test_generate_chunk_gpu.py)
    x = torch.randint(0, 500, (2, 9))
    noisy = copy.deepcopy(m)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in noisy.parameters():
            if p.dim() > 1:
                p.add_(torch.randn(p.shape, generator=g) * p.std() * 0.08)
    m, noisy, x = m.to(DEV).to(BF16).eval(), noisy.to(DEV).to(BF16).eval(), x.to(DEV)
    m32 = _fp32_twin(m, 256, 4)
    with torch.no_grad():
        out, st = speculative_generate(m, noisy, x, 119, draft_tokens=4, graph=graph, kv_fp8=True)
        assert out.shape == (2, 119) and st["rounds"] > 0
        seq = torch.cat((x, out), dim=1)
        with ops.backend("torch"):
            ref = m32(seq).double()[:, 8:-1]  # the logits each emitted token was chosen from
            a = _stepwise(m32, seq[:, :-1], KVCache(m32, 2, fp8=True)).double()
            e_q = (a - _stepwise(m32, seq[:, :-1], KVCache(m32, 2)).double()).abs().max().item()
        e_hip = (m(seq).double()[:, 8:-1] - ref).abs().max().item()
    E = 2 * (e_q + e_hip) + _ulp(BF16, ref.abs().max().item())
    short = (ref.max(dim=-1).values - ref.gather(-1, out[..., None]).squeeze(-1)).max().item()
    print(f"bf16 graph {graph}: {st} e_hip {e_hip:.4e} e_q {e_q:.4e} E {E:.4e} worst max(ref) - ref[token] {short:.4e}")
    assert short <= 2 * E, (short, E)
