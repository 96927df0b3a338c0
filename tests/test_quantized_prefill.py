"""``weights=`` on the cached forwards and ``generate(quantized_prefill=True)`` on the CPU, where the
quantized linears are the reference ones (``ops.skinny_linear_fp8_ref`` / ``skinny_linear_mxfp4_ref``). The
bound is that of ``test_decode_graph_fp8_gpu.py``: ``e16`` is the worst error of the bf16 model's forward
against the fp32 forward of its own weights, and the quantized prefill may be off by ``2 * e16 + ulp`` from
the fp32 forward of the dequantized weights."""

import math

import pytest
import torch

from cs336_systems.models import BasicsTransformerLM, DecodeGraph, Fp8DecodeWeights, Mxfp4DecodeWeights
from cs336_systems.models.kv_cache import KVCache

CFG = dict(vocab_size=97, context_length=32, d_model=64, num_layers=2, num_heads=2, d_ff=96, rope_theta=10000.0)
CLASSES = [Fp8DecodeWeights, Mxfp4DecodeWeights]


def _model(seed):
    torch.manual_seed(seed)
    return BasicsTransformerLM(**CFG).to(torch.bfloat16).eval()


def _greedy(logits):
    """``generate``'s own sampling at ``top_k=1``: a tie at the top is drawn from the generator."""
    from cs336_systems.models import softmax

    logits = logits[:, -1].float()
    logits = logits.masked_fill(logits < logits.max(dim=-1, keepdim=True).values, float("-inf"))
    return torch.multinomial(softmax(logits, dim=-1), 1)


@pytest.mark.parametrize("cls", CLASSES)
def test_cached_forwards_read_the_quantized_copy(cls):
    m = _model(3)
    qw = cls(m)
    x = torch.randint(0, 97, (2, 12))
    m32 = BasicsTransformerLM(**CFG).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad():
        e16 = (m(x).double() - m32(x).double()).abs().max().item()
        m32.load_state_dict(qw.dequantized_state_dict(torch.float32))
        ref = m32(x).double()
    ulp = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 7)
    cache, plain = KVCache(m, 2), KVCache(m, 2)
    first = m.forward_cached(x[:, :8], cache, weights=qw)
    rest = m.extend_cached(x[:, 8:], cache, weights=qw)
    e = (torch.cat((first, rest), dim=1).double() - ref).abs().max().item()
    assert e <= 2 * e16 + ulp, (e, e16, ulp)
    assert not torch.equal(first, m.forward_cached(x[:, :8], plain))  # the 16-bit prefill is another function
    again = KVCache(m, 2)
    m.forward_cached(x[:, :8], again, weights=qw)
    e = (m.verify_cached(x[:, 8:], again, weights=qw).double() - ref[:, 8:]).abs().max().item()
    assert e <= 2 * e16 + ulp, (e, e16, ulp)


@pytest.mark.parametrize("cls", CLASSES)
def test_generate_quantized_prefill(cls):
    m = _model(4)
    qw = cls(m)
    x = torch.randint(0, 97, (2, 9))
    with pytest.raises(ValueError, match="weights"):
        m.generate(x, 4, top_k=1, use_cache=True, quantized_prefill=True)
    dg = DecodeGraph(m, KVCache(m, 2), capture=False, weights=qw)

    def generate(**kw):
        torch.manual_seed(7)
        return m.generate(x, 6, top_k=1, use_cache=True, graph=dg, **kw)

    def by_hand(prefill_weights, pieces):
        torch.manual_seed(7)
        cache = KVCache(m, 2)
        de = DecodeGraph(m, cache, capture=False, weights=qw)
        logits = m.forward_cached(x[:, :pieces], cache, weights=prefill_weights)
        for s in range(pieces, x.shape[1], pieces):
            logits = m.extend_cached(x[:, s:s + pieces], cache, weights=prefill_weights)
        toks = [_greedy(logits)]
        for _ in range(5):
            toks.append(_greedy(de.step(toks[-1])))
        return torch.cat(toks, dim=1)

    # the default is today's generation: a 16-bit prefill, quantized steps
    assert torch.equal(generate(), by_hand(None, 9))
    assert torch.equal(generate(weights=qw), by_hand(None, 9))
    got = generate(weights=qw, quantized_prefill=True)
    assert torch.equal(got, by_hand(qw, 9))
    got = generate(weights=qw, quantized_prefill=True, prefill_chunk=4)
    assert torch.equal(got, by_hand(qw, 4))
