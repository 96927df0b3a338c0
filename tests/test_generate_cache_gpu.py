"""KV-cached forward and generation on the GPU (HIP kernels) against the fp32 eager forward.

Yardstick: the fp32 full forward of the same weights on the eager PyTorch backend. With ``e_hip``
the max logit error of the existing uncached HIP forward against it, the cached path (prefill +
teacher-forced steps) must stay within ``2 * e_hip + ulp``, ``ulp`` one unit in the last place of the
compute dtype at the largest reference logit: the cached path rounds where the uncached one does and
differs in reduction order, so twice the existing path's own error separates reordering noise from a
wrong key range or RoPE position (which moves logits by whole units)."""

import math
from unittest import mock

import pytest
import torch

from cs336_systems import ops
from cs336_systems.models import BasicsTransformerLM
from cs336_systems.models.kv_cache import KVCache

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _cfg(d_model, heads):
    return dict(vocab_size=500, context_length=128, d_model=d_model, num_layers=2, num_heads=heads, d_ff=512,
                rope_theta=10000.0)


def _ulp(dt, x):
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dt]
    return 2.0 ** (math.floor(math.log2(x)) - mant)


@pytest.mark.parametrize("d_model,heads,dt", [(256, 4, torch.bfloat16), (160, 2, torch.bfloat16), (256, 4, torch.float32)])
def test_teacher_forced_error_against_fp32(d_model, heads, dt):
    torch.manual_seed(0)
    m = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).to(dt).eval()
    seq = torch.randint(0, 500, (2, 128), device=DEV)
    # yardstick: the same (rounded) weights in fp32 on the eager backend
    m32 = BasicsTransformerLM(**_cfg(d_model, heads), device=DEV).eval()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    with torch.no_grad(), ops.backend("torch"):
        ref = m32(seq).double()[:, 8:]  # logits at positions 8 .. 127
    with torch.no_grad():
        full = m(seq)
        assert full.dtype == dt
        e_hip = (full.double()[:, 8:] - ref).abs().max().item()
        cache = KVCache(m, 2)
        assert cache.dtype == dt
        rows = [m.forward_cached(seq[:, :9], cache)[:, -1]]
        for n in range(9, 128):
            rows.append(m.forward_cached(seq[:, n:n + 1], cache)[:, -1])
        assert cache.length == 128 and cache.lengths.tolist() == [128, 128]
    cached = torch.stack(rows, dim=1)
    assert cached.dtype == dt and cached.shape == ref.shape
    e_cached = (cached.double() - ref).abs().max().item()
    ulp = _ulp(dt, ref.abs().max().item())
    print(f"d_model {d_model} heads {heads} {dt}: e_hip {e_hip:.4e} e_cached {e_cached:.4e} ulp {ulp:.3e} "
          f"max|ref| {ref.abs().max().item():.3f}")
    assert e_cached <= 2 * e_hip + ulp, (e_cached, e_hip, ulp)


@pytest.mark.parametrize("batch", [1, 3])
def test_generate_with_cache_shapes_past_the_window(batch):
    torch.manual_seed(1)
    m = BasicsTransformerLM(**_cfg(256, 4), device=DEV).to(torch.bfloat16).eval()
    x = torch.randint(0, 500, (batch, 9), device=DEV)
    out = m.generate(x, 125, top_k=5, use_cache=True)  # 9 + 125 > context_length 128
    assert out.shape == (batch, 125) and out.dtype == torch.int64 and out.is_cuda
    assert int(out.min()) >= 0 and int(out.max()) < 500
    out = m.generate(x[0], 4, use_cache=True)
    assert out.shape == (1, 4)


def test_cached_step_runs_the_hip_ops():
    """Every step calls decode_attention and kv_append_rope once per layer, and they go to the HIP
    ops (the eager references are never entered)."""
    from cs336_systems.ops import decode as dec

    torch.manual_seed(2)
    m = BasicsTransformerLM(**_cfg(160, 2), device=DEV).to(torch.bfloat16).eval()
    x = torch.randint(0, 500, (2, 12), device=DEV)
    cache = KVCache(m, 2)
    boom = AssertionError("the eager reference ran on the GPU path")
    with mock.patch.object(ops, "decode_attention", wraps=ops.decode_attention) as att, \
            mock.patch.object(ops, "kv_append_rope", wraps=ops.kv_append_rope) as app, \
            mock.patch.object(dec, "decode_attention_ref", side_effect=boom), \
            mock.patch.object(dec, "kv_append_rope_ref", side_effect=boom):
        m.forward_cached(x[:, :9], cache)
        assert att.call_count == 0 and app.call_count == 0  # the prefill is the ordinary attention
        for i in range(3):
            m.forward_cached(x[:, 9 + i:10 + i], cache)
            assert att.call_count == 2 * (i + 1) and app.call_count == 2 * (i + 1)
    assert cache.length == 12
