"""The fused sampler (``csrc/ops/sample.hip``) on the GPU against the rule of ``ops/sample.py`` in fp64.

The interval rule: a token ``t`` passes if it is in the fp64 kept set and
``cdf64[t-1] - 1e-5 <= u <= cdf64[t] + 1e-5`` with the CDF normalised. The 1e-5 is derived, not
measured: fp32 ``exp`` on an argument of magnitude below about 40 carries a relative error under 3e-6
and a sum of positive fp32 terms in a blocked order under 2e-6; a wrong index is off by whole
probability masses. At most 2 % of the rows may differ from fp64's own pick (the eager fp32 reference
differs in about 0.2 % on such inputs); no row is skipped."""

import pytest
import torch

from cs336_systems import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
U_TOP = 1.0 - 2.0 ** -24
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _rule64(x, temperature, top_k):
    """fp64, on the CPU: kept (B, V) bool, the unnormalised inclusive prefix sums (B, V) and S (B, 1)."""
    x = x.detach().cpu().double()
    V = x.shape[-1]
    if top_k and top_k < V:
        keep = x >= torch.topk(x, top_k, dim=-1).values[:, -1:]
    else:
        keep = torch.ones_like(x, dtype=torch.bool)
    w = torch.where(keep, torch.exp((x - x.amax(dim=-1, keepdim=True)) / temperature), 0.0)
    c = torch.cumsum(w, dim=-1)
    return keep, c, c[:, -1:]


def _check(tok, u, keep, c, S):
    """Every row obeys the interval rule; returns how many rows differ from fp64's own pick."""
    tok, u = tok.cpu(), u.cpu().double()
    B, V = keep.shape
    assert tok.dtype == torch.int64 and tok.shape == (B,) and bool(((tok >= 0) & (tok < V)).all())
    assert bool(keep.gather(1, tok[:, None]).all()), "a token outside the fp64 kept set"
    cdf = c / S
    hi = cdf.gather(1, tok[:, None])[:, 0]
    lo = torch.where(tok > 0, cdf.gather(1, (tok - 1).clamp(min=0)[:, None])[:, 0], 0.0)
    assert bool(((lo - TOL <= u) & (u <= hi + TOL)).all()), (tok, u, lo, hi)
    pick = ((c > u[:, None] * S) & keep).to(torch.int8).argmax(dim=-1)
    return int((pick != tok).sum())


@pytest.mark.parametrize("dt", DTYPES)
def test_kernel_against_fp64(dt):
    g = torch.Generator().manual_seed(0)
    rows = differ = n = 0
    for V in (1, 7, 63, 64, 65, 1000, 10000, 50257, 65539):
        for B in (1, 5):
            x = (torch.randn(B, V, generator=g) * 4).to(dt).to(DEV)
            for top_k in (None, 1, 2, 50, V, V + 7):
                for temperature in (0.7, 1.0, 1.5):
                    u = torch.rand(B, generator=g)
                    if n % 3 == 0:
                        u[0] = 0.0
                    elif n % 3 == 1:
                        u[-1] = U_TOP
                    n += 1
                    tok = ops.sample_logits(x, u.to(DEV), temperature, top_k)
                    differ += _check(tok, u, *_rule64(x, temperature, top_k))
                    rows += B
    print(f"{dt}: {differ} of {rows} rows differ from the fp64 pick")
    assert differ <= 0.02 * rows, (differ, rows)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("top_k", [3, 10])
def test_ties_and_signed_zeros(dt, top_k):
    g = torch.Generator().manual_seed(1)
    vals = torch.tensor([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, -0.0, 0.0, float("-inf")])
    row = vals[torch.randint(0, len(vals), (64,), generator=g)]
    row[5], row[40] = -0.0, 0.0
    if top_k == 10:
        row = row.clamp(max=0.0)  # the threshold falls on the zeros of both signs
    x = row.to(dt).to(DEV)[None].expand(4096, 64)  # one row, 4096 evenly spaced u
    u = torch.arange(4096, dtype=torch.float32) / 4096
    tok = ops.sample_logits(x, u.to(DEV), 1.0, top_k)
    keep, c, S = _rule64(x, 1.0, top_k)
    _check(tok, u, keep, c, S)
    p = torch.diff(c[0] / S[0], prepend=torch.zeros(1, dtype=torch.float64))
    seen = set(tok.cpu().tolist())
    assert seen <= set(torch.nonzero(keep[0])[:, 0].tolist())
    for i in torch.nonzero(p > 2 / 4096)[:, 0].tolist():
        assert i in seen, (i, float(p[i]))


@pytest.mark.parametrize("dt", DTYPES)
def test_top_k_1_is_argmax(dt):
    g = torch.Generator().manual_seed(2)
    for V in (5, 1000, 50257):
        x = (torch.randn(7, V, generator=g) * 4).to(dt)
        am = torch.randint(0, V, (7,), generator=g)
        x[torch.arange(7), am] = 30.0  # the unique max
        for u in (torch.zeros(7), torch.full((7,), U_TOP), torch.rand(7, generator=g)):
            assert ops.sample_logits(x.to(DEV), u.to(DEV), 0.9, 1).cpu().tolist() == am.tolist()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("V", [10000, 50257])
def test_strided_rows_equal_contiguous_and_determinism(dt, V):
    g = torch.Generator().manual_seed(3)
    full = (torch.randn(4, 3, V, generator=g) * 4).to(dt).to(DEV)
    x = full[:, -1]  # rows 3 V elements apart: at V 50257 not 16-byte aligned
    assert not x.is_contiguous()
    u = torch.rand(4, generator=g).to(DEV)
    for top_k in (None, 1, 40):
        a = ops.sample_logits(x, u, 0.8, top_k)
        assert torch.equal(a, ops.sample_logits(x.clone(), u, 0.8, top_k))
        assert torch.equal(a, ops.sample_logits(x, u, 0.8, top_k))  # the same inputs, the same tokens
        _check(a, u, *_rule64(x, 0.8, top_k))


def test_sample_advance():
    B, S, V, PAD = 3, 6, 1000, 64
    g = torch.Generator().manual_seed(4)
    table = torch.rand(S, B, generator=g).to(DEV)
    # tok, out and done are slices of sentinel-filled allocations: a store outside them shows
    tok_a = torch.full((B + 2 * PAD,), -7, dtype=torch.int64, device=DEV)
    out_a = torch.full((B * S + 2 * PAD,), -7, dtype=torch.int64, device=DEV)
    done_a = torch.full((B + 2 * PAD,), -7, dtype=torch.int32, device=DEV)
    tok, out, done = tok_a[PAD:PAD + B].view(B, 1), out_a[PAD:PAD + B * S].view(B, S), done_a[PAD:PAD + B]
    done.zero_()
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    logits = [(torch.randn(B, 2, V, generator=g) * 4).bfloat16().to(DEV)[:, -1] for _ in range(S)]
    want = [ops.sample_logits(logits[s], table[s], 0.9, 20) for s in range(S)]
    eos = int(want[2][1])  # row 1 ends at step 2 (or earlier, should the token come up before)
    ended = torch.zeros(B, dtype=torch.bool, device=DEV)
    for s in range(S):
        ops.sample_advance(logits[s], table, step, 0.9, 20, eos, tok, out, done)
        exp = torch.where(ended, eos, want[s])
        ended |= exp == eos
        assert torch.equal(out[:, s], exp) and torch.equal(tok[:, 0], exp)
        assert bool((out[:, s + 1:] == -7).all()) and torch.equal(done.bool(), ended)
        assert int(step) == s  # only read: the caller's loop advances it
        step += 1
    assert bool(ended[1])

    def guards_intact():
        return all(bool((a[:PAD] == -7).all()) and bool((a[-PAD:] == -7).all()) for a in (tok_a, out_a, done_a))

    assert guards_intact()
    before = (tok_a.clone(), out_a.clone(), done_a.clone())
    for s in (S, -1):  # outside the table: nothing is stored
        step.fill_(s)
        ops.sample_advance(logits[0], table, step, 0.9, 20, eos, tok, out, done)
        assert all(torch.equal(a, b) for a, b in zip(before, (tok_a, out_a, done_a)))
    done.zero_()
    step.zero_()
    ops.sample_advance(logits[2], table, step, 0.9, 20, -1, tok, out, done)  # no end token: never latches
    assert not bool(done.any()) and torch.equal(tok[:, 0], ops.sample_logits(logits[2], table[0], 0.9, 20))
    assert guards_intact()
    # the eager reference of the op agrees on what is stored where
    tok2, out2, done2 = torch.full_like(tok, -7), torch.full_like(out, -7), torch.zeros_like(done)
    step.fill_(3)
    ops.sample_advance(logits[3], table, step, 0.9, 20, -1, tok, out, done)
    ops.sample_advance_ref(logits[3], table, step, 0.9, 20, -1, tok2, out2, done2)
    assert bool((out2[:, :3] == -7).all()) and bool((out2[:, 4:] == -7).all()) and torch.equal(tok2[:, 0], out2[:, 3])
    _check(out[:, 3], table[3], *_rule64(logits[3], 0.9, 20))
    _check(out2[:, 3], table[3], *_rule64(logits[3], 0.9, 20))
