"""CPU test of what ``test_gemm_edges_gpu.py`` holds the training GEMMs to: its reference helpers (SwiGLU
forward and backward, the interleaved rotation, the either-neighbour fallback), its integer generators, the
per-split token ranges and the table of gemm8w cases, and the rule's teeth on GEMM-shaped mistakes.

The stand-in for a correct kernel is ``ref32`` rounded to the output type: it must pass ``check`` at k = 4,
and each mutation of it (an element moved by 3 ulps, swapped 8-column chunks, swapped SwiGLU halves, a dropped
8-wide k-chunk, an unrounded ``dh`` in epi 2, a slab over a token range one k-tile off) must fail."""

import pytest
import torch

from .test_gemm_edges_gpu import (BF16, BK, DW_CASES, DW_INT, EITHER_NEIGHBOUR, F32, F64, GEMM_K_CASE, ORIENTATIONS, PLAIN_GRID, PLAIN_INT,
                                  PLAIN_K, TILES, bf16_neighbours, check, check_either, dw_refs, dw_refused, int_bf16, other_neighbour,
                                  pair_alternates, pick_fn, plain_refs, randn_bf16, rope_rotate_ref, rope_tables, split_ranges,
                                  swiglu_bwd_ref, swiglu_fwd_ref, tile_operands, tile_refs)

CPU = "cpu"


def _fails(got, ref64, ref32, dt):
    with pytest.raises(pytest.fail.Exception, match="worst element|finiteness differs"):
        check(got, ref64, ref32, dt, None, 4.0)


def _ulp_bf16(x):
    return 2.0 ** (torch.floor(torch.log2(x.abs().double())) - 7)


def test_swiglu_backward_matches_autograd():
    g = torch.Generator().manual_seed(0)
    y = (3 * torch.randn(7, 16, generator=g)).to(BF16)
    dh = torch.randn(7, 8, generator=g).to(BF16)
    y64 = y.double().requires_grad_(True)
    h = torch.nn.functional.silu(y64[:, :8]) * y64[:, 8:]
    h.backward(dh.double())
    da, db = swiglu_bwd_ref(dh, y, 8, F64)
    torch.testing.assert_close(torch.cat((da, db), 1), y64.grad, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(swiglu_fwd_ref(y, 8, F64), h.detach(), rtol=1e-14, atol=0)
    # the fp32 evaluations are the same formulas within fp32's precision
    torch.testing.assert_close(swiglu_bwd_ref(dh, y, 8, F32)[0].double(), da, rtol=1e-5, atol=1e-6)


def test_rotation_matches_rope_ref():
    from cs336_systems.ops import rope_ref

    M, H, dk, ctx = 12, 3, 16, 20
    g = torch.Generator().manual_seed(1)
    plain = torch.randn(M, 3 * H * dk, generator=g).to(BF16)
    pos = torch.randint(0, ctx, (M,), generator=g)
    cos, sin = rope_tables(ctx, dk, CPU)
    rope_cols = 2 * H * dk
    got = rope_rotate_ref(plain, cos, sin, pos, rope_cols, dk, F64)
    heads = plain.double()[:, :rope_cols].view(M, 2 * H, dk).transpose(0, 1)  # (heads, seq = M, dk)
    ref = rope_ref(heads, cos.double(), sin.double(), pos).transpose(0, 1).reshape(M, rope_cols)
    assert torch.equal(got[:, :rope_cols], ref)
    assert torch.equal(got[:, rope_cols:], plain.double()[:, rope_cols:])
    assert not torch.equal(got[:, :rope_cols], plain.double()[:, :rope_cols])


def test_plain_product_mutations_fail():
    M, N, K = 64, 48, 192
    a, b = randn_bf16(M, K, seed=1, device=CPU), randn_bf16(N, K, seed=2, device=CPU)
    r64, r32 = plain_refs(a, b)
    good = r32.to(BF16)
    check(good, r64, r32, BF16, None, 4.0)
    check(r32, r64, r32, F32, None, 4.0)
    # one element moved by 3 bf16 ulps
    i = int(r64.abs().argmax())
    bad = good.clone().double()
    bad.view(-1)[i] += 3 * _ulp_bf16(bad.view(-1)[i])
    _fails(bad, r64, r32, BF16)
    mid = good.clone().double()
    r, c = 5, 7
    mid[r, c] += 3 * _ulp_bf16(mid[r, c])  # and an ordinary element
    _fails(mid, r64, r32, BF16)
    # two adjacent 8-column chunks of one row swapped
    bad = good.clone()
    bad[9, 16:24], bad[9, 24:32] = good[9, 24:32], good[9, 16:24]
    _fails(bad, r64, r32, BF16)
    # the contribution of one 8-wide k-chunk removed from one row
    a2 = a.clone()
    a2[11, 64:72] = 0
    bad = good.clone()
    bad[11] = (a2[11].float() @ b.float().t()).to(BF16)
    _fails(bad, r64, r32, BF16)
    bad32 = r32.clone()
    bad32[11] = a2[11].float() @ b.float().t()
    _fails(bad32, r64, r32, F32)


def test_swiglu_mutations_fail():
    M, half, K = 64, 32, 64
    x, w13 = randn_bf16(M, K, seed=3, device=CPU), randn_bf16(2 * half, K, 0.1, seed=4, device=CPU)
    y = plain_refs(x, w13)[1].to(BF16)
    h64, h32 = swiglu_fwd_ref(y, half, F64), swiglu_fwd_ref(y, half, F32)
    good = h32.to(BF16)
    check(good, h64, h32, BF16, None, 4.0)
    # the a and b halves of one row of h's input exchanged
    ysw = y.clone()
    ysw[13] = torch.cat((y[13, half:], y[13, :half]))
    bad = good.clone()
    bad[13] = swiglu_fwd_ref(ysw, half, F32)[13].to(BF16)
    _fails(bad, h64, h32, BF16)


def test_unrounded_dh_fails():
    """epi 2 rounds dh to bf16 before the SwiGLU backward. An evaluation from the unrounded fp32 dh differs
    from the reference (built from the rounded dh) by up to half a bf16 ulp of dh on top of its own rounding:
    on these inputs more than 1 % of the elements leave the bound, so the case cannot pass by leaving
    everything out."""
    M, half, K = 128, 64, 192
    dy, w2t = randn_bf16(M, K, seed=5, device=CPU), randn_bf16(half, K, 0.1, seed=6, device=CPU)
    y = randn_bf16(M, 2 * half, seed=7, device=CPU)
    dh32 = plain_refs(dy, w2t)[1]
    dh = dh32.to(BF16)
    for i in range(2):
        r64, r32 = swiglu_bwd_ref(dh, y, half, F64)[i], swiglu_bwd_ref(dh, y, half, F32)[i]
        check(r32.to(BF16), r64, r32, BF16, None, 4.0)
        bad = swiglu_bwd_ref(dh32, y, half, F32)[i].to(BF16)
        e32 = max((r32.double() - r64).abs().max().item(), 2.0**-23 * r64.abs().max().item())
        out = (bad.double() - r64).abs() > 4 * e32 + 2.0**-8 * r64.abs() + torch.finfo(BF16).tiny
        share = out.double().mean().item()
        assert share >= 0.01, share
        _fails(bad, r64, r32, BF16)


def test_slab_range_mutation_fails():
    K, M, N = 320, 16, 32
    a, b = randn_bf16(K, M, seed=8, device=CPU), randn_bf16(K, N, seed=9, device=CPU)
    assert split_ranges(320, 2) == [(0, 128), (128, 320)] and split_ranges(320, 3) == [(0, 64), (64, 192), (192, 320)]
    assert split_ranges(64, 3) == [(0, 0), (0, 0), (0, 64)] and split_ranges(128, 1) == [(0, 128)]
    for splits in (1, 2, 3, 5):
        for K_ in (64, 128, 192, 320):
            r = split_ranges(K_, splits)
            assert r[0][0] == 0 and r[-1][1] == K_ and all(r[i][1] == r[i + 1][0] for i in range(splits - 1))
            assert all(k0 % BK == 0 and k1 % BK == 0 and k0 <= k1 for k0, k1 in r)
    k0, k1 = split_ranges(K, 3)[1]
    r64, r32 = dw_refs(a, b, k0, k1)
    check(r32, r64, r32, F32, None, 4.0)
    for shift in (-BK, BK):  # the slab over a token range one k-tile off
        _fails(dw_refs(a, b, k0 + shift, k1 + shift)[1], r64, r32, F32)
    _fails(dw_refs(a, b, k0, k1 + BK)[1], r64, r32, F32)  # one k-tile too many
    # the slabs of every split sum to the whole product
    total = sum(dw_refs(a, b, *r)[0] for r in split_ranges(K, 3))
    torch.testing.assert_close(total, dw_refs(a, b)[0], rtol=1e-13, atol=1e-12)


def test_integer_generators_stay_exact():
    """|sum| <= 256 for the bf16 outputs (every integer up to 256 is a bf16 value), < 2^24 for fp32, for
    every K of the tables; and the fp32 product of such operands is the exact one."""
    for K in PLAIN_K:
        a, b = int_bf16(40, K, PLAIN_INT, seed=1, device=CPU), int_bf16(24, K, PLAIN_INT, seed=2, device=CPU)
        assert a.abs().max() == 1 and set(a.unique().tolist()) == {-1.0, 0.0, 1.0}
        r64, r32 = plain_refs(a, b)
        assert (a.double().abs() @ b.double().abs().t()).max() <= min(K, 256) and K <= 256
        assert torch.equal(r32.double(), r64) and torch.equal(r32.to(BF16).double(), r64)
    for K in sorted({c[0] for c in DW_CASES} | {128}):
        a, b = int_bf16(K, 40, DW_INT, seed=1, device=CPU), int_bf16(K, 24, DW_INT, seed=2, device=CPU)
        assert a.abs().max() == DW_INT
        assert (a.double().abs().t() @ b.double().abs()).max() <= K * DW_INT**2 < 2**24
        r64, r32 = dw_refs(a, b)
        assert torch.equal(r32.double(), r64)
    for ta, tb in ORIENTATIONS:
        a, b = tile_operands(32, 24, 64, ta, tb, lambda r, c, s: int_bf16(r, c, PLAIN_INT, seed=s, device=CPU))
        r64, r32 = tile_refs(a, b, ta, tb)
        assert r64.shape == (32, 24) and r64.abs().max() <= 64 and torch.equal(r32.to(BF16).double(), r64)
    assert len(TILES) == 4 and len(ORIENTATIONS) == 3


def test_dw_table_covers_every_axis():
    """Over the rows that reach the kernel: a refused row runs nothing, so it covers nothing."""
    ks, ms, nfs = (64, 128, 192, 320), (8, 248, 256, 264, 520), ((256, 0), (320, 0), (640, 5), (640, 0))
    run = [c for c in DW_CASES if not dw_refused(c[2], c[3])]
    for axis, values in ((lambda c: c[0], ks), (lambda c: c[1], ms), (lambda c: (c[2], c[3]), nfs)):
        assert {axis(c) for c in run} == set(values)
        for v in values:
            rows = [c for c in run if axis(c) == v]
            assert {c[4] for c in rows} == {False, True}, v
            assert {c[5] for c in rows} == {1, 2, 3}, v
    assert {(c[0], c[5]) for c in run} >= {(320, 2), (320, 3)}  # uneven ranges
    assert {(c[1], c[4]) for c in run} >= {(520, False), (520, True)}  # a padded third row tile, both stores
    assert len(set(DW_CASES)) == len(DW_CASES)
    # a forced width that does not divide N is refused by the launcher: only 640 at 256, pinned plain and transposed
    refused = [c for c in DW_CASES if dw_refused(c[2], c[3])]
    assert {(c[2], c[3]) for c in refused} == {(640, 4)} and {c[4] for c in refused} == {False, True} and len(refused) == 2
    assert not dw_refused(640, 5) and not dw_refused(640, 0) and not dw_refused(256, 4) and dw_refused(320, 4)
    assert all(c[1] % 8 == 0 and c[0] % BK == 0 for c in DW_CASES)


def test_plain_grid_and_pick_fn():
    for fn, bn in ((4, 256), (5, 320)):
        assert {n for f, n in PLAIN_GRID if f == fn} == {bn, 2 * bn, 8, bn - 8, bn + 8, 2 * bn + 8}
    assert PLAIN_K == (8, 56, 64, 72, 128, 136, 192, 200)
    assert [pick_fn(n) for n in (256, 320, 640, 328, 1032, 8, 12)] == [4, 5, 5, 4, 5, 4, 0]
    assert pick_fn(384, 1, 192) == 0 and pick_fn(1280, 1, 640) == 5 and pick_fn(512, 1, 256) == 4
    assert pick_fn(960, 3, 640) == 5


def test_neighbours_and_either_fallback():
    p = torch.tensor([1.0, 1.0 + 2.0**-8, 1.0 + 2.0**-7, -3.3, 0.0, 1e-3, 300.7], dtype=F64)
    lo, hi = bf16_neighbours(p)
    assert (lo.double() <= p).all() and (hi.double() >= p).all()
    exact = p.float().to(BF16).double() == p
    assert torch.equal(lo == hi, exact)
    gap = hi.double() - lo.double()
    assert torch.all(gap[~exact] == 2.0 ** (torch.floor(torch.log2(p[~exact].abs())) - 7))
    # a product just above a midpoint that the kernel's fp32 sum put just below it
    mid = 1.0 + 2.0**-8
    p64 = torch.tensor([mid + 1e-7, mid + 1e-3, 2.5], dtype=F64)
    kernel = torch.tensor([1.0, 1.0, 2.5], dtype=BF16)  # the lower neighbour for the first two
    other, allowed = other_neighbour(kernel, p64, e32=1e-7)
    assert other.tolist() == [1.0 + 2.0**-7, 1.0 + 2.0**-7, 2.5] and allowed.tolist() == [True, False, False]
    f = lambda t, ft: 3 * t.to(ft)  # noqa: E731  (an element-wise epilogue)
    got = f(other, F32).to(BF16)  # an epilogue that started from the other neighbour everywhere
    primary = (f(kernel, F64), f(kernel, F32))
    _fails(got, *primary, BF16)
    alts = [(f(other, F64), f(other, F32), allowed)]
    with pytest.raises(pytest.fail.Exception, match=r"worst element \(1,\)"):  # outside the cap it is still an error
        check_either(got, primary, alts, BF16, None, 4.0)
    ok = got.clone()
    ok[1] = f(kernel, F32).to(BF16)[1]
    ratio, n = check_either(ok, primary, alts, BF16, None, 4.0)
    assert n == 1 and ratio <= 4
    # pairs: an output may take an alternate only if every replaced input of its pair may
    plain = torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=BF16)
    oth = torch.tensor([[1.5, 2.5, 3.5, 4.5]], dtype=BF16)
    allow = torch.tensor([[True, False, True, True]])
    rot = lambda t, ft: torch.stack((t.to(ft)[:, 0::2] - t.to(ft)[:, 1::2], t.to(ft)[:, 0::2] + t.to(ft)[:, 1::2]), -1).reshape(1, 4)  # noqa: E731
    (a0, _, ok0), (a1, _, ok1), (a2, _, ok2) = pair_alternates(plain, oth, allow, rot)
    assert ok0.tolist() == [[True, True, True, True]] and ok1.tolist() == [[False, False, True, True]]
    assert ok2.tolist() == [[False, False, True, True]]
    assert a0.tolist() == [[-0.5, 3.5, -0.5, 7.5]] and a1.tolist() == [[-1.5, 3.5, -1.5, 7.5]] and a2.tolist() == [[-1.0, 4.0, -1.0, 8.0]]


def test_margins_follow_the_rule():
    assert all(k in (8, 16, 32) for k in GEMM_K_CASE.values())
    assert all(op.split(".")[0] in ("gemm8", "gemm8w", "gemm") for op in GEMM_K_CASE)
    assert all(op in ("gemm8.da", "gemm8.db", "gemm8.rope") for op in EITHER_NEIGHBOUR)
