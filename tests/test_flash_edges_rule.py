"""CPU test of what ``test_flash_edges_gpu.py`` holds the FlashAttention-2 kernels to: its references
(``attn_ref``), its value generators and the banded rule (``check_banded``), run on the CPU against an
FA2 emulation that is independent of the code under test.

The emulation (``fa2_emulate``) is an online-softmax forward over 64- or 32-key tiles with fp32
accumulators and the unnormalised P rounded to the input type per tile, and a tiled backward with
rounded P and dS that takes O and LSE from the emulated forward. It must pass the rule at k = 4 for
every value generator and on cross-length pairs; its four mutations (last key tile skipped, last query
tile skipped, causal mask off by one, delta omitted) must fail it. So the rule is neither vacuous nor
tighter than a correct implementation can meet."""

import pytest
import torch

from .test_flash_edges_gpu import (BF16, F16, F32, FA_K_CASE, FUSED, GENERATORS, HS, KP, TWO_KERNEL, VALUE_GENERATORS, _rnd, attn_ref,
                                   check, check_banded, expected_bwd_splits, expected_form, expected_fwd_splits, make_case)

CPU = "cpu"
MUTATIONS = ("skip_key_tile", "skip_query_tile", "mask_off_by_one", "no_delta")


def fa2_emulate(c, bn=64, mutation=None):
    """(O, LSE, dQ, dK, dV) of an FA2 implementation in the input type of case ``c``."""
    dt = c.dt
    q, k, v, do = (t.float() for t in (c.q, c.k, c.v, c.do))
    sc = torch.tensor(c.scale, dtype=F32).item()
    Nq, Nk = q.shape[2], k.shape[2]
    rows = torch.arange(Nq)[:, None]
    shift = 1 if mutation == "mask_off_by_one" else 0
    tiles = list(range(0, Nk, bn))
    if mutation == "skip_key_tile":
        tiles = tiles[:-1]
    live_q = Nq - ((Nq - 1) % 64 + 1) if mutation == "skip_query_tile" else Nq  # rows before the last 64-query tile

    def scores(j0):
        s = q @ k[:, :, j0 : j0 + bn].transpose(-1, -2) * sc
        if c.causal:
            s = s.masked_fill(torch.arange(j0, min(j0 + bn, Nk))[None, :] > rows + shift, float("-inf"))
        return s

    m = torch.full(q.shape[:3] + (1,), float("-inf"))
    l = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for j0 in tiles:
        s = scores(j0)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)  # rows with no visible key yet
        p = torch.exp(s - safe)
        alpha = torch.exp(m - safe)
        l = alpha * l + p.sum(-1, keepdim=True)
        acc = alpha * acc + _rnd(p, dt) @ v[:, :, j0 : j0 + bn]
        m = m_new
    o = (acc / l).to(dt)
    lse = (m + torch.log(l))[..., 0]
    if live_q < Nq:
        o[:, :, live_q:] = 0
        lse[:, :, live_q:] = 0

    of = o.float()
    delta = (do * of).sum(-1, keepdim=True)
    if mutation == "no_delta":
        delta = torch.zeros_like(delta)
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k)
    dv = torch.zeros_like(v)
    for j0 in tiles:
        p = torch.exp(scores(j0) - lse[..., None])
        p[:, :, live_q:] = 0
        ds = _rnd(p * (do @ v[:, :, j0 : j0 + bn].transpose(-1, -2) - delta), dt)
        dv[:, :, j0 : j0 + bn] = _rnd(p, dt).transpose(-1, -2) @ do
        dk[:, :, j0 : j0 + bn] = ds.transpose(-1, -2) @ q * sc
        dq += ds @ k[:, :, j0 : j0 + bn]
    return o, lse, (dq * sc).to(dt), dk.to(dt), dv.to(dt)


def _apply_rule(c, out, k=None):
    """The five comparisons the GPU tests make; returns the largest ratio."""
    o, lse, dq, dk, dv = out
    r = [check_banded(o, c.r64.o, c.rw.o, c.dt, None, k), check_banded(lse, c.r64.lse, c.rw.lse, F32, None, k)]
    for got, r64, rw, mag in ((dq, c.r64.dq, c.rw.dq, c.mdq), (dk, c.r64.dk, c.rw.dk, c.mdk), (dv, c.r64.dv, c.rw.dv, None)):
        r.append(check_banded(got, r64, rw, c.dt, None, k, mag=mag))
    return max(r)


def _fails(c, out):
    with pytest.raises(pytest.fail.Exception, match="worst element|finiteness differs"):
        _apply_rule(c, out, k=4.0)


VALUE_PARAMS = [(dt, gen) for dt in (F32, BF16, F16) for gen in VALUE_GENERATORS if gen != "bigdo" or dt == F16]


@pytest.mark.parametrize("dt,gen", VALUE_PARAMS, ids=str)
def test_emulation_passes_on_value_generators(dt, gen):
    """Every generator keeps ref64 and refw finite together (check_banded's own assert) and a correct
    FA2 evaluation meets the rule at k = 4 on it, at N 256 and at (130, 67), with 64- and 32-key tiles."""
    for Nq, Nk in ((256, 256), (130, 67)):
        for causal in (False, True):
            c = make_case(gen, 1, 2, Nq, Nk, 64, dt, causal, CPU)
            for ref in (c.r64, c.rw):
                assert all(torch.isfinite(t).all() for t in ref), gen
            for bn in (64, 32):
                _apply_rule(c, fa2_emulate(c, bn), k=4.0)


@pytest.mark.parametrize("Nq,Nk", [(1, 300), (67, 130), (257, 64), (256, 256)])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=str)
def test_emulation_passes_and_mutations_fail(dt, Nq, Nk):
    for causal in (False, True):
        c = make_case("randn", 2, 2, Nq, Nk, 64, dt, causal, CPU)
        _apply_rule(c, fa2_emulate(c), k=4.0)
        for mutation in MUTATIONS:
            if mutation == "mask_off_by_one" and (not causal or Nk < 2):
                continue
            if mutation == "skip_key_tile" and causal and Nk - (Nk - 1) % 64 - 1 >= Nq:
                continue  # the last key tile is wholly above the diagonal: skipping it is correct
            if mutation == "skip_query_tile" and Nq <= 64:
                continue  # it is the only tile: covered by the pairs with Nq > 64
            _fails(c, fa2_emulate(c, mutation=mutation))


def test_check_banded_is_check_per_band():
    """The vectorised evaluation gives the ratio of ``check`` applied to each (batch, head, band) on its
    own, a late-row error that a tensor-wide E would hide fails, and an exact-zero band demands zeros."""
    c = make_case("randn", 2, 2, 200, 130, 64, BF16, True, CPU)
    o, lse, dq, dk, dv = fa2_emulate(c)
    for got, r64, rw, dt in ((o, c.r64.o, c.rw.o, BF16), (lse, c.r64.lse, c.rw.lse, F32), (dk, c.r64.dk, c.rw.dk, BF16)):
        N = got.shape[2]
        per_band = max(check(got[b, h, n : n + 64], r64[b, h, n : n + 64], rw[b, h, n : n + 64], dt, None)
                       for b in range(2) for h in range(2) for n in range(0, N, 64))
        assert check_banded(got, r64, rw, dt, None) == pytest.approx(per_band, rel=1e-12)
    # causal rows 0..63 of O are large (few keys), rows 192..199 small: an error of 8 E_band there
    bad = o.clone().double()
    e_late = (c.rw.o[0, 1, 192:] - c.r64.o[0, 1, 192:]).abs().max().item()
    bad[0, 1, 195, 7] += 8 * e_late + 2 * 2.0**-8 * abs(c.r64.o[0, 1, 195, 7].item())
    check(bad, c.r64.o, c.rw.o, BF16, None)  # the tensor-wide rule lets it through
    with pytest.raises(pytest.fail.Exception, match=r"batch 0 head 1 rows 192\.\.199 of 200 .*worst element \(3, 7\)"):
        check_banded(bad, c.r64.o, c.rw.o, BF16, None)
    # keys past the last query: dK = dV = 0 exactly in both references
    c = make_case("randn", 1, 2, 33, 200, 64, F16, True, CPU)
    assert torch.all(c.r64.dk[:, :, 64:] == 0) and torch.all(c.rw.dv[:, :, 64:] == 0)
    out = list(fa2_emulate(c))
    _apply_rule(c, out)
    out[3] = out[3].clone()
    assert torch.all(c.mdk[:, :, 33:] == 0)  # the floor from M is 0 there too
    out[3][0, 1, 150, 3] = 2.0**-13  # a tenth of the smallest normal fp16 would pass; this must not
    with pytest.raises(pytest.fail.Exception, match="rows 128..191"):
        _apply_rule(c, out)


def test_cancellation_floor():
    """One visible key (N 1; row 0 under the causal mask): dP = delta exactly, dQ = dK = 0 in fp64, and
    E without the floor from M is at the mercy of how refw's two dot products round. With the floor a
    perturbation of dS by one fp32 ulp of |dP| + |delta| passes and one of 2^-16 |dP| does not."""
    c = make_case("randn", 2, 2, 1, 1, 64, BF16, False, CPU)
    assert torch.all(c.r64.dq == 0) and torch.all(c.r64.dk == 0) and (c.mdq.amax(-1) > 0.01).all()
    o, lse, dq, dk, dv = fa2_emulate(c)
    dp = (c.do.double() * c.v.double()).sum(-1, keepdim=True)
    for eps, ok in ((2.0**-24, True), (2.0**-16, False)):
        noisy = (dq.double() + 2 * eps * dp.abs() * c.k.double() * c.scale).float()
        if ok:
            check_banded(noisy, c.r64.dq, c.rw.dq, F32, None, mag=c.mdq)
        else:
            with pytest.raises(pytest.fail.Exception, match="worst element"):
                check_banded(noisy, c.r64.dq, c.rw.dq, F32, None, mag=c.mdq)
    for gen in VALUE_GENERATORS[:-1]:
        c = make_case(gen, 1, 2, 130, 67, 64, F32, True, CPU)
        assert (c.mdq >= c.r64.dq.abs()).all() and (c.mdk >= c.r64.dk.abs()).all(), gen


def test_generators_do_what_they_say():
    for causal in (False, True):
        mk = lambda gen, dt=BF16: make_case(gen, 1, 2, 256, 256, 64, dt, causal, CPU)  # noqa: E731
        c = mk("vconst")
        assert (c.r64.o - c.v.double()[:, :, :1]).abs().max() < 1e-12 and c.r64.dq.abs().max() < 1e-12 and c.r64.dk.abs().max() < 1e-12
        assert c.r64.dv.abs().max() > 0.1
        for gen in ("qzero", "ties"):
            c = mk(gen)
            n = torch.arange(1, 257, dtype=torch.float64) if causal else torch.full((256,), 256.0, dtype=torch.float64)
            lse0 = c.r64.lse - (c.q.double() @ c.k.double().transpose(-1, -2))[..., 0] * c.scale
            assert (lse0 - torch.log(n)).abs().max() < 1e-9, gen
        c = mk("dominant")
        j = 0 if causal else 170
        assert torch.equal(c.rw.o, c.v[:, :, j : j + 1].float().expand_as(c.rw.o))  # the other P are 0 in fp32
        assert (c.r64.o - c.v[:, :, j : j + 1].double()).abs().max() < 1e-40
        c = mk("ramp")
        s = c.q.double() @ c.k.double().transpose(-1, -2) * c.scale / 0.6931471805599453
        tile_max = torch.stack([s[..., 255, j : j + 64].amax(-1) for j in range(0, 256, 64)], -1)
        rise = tile_max[..., 1:] - tile_max[..., :-1]
        assert (rise > 2).all() and (rise < 8).all() and (tile_max[..., 2:] - tile_max[..., :-2] > 8).all(), rise
        c = mk("spike")
        s = (c.q.double() @ c.k.double().transpose(-1, -2) * c.scale / 0.6931471805599453)[..., 192:, :]
        jump = s[..., 254] - s[..., :254].amax(-1)
        assert (jump[..., 0::3] > 8).all() and (jump[..., 1::3] < 4).all() and (jump[..., 2::3] < 4).all()
        for gen, off in (("scores-1e3", -1e3), ("scores+1e3", 1e3)):
            c = mk(gen)
            s = c.q.double() @ c.k.double().transpose(-1, -2) * c.scale
            assert (s - off).abs().max() < 40, gen
        c = mk("dozero")
        assert all(torch.all(t == 0) for r in (c.r64, c.rw) for t in (r.dq, r.dk, r.dv))
        c = mk("bigdo", F16)
        assert c.do.abs().max() > 1024 and torch.isfinite(c.do).all()
        twice = (c.do.float() * 2).to(F16)
        assert not torch.isfinite(twice).all() or not all(
            torch.isfinite(t.to(F16)).all() for r in (attn_ref(c.q, c.k, c.v, twice, causal, c.scale, F32, F16),
                                                      attn_ref(c.q, c.k, c.v, twice, causal, c.scale, torch.float64, F32)) for t in r[2:])


def test_expected_form_table():
    """The selection table of the GPU tests at the shapes where each form applies."""
    for dt in (BF16, F16):
        assert expected_form(1, 2, 3, 64, 64, 64, dt) == FUSED and expected_form(1, 2, 3, 1088, 1088, 64, dt) == TWO_KERNEL
        assert expected_form(3, 2, 3, 128, 128, 64, dt) == HS and expected_form(3, 2, 3, 64, 64, 64, dt) == TWO_KERNEL
        assert expected_form(3, 2, 3, 1152, 1152, 64, dt) == HS
        assert expected_form(2, 2, 3, 64, 64, 80, dt) == KP and expected_form(None, 2, 3, 64, 64, 80, dt) == KP
        assert expected_form(2, 2, 3, 65, 65, 80, dt) == TWO_KERNEL and expected_form(2, 2, 3, 64, 64, 128, dt) == TWO_KERNEL
        assert expected_form(None, 2, 3, 256, 256, 64, dt) == TWO_KERNEL
        assert expected_form(None, 24, 25, 512, 512, 64, dt) == HS and expected_form(None, 24, 25, 320, 320, 64, dt) == FUSED
        for mode in (None, 0, 1, 2, 3):
            assert expected_form(mode, 2, 3, 130, 67, 64, dt) == TWO_KERNEL
    for mode in (None, 0, 1, 2, 3):
        assert expected_form(mode, 2, 3, 128, 128, 64, F32) == TWO_KERNEL
    assert expected_fwd_splits(1, 1, 33, 1100, 64) == 4 and expected_fwd_splits(2, 3, 300, 1100, 64) == 4
    assert expected_fwd_splits(1, 1, 1100, 448, 64) == 1 and expected_fwd_splits(2, 128, 128, 1100, 64) == 1
    assert expected_bwd_splits(1, 1, 33, 1100, 64) == (8, 1) and expected_bwd_splits(1, 1, 1100, 600, 64) == (4, 8)


def test_margins_follow_the_rule():
    assert all(k in (8, 16, 32) for k in FA_K_CASE.values())
    assert all(op.startswith("fa.") and dt in ("float32", "bfloat16", "float16") for op, dt in FA_K_CASE)
    assert "randn" in GENERATORS
