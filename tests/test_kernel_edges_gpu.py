"""Edge cases of the row-wise and multi-tensor HIP kernels against fp64 oracles (GPU only; the
comparison rule itself is tested on the CPU in ``test_kernel_edges_rule.py``).

Covers ``csrc/ops/xent.hip``, ``rmsnorm.hip``, ``swiglu.hip``, ``multi_tensor.hip`` and ``rope.hip`` at
the shapes where their code takes another path (vector/scalar loops, one sweep of a workgroup, the
``dispatch_nv`` boundaries, the capped backward grid, 4-wide fallbacks, misaligned views, zero-element
tensors), with masked (-inf), saturated and large-magnitude values, in fp32, bf16 and fp16.

One comparison rule (``check``): the kernel output ``got``, an fp64 oracle ``ref64`` and a plain fp32
evaluation ``ref32`` all come from the same rounded inputs. With

    E32 = max(max|ref32 - ref64|, 2^-23 * max|ref64|)        (over the tensor)

the kernel passes if, for every element, ``|got - ref64| <= k*E32 + u*|ref64| + tiny`` where ``u`` is one
ulp of the output dtype (0 fp32, 2^-8 bf16, 2^-10 fp16), ``tiny`` its smallest normal, and
``isfinite(got) == isfinite(ref64)`` everywhere. ``k = 4`` is a margin for a different summation order
and the fast ``__expf``/``__logf``; it is not a measured number.

Measured ``max (|got - ref64| - u*|ref64|) / E32`` per (op, output dtype) on an MI355X. No case needs more
than k = 4, so ``K_CASE`` is empty. A 0 in a 16-bit column means the error stayed within ``u*|ref64|``,
the one rounding to the output type; ``-`` means the output has no such type in these tests:

    op (suffix: the test group)   fp32     bf16     fp16
    --------------------------------------------------------
    add_rmsnorm.dw                1.666        -        -
    add_rmsnorm.dx                1.047    0.000        -
    add_rmsnorm.rstd              0.930        -        -
    add_rmsnorm.sum               0.465    0.000        -
    add_rmsnorm.y                 1.174    0.000        -
    rmsnorm.dw                    1.367        -        -
    rmsnorm.dw.bigM               0.377        -        -
    rmsnorm.dw.values             1.003        -        -
    rmsnorm.dx                    1.000    0.000    0.000
    rmsnorm.dx.bigM               1.245    0.017        -
    rmsnorm.dx.values             0.812    0.000    0.000
    rmsnorm.rstd                  0.877        -        -
    rmsnorm.rstd.bigM             0.906        -        -
    rmsnorm.rstd.values           0.460        -        -
    rmsnorm.y                     1.031    0.000    0.000
    rmsnorm.y.bigM                1.163    0.000        -
    rmsnorm.y.values              0.609    0.000    0.000
    rope.fwd                      0.473    0.000    0.000
    rope.inverse                  0.506    0.000    0.000
    swiglu.da                     0.641    0.000    0.000
    swiglu.da.saturated           0.329    0.000    0.000
    swiglu.da.view                    -    0.000    0.000
    swiglu.db                     0.704    0.000    0.000
    swiglu.db.saturated           0.002    0.000    0.000
    swiglu.db.view                    -    0.000    0.000
    swiglu.fused.da               0.708    0.000    0.000
    swiglu.fused.db               0.633    0.000    0.000
    swiglu.fused.h                0.585    0.000    0.000
    swiglu.h                      1.000    0.000    0.000
    swiglu.h.saturated            0.002    0.000    0.000
    swiglu.h.view                     -    0.000    0.000
    xent.dz                       2.742    0.000    0.000
    xent.dz.masked                2.092    0.000    0.000
    xent.loss                     0.824        -        -
    xent.loss.magnitude           0.349        -        -
    xent.loss.masked              0.450        -        -
    xent.lse                      0.618        -        -
    xent.lse.magnitude            0.402        -        -
    xent.lse.masked               0.475        -        -
    xent.wrapper.dz               1.545    0.000    0.000
    xent.wrapper.loss             0.791        -        -
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
U = {F32: 0.0, BF16: 2.0**-8, F16: 2.0**-10}
K = 4.0
# per-op margins above 4 (none needed so far): the next power of two above twice the measured ratio,
# never above 32, each with its reason; a ratio above 32 is a finding about the kernel
K_CASE: dict = {}
_RATIOS: dict = {}


def _name(dt):
    return str(dt).replace("torch.", "")


def _unravel(i, shape):
    idx = []
    for n in reversed(shape):
        idx.append(i % n)
        i //= n
    return tuple(reversed(idx))


def check(got, ref64, ref32, out_dtype, op, k=None):
    """The comparison rule of the module docstring. Fails with the worst element (index, got, ref,
    bound); every element is checked. Returns the ratio (|got - ref64| - u*|ref64|)_max / E32."""
    k = K_CASE.get(op, K) if k is None else k
    assert k <= 32
    u, tiny = U[out_dtype], torch.finfo(out_dtype).tiny
    g, r64, r32 = got.detach().double(), ref64.detach().double(), ref32.detach().double()
    assert g.shape == r64.shape == r32.shape, (op, g.shape, r64.shape, r32.shape)
    if g.numel() == 0:
        return 0.0
    fin = torch.isfinite(r64)
    assert torch.equal(torch.isfinite(r32), fin), f"{op}: the fp32 and fp64 references disagree on where values are finite"
    bad = torch.isfinite(g) != fin
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        idx = _unravel(i, g.shape)
        pytest.fail(f"{op} [{_name(out_dtype)}]: finiteness differs at {idx}: got {g.flatten()[i].item()!r}, ref {r64.flatten()[i].item()!r} ({int(bad.sum())} elements)")
    zero = torch.zeros_like(r64)
    a64 = torch.where(fin, r64.abs(), zero)
    e32 = max(torch.where(fin, (r32 - r64).abs(), zero).max().item(), 2.0**-23 * a64.max().item())
    err = torch.where(fin, (g - r64).abs(), zero)
    bound = k * e32 + u * a64 + tiny
    ratio = (err - u * a64).clamp_min(0).max().item() / max(e32, tiny)
    if op is not None:
        key = (op, _name(out_dtype))
        _RATIOS[key] = max(_RATIOS.get(key, 0.0), ratio)
    excess = (err - bound).flatten()
    i = int(excess.argmax())
    if excess[i].item() > 0:
        idx = _unravel(i, g.shape)
        pytest.fail(
            f"{op} [{_name(out_dtype)}]: worst element {idx}: got {g.flatten()[i].item()!r}, ref {r64.flatten()[i].item()!r}, "
            f"|err| {err.flatten()[i].item():.3e} > bound {bound.flatten()[i].item():.3e} (k={k}, E32={e32:.3e}, ratio={ratio:.2f}, "
            f"{int((excess > 0).sum())} of {g.numel()} elements out of bound)"
        )
    return ratio


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    yield
    if _RATIOS:
        print("\nmax (|got-ref64| - u|ref64|)/E32 per (op, output dtype):")
        for (op, dt), r in sorted(_RATIOS.items()):
            print(f"  edge-ratio {op:<24s} {dt:<9s} {r:8.3f}")


def _hip():
    from cs336_systems.ops._ext import ops

    return ops()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _f32(v):
    """The value a C++ ``(float)v`` cast hands the kernel, as a Python float."""
    return torch.tensor(v, dtype=F32).item()


# ------------------------------------------------------------------------------------ cross entropy
XENT_G = 0.37


def _xent_check(z, t, tag, bwd=True):
    """xent_fwd's per-row loss and lse, and xent_bwd with g = 0.37, mult = 1/M, against fp64."""
    from cs336_systems.ops.cross_entropy import log_softmax_ref

    hip = _hip()
    M, V = z.shape
    dt = z.dtype
    loss, lse = hip.xent_fwd(z, t)
    assert loss.dtype == F32 and lse.dtype == F32
    z64, z32, ti = z.double(), z.float(), t[:, None]
    lse64 = torch.logsumexp(z64, -1)
    loss64 = lse64 - z64.gather(-1, ti)[:, 0]
    ls32 = log_softmax_ref(z32)
    mx = z32.max(-1)[0]
    lse32 = mx + torch.log(torch.exp(z32 - mx[:, None]).sum(-1))
    check(loss, loss64, -ls32.gather(-1, ti)[:, 0], F32, f"xent.loss{tag}")
    check(lse, lse64, lse32, F32, f"xent.lse{tag}")
    if not bwd:
        return loss, lse, None
    mult = 1.0 / M
    gs = torch.tensor(XENT_G, device=DEV, dtype=F32)
    dz = hip.xent_bwd(gs, z, t, lse, mult)
    assert dz.dtype == dt and dz.shape == z.shape
    onehot = torch.zeros_like(z64).scatter_(-1, ti, 1.0)
    sc = _f32(XENT_G) * _f32(mult)
    dz64 = (torch.softmax(z64, -1) - onehot) * sc
    dz32 = (torch.exp(ls32) - onehot.float()) * gs * torch.tensor(mult, device=DEV, dtype=F32)
    check(dz, dz64, dz32, dt, f"xent.dz{tag}")
    tgt = dz.double().gather(-1, ti)[:, 0]
    if V > 1:
        assert (tgt < 0).all(), f"target entries of dz must be negative: {tgt}"
    # each row of softmax - onehot sums to 0. 16-bit: V roundings of u relative to entries whose
    # magnitudes sum to <= 2. fp32 (u = 0 in the rule): the row sum inherits the relative errors of
    # exp(z - lse), about (|lse| + ln V + 6) * 2^-24 from the rounded lse, the argument scaling inside
    # __expf and its last ulps, weighted by probabilities that sum to 1; allowed twice that.
    rowsum = dz.double().sum(-1).abs()
    if dt == F32:
        lim = (lse64.abs() + math.log(V) + 6.0) * 2.0**-23 * abs(sc)
    else:
        lim = torch.full_like(rowsum, V * U[dt] * abs(sc))
    assert (rowsum <= lim).all(), f"rows of dz must sum to 0: {rowsum.max().item():.3e} > {lim.min().item():.3e}"
    return loss, lse, dz


@pytest.mark.parametrize("V", [1, 3, 4, 8, 255, 257, 1020, 1024, 1028, 2052, 4099])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_xent_shapes(dt, V):
    """Below, at and above one sweep of the workgroup (256 scalar, 1024 vector), above two; both loops."""
    for M in (1, 5):
        g = _gen(100 + V + M)
        z = (3 * torch.randn(M, V, device=DEV, generator=g)).to(dt)
        t = torch.randint(0, V, (M,), device=DEV, generator=g)
        loss, lse, dz = _xent_check(z, t, "")
        if V == 1:
            assert torch.all(loss == 0) and torch.all(dz == 0), (loss, dz)


@pytest.mark.parametrize("V", [1003, 1024, 2052])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_xent_targets(dt, V):
    """Targets pinned to column 0, V-1 and (vector path) each slot of one quad in the first and in the
    second sweep; the target logit is -7.25, so a read of a neighbouring column misses by a wide margin."""
    cols = [0, V - 1, 1, V - 2]
    if V % 4 == 0:
        cols += [4 * 37 + s for s in range(4)] + [4 * (256 + 44) + s for s in range(4) if 4 * (256 + 44) + s < V]
    else:
        cols += [37, 256 + 44, 511, 512]
    t = torch.tensor(cols, device=DEV, dtype=torch.int64)
    z = (3 * torch.randn(len(cols), V, device=DEV, generator=_gen(7))).to(dt)
    z.scatter_(-1, t[:, None], -7.25)
    _xent_check(z, t, "")


def _masked_case(dt, kind, V):
    g = _gen(11)
    M = 5
    z = 3 * torch.randn(M, V, device=DEV, generator=g)
    if kind == "half":
        mask = torch.rand(M, V, device=DEV, generator=g) < 0.5
        t = torch.randint(0, V, (M,), device=DEV, generator=g)
    else:  # the whole prefix [0, 2048): every lane's first sweep is -inf in both loops
        mask = torch.zeros(M, V, dtype=torch.bool, device=DEV)
        mask[:, :2048] = True
        t = torch.randint(2048, V, (M,), device=DEV, generator=g)
    mask.scatter_(-1, t[:, None], False)  # the target column is never masked
    return z.masked_fill(mask, float("-inf")).to(dt), t, mask


@pytest.mark.parametrize("kind,V", [("half", 1003), ("half", 1024), ("prefix", 4099), ("prefix", 4100)])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_xent_masked_logits(dt, kind, V):
    """-inf logits (masked vocabulary): finite loss and lse within the rule, gradient exactly 0 at the
    masked columns. (A row that is entirely -inf is NaN in the reference too and is not specified.)"""
    z, t, mask = _masked_case(dt, kind, V)
    loss, lse, dz = _xent_check(z, t, ".masked")
    assert torch.isfinite(loss).all() and torch.isfinite(lse).all(), (loss, lse)
    assert torch.all(dz[mask] == 0), f"{int((dz[mask] != 0).sum())} masked columns have a non-zero gradient"
    assert torch.isfinite(dz).all()


@pytest.mark.parametrize("V", [1003, 1024])
@pytest.mark.parametrize("case", ["f32-1e4", "f32+1e4", "f16-spread"])
def test_xent_magnitude(case, V):
    """Large offsets: the row loss must not inherit the rounding of M + log S to an ulp of |M|
    (formed as M + log S - z[t] the fp32 +-1e4 cases measured a ratio of 271; as log S - (z[t] - M), 0.35)."""
    g = _gen(5)
    if case == "f16-spread":
        z = ((2 * torch.rand(5, V, device=DEV, generator=g) - 1) * 6e4).to(F16)
    else:
        z = 3 * torch.randn(5, V, device=DEV, generator=g) + (1e4 if case == "f32+1e4" else -1e4)
    t = torch.randint(0, V, (5,), device=DEV, generator=g)
    _xent_check(z, t, ".magnitude", bwd=False)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_xent_autograd_wrapper(dt):
    """ops.cross_entropy passes the upstream gradient and 1/M to the backward kernel."""
    from cs336_systems import ops

    g = _gen(3)
    V, M = 257, 6
    z = (3 * torch.randn(2, 3, V, device=DEV, generator=g)).to(dt).requires_grad_(True)
    t = torch.randint(0, V, (2, 3), device=DEV, generator=g)
    loss = ops.cross_entropy(z, t)
    (XENT_G * loss).backward()
    z64 = z.detach().double().view(M, V)
    rows64 = torch.logsumexp(z64, -1) - z64.gather(-1, t.view(M, 1))[:, 0]
    check(loss.detach(), rows64.mean(), ops.cross_entropy_ref(z.detach().float(), t), F32, "xent.wrapper.loss")
    onehot = torch.zeros_like(z64).scatter_(-1, t.view(M, 1), 1.0)
    dz64 = (torch.softmax(z64, -1) - onehot) * (_f32(XENT_G) * _f32(1.0 / M))
    dz32 = (torch.softmax(z.detach().float().view(M, V), -1) - onehot.float()) * torch.tensor(XENT_G, device=DEV) / M
    check(z.grad.view(M, V), dz64, dz32, dt, "xent.wrapper.dz")


# ------------------------------------------------------------------------------------ RMSNorm
EPS = 1e-5


def _rms_eval(x, w, dy, ft, eps):
    """y, rstd, dx, dw of y = w * x * rsqrt(mean(x^2) + eps) in the float type ft (fp64: the oracle;
    fp32: the plain evaluation whose own error sets E32; dw there is a plain fp32 column sum)."""
    from cs336_systems.ops import rmsnorm_ref

    xf, wf, dyf = x.to(ft), w.to(ft), dy.to(ft)
    H = x.shape[-1]
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    y = rmsnorm_ref(xf, wf, eps) if ft == F32 else wf * (xf * rstd)
    wdy = wf * dyf
    dx = rstd * wdy - rstd.pow(3) / H * (wdy * xf).sum(-1, keepdim=True) * xf
    dw = (dyf * xf * rstd).sum(0)
    return y, rstd[:, 0], dx, dw


def _rms_check(x, w, odt, tag, seed=0, dy=None):
    hip = _hip()
    eps = _f32(EPS)
    M, H = x.shape
    y, rstd = hip.rmsnorm_fwd(x, w, EPS, odt)
    assert y.dtype == odt and rstd.dtype == F32 and rstd.shape == (M,)
    if dy is None:
        dy = torch.randn(M, H, device=DEV, generator=_gen(seed + 1)).to(odt)
    dx, dw = hip.rmsnorm_bwd(dy, x, w, rstd)
    assert dx.dtype == x.dtype and dw.dtype == F32 and dw.shape == (H,)
    r64, r32 = _rms_eval(x, w, dy, torch.float64, eps), _rms_eval(x, w, dy, F32, eps)
    for i, (name, got, gdt) in enumerate((("y", y, odt), ("rstd", rstd, F32), ("dx", dx, x.dtype), ("dw", dw, F32))):
        check(got, r64[i], r32[i], gdt, f"rmsnorm.{name}{tag}")
    return y, rstd, dx, dw


def _rms_inputs(M, H, xdt, wdt=F32, seed=0, scale=1.0):
    g = _gen(seed + H + 7 * M)
    x = (scale * torch.randn(M, H, device=DEV, generator=g)).to(xdt)
    w = (1 + 0.1 * torch.randn(H, device=DEV, generator=g)).to(wdt)
    return x, w


RMS_H = [4, 8, 508, 512, 516, 1028, 2052, 2564, 3076, 4096, 8188, 8192]
RMS_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (F16, F16)]
_pair_id = lambda p: _name(p) if isinstance(p, torch.dtype) else str(p)


@pytest.mark.parametrize("H", RMS_H)
@pytest.mark.parametrize("xdt,odt", RMS_PAIRS, ids=_pair_id)
def test_rmsnorm_h_boundaries(xdt, odt, H):
    """Every per-lane register count of dispatch_nv (2 .. 32), at and around its boundary in H."""
    x, w = _rms_inputs(5, H, xdt)
    _rms_check(x, w, odt, "")


@pytest.mark.parametrize("dt", [BF16, F16], ids=_name)
def test_rmsnorm_16bit_weight(dt):
    x, w = _rms_inputs(5, 516, dt, wdt=dt)
    _rms_check(x, w, dt, "")


@pytest.mark.parametrize("M", [1, 2, 3, 4, 13])
@pytest.mark.parametrize("xdt,odt", [(F32, F32), (BF16, BF16)], ids=_pair_id)
def test_rmsnorm_m_boundaries(xdt, odt, M):
    """M < 4: whole waves own no row and still contribute a (zero) dw partial."""
    x, w = _rms_inputs(M, 256, xdt)
    _rms_check(x, w, odt, "")


@pytest.mark.parametrize("xdt,odt", [(F32, F32), (BF16, BF16)], ids=_pair_id)
def test_rmsnorm_capped_backward_grid(xdt, odt):
    """M = 12293 > 12288: 1024 workgroups, rows strided by 4096 waves, colsum over 64 partial rows per
    split. dy*x >= 0 in columns 0..3 so that a dropped partial row cannot cancel there."""
    M, H = 12293, 64
    x, w = _rms_inputs(M, H, xdt)
    dy = torch.randn(M, H, device=DEV, generator=_gen(1))
    dy[:, :4] = dy[:, :4].abs() * torch.where(x[:, :4].float() < 0, -1.0, 1.0)
    _rms_check(x, w, odt, ".bigM", dy=dy.to(odt))


@pytest.mark.parametrize("xdt,odt", RMS_PAIRS, ids=_pair_id)
def test_rmsnorm_zero_row_and_tiny_rows(xdt, odt):
    """An all-zero row (y = 0, rstd = eps^-1/2, dx = rstd*w*dy) and rows scaled by 1e-4 (eps dominates)."""
    x, w = _rms_inputs(5, 512, xdt)
    x[2] = 0
    x[3] *= 1e-4
    x[4] *= 1e-4
    y, rstd, dx, dw = _rms_check(x, w, odt, ".values")
    assert torch.all(y[2] == 0)
    assert rstd[2].item() == pytest.approx(_f32(EPS) ** -0.5, rel=2.0**-22)
    for t in (y, rstd, dx, dw):
        assert torch.isfinite(t).all()


def test_rmsnorm_fp16_large_rows():
    """fp16 rows of magnitude 3e4: x^2 ~ 1e9 is past the fp16 range but the fp32 mean stays finite."""
    g = _gen(9)
    H = 516
    x = (3e4 * (0.5 + torch.rand(5, H, device=DEV, generator=g)) * torch.where(torch.rand(5, H, device=DEV, generator=g) < 0.5, -1.0, 1.0)).to(F16)
    w = (1 + 0.1 * torch.randn(H, device=DEV, generator=g)).to(F32)
    y, rstd, dx, dw = _rms_check(x, w, F16, ".values")
    for t in (y, rstd, dx, dw):
        assert torch.isfinite(t).all()


# (x / stream dtype, r / branch dtype, out dtype): what the binding accepts (fp32 or bf16 each)
ADD_TRIPLES = [(x, r, o) for x in (F32, BF16) for r in (F32, BF16) for o in (F32, BF16)]


@pytest.mark.parametrize("H", RMS_H)
@pytest.mark.parametrize("xdt,rdt,odt", ADD_TRIPLES, ids=_pair_id)
def test_add_rmsnorm(xdt, rdt, odt, H):
    """s = x + r stored in the stream dtype; y is the norm of the *rounded* s (the (bf16, bf16, fp32)
    triple tells the two apart: a norm of the unrounded sum is off by 2^-9 relative, far beyond E32)."""
    hip = _hip()
    eps = _f32(EPS)
    M = 5
    g = _gen(31 + H)
    x = torch.randn(M, H, device=DEV, generator=g).to(xdt)
    r = torch.randn(M, H, device=DEV, generator=g).to(rdt)
    w = 1 + 0.1 * torch.randn(H, device=DEV, generator=g)
    s, y, rstd = hip.add_rmsnorm_fwd(x, r, w, EPS, odt)
    assert s.dtype == xdt and y.dtype == odt and rstd.dtype == F32
    check(s, x.double() + r.double(), x.float() + r.float(), xdt, "add_rmsnorm.sum")
    s_ref = (x.float() + r.float()).to(xdt)  # fp32 add, one rounding: what the kernel stores
    assert torch.equal(s, s_ref)
    dy = torch.randn(M, H, device=DEV, generator=g).to(odt)
    dres = torch.randn(M, H, device=DEV, generator=g).to(xdt)
    emit = xdt == F32
    dx, dx16, dw = hip.rmsnorm_bwd_add(dy, s, w, rstd, dres, emit)
    assert dx.dtype == xdt and dw.dtype == F32
    r64, r32 = _rms_eval(s_ref, w, dy, torch.float64, eps), _rms_eval(s_ref, w, dy, F32, eps)
    check(y, r64[0], r32[0], odt, "add_rmsnorm.y")
    check(rstd, r64[1], r32[1], F32, "add_rmsnorm.rstd")
    check(dx, r64[2] + dres.double(), r32[2] + dres.float(), xdt, "add_rmsnorm.dx")
    check(dw, r64[3], r32[3], F32, "add_rmsnorm.dw")
    if emit:
        assert torch.equal(dx16, dx.bfloat16())


# ------------------------------------------------------------------------------------ SwiGLU
def _swiglu_eval(a, b, dh, ft):
    from cs336_systems.ops import silu_mul_ref

    af, bf, gf = a.to(ft), b.to(ft), dh.to(ft)
    s = torch.sigmoid(af)
    return silu_mul_ref(af, bf), gf * bf * (s + af * s * (1 - s)), gf * af * s


def _swiglu_check_flat(a, b, dh, tag):
    from cs336_systems import ops

    dt = a.dtype
    a = a.detach().requires_grad_(True)
    b = b.detach().requires_grad_(True)
    h = ops.silu_mul(a, b)
    assert h.dtype == dt and h.shape == a.shape
    h.backward(dh)
    r64, r32 = _swiglu_eval(a.detach(), b.detach(), dh, torch.float64), _swiglu_eval(a.detach(), b.detach(), dh, F32)
    check(h, r64[0], r32[0], dt, f"swiglu.h{tag}")
    check(a.grad, r64[1], r32[1], dt, f"swiglu.da{tag}")
    check(b.grad, r64[2], r32[2], dt, f"swiglu.db{tag}")
    return h.detach(), a.grad, b.grad


@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 2047, 16388])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_silu_mul_flat_sizes(dt, n):
    """Tail only (n < 4), 4-wide plus tail, and the 16-byte kernel."""
    g = _gen(n)
    a, b, dh = (torch.randn(n, device=DEV, generator=g).to(dt) for _ in range(3))
    _swiglu_check_flat(a, b, dh, "")


@pytest.mark.parametrize("dt,F", [(BF16, 4), (BF16, 12), (BF16, 388), (BF16, 384), (F16, 4), (F16, 12), (F16, 388), (F16, 384), (F32, 4), (F32, 388)], ids=_pair_id)
def test_swiglu_fused_layout(dt, F):
    """[a | b] = (M, 2F): F % 8 == 4 in a 16-bit type takes the 4-wide fallback with M > 1 and ld = 2F
    (F = 384: the 16-byte kernel, as the control); da | db must land in their own halves of dy."""
    from cs336_systems.models.fused import SwiGLUGate

    g = _gen(F)
    M = 5
    y = torch.randn(M, 2 * F, device=DEV, generator=g).to(dt).requires_grad_(True)
    dh = torch.randn(M, F, device=DEV, generator=g).to(dt)
    h = SwiGLUGate.apply(y)
    assert h.shape == (M, F) and h.dtype == dt
    h.backward(dh)
    a, b = y.detach()[:, :F], y.detach()[:, F:]
    r64, r32 = _swiglu_eval(a, b, dh, torch.float64), _swiglu_eval(a, b, dh, F32)
    check(h, r64[0], r32[0], dt, "swiglu.fused.h")
    check(y.grad[:, :F], r64[1], r32[1], dt, "swiglu.fused.da")
    check(y.grad[:, F:], r64[2], r32[2], dt, "swiglu.fused.db")


@pytest.mark.parametrize("dt", [BF16, F16], ids=_name)
def test_silu_mul_view_8_bytes_in(dt):
    """16-bit operands that start 4 elements (8 bytes) into a larger buffer, length a multiple of 8: the
    16-byte kernel must refuse them, the 4-wide fallback (8-byte accesses) takes them."""
    g = _gen(2)
    n = 2056
    bufs = [torch.randn(n + 16, device=DEV, generator=g).to(dt) for _ in range(2)]
    a, b = (buf[4 : 4 + n] for buf in bufs)
    assert a.data_ptr() % 16 == 8 and b.data_ptr() % 16 == 8 and a.is_contiguous()
    dh = torch.randn(n, device=DEV, generator=g).to(dt)
    _swiglu_check_flat(a, b, dh, ".view")


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_silu_mul_saturation(dt):
    """sigmoid is 1 / (1 + __expf(-a)), which overflows to inf below a = -88: nothing may be NaN. The
    16-bit types run the subset of the grid whose results fit their range."""
    av = [-200.0, -89.0, -88.0, -20.0, -1e-3, 0.0, 1e-3, 20.0, 88.0, 200.0]
    sv = [1.0, -1.0, 1e3, -1e3]
    grid = torch.cartesian_prod(*(torch.tensor(v, device=DEV) for v in (av, sv, sv)))
    a, b, dh = (grid[:, i].to(dt) for i in range(3))
    r64 = _swiglu_eval(a, b, dh, torch.float64)
    keep = torch.ones_like(a, dtype=torch.bool)
    for r in r64:
        keep &= r.abs() < 0.9 * torch.finfo(dt).max
    assert int(keep.sum()) >= (160 if dt != F16 else 40)
    a, b, dh = a[keep].contiguous(), b[keep].contiguous(), dh[keep].contiguous()
    for t in _swiglu_check_flat(a, b, dh, ".saturated"):
        assert not torch.isnan(t).any()


# ------------------------------------------------------------------------------------ multi-tensor
MT_SIZES = (1, 5, 32767, 32768, 32769, 65541)  # around one and two 32 Ki-element chunks, mixed in one list
HP = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.1)
GUARD = 7.0


class _Placed:
    """Copies of `vals` as fresh (16-byte aligned) tensors, or as views `off` elements into larger
    buffers whose other elements hold a guard value that must survive the kernels."""

    def __init__(self, vals, off, dtype=None):
        self.t, self.bufs, self.off = [], [], off
        for v in vals:
            v = v if dtype is None else v.to(dtype)
            n = v.numel()
            if off == 0 or n == 0:
                t = v.clone()
            else:
                buf = torch.full((n + off + 5,), GUARD, dtype=v.dtype, device=DEV)
                t = buf[off : off + n]
                t.copy_(v)
                assert t.data_ptr() % 16 == off * v.element_size() and t.is_contiguous()
                self.bufs.append((buf, n))
            if off == 0 and n:
                assert t.data_ptr() % 16 == 0
            self.t.append(t)

    def guards_intact(self):
        return all(torch.all(b[: self.off] == GUARD) and torch.all(b[self.off + n :] == GUARD) for b, n in self.bufs)


@functools.lru_cache(maxsize=None)
def _adamw_vals(sizes, gdt):
    """p0 and three steps of gradients (rounded to gdt, held as fp32); shared, never modified. The
    values of the non-empty tensors do not depend on where zero-element tensors sit in the list."""
    g = _gen(77)
    nz = [n for n in sizes if n]
    vals = [[torch.randn(n, device=DEV, generator=g) for n in nz] for _ in range(4)]
    it = [iter(v) for v in vals]
    full = [[next(i) if n else torch.empty(0, device=DEV) for n in sizes] for i in it]
    return full[0], [[x.to(gdt).float() for x in step] for step in full[1:]]


def _adamw_run(sizes, off=(0, 0, 0, 0), gdt=F32, g_as=F32, shadow_off=None):
    """Three adamw_step calls on the shared values; p, g, m, v (and the bf16 shadows) placed aligned or
    as offset views. Returns (p, m, v, shadows) lists."""
    hip = _hip()
    p0, gs = _adamw_vals(sizes, gdt)
    P = _Placed(p0, off[0])
    Mm = _Placed([torch.zeros_like(p) for p in p0], off[2])
    Vv = _Placed([torch.zeros_like(p) for p in p0], off[3])
    S = _Placed([torch.zeros_like(p) for p in p0], shadow_off, BF16) if shadow_off is not None else None
    placed = [P, Mm, Vv] + ([S] if S else [])
    for step in range(1, 4):
        G = _Placed(gs[step - 1], off[1], g_as)
        hip.adamw_step(P.t, G.t, Mm.t, Vv.t, S.t if S else [], HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], step, None)
        assert all(torch.equal(a, b.to(g_as)) for a, b in zip(G.t, gs[step - 1])), "gradients were modified"
        placed.append(G)
    torch.cuda.synchronize()
    assert all(x.guards_intact() for x in placed), "a kernel wrote outside its tensor"
    return P.t, Mm.t, Vv.t, (S.t if S else None)


def _assert_bitwise(run, base, what):
    for name, xs, ys in zip("pmv", run[:3], base[:3]):
        for i, (x, y) in enumerate(zip(xs, ys)):
            if not torch.equal(x, y):
                j = int((x != y).flatten().nonzero()[0])
                pytest.fail(f"{what}: {name}[{i}] (numel {x.numel()}) differs at {j}: {x[j].item()!r} vs {y[j].item()!r} ({int((x != y).sum())} elements)")


@pytest.mark.parametrize("which", ["p", "g", "m", "v", "all"])
def test_adamw_misaligned_views_bitwise(which):
    """Views that start one element into a buffer take the scalar branch; the arithmetic per element
    is the same and contraction is off, so p, m, v match the aligned placement bit for bit."""
    off = tuple(int(which in (name, "all")) for name in "pgmv")
    base = _adamw_run(MT_SIZES)
    _assert_bitwise(_adamw_run(MT_SIZES, off=off), base, f"misaligned {which}")
    assert all(not torch.equal(p, p0) for p, p0 in zip(base[0], _adamw_vals(MT_SIZES, F32)[0]))


@pytest.mark.parametrize("shadow_off", [0, 1])
@pytest.mark.parametrize("off", [(0, 0, 0, 0), (1, 1, 1, 1)], ids=["aligned", "offset"])
def test_adamw_shadows(off, shadow_off):
    base = _adamw_run(MT_SIZES)
    run = _adamw_run(MT_SIZES, off=off, shadow_off=shadow_off)
    _assert_bitwise(run, base, "with bf16 shadows")
    for p, s in zip(run[0], run[3]):
        assert s.dtype == BF16 and torch.equal(s, p.bfloat16())


@pytest.mark.parametrize("g_off", [0, 1])
@pytest.mark.parametrize("gdt", [BF16, F16], ids=_name)
def test_adamw_16bit_gradients(gdt, g_off):
    """16-bit gradient instantiations, aligned and offset by one element: bitwise the fp32-gradient run on g.float()."""
    base = _adamw_run(MT_SIZES, gdt=gdt, g_as=F32)
    _assert_bitwise(_adamw_run(MT_SIZES, off=(0, g_off, 0, 0), gdt=gdt, g_as=gdt), base, f"{_name(gdt)} gradients")
    _assert_bitwise(_adamw_run(MT_SIZES, off=(0, g_off, 0, 0), gdt=gdt, g_as=gdt, shadow_off=g_off), base, f"{_name(gdt)} gradients + shadows")


ZSIZES = (0, 5, 0, 0, 32769, 1, 65541, 0)


@pytest.mark.parametrize("off", [(0, 0, 0, 0), (1, 1, 1, 1)], ids=["aligned", "offset"])
def test_adamw_zero_element_tensors_and_reference(off):
    """Zero-element tensors at the front, in the middle and at the end duplicate entries of chunk_base;
    find_tensor must step over them and every other tensor must be fully updated (against adamw_ref_)."""
    from cs336_systems.ops.adamw import adamw_ref_

    p, m, v, _ = _adamw_run(ZSIZES, off=off)
    p0, gs = _adamw_vals(ZSIZES, F32)
    for i, n in enumerate(ZSIZES):
        pr, mr, vr = p0[i].clone(), torch.zeros_like(p0[i]), torch.zeros_like(p0[i])
        for step in range(1, 4):
            adamw_ref_(pr, gs[step - 1][i], mr, vr, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], step)
        assert p[i].numel() == n
        # the tolerance of test_fused_adamw_matches_reference; for m and v too: add_(g, alpha) may fuse
        # where the kernel rounds (1-b)*g on its own, half an ulp of a term <= 0.4 (1.5e-8) per step
        torch.testing.assert_close(p[i], pr, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(m[i], mr, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(v[i], vr, rtol=1e-6, atol=1e-7)
    # and bit for bit what the same tensors give in a list without the empty ones
    keep = [i for i, n in enumerate(ZSIZES) if n]
    base = _adamw_run(tuple(ZSIZES[i] for i in keep))
    _assert_bitwise([[x[i] for i in keep] for x in (p, m, v)], base, "with zero-element tensors")


def test_adamw_matches_reference_mixed_sizes():
    from cs336_systems.ops.adamw import adamw_ref_

    p, m, v, _ = _adamw_run(MT_SIZES, off=(1, 1, 1, 1))
    p0, gs = _adamw_vals(MT_SIZES, F32)
    for i in range(len(MT_SIZES)):
        pr, mr, vr = p0[i].clone(), torch.zeros_like(p0[i]), torch.zeros_like(p0[i])
        for step in range(1, 4):
            adamw_ref_(pr, gs[step - 1][i], mr, vr, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], step)
        torch.testing.assert_close(p[i], pr, rtol=1e-6, atol=1e-7)


def _mt_vals(dt, sizes):
    g = _gen(13)
    return [torch.randn(n, device=DEV, generator=g).to(dt) for n in sizes]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_multi_tensor_l2norm_views(dt, off):
    hip = _hip()
    vals = _mt_vals(dt, MT_SIZES[:3] + (0,) + MT_SIZES[3:])
    X = _Placed(vals, off)
    ref = math.sqrt(sum((v.double() ** 2).sum().item() for v in vals))
    out = hip.multi_tensor_l2norm(X.t)
    assert out.dtype == F32
    assert out.item() == pytest.approx(ref, rel=1e-5)
    assert all(torch.equal(a, b) for a, b in zip(X.t, vals)) and X.guards_intact()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_multi_tensor_scale_views(dt, off):
    hip = _hip()
    vals = _mt_vals(dt, (0,) + MT_SIZES[:3] + (0,) + MT_SIZES[3:] + (0,))
    X = _Placed(vals, off)
    c = torch.tensor([0.37], device=DEV)
    hip.multi_tensor_scale_(X.t, c)
    for x, v in zip(X.t, vals):
        assert torch.equal(x, (v.float() * c).to(dt))
    assert X.guards_intact()


# ------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("D", [8, 256])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_rope_limits_and_fused_slice(dt, D, with_pos):
    """Head dims 8 and 256 (the binding's limits), fp16 included, on the q slice of a fused (B, N, 3HD)
    projection that starts 16 elements into its storage; forward and inverse against rope_ref in fp64."""
    from cs336_systems import ops
    from cs336_systems.models import RotaryEmbedding

    B, N, H, ctx = 2, 65, 3, 128
    g = _gen(D)
    re = RotaryEmbedding(ctx, D, 10000.0).to(DEV)
    cos, sin = re.cos.float().contiguous(), re.sin.float().contiguous()
    store = torch.randn(16 + B * N * 3 * H * D, device=DEV, generator=g).to(dt)
    qkv = store[16:].view(B, N, 3 * H * D)
    x = qkv[..., : H * D].view(B, N, H, D).transpose(1, 2)  # (B, H, N, D)
    assert x.storage_offset() == 16 and not x.is_contiguous()
    from cs336_systems.ops.rope import _hip_layout_ok

    assert _hip_layout_ok(x)
    pos = torch.randint(0, ctx, (B, N), device=DEV, generator=g) if with_pos else None
    p = pos[:, None, :] if with_pos else torch.arange(N, device=DEV)
    xg = x.detach().requires_grad_(True)
    y = ops.rope(xg, cos, sin, pos)
    assert y.dtype == dt and y.shape == x.shape
    check(y, ops.rope_ref(x.double(), cos, sin, p), ops.rope_ref(x.float(), cos, sin, p), dt, "rope.fwd")
    dy = torch.randn(B, N, H, D, device=DEV, generator=g).to(dt).transpose(1, 2)
    y.backward(dy)
    # R is orthogonal: the backward is the rotation by -theta
    check(xg.grad, ops.rope_ref(dy.double(), cos, -sin, p), ops.rope_ref(dy.float(), cos, -sin, p), dt, "rope.inverse")
