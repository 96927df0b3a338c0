"""Edge cases of the FlashAttention-2 HIP kernels (``csrc/flash_attn/fa_fwd.hip``, ``fa_bwd.hip``,
``fa_bwd_fused.hip``, ``fa_bwd_hs.hip``, ``fa_bwd_kp.hip`` and the split reduce kernels) against fp64
(GPU only; the references and the banded rule are tested on the CPU in ``test_flash_edges_rule.py``).

Covers Nq != Nk, N from 1 to 129, VGPR and LDS-DMA staging, forced and automatic key / query splits,
every backward form at the smallest N that reaches each of its paths, host-padded head dims, and
structured values (constant V, uniform P, ties, a dominating key, a ramp and a late spike for the
deferred rescale, scores near -1e3 / +1e3, dO = 0, fp16 dO at the edge of the fp16 range).

Three evaluations of the same rounded inputs with a materialised Nq x Nk matrix (``attn_ref``):
``ref64`` in fp64; ``refw``, the working-precision reference (plain fp32 for fp32 inputs; for 16-bit
inputs fp32 with a round to the input type where the data must pass through it: P before P@V and
P^T@dO, dS before dS@K and dS^T@Q, O before delta = rowsum(dO*O)); and the kernel, which gets its own
O and LSE for the backward. LSE is fp32 and is held to the plain fp32 evaluation with u = 0.

The rule is ``check`` of ``test_kernel_edges_gpu.py`` (|got - ref64| <= k*E + u*|ref64| + tiny with
E = max(max|refw - ref64|, 2^-23 max|ref64|), k = 4), applied per (batch, head) and per band of 64
rows (``check_banded``): query rows for O, LSE and dQ, key rows for dK and dV, so E follows the band's
own magnitude. Where a band's reference is exactly zero (causal with keys past the last query, dO = 0)
E is zero and the kernel must write zeros within ``tiny``. Which kernel produced the numbers is asserted
through ``torch.ops.cs336.fa_last_launch()``.

The floor of E for dQ and dK is 2^-23 max M with M >= |ref64| the magnitude of what cancels in
dS = P (dP - delta) (``cancel_mag``; the reasoning is in ``check_banded``): with one visible key, constant
V or a dominating key the gradient is zero or tiny, refw cancelled to an exact 0 on the GPU, and the
kernels, which form dP on the matrix cores and delta on the vector ALU, left 7e-8 .. 2.6e-7 (ratios of
1e8 .. 1e31 against an E of 0 .. 2e-16). For O, LSE and dV the floor is 2^-23 max|ref64| as in ``check``.

Measured ``max (|got - ref64| - u*|ref64|) / E`` per (op, output dtype) over the bands, on an MI355X
(236 test cases, each looping over causal / non-causal and its switches; the whole file takes 12 s). 0 in a 16-bit
column: the error stayed within ``u*|ref64|``; ``-``: no such case. Suffixes: cross = Nq != Nk, tiny = N 1 ..
129, staging / splits = the CS336_FA_DMA / split cases, self = the forwards of the one-kernel cases, fused /
hs / kp = those backwards, pad = host-padded head dims, and the value generators: cancel (vconst,
dominant), uniform (qzero, ties), rescale (ramp, spike), offset (scores -1e3 / +1e3), dozero, range (bigdo).
Ratios above 4 are listed in ``FA_K_CASE`` with their reasons; none is above 16:

    op (suffix: the test group)   fp32     bf16     fp16
    ----------------------------------------------------
    fa.dk.cancel               1.396    0.240    0.079
    fa.dk.cross                9.216    1.241    1.000
    fa.dk.dozero               0.000    0.000    0.000
    fa.dk.fused                    -    1.428    1.173
    fa.dk.hs                       -    1.163    1.220
    fa.dk.kp                       -    1.428    1.173
    fa.dk.offset               1.917    1.161    1.790
    fa.dk.pad                  5.718    1.283        -
    fa.dk.range                    -        -    0.930
    fa.dk.rescale              3.515    4.136    2.120
    fa.dk.splits                   -    0.981        -
    fa.dk.staging                  -    1.065        -
    fa.dk.tiny                 4.531    6.020    1.101
    fa.dk.uniform              1.320    0.997    0.996
    fa.dq.cancel               2.500    0.636    0.810
    fa.dq.cross                3.410    1.295    1.136
    fa.dq.dozero               0.000    0.000    0.000
    fa.dq.fused                    -    1.201    1.191
    fa.dq.hs                       -    1.334    1.187
    fa.dq.kp                       -    1.870    1.239
    fa.dq.offset               1.513    5.534    3.402
    fa.dq.pad                  2.990    1.383        -
    fa.dq.range                    -        -    0.993
    fa.dq.rescale              2.079    2.103    2.457
    fa.dq.splits                   -    1.032        -
    fa.dq.staging                  -    1.289        -
    fa.dq.tiny                 2.156    1.388    1.088
    fa.dq.uniform              1.774    1.150    1.176
    fa.dv.cancel              15.681    0.992    0.928
    fa.dv.cross                5.986    0.995    0.977
    fa.dv.dozero               0.000    0.000    0.000
    fa.dv.fused                    -    0.990    0.983
    fa.dv.hs                       -    1.002    0.989
    fa.dv.kp                       -    1.065    1.022
    fa.dv.offset               1.333    1.051    1.059
    fa.dv.pad                  5.137    1.001        -
    fa.dv.range                    -        -    0.928
    fa.dv.rescale              4.431    0.975    0.913
    fa.dv.splits                   -    0.990        -
    fa.dv.staging                  -    0.999        -
    fa.dv.tiny                 2.986    0.998    0.963
    fa.dv.uniform              1.667    0.985    0.921
    fa.lse.cancel              1.660        -        -
    fa.lse.cross               8.035        -        -
    fa.lse.dozero              1.277        -        -
    fa.lse.offset              1.439        -        -
    fa.lse.range               1.259        -        -
    fa.lse.rescale             2.329        -        -
    fa.lse.self                1.294        -        -
    fa.lse.splits              1.138        -        -
    fa.lse.staging             1.234        -        -
    fa.lse.tiny                8.035        -        -
    fa.lse.uniform             1.456        -        -
    fa.o.cancel                2.000    0.000    0.000
    fa.o.cross                 4.149    2.284    1.100
    fa.o.dozero                3.327    1.278    1.527
    fa.o.offset                1.005    1.758    1.022
    fa.o.pad                   2.482    1.537        -
    fa.o.range                     -        -    1.527
    fa.o.rescale               2.234    2.205    1.824
    fa.o.self                      -    1.916    1.527
    fa.o.splits                    -    1.358        -
    fa.o.staging                   -    1.441        -
    fa.o.tiny                  2.305    1.458    1.698
    fa.o.uniform               2.322    0.000    0.000
"""

import collections
import contextlib
import functools
import math
import os

import pytest
import torch

from .test_kernel_edges_gpu import BF16, DEV, F16, F32, K, K_CASE, U, _RATIOS, _f32, _name, _ratio_report, _unravel, check  # noqa: F401

pytestmark = pytest.mark.gpu

BAND = 64
FA_ENV = ("CS336_FA_BWD", "CS336_FA_DMA", "CS336_FA_SPLITS", "CS336_FA_BWD_SPLITS", "CS336_FA_HS_DELTA",
          "CS336_FA_HS_ROPE", "CS336_FA_KP_WAVES", "CS336_FA_KP_SLAB")
TWO_KERNEL, FUSED, KP, HS = 0, 1, 2, 3  # as CS336_FA_BWD numbers the backward forms

# margins above 4 per (op, output dtype), by the rule of test_kernel_edges_gpu.K_CASE: the next power of two
# above twice the measured ratio, never above 32, each with its reason. Two reasons recur.
# "fp32": for fp32 inputs refw's own error over a band is often below 2^-23 of the band's maximum, so E is
#   the floor, one rounding of the result, while the kernel chains 32 fp32 MFMAs per dot product and
#   evaluates exp2 of s*scale*log2(e) - lse*log2(e), whose argument is 1.44 times the reference's (in nats)
#   and whose lse was stored in natural-log units and scaled back: 2-3 roundings of |lse|*log2(e) reach P.
# "few rows": a band of 1-3 rows (N 1, 2; the ragged last band of N 65, 67, 129, 130) takes E from the
#   maximum over a handful of elements of one sample of refw's rounding error; the kernel's error is
#   another sample of the same distribution.
FA_K_CASE: dict = {
    ("fa.lse.tiny", "float32"): 32,   # 8.04: fp32, few rows -- N 1, lse = s*scale: one 64-term dot product, E one element
    ("fa.lse.cross", "float32"): 32,  # 8.04: the same case, (1, 1)
    ("fa.o.cross", "float32"): 16,    # 4.15: fp32, few rows -- (1, 300), one query row per band
    ("fa.dk.cross", "float32"): 32,   # 9.22: fp32 -- (1, 300): every dK row is one query's P (dP - delta) q, no averaging over queries
    ("fa.dv.cross", "float32"): 16,   # 5.99: fp32 -- (1, 300), as dK
    ("fa.dk.tiny", "float32"): 16,    # 4.53: fp32, few rows -- row 128 of N 129
    ("fa.dk.tiny", "bfloat16"): 16,   # 6.02: few rows -- row 128 of N 129 at d 16: E from 16 elements
    ("fa.dk.pad", "float32"): 16,     # 5.72: fp32, few rows -- row 64 of N 65, rows 128-129 of 130
    ("fa.dv.pad", "float32"): 16,     # 5.14: fp32, few rows -- row 64 of N 65
    ("fa.dv.cancel", "float32"): 32,  # 15.7: fp32 -- dominant: |lse*log2(e)| = 173, P = exp2(s c - lse log2 e) is 1 +- 2e-5 where refw's exp(s - lse) is exp(0)
    ("fa.dv.rescale", "float32"): 16, # 4.43: fp32 -- ramp / spike: |lse*log2(e)| up to 30
    ("fa.dk.rescale", "bfloat16"): 16,  # 4.14: few rows -- rows 64-66 of Nk 67 (ramp)
    ("fa.dq.offset", "bfloat16"): 16,   # 5.53: few rows -- rows 128-129 of Nq 130; dQ[:, 0] = 31 sum_j rnd(dS_ij) sums 67 bf16 roundings of terms that cancel
}


# ------------------------------------------------------------------------------------ references
def _rnd(x, rdt):
    return x if rdt == F32 else x.to(rdt).to(x.dtype)


Ref = collections.namedtuple("Ref", "o lse dq dk dv")


def attn_ref(q, k, v, do, causal, scale, ft, rdt):
    """O, LSE, dQ, dK, dV of softmax(scale * Q K^T [key <= query]) V on (B, H, N, D) tensors, evaluated
    in the float type ``ft`` with the full score matrix; ``rdt`` is the type P, dS and O are rounded
    through on their way into the matrix products / delta (F32: no rounding)."""
    qf, kf, vf, gf = (t.to(ft) for t in (q, k, v, do))
    sc = _f32(scale)
    s = qf @ kf.transpose(-1, -2) * sc
    if causal:
        nq, nk = s.shape[-2:]
        keep = torch.arange(nk, device=s.device)[None, :] <= torch.arange(nq, device=s.device)[:, None]
        s = s.masked_fill(~keep, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    o = (_rnd(e, rdt) @ vf) / l
    p = torch.exp(s - lse)
    dv = _rnd(p, rdt).transpose(-1, -2) @ gf
    dp = gf @ vf.transpose(-1, -2)
    delta = (gf * _rnd(o, rdt)).sum(-1, keepdim=True)
    ds = _rnd(p * (dp - delta), rdt)
    dq = ds @ kf * sc
    dk = ds.transpose(-1, -2) @ qf * sc
    return Ref(o, lse[..., 0], dq, dk, dv)


def cancel_mag(q, k, v, do, r64, causal, scale):
    """fp64 magnitudes (M_dQ, M_dK) of what cancels in dS = P (dP - delta): dQ and dK evaluated with
    |dP| + |delta| in place of dP - delta and |K|, |Q| in place of K, Q. See ``check_banded``."""
    qf, kf, vf, gf = (t.double() for t in (q, k, v, do))
    sc = _f32(scale)
    s = qf @ kf.transpose(-1, -2) * sc
    if causal:
        nq, nk = s.shape[-2:]
        keep = torch.arange(nk, device=s.device)[None, :] <= torch.arange(nq, device=s.device)[:, None]
        s = s.masked_fill(~keep, float("-inf"))
    p = torch.exp(s - r64.lse[..., None])
    ds = p * ((gf @ vf.transpose(-1, -2)).abs() + (gf * r64.o).sum(-1, keepdim=True).abs())
    return ds @ kf.abs() * sc, ds.transpose(-1, -2) @ qf.abs() * sc


def check_banded(got, ref64, refw, out_dtype, op, k=None, band=BAND, mag=None):
    """``check`` per (batch, head) and per band of ``band`` rows of (B, H, N, D) (or (B, H, N)) tensors.
    All bands are evaluated at once; the worst failing band goes through ``check`` itself, which
    reports its worst element. Returns the largest per-band ratio.

    ``mag`` (dQ and dK only, from ``cancel_mag``) replaces |ref64| in the floor of E, which becomes
    max(max|refw - ref64|, 2^-23 max M). Reason: dS = P (dP - delta) subtracts two fp32 dot products
    over d. Each is at best the correctly rounded value, so dS carries an absolute error of at least
    2^-24 P (|dP| + |delta|) in any implementation, and dQ, dK inherit it through |K|, |Q|. Where the
    difference cancels (one visible key: dP = delta exactly; V constant; dO = c O) the true result is
    zero or tiny and 2^-23 |ref64| says nothing about that error, while ``refw`` can cancel to an exact 0
    when its two dot products happen to round alike -- E would then be 0 by accident and no kernel that
    forms dP on the matrix cores and delta on the vector ALU could meet it. M >= |ref64| element-wise, M
    is 0 wherever the gradient is structurally 0 (masked keys, dO = 0), and it depends on the inputs alone."""
    k = FA_K_CASE.get((op, _name(out_dtype)), K_CASE.get(op, K)) if k is None else k
    assert k <= 32
    u, tiny = U[out_dtype], torch.finfo(out_dtype).tiny
    g, r64, rw = got.detach().double(), ref64.detach().double(), refw.detach().double()
    assert g.shape == r64.shape == rw.shape, (op, g.shape, r64.shape, rw.shape)
    if g.dim() == 3:
        g, r64, rw = g[..., None], r64[..., None], rw[..., None]
    B, H, N, D = g.shape
    if g.numel() == 0:
        return 0.0
    fin = torch.isfinite(r64)
    assert torch.equal(torch.isfinite(rw), fin), f"{op}: the working-precision and fp64 references disagree on where values are finite"
    if not torch.equal(torch.isfinite(g), fin):
        check(g, r64, rw, out_dtype, None, k)  # fails, naming the first element
    nb = (N + band - 1) // band
    pad = nb * band - N
    zero = torch.zeros_like(r64)
    a64 = torch.where(fin, r64.abs(), zero)
    dw = torch.where(fin, (rw - r64).abs(), zero)
    err = torch.where(fin, (g - r64).abs(), zero)

    def bands(x):  # (B, H, nb, band * D); padding rows are zero and change no maximum
        return torch.nn.functional.pad(x, (0, 0, 0, pad)).reshape(B, H, nb, band * D)

    a64, dw, err = bands(a64), bands(dw), bands(err)
    if mag is not None:
        m64 = mag.detach().double()
        assert m64.shape == r64.shape and bool((m64 >= torch.where(fin, r64.abs(), zero) * (1 - 1e-12)).all()), op
    e = torch.maximum(dw.amax(-1), 2.0**-23 * (a64 if mag is None else bands(m64)).amax(-1))  # (B, H, nb)
    ratio_b = (err - u * a64).clamp_min(0).amax(-1) / e.clamp_min(tiny)
    ratio = ratio_b.max().item()
    if op is not None:
        key = (op, _name(out_dtype))
        _RATIOS[key] = max(_RATIOS.get(key, 0.0), ratio)
    excess = (err - (k * e[..., None] + u * a64 + tiny)).amax(-1)
    if excess.max().item() > 0:
        b, h, n = (int(i) for i in (excess == excess.max()).nonzero()[0])
        rows = slice(n * band, min(N, (n + 1) * band))
        where = (f"{op} batch {b} head {h} rows {rows.start}..{rows.stop - 1} of {N} ({int((excess > 0).sum())} of "
                 f"{excess.numel()} bands out of bound)")
        if mag is not None:  # the band's own E, with the floor from M
            eb = e[b, h, n].item()
            gb, rb = g[b, h, rows], r64[b, h, rows]
            ex = ((gb - rb).abs() - (k * eb + u * rb.abs() + tiny)).flatten()
            i = int(ex.argmax())
            pytest.fail(f"{where}: [{_name(out_dtype)}]: worst element {_unravel(i, gb.shape)}: got {gb.flatten()[i].item()!r}, ref "
                        f"{rb.flatten()[i].item()!r}, |err| {(gb - rb).abs().flatten()[i].item():.3e} > bound "
                        f"{k * eb + u * rb.abs().flatten()[i].item() + tiny:.3e} (k={k}, E={eb:.3e}, ratio={ratio_b[b, h, n].item():.2f})")
        try:
            check(g[b, h, rows], r64[b, h, rows], rw[b, h, rows], out_dtype, None, k)
        except pytest.fail.Exception as exc:
            pytest.fail(f"{where}: {exc.msg}")
        raise AssertionError(f"{op}: check_banded and check disagree on band {(b, h, n)}")
    return ratio


# ------------------------------------------------------------------------------------ inputs
def _randn(B, H, N, D, dt, g, dev):
    """(B, N, H, D) memory viewed as (B, H, N, D), as in the model."""
    return torch.randn(B, N, H, D, device=dev, generator=g).to(dt).transpose(1, 2)


def _base(B, H, Nq, Nk, D, dt, g, dev):
    return [_randn(B, H, n, D, dt, g, dev) for n in (Nq, Nk, Nk, Nq)]  # q, k, v, dO


def gen_randn(B, H, Nq, Nk, D, dt, causal, g, dev):
    return _base(B, H, Nq, Nk, D, dt, g, dev)


def gen_vconst(B, H, Nq, Nk, D, dt, causal, g, dev):
    """V constant per column: O equals it, dP - delta cancels exactly, dQ and dK are pure cancellation."""
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    v.copy_(v[:, :, :1].clone().expand_as(v))
    return q, k, v, do


def gen_qzero(B, H, Nq, Nk, D, dt, causal, g, dev):
    """q = 0: every score is 0, P is uniform over the visible keys."""
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    q.zero_()
    return q, k, v, do


def gen_ties(B, H, Nq, Nk, D, dt, causal, g, dev):
    """All keys identical: every row's scores tie."""
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    k.copy_(k[:, :, :1].clone().expand_as(k))
    return q, k, v, do


def gen_dominant(B, H, Nq, Nk, D, dt, causal, g, dev):
    """One key (the first under the causal mask, else one in the last third) scores about 120 above the
    rest for every row: the other P underflow, in fp32 too (e^-118 < 2^-149)."""
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    q[..., 0] = 8.0
    k[:, :, 0 if causal else (2 * Nk) // 3, 0] = 120.0 / (8.0 * _f32(D**-0.5))
    return q, k, v, do


def gen_ramp(B, H, Nq, Nk, D, dt, causal, g, dev):
    """Scores rise 5 log2 units per 64 keys: the running max goes stale on one tile (5 < kRescaleThr = 8)
    and is raised on the next."""
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    q[..., 0] = 8.0
    k[..., 0] = (5.0 * math.log(2.0) / 64.0) * torch.arange(Nk, device=dev, dtype=torch.float32)[None, None, :] / (8.0 * _f32(D**-0.5))
    return q, k, v, do


def gen_spike(B, H, Nq, Nk, D, dt, causal, g, dev):
    """Key Nk - 2 (the last tile) scores 16 (23 log2 units) for every third query and 0 for the others:
    the rescale ballot fires for some lanes of a wave only."""
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    q[..., 1] = 0.0
    q[:, :, ::3, 1] = 8.0
    k[..., 1] = 0.0
    k[:, :, Nk - 2, 1] = 16.0 / (8.0 * _f32(D**-0.5))
    return q, k, v, do


def _offset_scores(off):
    def gen(B, H, Nq, Nk, D, dt, causal, g, dev):
        q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
        q[..., 0] = 32.0
        k[..., 0] = off / (32.0 * _f32(D**-0.5))
        return q, k, v, do

    gen.__doc__ = f"All scores near {off:+.0e}."
    return gen


def gen_dozero(B, H, Nq, Nk, D, dt, causal, g, dev):
    """dO = 0: every gradient is exactly zero."""
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    do.zero_()
    return q, k, v, do


def _all_finite(ref, dt):
    return all(bool(torch.isfinite(t.to(dt) if t is not ref.lse else t).all()) for t in ref)


def gen_bigdo(B, H, Nq, Nk, D, dt, causal, g, dev):
    """fp16: dO scaled by the largest power of two at which the working-precision reference (dS rounded
    to fp16) and the fp64 one, with their results stored as fp16, are finite everywhere."""
    assert dt == F16
    q, k, v, do = _base(B, H, Nq, Nk, D, dt, g, dev)
    sc = D**-0.5
    for e in range(15, -1, -1):
        big = (do.float() * 2.0**e).to(F16)
        if not torch.isfinite(big).all():
            continue
        if _all_finite(attn_ref(q, k, v, big, causal, sc, F32, F16), F16) and _all_finite(attn_ref(q, k, v, big, causal, sc, torch.float64, F32), F16):
            return q, k, v, big
    raise AssertionError("no finite scale")


GENERATORS = {
    "randn": gen_randn,
    "vconst": gen_vconst,
    "qzero": gen_qzero,
    "ties": gen_ties,
    "dominant": gen_dominant,
    "ramp": gen_ramp,
    "spike": gen_spike,
    "scores-1e3": _offset_scores(-1e3),
    "scores+1e3": _offset_scores(1e3),
    "dozero": gen_dozero,
    "bigdo": gen_bigdo,
}
VALUE_GENERATORS = [n for n in GENERATORS if n != "randn"]
# the op suffix a generator's results are reported (and given a margin) under
VALUE_GROUP = {"vconst": "cancel", "qzero": "uniform", "ties": "uniform", "dominant": "cancel", "ramp": "rescale", "spike": "rescale",
               "scores-1e3": "offset", "scores+1e3": "offset", "dozero": "dozero", "bigdo": "range"}

Case = collections.namedtuple("Case", "q k v do causal scale dt r64 rw mdq mdk")


def make_case(gen, B, H, Nq, Nk, D, dt, causal, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * seed + 7 * Nq + 3 * Nk + D)
    q, k, v, do = GENERATORS[gen](B, H, Nq, Nk, D, dt, causal, g, dev)
    scale = D**-0.5
    r64 = attn_ref(q, k, v, do, causal, scale, torch.float64, F32)
    rw = attn_ref(q, k, v, do, causal, scale, F32, dt)
    return Case(q, k, v, do, causal, scale, dt, r64, rw, *cancel_mag(q, k, v, do, r64, causal, scale))


@functools.lru_cache(maxsize=None)
def _case(gen, B, H, Nq, Nk, D, dt, causal, seed=0):
    """Inputs and both references, computed once per (generator, shape, seed) and never modified."""
    return make_case(gen, B, H, Nq, Nk, D, dt, causal, DEV, seed)


# ------------------------------------------------------------------------------------ running the kernels
def _hip():
    from cs336_systems.ops._ext import ops

    return ops()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in FA_ENV:
        monkeypatch.delenv(name, raising=False)


@contextlib.contextmanager
def _env(**kv):
    """CS336_FA_<NAME>=value for the block; None leaves the switch unset."""
    old = {}
    for name, val in kv.items():
        key = "CS336_FA_" + name
        assert key in FA_ENV
        old[key] = os.environ.pop(key, None)
        if val is not None:
            os.environ[key] = str(val)
    try:
        yield
    finally:
        for key, val in old.items():
            os.environ.pop(key, None)
            if val is not None:
                os.environ[key] = val


def _fwd(c, tag):
    """fa_fwd under the rule; returns (O, LSE, forward splits launched)."""
    o, lse = _hip().fa_fwd(c.q, c.k, c.v, c.causal, c.scale)
    splits = _hip().fa_last_launch()[0]
    assert o.dtype == c.dt and o.shape == c.q.shape and lse.dtype == F32 and lse.shape == c.q.shape[:3]
    check_banded(o, c.r64.o, c.rw.o, c.dt, f"fa.o{tag}")
    check_banded(lse, c.r64.lse, c.rw.lse, F32, f"fa.lse{tag}")
    return o, lse, splits


def _bwd(c, o, lse, tag, rule=True):
    """fa_bwd on the kernel's own O and LSE under the rule; returns ((dQ, dK, dV), [form, ksplit, qsplit])."""
    grads = _hip().fa_bwd(c.do, c.q, c.k, c.v, o, lse, c.causal, c.scale)
    launch = list(_hip().fa_last_launch()[1:])
    if rule:
        for name, got, r64, rw, like, mag in (("dq", grads[0], c.r64.dq, c.rw.dq, c.q, c.mdq), ("dk", grads[1], c.r64.dk, c.rw.dk, c.k, c.mdk),
                                              ("dv", grads[2], c.r64.dv, c.rw.dv, c.v, None)):
            assert got.dtype == c.dt and got.shape == like.shape, (name, got.dtype, got.shape)
            check_banded(got, r64, rw, c.dt, f"fa.{name}{tag}", mag=mag)
    return grads, launch


def _assert_bitwise(a, b, what):
    for name, x, y in zip(("dq", "dk", "dv"), a, b):
        if not torch.equal(x, y):
            pytest.fail(f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} elements")


def expected_form(mode, B, H, Nq, Nk, D, dt):
    """The backward fa_bwd_run launches, from the ``*_ok()`` predicates and its selection (no RoPE, the
    strides of these tests): hs needs 16-bit d 64 self-attention with N % 128 == 0; fused N % 64 == 0
    and N <= 1024; kp d 64 or 80 and N % 64 == 0. ``mode`` is CS336_FA_BWD (None: unset)."""
    self16 = dt != F32 and Nq == Nk and Nq > 0
    hs_ok = self16 and D == 64 and Nq % 128 == 0
    fused_ok = self16 and D == 64 and Nq % 64 == 0 and Nq <= 1024
    kp_ok = self16 and D in (64, 80) and Nq % 64 == 0
    nbh = B * H
    if (mode == 3 or (mode is None and nbh >= 512 and Nq <= 1024)) and hs_ok:
        return HS
    if mode not in (0, 2) and (mode == 1 or nbh >= 512) and fused_ok:
        return FUSED
    kp_default = D == 80 or (D == 64 and Nq >= 2048 and nbh * ((Nq + 255) // 256) >= 512)
    if (mode == 2 or (mode is None and kp_default)) and kp_ok:
        return KP
    return TWO_KERNEL


def expected_fwd_splits(B, H, Nq, Nk, D):
    """flash_attn_fwd_splits: fewer than 256 workgroups and at least 8 key tiles."""
    wgs, tiles = (Nq + 127) // 128 * B * H, (Nk + 63) // 64
    if wgs >= 256 or tiles < 8:
        return 1
    return max(1, min((512 + wgs - 1) // wgs, tiles // 4, 16))


def expected_bwd_splits(B, H, Nq, Nk, D):
    """flash_attn_bwd_splits: (ksplit, qsplit) of the two-kernel form."""
    bh, nqb, nkb = B * H, (Nq + 127) // 128, (Nk + 127) // 128
    ks = max(1, min((512 + nqb * bh - 1) // (nqb * bh), Nk // 32 // 4, 16)) if nqb * bh < 256 else 1
    qs = max(1, min((512 + nkb * bh - 1) // (nkb * bh), Nq // 32 // 4, 16)) if nkb * bh < 256 else 1
    return ks, qs


CAUSAL = (False, True)
_dt_id = lambda v: _name(v) if isinstance(v, torch.dtype) else None  # noqa: E731
D_DT = [(64, F32), (64, BF16), (64, F16), (16, BF16), (32, BF16), (80, BF16), (128, BF16)]


# ------------------------------------------------------------------------------------ 1. cross lengths
CROSS = [(1, 1), (1, 300), (33, 200), (200, 33), (67, 130), (130, 67), (128, 129), (129, 128), (257, 64)]


@pytest.mark.parametrize("Nq,Nk", CROSS)
@pytest.mark.parametrize("D,dt", D_DT, ids=_dt_id)
def test_cross_lengths(D, dt, Nq, Nk):
    """Nq != Nk through raw fa_fwd + fa_bwd: the two-kernel form runs whatever CS336_FA_BWD says (every
    one-kernel form requires Nq == Nk) and, having no atomics, gives the same bits each time. Under the
    causal mask keys past the last query get exact zeros."""
    for causal in CAUSAL:
        c = _case("randn", 2, 3, Nq, Nk, D, dt, causal)
        o, lse, _ = _fwd(c, ".cross")
        grads, launch = _bwd(c, o, lse, ".cross")
        if Nq != Nk:
            assert launch[0] == TWO_KERNEL, launch
        assert launch[0] == expected_form(None, 2, 3, Nq, Nk, D, dt), launch
        if causal and Nk > Nq:
            assert torch.all(grads[1][:, :, Nq:] == 0) and torch.all(grads[2][:, :, Nq:] == 0)
        if Nq != Nk:
            for mode in (1, 2, 3):
                with _env(BWD=mode):
                    forced, fl = _bwd(c, o, lse, ".cross", rule=False)
                assert fl[0] == TWO_KERNEL, (mode, fl)
                _assert_bitwise(forced, grads, f"CS336_FA_BWD={mode} causal={causal}")


# ------------------------------------------------------------------------------------ 2. staging and splits
@pytest.mark.parametrize("Nq,Nk", [(67, 130), (130, 67), (300, 1100)])
@pytest.mark.parametrize("dma,D", [(0, 64), (1, 64), (2, 64), (4, 64), (4, 128)])
def test_staging_cross_lengths(dma, D, Nq, Nk):
    """CS336_FA_DMA = 0 (VGPR staging everywhere), 1, 2 (LDS-DMA backward too) and 4 (the pipelined
    forward) on Nq != Nk."""
    for causal in CAUSAL:
        c = _case("randn", 2, 3, Nq, Nk, D, BF16, causal)
        with _env(DMA=dma):
            o, lse, _ = _fwd(c, ".staging")
            _, launch = _bwd(c, o, lse, ".staging")
        assert launch[0] == TWO_KERNEL, launch


@pytest.mark.parametrize("Nq,Nk", [(33, 1100), (600, 1100), (1100, 600)])
def test_splits_cross_lengths(Nq, Nk):
    """B = H = 1: the forward splits the keys, the two-kernel backward splits keys (dQ) and queries
    (dK / dV) by the host formulas; forced split counts and the unsplit kernels give the same result."""
    B = H = 1
    fs, (ks, qs) = expected_fwd_splits(B, H, Nq, Nk, 64), expected_bwd_splits(B, H, Nq, Nk, 64)
    assert fs > 1 and (ks > 1 or qs > 1), "the shape must reach the split kernels"
    for causal in CAUSAL:
        c = _case("randn", B, H, Nq, Nk, 64, BF16, causal)
        for splits in (None, 1, 7):
            with _env(SPLITS=splits):
                o, lse, launched = _fwd(c, ".splits")
            assert launched == (fs if splits is None else splits), (splits, launched)
        for bs in (None, 1):
            with _env(BWD_SPLITS=bs):
                _, launch = _bwd(c, o, lse, ".splits")
            assert launch == [TWO_KERNEL, *((ks, qs) if bs is None else (1, 1))], (bs, launch)


# ------------------------------------------------------------------------------------ 3. tiny and ragged N
@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 63, 65, 127, 129])
@pytest.mark.parametrize("D,dt", [(64, F32), (64, BF16), (64, F16), (16, BF16), (16, F16), (80, BF16), (80, F16)], ids=_dt_id)
def test_tiny_self_attention(D, dt, N):
    """A partial first tile, one wave with a single live row, one row past a tile; every CS336_FA_BWD
    value falls back to the form the ``*_ok()`` predicates allow."""
    B, H = 2, 3
    for causal in CAUSAL:
        c = _case("randn", B, H, N, N, D, dt, causal)
        o, lse, _ = _fwd(c, ".tiny")
        for mode in (None, 0, 1, 2, 3):
            with _env(BWD=mode):
                _, launch = _bwd(c, o, lse, ".tiny")
            assert launch[0] == expected_form(mode, B, H, N, N, D, dt), (mode, launch)


# ------------------------------------------------------------------------------------ 4. one-kernel backwards
def _one_kernel(c, form, tag, o_lse, repeat_bitwise, **env):
    o, lse = o_lse
    with _env(**env):
        grads, launch = _bwd(c, o, lse, tag)
        assert launch[0] == form, (env, launch)
        again, _ = _bwd(c, o, lse, tag, rule=False)
    if repeat_bitwise:
        _assert_bitwise(again, grads, f"{tag} {env} run twice")
    else:  # dQ by fp32 atomics; dK and dV have none
        _assert_bitwise(again[1:], grads[1:], f"{tag} {env} run twice (dK, dV)")
    return grads


@pytest.mark.parametrize("N", [64, 128, 192, 320, 1024])
@pytest.mark.parametrize("dt", [BF16, F16], ids=_name)
def test_fused_backward(dt, N):
    """fa_bwd_fused.hip: one and several 64-row slices, and past one 256-key block (N 320), where dQ
    is summed from the dq_acc partials."""
    for causal in CAUSAL:
        c = _case("randn", 2, 3, N, N, 64, dt, causal)
        o, lse, _ = _fwd(c, ".self")
        _one_kernel(c, FUSED, ".fused", (o, lse), True, BWD=1)


@pytest.mark.parametrize("N", [128, 256, 384, 1024, 1152])
@pytest.mark.parametrize("dt", [BF16, F16], ids=_name)
def test_hs_backward(dt, N):
    """fa_bwd_hs.hip: one key block, several (dQ partials), in-kernel delta (N <= 1024) and the prep
    kernel (N 1152, and CS336_FA_HS_DELTA=0 at 128 and 1024, bitwise the in-kernel delta)."""
    for causal in CAUSAL:
        c = _case("randn", 2, 3, N, N, 64, dt, causal)
        o, lse, _ = _fwd(c, ".self")
        grads = _one_kernel(c, HS, ".hs", (o, lse), True, BWD=3)
        if N in (128, 1024):
            prep = _one_kernel(c, HS, ".hs", (o, lse), True, BWD=3, HS_DELTA=0)
            _assert_bitwise(prep, grads, "CS336_FA_HS_DELTA=0")


@pytest.mark.parametrize("N", [64, 256, 320, 1024, 1088])
@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("dt", [BF16, F16], ids=_name)
def test_kp_backward(dt, D, N):
    """fa_bwd_kp.hip with 4 and 8 waves; dQ by slabs (unset up to N 1024, or forced) repeats bitwise,
    by atomics (CS336_FA_KP_SLAB=0, unset at N 1088) only dK and dV do."""
    for causal in CAUSAL:
        c = _case("randn", 2, 3, N, N, D, dt, causal)
        o, lse, _ = _fwd(c, ".self")
        for waves in (4, 8):
            for slab in (0, 1, None):
                slabs = slab == 1 or (slab is None and N <= 1024)
                _one_kernel(c, KP, ".kp", (o, lse), slabs, BWD=2, KP_WAVES=waves, KP_SLAB=slab)


# ------------------------------------------------------------------------------------ 5. values
@pytest.mark.parametrize("dt,gen", [(dt, gen) for dt in (F32, BF16, F16) for gen in VALUE_GENERATORS if gen != "bigdo" or dt == F16], ids=_dt_id)
def test_values(dt, gen):
    """Structured inputs at N 256 (the default form and, for 16-bit inputs, each one-kernel form) and at
    (Nq, Nk) = (130, 67); "bigdo" is the fp16 range case."""
    tag = "." + VALUE_GROUP[gen]
    for causal in CAUSAL:
        c = _case(gen, 2, 3, 256, 256, 64, dt, causal)
        o, lse, _ = _fwd(c, tag)
        for mode in (None,) if dt == F32 else (None, 1, 2, 3):
            with _env(BWD=mode):
                grads, launch = _bwd(c, o, lse, tag)
            assert launch[0] == (TWO_KERNEL if mode is None else mode), (mode, launch)
            _values_exact(gen, c, o, grads)
        c = _case(gen, 2, 3, 130, 67, 64, dt, causal)
        o, lse, _ = _fwd(c, tag)
        grads, launch = _bwd(c, o, lse, tag)
        assert launch[0] == TWO_KERNEL, launch
        _values_exact(gen, c, o, grads)


def _values_exact(gen, c, o, grads):
    for t in (o, *grads):
        assert torch.isfinite(t).all()
    if gen == "dozero":
        for t in grads:
            assert torch.all(t == 0)
    if gen == "dominant" and c.dt != F32:  # P is 1 and 0 exactly after the round to 16 bits
        j = 0 if c.causal else (2 * c.k.shape[2]) // 3
        assert torch.equal(o, c.v[:, :, j : j + 1].expand_as(o)), "O must be the dominating key's V row"


# ------------------------------------------------------------------------------------ 6. host-padded head dims
@pytest.mark.parametrize("ndim", [4, 3, 2])
@pytest.mark.parametrize("D,dt", [(8, BF16), (24, BF16), (40, BF16), (96, BF16), (120, BF16), (16, F32), (80, F32), (100, F32)], ids=_dt_id)
def test_host_padded_head_dims(D, dt, ndim):
    """FlashAttentionHIP.apply with autograd at head dims the kernels do not run natively (zero-padded
    on the host to 32 / 64 / 128), on 4-D, 3-D and 2-D inputs, self-attention and one Nq != Nk pair."""
    from cs336_systems.ops.flash_attention import FlashAttentionHIP

    B, H = {4: (2, 3), 3: (3, 1), 2: (1, 1)}[ndim]
    for Nq, Nk in ((65, 65), (67, 130)):
        for causal in CAUSAL:
            c = _case("randn", B, H, Nq, Nk, D, dt, causal)

            def user(t):  # the caller's view of a (B, H, N, D) tensor
                t = t if ndim == 4 else (t[:, 0] if ndim == 3 else t[0, 0])
                return t.detach().clone().requires_grad_(True)

            q, k, v = user(c.q), user(c.k), user(c.v)
            o = FlashAttentionHIP.apply(q, k, v, causal)
            assert o.dtype == dt and o.shape == q.shape
            o.backward(user(c.do).detach())
            assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape
            as4 = lambda t: t.detach().reshape(B, H, t.shape[-2], D)  # noqa: E731
            check_banded(as4(o), c.r64.o, c.rw.o, dt, "fa.o.pad")
            check_banded(as4(q.grad), c.r64.dq, c.rw.dq, dt, "fa.dq.pad", mag=c.mdq)
            check_banded(as4(k.grad), c.r64.dk, c.rw.dk, dt, "fa.dk.pad", mag=c.mdk)
            check_banded(as4(v.grad), c.r64.dv, c.rw.dv, dt, "fa.dv.pad")
