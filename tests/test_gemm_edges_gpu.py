"""Element-wise fp64 tests of the training GEMMs: ``csrc/gemm/gemm8.hip`` (epilogues 0-3),
``gemm8w.hip`` with ``splitk_sum``, and the tile GEMM ``gemm.hip`` (GPU only; the references, the value
generators, the case table and the rule's teeth are tested on the CPU in ``test_gemm_edges_rule.py``).

The rule is ``check`` of ``test_kernel_edges_gpu.py``: for every element
``|got - ref64| <= k*E32 + u*|ref64| + tiny`` with ``E32 = max(max|ref32 - ref64|, 2^-23 max|ref64|)``,
``u`` one ulp of the output type (0 for fp32 outputs) and ``k = 4``.

References. Plain products (gemm8 epi 0, gemm8w, gemm): the bf16 operands in fp64 and in fp32, multiplied.
Epilogues: the kernel rounds its accumulators to bf16 before epi 1, 2 and 3 do their arithmetic, so the
epilogue references start from the kernel's own rounded product, which is checked against fp64 on the same
shape: epi 1's ``h`` from the stored ``y``; epi 2's ``da|db`` from ``dh = gemm8(epi 0, same fn)`` and the
given ``y``; epi 3 from ``plain = gemm8(epi 0)`` rotated with the fp32 tables, the columns past ``rope_cols``
bit for bit. That rests on every epilogue instantiation leaving the accumulator bits of epi 0 for the same
operands and tile width; ``test_swiglu_epilogues`` asserts it where it can be seen (epi 1's stored ``y``
equals the epi 0 output bit for bit). ``EITHER_NEIGHBOUR`` lists the epilogues for which that did not hold
and an element may instead meet the rule against the reference built from the other bf16 neighbour of the
fp64 product (only where that product lies within 4 E32 of the midpoint of the two): it is empty.

Exact cases: operands drawn from small integers make every sum exact, so placement (row, column, k-chunk,
split range) is tested with ``torch.equal`` and no tolerance.

Measured ``max (|got - ref64| - u*|ref64|) / E32`` per (op, output dtype) on an MI355X (137 test cases; the
whole file takes 5 s). No case needs more than k = 4, so ``GEMM_K_CASE`` is empty, and no element needed the
other neighbour. A 0 in the bf16 column means the error stayed within ``u*|ref64|``, the one rounding to the
output type; ``-`` means no such case. Suffixes: tiles = the tile, tail and k-tile grids, views = strided
operands in NaN buffers, swiglu / rope = the epilogue cases and their epi 0 products, saturated = the
saturation grids (held per magnitude of b; the one figure measured column by column is in
``test_swiglu_saturation``), grid / empty / splitk_sum = the gemm8w table, its empty splits and the slab sum,
splitk = the tile GEMM's split-K:

    op (suffix: the test group)   fp32     bf16
    -------------------------------------------
    gemm.c.splitk                0.267        -
    gemm.c.tiles                 1.046    0.079
    gemm8.c.rope                     -    0.067
    gemm8.c.saturated                -    0.000
    gemm8.c.swiglu                   -    0.063
    gemm8.c.tiles                    -    0.123
    gemm8.c.views                    -    0.028
    gemm8.da.saturated               -    0.000
    gemm8.da.swiglu                  -    0.000
    gemm8.db.saturated               -    0.000
    gemm8.db.swiglu                  -    0.000
    gemm8.h.saturated                -    0.000
    gemm8.h.swiglu                   -    0.000
    gemm8.rope                       -    0.000
    gemm8.y.swiglu                   -    0.104
    gemm8w.dw.empty              0.604        -
    gemm8w.dw.grid               0.847        -
    gemm8w.dw.splitk_sum         0.631        -
    gemm8w.dw.views              1.028        -
"""

import pytest
import torch

from .test_kernel_edges_gpu import BF16, DEV, F32, K_CASE, _RATIOS, _name, _ratio_report, check  # noqa: F401

pytestmark = pytest.mark.gpu

F64 = torch.float64
BK = 64  # k-tile of all three kernels
BN_OF = {4: 256, 5: 320}

# margins above 4 per op, by the rule at test_kernel_edges_gpu.K_CASE: the next power of two above twice the
# measured ratio, never above 32, each with its reason; a ratio above 32 is a finding about the kernel
GEMM_K_CASE: dict = {}
# epilogue ops (prefixes) for which the either-neighbour fallback of the module docstring is on
EITHER_NEIGHBOUR: tuple = ()


def gcheck(got, ref64, ref32, out_dtype, op):
    r = check(got, ref64, ref32, out_dtype, op, GEMM_K_CASE.get(op))
    print(f"  {op} [{_name(out_dtype)}] {tuple(got.shape)}: ratio {r:.3f}")
    return r


# ------------------------------------------------------------------------------------ helpers (CPU-testable)
def pick_fn(N, epi=0, half=0):
    """gemm8.hip's ``pick_fn``: the tile width (in units of 64 columns) of an automatic launch."""
    if epi == 1:
        return 5 if half % 160 == 0 else 4 if half % 128 == 0 else 0
    if N % 320 == 0:
        return 5
    if N % 256 == 0:
        return 4
    if epi == 0 and N % 8 == 0 and N > 0:
        p5, p4 = (N + 319) // 320 * 320, (N + 255) // 256 * 256
        return 4 if p4 < p5 else 5
    return 0


def _g(device, *shape_and_seed):
    seed = 0
    for v in shape_and_seed:
        seed = (seed * 1000003 + int(v) + 1) % (2**31 - 1)
    return torch.Generator(device=device).manual_seed(seed)


def randn_bf16(rows, cols, scale=1.0, seed=0, device=DEV):
    """bf16 operand from randn with a generator seeded from the shape."""
    return (torch.randn(rows, cols, device=device, generator=_g(device, rows, cols, seed)) * scale).to(BF16)


def int_bf16(rows, cols, amax, seed=0, device=DEV):
    """bf16 operand of integers in [-amax, amax]: K products sum exactly while K*amax^2 stays in range."""
    return torch.randint(-amax, amax + 1, (rows, cols), device=device, generator=_g(device, rows, cols, seed, amax)).to(BF16)


def plain_refs(a, b):
    """(ref64, ref32) of a @ b.T for row-major (M, K), (N, K) operands."""
    assert not torch.backends.cuda.matmul.allow_tf32
    return a.double() @ b.double().t(), a.float() @ b.float().t()


def dw_refs(a, b, k0=0, k1=None):
    """(ref64, ref32) of gemm8w's a.T @ b over token rows [k0, k1) of the (K, M), (K, N) operands."""
    assert not torch.backends.cuda.matmul.allow_tf32
    a, b = a[k0:k1], b[k0:k1]
    return a.double().t() @ b.double(), a.float().t() @ b.float()


def swiglu_fwd_ref(y, half, ft):
    """h = silu(a) * b from y = [a|b], evaluated in ``ft``."""
    a, b = y[:, :half].to(ft), y[:, half:].to(ft)
    return a * torch.sigmoid(a) * b


def swiglu_bwd_ref(dh, y, half, ft):
    """(da, db) of h = silu(a) * b for the upstream dh, from y = [a|b], evaluated in ``ft``."""
    a, b, g = y[:, :half].to(ft), y[:, half:].to(ft), dh.to(ft)
    s = torch.sigmoid(a)
    return g * b * s * (1 + a * (1 - s)), g * a * s


def rope_tables(ctx, dk, device=DEV, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, dk, 2, device=device, dtype=F64) / dk))
    ang = torch.arange(ctx, device=device, dtype=F64)[:, None] * inv[None, :]
    return torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()


def rope_rotate_ref(plain, cos, sin, pos, rope_cols, dk, ft):
    """Interleaved-pair rotation of the columns < rope_cols of plain (M, N) with the fp32 tables, in ``ft``;
    the other columns pass through. Column c of a rotated head is pair (c % dk) // 2, slot c % 2."""
    y = plain.to(ft).clone()
    M = y.shape[0]
    qk = y[:, :rope_cols].reshape(M, -1, dk // 2, 2)
    c, s = cos[pos].to(ft)[:, None, :], sin[pos].to(ft)[:, None, :]
    x0, x1 = qk[..., 0], qk[..., 1]
    y[:, :rope_cols] = torch.stack((c * x0 - s * x1, s * x0 + c * x1), -1).reshape(M, rope_cols)
    return y


def split_ranges(K, splits):
    """Token ranges [k0, k1) of gemm8w's splits: k-tiles [nkt*s/S, nkt*(s+1)/S) of 64 tokens each."""
    nkt = K // BK
    return [(nkt * s // splits * BK, nkt * (s + 1) // splits * BK) for s in range(splits)]


def _bf16_step(x, up):
    """The next bf16 above (up) or below x."""
    bits = x.view(torch.int16).to(torch.int32) & 0xFFFF
    neg = bits >= 0x8000
    mag = bits & 0x7FFF
    away = neg != up  # moving away from zero
    mag2 = torch.where(away, mag + 1, mag - 1)
    flip = (mag == 0) & ~away  # crossing zero: the smallest value of the other sign
    sign = torch.where(flip, ~neg, neg)
    mag2 = torch.where(flip, torch.ones_like(mag), mag2)
    out = (mag2 | (sign.to(torch.int32) << 15))
    out = torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)
    return out.view(BF16)


def bf16_neighbours(p64):
    """(lo, hi): the bf16 values that bracket p64 (equal where p64 is a bf16 value)."""
    n = p64.float().to(BF16)
    nd = n.double()
    lo = torch.where(nd <= p64, n, _bf16_step(n, False))
    hi = torch.where(nd >= p64, n, _bf16_step(n, True))
    return lo, hi


def other_neighbour(rounded, p64, e32):
    """For the kernel's bf16 product ``rounded`` of the fp64 product p64 (E32 of that product: e32): the other
    bf16 neighbour of p64, and where it may stand in -- p64 within 4*e32 of the midpoint of the two."""
    lo, hi = bf16_neighbours(p64)
    other = torch.where(rounded == lo, hi, lo)
    mid = (lo.double() + hi.double()) / 2
    allowed = ((p64 - mid).abs() <= 4 * e32) & (lo != hi)
    return other, allowed


def pair_alternates(plain, other, allowed, rotate):
    """The alternates of an output that depends on a pair of adjacent columns (the rotation): the pair's
    first, second or both inputs replaced by their other neighbour, allowed where every replaced input is."""
    M, N = plain.shape
    even = torch.arange(N, device=plain.device) % 2 == 0
    alts = []
    for slots in (even, ~even, torch.ones_like(even)):
        sel = slots[None, :].expand(M, N)
        mixed = torch.where(sel, other, plain)
        ok = (allowed | ~sel).reshape(M, N // 2, 2).all(-1, keepdim=True).expand(M, N // 2, 2).reshape(M, N)
        alts.append((rotate(mixed, F64), rotate(mixed, F32), ok))
    return alts


def check_either(got, primary, alternates, out_dtype, op, k=None):
    """``check`` against (ref64, ref32) = primary, where each element may instead take the references of one
    of ``alternates`` [(ref64, ref32, allowed)] if that one is allowed there and closer. Returns the ratio and
    the number of elements that took an alternate."""
    r64, r32 = primary[0].clone(), primary[1].clone()
    best = (got.double() - r64).abs()
    used = torch.zeros_like(best, dtype=torch.bool)
    for a64, a32, allowed in alternates:
        err = (got.double() - a64).abs()
        take = allowed & (err < best)
        r64, r32, best = torch.where(take, a64, r64), torch.where(take, a32, r32), torch.where(take, err, best)
        used |= take
    return check(got, r64, r32, out_dtype, op, k), int(used.sum())


# (fn, N) of the epi 0 grid: full tiles BN and 2 BN, the tails 8, BN - 8, BN + 8, 2 BN + 8 for the forced
# widths; for fn 0 an N that picks each width outright, 328 (pads to 512 against 640: 256 wins), 1032 (pads to
# 1280 either way: the tie goes to 320) and 8
PLAIN_GRID = ([(fn, n) for fn, bn in BN_OF.items() for n in (bn, 2 * bn, 8, bn - 8, bn + 8, 2 * bn + 8)]
              + [(0, n) for n in (256, 320, 640, 328, 1032, 8)])
PLAIN_K = (8, 56, 64, 72, 128, 136, 192, 200)  # 1, 2, 3 full k-tiles with and without a partial last one, and a lone partial
PLAIN_INT = 1  # integer operands of the exact bf16-out cases: |sum| <= K <= 256

# gemm8w cases (K tokens, M, N, fn, trans_out, splits). Among the rows the launcher accepts, every K, M and
# (N, fn) meets both trans_out and all three splits (asserted in test_gemm_edges_rule.py). 640 forced to 256-wide
# tiles is refused whatever the other arguments: two rows pin that, and the 256-wide kernel runs on N = 256
DW_CASES = [
    (64, 8, 256, 0, False, 1),     # one k-tile, an 8-row sliver of a row tile, BN 256
    (128, 248, 320, 0, True, 1),   # rows 248..255 padded, transposed store, BN 320
    (192, 256, 640, 4, False, 1),  # forced 256 does not divide 640: refused (dw_refused)
    (192, 256, 256, 0, False, 1),  # exact row tile, 3 k-tiles
    (320, 264, 640, 5, True, 1),   # second row tile of 8 rows, 5 k-tiles, forced 320
    (64, 520, 640, 0, True, 1),    # three row tiles, automatic width (320)
    (128, 8, 640, 4, True, 2),     # refused, transposed and split
    (64, 248, 256, 0, False, 2),   # 2 splits of 1 k-tile: split 0 is empty, padded rows
    (128, 256, 640, 5, True, 2),   # one k-tile per split
    (192, 264, 640, 0, False, 2),  # uneven: 1 and 2 k-tiles
    (320, 520, 256, 0, True, 2),   # uneven: 2 and 3 k-tiles, three row tiles
    (320, 8, 320, 0, False, 2),    # uneven, sliver
    (192, 248, 640, 5, True, 2),   # uneven, padded rows, transposed
    (64, 256, 640, 0, True, 3),    # 3 splits of 1 k-tile: two are empty
    (128, 264, 256, 0, False, 3),  # 3 splits of 2 k-tiles: split 0 is empty
    (192, 520, 320, 0, True, 3),   # one k-tile per split
    (320, 8, 640, 0, True, 3),     # uneven: 1, 2, 2 k-tiles, sliver, transposed
    (320, 248, 640, 5, False, 3),  # uneven, padded rows
    (128, 520, 320, 0, False, 3),  # split 0 is empty, three row tiles with a padded third, plain store
    (192, 256, 320, 0, False, 3),  # one k-tile per split, plain store
    (64, 264, 640, 5, True, 3),    # two empty splits, transposed
]


def dw_refused(N, fn):
    """launch_w: a forced tile width must divide N (gemm8w has no N tail), so 640 forced to 256 is refused."""
    return fn != 0 and N % (64 * fn) != 0


DW_INT = 4  # integer operands of the exact fp32-out cases: |sum| <= 16 K < 2^24

TILES = [(256, 160), (160, 256), (192, 160), (160, 160)]
ORIENTATIONS = [(False, True), (False, False), (True, False)]  # X.W^T, dY.W, dY^T.X


def tile_operands(M, N, K, ta, tb, make):
    return make(*((K, M) if ta else (M, K)), 1), make(*((N, K) if tb else (K, N)), 2)


def tile_refs(a, b, ta, tb):
    assert not torch.backends.cuda.matmul.allow_tf32
    f = lambda x, t: x.t() if t else x  # noqa: E731
    return f(a.double(), ta) @ f(b.double(), tb), f(a.float(), ta) @ f(b.float(), tb)


# ------------------------------------------------------------------------------------ GPU plumbing
def _cs():
    from cs336_systems import ops

    assert ops.load_ext(), ops.load_error()
    return torch.ops.cs336


def _nan(*shape, dtype=BF16):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _framed(rows, cols, ld, dtype=BF16, fill=None):
    """A (rows, cols) view with row stride ld inside a NaN (or ``fill``) buffer with a guard row on each side
    and 8 guard columns to the left; returns (buffer, view)."""
    assert ld >= cols + 8 and ld % 8 == 0
    buf = _nan(rows + 2, ld, dtype=dtype) if fill is None else fill(rows + 2, ld)
    return buf, buf[1 : rows + 1, 8 : 8 + cols]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _unchanged_around(buf, before_bits, rows, cols):
    after = _bits(buf).clone()
    after[1 : rows + 1, 8 : 8 + cols] = before_bits[1 : rows + 1, 8 : 8 + cols]
    return torch.equal(after, before_bits)


def _gemm8(a, b, fn, c=None):
    c = torch.empty(a.shape[0], b.shape[0], device=DEV, dtype=BF16) if c is None else c
    _cs().gemm8(a, b, c, 0, fn, None, None, 0)
    return c


# ------------------------------------------------------------------------------------ gemm8 epi 0
def test_pick_fn_grid():
    """By the Python copy of gemm8.hip's pick_fn above, the fn 0 rows of the grid hold an N for each outcome of
    its tail rule and for both full widths, and the host gate takes them. No binding reports the width a launch
    chose, and both widths leave the same bits, so the kernel's own choice (ties go to 320) is not pinned here."""
    ns = [n for fn, n in PLAIN_GRID if fn == 0]
    assert 328 in ns and pick_fn(328) == 4 and (328 + 255) // 256 * 256 < (328 + 319) // 320 * 320
    assert 1032 in ns and pick_fn(1032) == 5 and (1032 + 255) // 256 * 256 == (1032 + 319) // 320 * 320
    assert pick_fn(256) == 4 and pick_fn(320) == 5 and pick_fn(640) == 5 and pick_fn(8) == 4
    cs = _cs()
    for n in ns:
        assert cs.gemm8_ok(256, n, 64, 0, 0)


@pytest.mark.parametrize("fn,N", PLAIN_GRID)
def test_plain_tiles_and_tails(fn, N):
    """Full tiles, the smallest and the off-by-8 N tails, and every branch of the k pipeline's look-ahead
    (1, 2, 3 k-tiles, each with and without a partial last one; K = 8 is a lone partial tile)."""
    for M in (256, 512):
        for K in PLAIN_K:
            a, b = randn_bf16(M, K, seed=1), randn_bf16(N, K, seed=2)
            c = _gemm8(a, b, fn)
            gcheck(c, *plain_refs(a, b), BF16, "gemm8.c.tiles")
            if fn == 0:  # an automatic launch gives the bits of a forced one (this does not show which width it took)
                assert torch.equal(c, _gemm8(a, b, pick_fn(N)))


@pytest.mark.parametrize("fn,N", PLAIN_GRID)
def test_plain_exact_integers(fn, N):
    """Operands in {-1, 0, 1}: every sum is an integer of magnitude <= K <= 256, exact in bf16, so an element
    taken from a neighbouring row, column or k-chunk is wrong by an integer."""
    M = 512
    for K in PLAIN_K:
        a, b = int_bf16(M, K, PLAIN_INT, seed=1), int_bf16(N, K, PLAIN_INT, seed=2)
        c = _gemm8(a, b, fn)
        assert torch.equal(c.float(), a.float() @ b.float().t()), (fn, N, K)


@pytest.mark.parametrize("fn", [4, 5])
def test_plain_views_and_poison(fn):
    """a and b are views with row strides wider than K inside NaN buffers, c a column slice of a NaN buffer: a
    row, a k-chunk or a B row outside the operands that reached a stored value, or a store outside c, shows."""
    bn = BN_OF[fn]
    for M, N, K in ((512, 2 * bn, 192), (512, bn + 8, 72), (256, 8, 8)):
        a, b = randn_bf16(M, K, seed=3), randn_bf16(N, K, seed=4)
        _, av = _framed(M, K, K + 16)
        _, bv = _framed(N, K, K + 40)
        av.copy_(a)
        bv.copy_(b)
        cbuf, cv = _framed(M, N, N + 24)
        before = _bits(cbuf).clone()
        _gemm8(av, bv, fn, cv)
        assert torch.isfinite(cv).all()
        assert torch.equal(cv, _gemm8(a, b, fn))
        gcheck(cv, *plain_refs(a, b), BF16, "gemm8.c.views")
        assert _unchanged_around(cbuf, before, M, N)


# ------------------------------------------------------------------------------------ gemm8 epi 1 / 2
def _epi_check(got, primary, alternates, op):
    """An epilogue output against the references built from the kernel's own rounded product; the other
    bf16 neighbour of the fp64 product stands in only for ops listed in EITHER_NEIGHBOUR."""
    if op.startswith(EITHER_NEIGHBOUR):
        r, n = check_either(got, primary, alternates(), BF16, op, GEMM_K_CASE.get(op))
        print(f"  {op} [bfloat16] {tuple(got.shape)}: ratio {r:.3f} ({n} elements by the other neighbour)")
        return r
    return gcheck(got, *primary, BF16, op)


def _run_epi1(x, w13, half, fn, y=None, h=None):
    M = x.shape[0]
    y = torch.empty(M, 2 * half, device=DEV, dtype=BF16) if y is None else y
    h = torch.empty(M, half, device=DEV, dtype=BF16) if h is None else h
    _cs().gemm8(x, w13, y, 1, fn, h, None, half)
    return y, h


def _run_epi2(dy, w2t, y, half, fn, c=None):
    c = torch.empty(dy.shape[0], 2 * half, device=DEV, dtype=BF16) if c is None else c
    _cs().gemm8(dy, w2t, c, 2, fn, None, y, half)
    return c


def _epi2_check(dy, w2t, y, dab, half, fn, tag):
    """dh = gemm8(epi 0, same fn) against fp64, then da|db against the SwiGLU backward of that dh."""
    dh = _gemm8(dy, w2t, fn)
    p64, p32 = plain_refs(dy, w2t)
    gcheck(dh, p64, p32, BF16, f"gemm8.c{tag}")
    r64, r32 = swiglu_bwd_ref(dh, y, half, F64), swiglu_bwd_ref(dh, y, half, F32)

    def alternates(i):
        def make():
            e32 = max((p32.double() - p64).abs().max().item(), 2.0**-23 * p64.abs().max().item())
            other, allowed = other_neighbour(dh, p64, e32)
            return [(swiglu_bwd_ref(other, y, half, F64)[i], swiglu_bwd_ref(other, y, half, F32)[i], allowed)]
        return make

    _epi_check(dab[:, :half], (r64[0], r32[0]), alternates(0), f"gemm8.da{tag}")
    _epi_check(dab[:, half:], (r64[1], r32[1]), alternates(1), f"gemm8.db{tag}")


@pytest.mark.parametrize("half,fn", [(256, 4), (320, 5), (640, 4), (640, 5)])
@pytest.mark.parametrize("K", [64, 192])
def test_swiglu_epilogues(half, fn, K):
    """epi 1 (y, h) and epi 2 (da|db) contiguous, then with every epilogue stream a column slice of a wider NaN
    buffer with its own row stride (two row tiles, so m0 * ld differs from m0 * width for each of c, h and y):
    bit-equal results and untouched bytes around c and h."""
    M = 512
    # epi 1
    x, w13 = randn_bf16(M, K, seed=5), randn_bf16(2 * half, K, 0.1, seed=6)
    y, h = _run_epi1(x, w13, half, fn)
    gcheck(y, *plain_refs(x, w13), BF16, "gemm8.y.swiglu")
    gcheck(h, swiglu_fwd_ref(y, half, F64), swiglu_fwd_ref(y, half, F32), BF16, "gemm8.h.swiglu")
    # the k-loop is one template and an element's accumulator depends on its k order only, not on the tile
    # column epi 1 computes it in: epi 1 stores the bits of epi 0
    assert torch.equal(y, _gemm8(x, w13, fn))
    ybuf, yv = _framed(M, 2 * half, 2 * half + 24)
    hbuf, hv = _framed(M, half, half + 40)
    yb0, hb0 = _bits(ybuf).clone(), _bits(hbuf).clone()
    _run_epi1(x, w13, half, fn, yv, hv)
    assert torch.equal(yv, y) and torch.equal(hv, h)
    assert _unchanged_around(ybuf, yb0, M, 2 * half) and _unchanged_around(hbuf, hb0, M, half)
    # epi 2
    dy, w2t = randn_bf16(M, K, seed=7), randn_bf16(half, K, 0.1, seed=8)
    yin = randn_bf16(M, 2 * half, seed=9)
    if half % (64 * fn):  # launch(): an epilogue takes no N tail, so half 640 cannot be forced to 256-wide tiles
        with pytest.raises(RuntimeError, match="gemm8 launch"):
            _run_epi2(dy, w2t, yin, half, fn)
        return
    dab = _run_epi2(dy, w2t, yin, half, fn)
    _epi2_check(dy, w2t, yin, dab, half, fn, ".swiglu")
    cbuf, cv = _framed(M, 2 * half, 2 * half + 24)
    _, yinv = _framed(M, 2 * half, 2 * half + 8)
    yinv.copy_(yin)
    cb0 = _bits(cbuf).clone()
    _run_epi2(dy, w2t, yinv, half, fn, cv)
    assert torch.equal(cv, dab)
    assert _unchanged_around(cbuf, cb0, M, 2 * half)


SAT_A = [-200.0, -89.0, -88.0, -20.0, -1e-3, 0.0, 1e-3, 20.0, 88.0, 200.0]
SAT_B = [1.0, -1.0, 1e3, -1e3]


@pytest.mark.parametrize("half,fn", [(256, 4), (320, 5)])
def test_swiglu_saturation(half, fn):
    """sigmoid is 1 / (1 + __expf(-a)), which overflows to inf below a = -88: nothing may be NaN and the rule
    holds. epi 2: the (a, b) grid of test_silu_mul_saturation in the first columns of y, held as one tensor per
    magnitude of b. epi 1: exact products a in {-256, -128, 0, 128, 256}, b in {+-1, +-1024} from constant
    operand rows, held per (a, b)."""
    M, K = 256, 64
    # epi 2
    grid = torch.cartesian_prod(torch.tensor(SAT_A, device=DEV), torch.tensor(SAT_B, device=DEV)).to(BF16)
    dy, w2t = randn_bf16(M, K, seed=10), randn_bf16(half, K, 0.1, seed=11)
    dh = _gemm8(dy, w2t, fn)
    yin = randn_bf16(M, 2 * half, seed=12)
    ng = grid.shape[0]
    yin[:, :ng] = grid[:, 0]
    yin[:, half : half + ng] = grid[:, 1]
    r64, r32 = swiglu_bwd_ref(dh, yin, half, F64), swiglu_bwd_ref(dh, yin, half, F32)
    keep = [j for j in range(ng) if all(r[:, j].abs().max() < 0.9 * torch.finfo(BF16).max for r in r64)]
    assert len(keep) == 40  # everything fits bf16: |da| <= 1e3 |dh|, |db| <= 200 |dh|
    dab = _run_epi2(dy, w2t, yin, half, fn)
    assert not torch.isnan(dab).any()
    # the grid as one tensor per magnitude of b, as test_silu_mul_saturation holds its grid (one E32 per tensor).
    # Held column by column, one column of da measured a ratio of 86.8: the kernel stored 0 where fp64 has 1e-36,
    # against a column E32 of 1e-43. Presumably that column is a = -88, b = +-1 (the magnitude fits, and at
    # a = -89 the fp32 reference underflows too): sigmoid(-88) = 6e-39 is an fp32 subnormal, and sigmoid_f's
    # hardware reciprocal (v_rcp_f32) presumably returns 0 for it; the run did not record the column. If so the
    # absolute error is below 88 * 2^-126 * |dh b|.
    for cols in ([j for j in keep if j % 4 < 2], [j for j in keep if j % 4 >= 2]):  # b = +-1, b = +-1e3
        assert len(cols) == 20 and len({float(yin[0, half + j].abs()) for j in cols}) == 1
        gcheck(dab[:, cols], r64[0][:, cols], r32[0][:, cols], BF16, "gemm8.da.saturated")
        gcheck(dab[:, [half + j for j in cols]], r64[1][:, cols], r32[1][:, cols], BF16, "gemm8.db.saturated")
    _epi2_check(dy, w2t, yin, dab, half, fn, ".saturated")
    # epi 1
    av, bv = [-2.0, -1.0, 0.0, 1.0, 2.0], [2.0**-7, -(2.0**-7), 8.0, -8.0]
    x = torch.full((M, K), 2.0, device=DEV, dtype=BF16)
    cols = torch.arange(half, device=DEV)
    w1 = torch.tensor(av, device=DEV)[cols % 5]
    w3 = torch.tensor(bv, device=DEV)[(cols // 5) % 4]
    w13 = torch.cat((w1, w3))[:, None].expand(2 * half, K).to(BF16).contiguous()
    y, h = _run_epi1(x, w13, half, fn)
    assert torch.equal(y.float(), x.float() @ w13.float().t())  # a = 128 w1, b = 128 w3, exact
    assert not torch.isnan(h).any()
    h64, h32 = swiglu_fwd_ref(y, half, F64), swiglu_fwd_ref(y, half, F32)
    kept = [j for j in range(20) if h64[:, j].abs().max() < 0.9 * torch.finfo(BF16).max]
    assert len(kept) == 20  # |h| <= 256 * 1024
    for j in kept:  # columns j, j + 20, ... share one (a, b)
        check(h[:, j::20], h64[:, j::20], h32[:, j::20], BF16, "gemm8.h.saturated", GEMM_K_CASE.get("gemm8.h.saturated"))
    print(f"  saturation ratios: { {k: round(v, 3) for k, v in _RATIOS.items() if 'saturated' in k[0]} }")


# ------------------------------------------------------------------------------------ gemm8 epi 3
@pytest.mark.parametrize("B,N,H,dk,K", [(1, 256, 5, 64, 64), (2, 256, 4, 80, 128), (2, 128, 10, 96, 72)])
@pytest.mark.parametrize("given_pos", [False, True])
def test_rope_store(B, N, H, dk, K, given_pos):
    """RoPE in the store: two rotated column tiles and one unrotated (3 H dk = 960 = 3 x 320, rope_cols 640),
    against the rotation of gemm8's own epi 0 output; K = 72 is refused (epi 3 has no k tail)."""
    cs = _cs()
    M, Nout, rope_cols = B * N, 3 * H * dk, 2 * H * dk
    x, w = randn_bf16(M, K, seed=13), randn_bf16(Nout, K, 0.1, seed=14)
    ctx = N + 44
    cos, sin = rope_tables(ctx, dk)
    if given_pos:
        pos = torch.randint(0, ctx, (M,), device=DEV, dtype=torch.int64, generator=_g(DEV, M, ctx))
        pos[3], pos[M - 2] = 0, ctx - 1
    else:
        pos = torch.arange(N, device=DEV, dtype=torch.int64).repeat(B)
    out = _nan(M, Nout)
    run = lambda: cs.gemm8_rope(x, w, out, cos, sin, pos if given_pos else None, N, rope_cols, dk)  # noqa: E731
    if K % 64:
        assert not cs.gemm8_ok(M, Nout, K, 3, rope_cols)
        with pytest.raises(RuntimeError, match="gemm8_rope does not take"):
            run()
        return
    assert Nout // 320 == 3 and rope_cols // 320 == 2 and pick_fn(Nout) == 5
    run()
    plain = _gemm8(x, w, 0)
    p64, p32 = plain_refs(x, w)
    gcheck(plain, p64, p32, BF16, "gemm8.c.rope")
    r64 = rope_rotate_ref(plain, cos, sin, pos, rope_cols, dk, F64)
    r32 = rope_rotate_ref(plain, cos, sin, pos, rope_cols, dk, F32)

    def alternates():
        e32 = max((p32.double() - p64).abs().max().item(), 2.0**-23 * p64.abs().max().item())
        other, allowed = other_neighbour(plain, p64, e32)
        alts = pair_alternates(plain, other, allowed, lambda t, ft: rope_rotate_ref(t, cos, sin, pos, rope_cols, dk, ft))
        return [(a[:, :rope_cols], b[:, :rope_cols], c[:, :rope_cols]) for a, b, c in alts]

    _epi_check(out[:, :rope_cols], (r64[:, :rope_cols], r32[:, :rope_cols]), alternates, "gemm8.rope")
    assert torch.equal(out[:, rope_cols:], plain[:, rope_cols:])  # v: bit for bit


# ------------------------------------------------------------------------------------ gemm8 rejections
def test_rejections():
    cs = _cs()

    def refused(M, N, K, epi, half, fn=0):
        assert not cs.gemm8_ok(M, N, K, epi, half), (M, N, K, epi, half)
        a, b = torch.zeros(M, K, device=DEV, dtype=BF16), torch.zeros(N, K, device=DEV, dtype=BF16)
        c = torch.zeros(M, 2 * half if epi == 2 else N, device=DEV, dtype=BF16)
        h = torch.zeros(M, half, device=DEV, dtype=BF16) if epi == 1 else None
        y = torch.zeros(M, 2 * half, device=DEV, dtype=BF16) if epi == 2 else None
        with pytest.raises(RuntimeError):
            cs.gemm8(a, b, c, epi, fn, h, y, half)

    refused(128, 256, 64, 0, 0)      # M % 256
    refused(264, 256, 64, 0, 0)
    refused(256, 384, 64, 1, 192)    # epi 1: half is a multiple of neither 128 nor 160
    refused(256, 512, 72, 1, 256)    # epi 1 and 2 have no k tail
    refused(256, 256, 72, 2, 256)
    refused(256, 12, 64, 0, 0)       # epi 0: N % 8
    refused(256, 256, 12, 0, 0)      # epi 0: K % 8
    a, b = torch.zeros(256, 64, device=DEV, dtype=BF16), torch.zeros(256, 64, device=DEV, dtype=BF16)
    c = torch.zeros(256, 256, device=DEV, dtype=BF16)
    assert cs.gemm8_ok(256, 256, 64, 0, 0)
    cs.gemm8(a, b, c, 0, 0, None, None, 0)  # the accepted form of the next four
    wide = torch.zeros(256, 68, device=DEV, dtype=BF16)
    flat = torch.zeros(256 * 64 + 8, device=DEV, dtype=BF16)
    off = flat[4 : 4 + 256 * 64].view(256, 64)
    assert wide[:, :64].stride(0) % 8 == 4 and off.data_ptr() % 16 == 8
    for bad_a, bad_b in ((wide[:, :64], b), (a, wide[:, :64]), (off, b), (a, off)):
        with pytest.raises(RuntimeError, match="16-B aligned"):
            cs.gemm8(bad_a, bad_b, c, 0, 0, None, None, 0)
    cw = torch.zeros(256, 260, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        cs.gemm8(a, b, cw[:, :256], 0, 0, None, None, 0)
    with pytest.raises(RuntimeError, match="gemm8 launch"):  # a forced width must divide an epilogue's N
        cs.gemm8(a, torch.zeros(640, 64, device=DEV, dtype=BF16), torch.zeros(256, 1280, device=DEV, dtype=BF16), 2, 4,
                 None, torch.zeros(256, 1280, device=DEV, dtype=BF16), 640)


# ------------------------------------------------------------------------------------ gemm8w
def _run_dw(a, b, fn, trans, splits, out=None, accumulate=False):
    M, N = a.shape[1], b.shape[1]
    shape = (N, M) if trans else (M, N)
    if out is None:
        out = _nan(*(((splits,) if splits > 1 else ()) + shape), dtype=F32)
    _cs().gemm8w(a, b, out, splits, trans, accumulate, fn)
    return out


def _slabs(out, trans, splits):
    """(splits, M, N) view of gemm8w's output, whatever its orientation."""
    s = out if splits > 1 else out[None]
    return s.transpose(1, 2) if trans else s


@pytest.mark.parametrize("K,M,N,fn,trans,splits", DW_CASES)
def test_dw_grid(K, M, N, fn, trans, splits):
    """The product through check; split slabs summed by splitk_sum and by .sum(0), splitk_sum against the fp64
    sum of the slabs."""
    cs = _cs()
    a, b = randn_bf16(K, M, seed=15), randn_bf16(K, N, seed=16)
    if dw_refused(N, fn):
        with pytest.raises(RuntimeError, match="gemm8w does not take"):
            _run_dw(a, b, fn, trans, splits)
        return
    out = _run_dw(a, b, fn, trans, splits)
    assert torch.isfinite(out).all()
    r64, r32 = dw_refs(a, b)
    if splits == 1:
        gcheck(_slabs(out, trans, 1)[0], r64, r32, F32, "gemm8w.dw.grid")
        return
    total = _nan(*out.shape[1:], dtype=F32)
    cs.splitk_sum(out, total, False)
    gcheck(total, out.double().sum(0), out.sum(0), F32, "gemm8w.dw.splitk_sum")
    for got in (total, out.sum(0)):
        gcheck(got.t() if trans else got, r64, r32, F32, "gemm8w.dw.grid")


@pytest.mark.parametrize("K,M,N,fn,trans,splits", [c for c in DW_CASES if not dw_refused(c[2], c[3])])
def test_dw_exact_integers(K, M, N, fn, trans, splits):
    """Operands in {-4 .. 4}, fp32 out: every slab equals the fp32 product over exactly its own token range."""
    a, b = int_bf16(K, M, DW_INT, seed=17), int_bf16(K, N, DW_INT, seed=18)
    slabs = _slabs(_run_dw(a, b, fn, trans, splits), trans, splits)
    for s, (k0, k1) in enumerate(split_ranges(K, splits)):
        assert torch.equal(slabs[s], dw_refs(a, b, k0, k1)[1]), (s, k0, k1)
    assert torch.equal(slabs.sum(0), dw_refs(a, b)[1])


@pytest.mark.parametrize("splits", [3, 5])
@pytest.mark.parametrize("M,N,trans", [(264, 320, False), (264, 256, True), (8, 640, True)])
def test_dw_empty_split(splits, M, N, trans):
    """More splits than k-tiles (K = 128: two k-tiles). launch_w takes up to 64 splits and the binding only
    bounds the longest split, so the launch is accepted: a split with no k-tile writes a slab of zeros over
    the NaN that was there, the other slabs hold their own k-tile, and the slabs sum to the product."""
    K = 128
    ranges = split_ranges(K, splits)
    assert ranges == ([(0, 0), (0, 64), (64, 128)] if splits == 3 else [(0, 0), (0, 0), (0, 64), (64, 64), (64, 128)])
    a, b = int_bf16(K, M, DW_INT, seed=19), int_bf16(K, N, DW_INT, seed=20)
    slabs = _slabs(_run_dw(a, b, 0, trans, splits), trans, splits)
    for s, (k0, k1) in enumerate(ranges):
        if k0 == k1:
            assert torch.all(slabs[s] == 0), s
        else:
            assert torch.equal(slabs[s], dw_refs(a, b, k0, k1)[1]), s
    a, b = randn_bf16(K, M, seed=19), randn_bf16(K, N, seed=20)
    out = _run_dw(a, b, 0, trans, splits)
    total = _nan(*out.shape[1:], dtype=F32)
    _cs().splitk_sum(out, total, False)
    gcheck(total.t() if trans else total, *dw_refs(a, b), F32, "gemm8w.dw.empty")


@pytest.mark.parametrize("M", [264, 8])
@pytest.mark.parametrize("trans", [False, True])
def test_dw_views_poison_accumulate(M, trans):
    """a and b are columns [16, 16 + width) of NaN buffers 48 columns wider, so the row tile's padded rows >= M
    read NaN (or zeros past the operand's end) and must be dropped; out is a row-strided view inside a guard
    buffer holding a known fp32 tensor, accumulated into."""
    cs = _cs()
    K, N = 128, 320
    a, b = randn_bf16(K, M, seed=21), randn_bf16(K, N, seed=22)
    abuf, bbuf = _nan(K, M + 48), _nan(K, N + 48)
    av, bv = abuf[:, 16 : 16 + M], bbuf[:, 16 : 16 + N]
    av.copy_(a)
    bv.copy_(b)
    rows, cols = (N, M) if trans else (M, N)
    guard = torch.randn(rows + 2, cols + 8, device=DEV, generator=_g(DEV, rows, cols))
    before = guard.clone()
    out = guard[1 : rows + 1, 4 : 4 + cols]
    assert out.stride(0) == cols + 8 and out.data_ptr() % 16 == 0
    cs.gemm8w(av, bv, out, 1, trans, True, 0)
    assert torch.isfinite(guard).all()
    delta = out.double() - before[1 : rows + 1, 4 : 4 + cols].double()
    gcheck(delta.t() if trans else delta, *dw_refs(a, b), F32, "gemm8w.dw.views")
    after = guard.clone()
    after[1 : rows + 1, 4 : 4 + cols] = before[1 : rows + 1, 4 : 4 + cols]
    assert torch.equal(_bits(after), _bits(before))  # the guards are untouched
    with pytest.raises(RuntimeError, match="split-K out"):
        cs.gemm8w(av, bv, torch.zeros(2, rows, cols, device=DEV), 2, trans, True, 0)


# ------------------------------------------------------------------------------------ gemm.hip
@pytest.mark.parametrize("ta,tb", ORIENTATIONS)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("out_dtype", [BF16, F32], ids=_name)
def test_tile_gemm_elementwise(ta, tb, tile, out_dtype):
    cs = _cs()
    bm, bn = tile
    M, N = 2 * bm, 2 * bn
    for K in (64, 320):
        a, b = tile_operands(M, N, K, ta, tb, lambda r, c, s: randn_bf16(r, c, seed=22 + s))
        c = cs.gemm(a, b, ta, tb, out_dtype, bm, bn, 1)
        assert c.shape == (M, N) and c.dtype == out_dtype
        gcheck(c, *tile_refs(a, b, ta, tb), out_dtype, "gemm.c.tiles")
    a, b = tile_operands(M, N, 64, ta, tb, lambda r, c, s: int_bf16(r, c, PLAIN_INT, seed=24 + s))
    c = cs.gemm(a, b, ta, tb, out_dtype, bm, bn, 1)
    assert torch.equal(c.float(), tile_refs(a, b, ta, tb)[1])


@pytest.mark.parametrize("splits", [2, 3, 5])
@pytest.mark.parametrize("accumulate", [False, True])
def test_tile_gemm_splitk_strided(splits, accumulate):
    """Split-K over 23 k-tiles (uneven ranges) into a strided fp32 view, plain and accumulating; the margins
    of the buffer against a clone taken before the call, bit for bit."""
    cs = _cs()
    ta, tb = True, False
    M, N, K = 320, 480, 64 * 23
    a, b = tile_operands(M, N, K, ta, tb, lambda r, c, s: randn_bf16(r, c, seed=26 + s))
    big = torch.randn(M, N + 32, device=DEV, generator=_g(DEV, M, N, splits))
    before = big.clone()
    out = big[:, 16 : 16 + N]
    cs.gemm_out(a, b, ta, tb, out, accumulate, 160, 160, splits)
    got = out.double() - before[:, 16 : 16 + N].double() if accumulate else out
    gcheck(got, *tile_refs(a, b, ta, tb), F32, "gemm.c.splitk")
    assert torch.equal(_bits(big[:, :16]), _bits(before[:, :16])) and torch.equal(_bits(big[:, 16 + N :]), _bits(before[:, 16 + N :]))


# ------------------------------------------------------------------------------------ all three
def test_bitwise_reproducible():
    """Two runs of one case per kernel and epilogue give equal bits."""
    cs = _cs()
    M, K, half = 512, 192, 320
    a, b = randn_bf16(M, K, seed=30), randn_bf16(648, K, seed=31)
    assert torch.equal(_gemm8(a, b, 0), _gemm8(a, b, 0))
    w13, w2t, yin = randn_bf16(2 * half, K, 0.1, seed=32), randn_bf16(half, K, 0.1, seed=33), randn_bf16(M, 2 * half, seed=34)
    (y1, h1), (y2, h2) = _run_epi1(a, w13, half, 0), _run_epi1(a, w13, half, 0)
    assert torch.equal(y1, y2) and torch.equal(h1, h2)
    assert torch.equal(_run_epi2(a, w2t, yin, half, 0), _run_epi2(a, w2t, yin, half, 0))
    cos, sin = rope_tables(256, 64)
    w = randn_bf16(960, K, 0.1, seed=35)
    outs = [_nan(M, 960), _nan(M, 960)]
    for o in outs:
        cs.gemm8_rope(a, w, o, cos, sin, None, 256, 640, 64)
    assert torch.equal(outs[0], outs[1])
    ta, tb_ = randn_bf16(320, 264, seed=36), randn_bf16(320, 640, seed=37)
    for splits in (1, 3):
        assert torch.equal(_run_dw(ta, tb_, 0, True, splits), _run_dw(ta, tb_, 0, True, splits))
    slabs = _run_dw(ta, tb_, 0, False, 3)
    s1, s2 = _nan(264, 640, dtype=F32), _nan(264, 640, dtype=F32)
    cs.splitk_sum(slabs, s1, False)
    cs.splitk_sum(slabs, s2, False)
    assert torch.equal(s1, s2)
    x, wt = randn_bf16(64 * 23, 320, seed=38), randn_bf16(64 * 23, 480, seed=39)
    for splits in (1, 3):
        assert torch.equal(cs.gemm(x, wt, True, False, F32, 160, 160, splits), cs.gemm(x, wt, True, False, F32, 160, 160, splits))
