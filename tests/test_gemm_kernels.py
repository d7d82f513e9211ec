"""The hand-written bf16 GEMMs (csrc/gemm4.hip, csrc/gemm.hip) element by element against fp64 references
written here, at every native entry, tile edge and epilogue:

* gemm4 plain products (``matmul4``; entry pinned by ``_decide``): the four operand layouts, one / odd / even
  counts of 128-deep K pairs, the minimum M = 64, a last column tile of 8 columns, row and column edge tiles,
  with and without a pitched residual;
* gemm4 forward epilogues: all 20 instantiations of ``launch4`` (5 activations x bias x residual) on edge
  tiles, ``alpha != 1`` with a bias, a bias view at an odd element offset (``_aligned_bias``);
* split-K (``lta_gemm4_bf16_splitk``, kernel TAIL == 2) at hand-built slice counts: even and uneven deals of
  the K pairs (``r > 0``), one pair per slice, a bias and alpha in the fixup, the -2 return codes;
* the wave-tail split (``lta_gemm4_bf16_ws``, TAIL == 1 + TAIL == 2 + fixup) with a full last group of 8 tile
  rows and with a last group of a single tile row (``tile_coords``);
* grouped mode 1 (forward, dgrad) and mode 2 (wgrad, Stager KEDGE): groups of 0 (first and last), 1, 63, 65,
  129, 256, 257, 513 rows, one group alone, N = 8;
* the fused SwiGLU epilogues EPI 1 / EPI 2 and the qkv + RoPE epilogue EPI 3 on edge row tiles, a tile that
  spans two batches, a k head and a v head in the two wave columns of one tile;
* the 8-wave kernel: ``gemm_nt`` variants 0 / 1 and its 20 epilogues, ``matmul_hip`` in the four layouts,
  the grouped NT kernel behind ``grouped_mm`` for K % 128 != 0.
The ``!SW`` epilogue of ``gemm4_bf16_kernel`` is never built and not tested.

Error model (kernel_checks.assert_within), per element:  |out - ref64| <= ulp(bf16) |ref64| + 8 e32 + 1e-6.
``ref64`` is the operation in fp64 on the exactly upcast bf16 inputs, ``e32`` the largest error of the same
formula in torch fp32 (TF32 off).  Where a kernel rounds twice, the first rounding is passed as ``extra`` and
nothing else is:
  * residual epilogues store bf16(bf16(y) + r): the reference rounds y64 to bf16 (straight from fp64, ties to
    even), then adds; extra = ulp |y64|.  ref32 = bf16(y32) + r differs from ref64 by a whole bf16 spacing
    where y64 is within fp32's error of a tie (gemm_nt (256, 512, 192) seed 15, element (97, 115): y64 =
    2.101562526, y32 = 2.1015625 exactly, so fp32 rounds to 2.09375 and fp64 to 2.109375; err 2.15e-2 against
    1.78e-2, ratio 1.21, without it).  That difference is charged to its own element (added to ``extra``
    there) instead of entering e32, the maximum over the matrix: no element's tolerance is wider than the
    plain model's, and all but the few flipped ones lose the 8 spacings it would have given them;
  * EPI 2 (da, db from the bf16-rounded g): extra = ulp |ref64|;
  * EPI 3 q / k heads (rotation of the bf16-rounded projection): extra = ulp (|x1 cos| + |x2 sin|);
  * EPI 1's y is checked against silu(a) b in fp64 on the kernel's own stored a, b (one rounding, no extra);
    a, b against the projection; v heads are single-rounded products and bitwise the unfused path's.
The worst-case fp32 summation bound K 2^-24 (|a| @ |b|) is NOT used: no case needed it.

Every product also runs on integers in [-3, 3] (bias and residual too): with K <= 1024 every partial sum is
exact in fp32 and the output must be bit-equal to the rounded fp64 reference.

Guards (kernel_checks): outputs and residuals are views [:M, :N] of sentinel-filled buffers (>= 8 more rows,
pitch >= N + 64) whose outside must be untouched; operands are views of NaN-filled buffers with padded
pitches; the cached split workspace is filled with NaN before every split call, and two calls are bit-equal.
"""
import pytest
import torch
import torch.nn.functional as F

from kernel_checks import (BF16, SENTINEL, ULP, _WORST, assert_guard_intact, assert_within, bits_equal, guarded,
                           nan_padded, poison)

gpu = pytest.mark.gpu

# Largest err / tol measured on MI355X per group (every run prints them with -s):
#   gemm4 plain      0.993   (nt (328, 264, 128); with a residual 0.977)
#   gemm4 epilogue   0.993
#   gemm4 splitk     0.994
#   gemm4 tail       0.994   (16.1 M elements per case)
#   gemm4 grouped    0.994
#   swiglu EPI 1     0.994
#   swiglu EPI 2     0.995
#   qkv rope EPI 3   0.996
#   gemm 8-wave      0.994   (with a residual 0.992; 1.209 at one element of gemm_nt (256, 512, 192) + residual
#                             before the fp32 tie of the reference was charged to its element, see above)
# 2^-8 |x| is exactly the largest half-spacing of bf16, so a correctly rounded output sits at up to 1.0 of the
# first term alone; no case needed the factor 8, let alone the summation bound.  Every exact run is bit-equal.
# No kernel or host bug was found in csrc/gemm4.hip, csrc/gemm.hip or ops/gemm.py.
# Wall time of the file on MI355X: 6.7 s (334 GPU cases; the 9 CPU tests take 2.5 s).

LAYOUTS = ["nt", "nn", "tn", "tt"]  # a stored [K][M] when layout[0] == "t"; b stored [N][K] when layout[1] == "t"
ACTS = [None, "gelu_tanh", "gelu", "silu", "relu"]
RAGGED = [0, 1, 63, 65, 129, 256, 257, 513, 0]  # empty first and last groups, every reduction tail, tile +- 1
SIZE_LISTS = {"ragged": RAGGED, "one": [300]}


@pytest.fixture(autouse=True)
def _tf32_off():
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = prev


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def round_bf16(x64):
    """fp64 -> the nearest bf16 value (ties to even), kept in fp64: one rounding, not fp64 -> fp32 -> bf16."""
    m, e = torch.frexp(x64)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def ref_act(y, act):
    if act in (None, "none"):
        return y
    if act == "gelu_tanh":
        return 0.5 * y * (1.0 + torch.tanh(0.7978845608028654 * (y + 0.044715 * y * y * y)))
    if act == "gelu":
        return 0.5 * y * (1.0 + torch.erf(y * 0.7071067811865476))
    if act == "silu":
        return y / (1.0 + torch.exp(-y))
    assert act == "relu"
    return y.clamp_min(0.0)


def ref_linear(a, b, bias, act, alpha, dt):
    """act(alpha * a @ b + bias) for the logical a [M, K], b [K, N] in ``dt``."""
    y = (a.to(dt) @ b.to(dt)) * alpha
    if bias is not None:
        y = y + bias.to(dt)
    return ref_act(y, act)


def ref_grouped_rows(a, b, sizes, dt):
    """rows of group g of a [M, K] times b[g] [K, N]: the per-group loop."""
    out = torch.zeros(a.shape[0], b.shape[2], dtype=dt, device=a.device)
    start = 0
    for g, n in enumerate(sizes):
        out[start:start + n] = a[start:start + n].to(dt) @ b[g].to(dt)
        start += n
    return out


def ref_grouped_wgrad(x, dy, sizes, dt):
    """[G, N, K]: per group dy_g^T x_g (x [M, K], dy [M, N]); an empty group gives zeros."""
    out = torch.zeros(len(sizes), dy.shape[1], x.shape[1], dtype=dt, device=x.device)
    start = 0
    for g, n in enumerate(sizes):
        out[g] = dy[start:start + n].to(dt).t() @ x[start:start + n].to(dt)
        start += n
    return out


def ref_swiglu(a, b, dt):
    a, b = a.to(dt), b.to(dt)
    return a / (1.0 + torch.exp(-a)) * b


def ref_swiglu_bwd(g, a, b, dt):
    g, a, b = g.to(dt), a.to(dt), b.to(dt)
    s = 1.0 / (1.0 + torch.exp(-a))
    return g * b * (s * (1.0 + a * (1.0 - s))), g * (a * s)


def ref_rope_split(proj, cos, sin, B, T, nh, ng):
    """proj [B T, (nh + 2 ng) 128] -> (q [B, nh, T, 128], k, v [B, ng, T, 128], qmag, kmag): rotate-half
    with the first 64 columns of cos / sin [>= T, 128] (both halves equal); ``mag`` = |x1 cos| + |x2 sin| of
    every rotated element (what a relative error of the projection turns into)."""
    dt = proj.dtype
    nq = nh + 2 * ng
    x = proj.view(B, T, nq, 2, 64).permute(0, 2, 1, 3, 4)  # [B, nq, T, half, 64]
    x1, x2 = x[..., 0, :], x[..., 1, :]
    c, s = cos[:T, :64].to(dt), sin[:T, :64].to(dt)
    rot = torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1)
    mag = torch.cat(((x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()), dim=-1)
    v = torch.cat((x1, x2), dim=-1)[:, nh + ng:]
    return rot[:, :nh], rot[:, nh:nh + ng], v, mag[:, :nh], mag[:, nh:nh + ng]


# ------------------------------------------------------------------------------------------------
# inputs and checks
# ------------------------------------------------------------------------------------------------
def _values(shape, gen, exact, scale=1.0):
    if exact:
        return torch.randint(-3, 4, shape, generator=gen).to(BF16)
    return (torch.randn(shape, generator=gen) * scale).to(BF16)


def _inputs(M, N, K, seed, exact, device, bias=False, residual=False):
    """Logical a [M, K], b [K, N] (~ N(0, 1/K)), bias [N], residual [M, N] in bf16, drawn on the CPU (the same
    values on every device)."""
    gen = torch.Generator().manual_seed(seed)
    a = _values((M, K), gen, exact)
    b = _values((K, N), gen, exact, K ** -0.5)
    bi = _values((N,), gen, exact) if bias else None
    r = _values((M, N), gen, exact) if residual else None
    a, b, bi, r = (None if t is None else t.to(device) for t in (a, b, bi, r))
    if bi is not None:  # the bias too is followed by NaN
        wide = torch.full((N + 16,), float("nan"), dtype=BF16, device=device)
        wide[:N] = bi
        bi = wide[:N]
    return a, b, bi, r


def _place(a, b, layout):
    """a [M, K], b [K, N] as views with the storage of ``layout`` inside NaN-filled, pitch-padded buffers."""
    a = nan_padded(a.t()).t() if layout[0] == "t" else nan_padded(a)
    b = nan_padded(b.t()).t() if layout[1] == "t" else nan_padded(b)
    return a, b


def _guarded_copy(t):
    buf, view = guarded(t.shape, t.device)
    view.copy_(t)
    return buf, view


def assert_bits(out, ref64, what):
    """``out`` is bit for bit the fp64 reference rounded to bf16."""
    ref = round_bf16(ref64).to(BF16)
    if not bits_equal(out.contiguous(), ref.contiguous()):
        bad = (out.contiguous().view(torch.int16) != ref.contiguous().view(torch.int16))
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {out.numel()} elements differ from the exact result, the "
                             f"first at {i}: {out[i].item()} != {ref[i].item()}")


def check_product(out, a, b, *, group, what, bias=None, act=None, alpha=1.0, residual=None, exact=False):
    """``out`` against act(alpha a b + bias) (+ residual, added to the bf16-rounded value)."""
    y64 = ref_linear(a, b, bias, act, alpha, torch.float64)
    if exact:
        assert act is None
        if residual is not None:
            y64 = round_bf16(y64) + residual.double()
        return assert_bits(out, y64, what)
    y32 = ref_linear(a, b, bias, act, alpha, torch.float32)
    if residual is None:
        return assert_within(out, y64, y32, BF16, group, what)
    # ref32 is the same formula in fp32: bf16(y32) + r.  Where y64 lies within fp32's error of a bf16 tie, y32
    # rounds to the other neighbour and ref32 is off by a whole bf16 spacing; as a maximum over the matrix that
    # single element would widen every element's tolerance by 8 spacings.  It is charged to that element alone
    # (``flip``), so no element's tolerance is wider than with the global e32 and nearly all are far tighter.
    lo64, lo32 = round_bf16(y64), round_bf16(y32.double())
    flip = (lo32 - lo64).abs()
    ref64 = lo64 + residual.double()
    ref32 = torch.where(flip > 0, ref64, (lo32.float() + residual.float()).double())
    assert_within(out, ref64, ref32, BF16, group, what, extra=ULP[BF16] * y64.abs() + flip)


# ------------------------------------------------------------------------------------------------
# CPU: the references against independent formulations, and what the checks notice
# ------------------------------------------------------------------------------------------------
def test_round_bf16_is_one_rounding_cpu():
    torch.manual_seed(0)
    x = torch.randn(4096, dtype=torch.float64) * torch.logspace(-6, 6, 4096, dtype=torch.float64)
    r = round_bf16(x)
    assert torch.equal(r.to(BF16).double(), r)  # representable
    bits = r.to(BF16).view(torch.int16)
    for step in (1, -1):  # no neighbouring bf16 value is nearer
        assert ((r - x).abs() <= ((bits + step).view(BF16).double() - x).abs()).all()
    # a value that fp64 -> fp32 -> bf16 rounds the wrong way: just above a tie, by less than fp32 resolves
    tie = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert round_bf16(tie).item() == 1.0 + 2.0 ** -7 and tie.float().to(BF16).item() == 1.0
    assert round_bf16(torch.zeros(1, dtype=torch.float64)).item() == 0.0
    ints = torch.arange(-4000, 4000, dtype=torch.float64)
    assert torch.equal(round_bf16(ints), ints.to(BF16).double())


def test_ref_act_matches_torch_cpu():
    y = torch.linspace(-9, 9, 2001, dtype=torch.float64)
    for act, fn in (("gelu_tanh", lambda t: F.gelu(t, approximate="tanh")), ("gelu", F.gelu), ("silu", F.silu),
                    ("relu", torch.relu), (None, lambda t: t)):
        torch.testing.assert_close(ref_act(y, act), fn(y), atol=1e-14, rtol=1e-13)
    a, b, g = (torch.randn(64, 32, dtype=torch.float64, requires_grad=i < 2) for i in range(3))
    (F.silu(a) * b).backward(g)
    da, db = ref_swiglu_bwd(g, a.detach(), b.detach(), torch.float64)
    torch.testing.assert_close(da, a.grad, atol=1e-13, rtol=1e-12)
    torch.testing.assert_close(db, b.grad, atol=1e-13, rtol=1e-12)
    torch.testing.assert_close(ref_swiglu(a.detach(), b.detach(), torch.float64), F.silu(a.detach()) * b.detach(),
                               atol=1e-14, rtol=1e-13)


def test_ref_grouped_matches_dense_masking_cpu():
    torch.manual_seed(0)
    sizes = [0, 3, 1, 0, 5, 0]
    M, K, N, G = sum(sizes), 7, 5, len(sizes)
    a = torch.randn(M, K, dtype=torch.float64)
    b = torch.randn(G, K, N, dtype=torch.float64)
    dy = torch.randn(M, N, dtype=torch.float64)
    gid = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    onehot = (gid[:, None] == torch.arange(G)[None, :]).double()  # [M, G]
    dense = torch.einsum("mg,mk,gkn->mn", onehot, a, b)
    torch.testing.assert_close(ref_grouped_rows(a, b, sizes, torch.float64), dense, atol=1e-13, rtol=1e-13)
    dense_w = torch.einsum("mg,mn,mk->gnk", onehot, dy, a)
    got = ref_grouped_wgrad(a, dy, sizes, torch.float64)
    torch.testing.assert_close(got, dense_w, atol=1e-13, rtol=1e-13)
    assert not got[0].any() and not got[3].any() and not got[5].any()


def test_ref_rope_split_matches_decode_reference_cpu():
    from test_decode_kernels import ref_qkv_rope

    torch.manual_seed(0)
    for B, T, nh, ng in ((2, 5, 2, 1), (1, 3, 4, 2)):
        proj = torch.randn(B * T, (nh + 2 * ng) * 128, dtype=torch.float64)
        cos = (torch.rand(T + 2, 64, dtype=torch.float64) * 2 - 1).repeat(1, 2)
        sin = (torch.rand(T + 2, 64, dtype=torch.float64) * 2 - 1).repeat(1, 2)
        q, k, v, qm, km = ref_rope_split(proj, cos, sin, B, T, nh, ng)
        eq, ek, ev = ref_qkv_rope(proj.view(B, T, -1), cos, sin, nh, ng, 128, 128)
        for got, exp in ((q, eq), (k, ek), (v, ev)):
            torch.testing.assert_close(got, exp, atol=1e-14, rtol=1e-14)
        assert (qm >= q.abs() - 1e-14).all() and (km >= k.abs() - 1e-14).all()


@pytest.fixture
def worst_restored():
    """The mutated outputs' ratios are not measurements: the record of worst ratios is put back."""
    saved = dict(_WORST)
    yield
    _WORST.clear()
    _WORST.update(saved)


def _sensitivity_case(exact):
    M, N, K = 328, 264, 128
    a, b, bias, _ = _inputs(M, N, K, 11, exact, "cpu", bias=True)
    kw = dict(bias=bias, alpha=0.5, act=None if exact else "gelu_tanh", exact=exact, group="sensitivity")
    pre = (a.double() @ b.double()) * 0.5 + bias.double()
    return a, b, bias, kw, pre


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_checks_notice_a_subtly_wrong_kernel_cpu(exact, worst_restored):
    """A fake kernel output (the correctly rounded reference) passes; each mutation of it makes the check raise."""
    a, b, bias, kw, pre = _sensitivity_case(exact)
    act = kw["act"]
    fake = round_bf16(ref_act(pre, act)).to(BF16)
    check_product(fake, a, b, what="unmutated", **kw)  # ratio <= 1.0 (at most the half spacing of bf16)

    def raises(out, what):
        with pytest.raises(AssertionError):
            check_product(out, a, b, what=what, **kw)

    # 1. one element of the last partial tile off by 2 bf16 spacings
    sub = ref_act(pre, act)[256:, 256:].abs()
    i, j = divmod(int(sub.argmax()), sub.shape[1])
    i, j = i + 256, j + 256
    m = fake.clone()
    m.view(torch.int16)[i, j] += 2
    assert m[i, j] != fake[i, j]
    raises(m, "2 spacings")
    # 2. two rows swapped inside the last partial tile
    m = fake.clone()
    m[[300, 301]] = fake[[301, 300]]
    raises(m, "rows swapped")
    # 3. one a[i, k] b[k, j] product missing from the sum
    k = int((a[i].double() * b[:, j].double()).abs().argmax())
    assert a[i, k] != 0 and b[k, j] != 0
    less = pre.clone()
    less[i, j] -= 0.5 * a[i, k].double() * b[k, j].double()
    m = round_bf16(ref_act(less, act)).to(BF16)
    assert m[i, j] != fake[i, j]
    raises(m, "product missing")
    # 4. bias added after the activation (what only an activation makes visible)
    if not exact:
        m = round_bf16(ref_act(pre - bias.double(), act) + bias.double()).to(BF16)
        raises(m, "bias after act")
    # 5. a sentinel word changed one column past N
    buf, view = guarded((328, 264), "cpu")
    view.copy_(fake)
    assert_guard_intact(buf, (328, 264), "untouched")
    buf[5, 264] = SENTINEL + 1
    with pytest.raises(AssertionError):
        assert_guard_intact(buf, (328, 264), "one word past N")
    buf[5, 264] = SENTINEL
    buf[328, 0] = 0
    with pytest.raises(AssertionError):
        assert_guard_intact(buf, (328, 264), "one word past M")


def test_residual_check_notices_cpu(worst_restored):
    """The two-rounding model of the residual epilogues: the exactly computed bf16(bf16(y) + r) passes, a result
    that skipped the first rounding and is off by 2 spacings does not."""
    M, N, K = 328, 264, 128
    a, b, _, r = _inputs(M, N, K, 12, False, "cpu", residual=True)
    y = a.double() @ b.double()
    fake = round_bf16(round_bf16(y) + r.double()).to(BF16)
    check_product(fake, a, b, residual=r, group="sensitivity", what="residual")
    m = fake.clone()
    i, j = divmod(int(fake.abs().argmax()), N)
    m.view(torch.int16)[i, j] += 2
    with pytest.raises(AssertionError):
        check_product(m, a, b, residual=r, group="sensitivity", what="residual 2 spacings")


def test_nan_padded_operand_poisons_cpu():
    t = torch.arange(12.0).view(3, 4).to(BF16)
    v = nan_padded(t)
    assert torch.equal(v, t) and v.stride(0) % 8 == 0 and v.stride(0) >= 4 + 8
    whole = v.as_strided((3 + 8, v.stride(0)), (v.stride(0), 1))
    assert torch.isnan(whole[:, 4:]).all() and torch.isnan(whole[3:]).all()
    g = nan_padded(torch.ones(2, 3, 4, dtype=BF16))
    assert g.stride(0) == (3 + 8) * g.stride(1)


# ------------------------------------------------------------------------------------------------
# 1. gemm4 plain products
# ------------------------------------------------------------------------------------------------
def _gemm():
    from lightning_thunder_amd.ops import gemm as G

    return G


def _run_guarded(G, d, a, b, bias, res, alpha, M, N, what):
    """Launch record ``d`` into a guarded output (twice when it uses the workspace, which is poisoned)."""
    obuf, out = guarded((M, N), a.device)
    if d.ws:
        poison(G._workspace(d.ws, a.device))
    G._run(d, a, b, bias, res, alpha, out)
    assert_guard_intact(obuf, (M, N), what)
    if d.ws:
        obuf2, out2 = guarded((M, N), a.device)
        poison(G._workspace(d.ws, a.device))
        G._run(d, a, b, bias, res, alpha, out2)
        assert bits_equal(out.contiguous(), out2.contiguous()), f"{what}: two calls differ"
    return out


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("shape", [(64, 8, 128), (328, 264, 128), (256, 256, 256), (520, 776, 384)], ids=str)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gemm4_plain(layout, shape, residual, exact):
    G = _gemm()
    M, N, K = shape
    a, b, _, r = _inputs(M, N, K, 1, exact, "cuda", residual=residual)
    pa, pb = _place(a, b, layout)
    rbuf, res = _guarded_copy(r) if residual else (None, None)
    assert G._decide(pa, pb, None, res, None, "auto", linear=False).entry == G.GEMM4
    obuf, out = guarded((M, N), "cuda")
    got = G.matmul4(pa, pb, residual=res, out=out)
    assert got.data_ptr() == out.data_ptr()
    what = f"gemm4 {layout} {shape} res={residual}"
    assert_guard_intact(obuf, (M, N), what)
    if residual:
        assert_guard_intact(rbuf, (M, N), what + " residual")
        assert bits_equal(res.contiguous(), r)
    check_product(out, a, b, residual=r, exact=exact, group="gemm4 plain", what=what)


# ------------------------------------------------------------------------------------------------
# 2. gemm4 forward epilogues
# ------------------------------------------------------------------------------------------------
def _forward_call(G, a, b, bias, r, act, alpha, entry, what):
    """linear-rule launch of the forward layout (a row-major, b stored [N][K]) into guarded buffers."""
    M, N = a.shape[0], b.shape[1]
    pa, pb = _place(a, b, "nt")
    rbuf, res = (None, None) if r is None else _guarded_copy(r)
    d = G._decide(pa, pb.t(), bias, res, act, "auto", linear=True)
    assert d.entry == entry, d
    out = _run_guarded(G, d, pa, pb.t(), bias, res, alpha, M, N, what)
    if r is not None:
        assert_guard_intact(rbuf, (M, N), what + " residual")
    return out


@gpu
@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("act", ACTS, ids=str)
def test_gemm4_forward_epilogues(act, bias, residual):
    G = _gemm()
    M, N, K = 328, 264, 128
    a, b, bi, r = _inputs(M, N, K, 2, False, "cuda", bias=bias, residual=residual)
    what = f"gemm4 epilogue act={act} bias={bias} res={residual}"
    out = _forward_call(G, a, b, bi, r, act, 1.0, G.GEMM4, what)
    check_product(out, a, b, bias=bi, act=act, residual=r, group="gemm4 epilogue", what=what)


@gpu
@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
def test_gemm4_forward_bias_exact(residual):
    G = _gemm()
    M, N, K = 328, 264, 128
    a, b, bi, r = _inputs(M, N, K, 3, True, "cuda", bias=True, residual=residual)
    for alpha in (1.0, 0.5):
        what = f"gemm4 exact bias alpha={alpha} res={residual}"
        out = _forward_call(G, a, b, bi, r, None, alpha, G.GEMM4, what)  # one K pair: no split on any device
        check_product(out, a, b, bias=bi, alpha=alpha, residual=r, exact=True, group="gemm4 epilogue", what=what)


@gpu
def test_gemm4_alpha_with_bias_and_act():
    G = _gemm()
    M, N, K = 328, 264, 128
    a, b, bi, _ = _inputs(M, N, K, 4, False, "cuda", bias=True)
    what = "gemm4 alpha=0.5 bias gelu_tanh"
    out = _forward_call(G, a, b, bi, None, "gelu_tanh", 0.5, G.GEMM4, what)
    check_product(out, a, b, bias=bi, act="gelu_tanh", alpha=0.5, group="gemm4 epilogue", what=what)


@gpu
def test_gemm4_bias_view_at_odd_offset():
    """A bias that is a view at element offset 3 is copied by _aligned_bias: bitwise the aligned bias's result."""
    G = _gemm()
    M, N, K = 328, 264, 128
    a, b, bi, _ = _inputs(M, N, K, 5, False, "cuda", bias=True)
    pa, pb = _place(a, b, "nt")
    wide = torch.full((N + 16,), float("nan"), dtype=BF16, device="cuda")
    wide[3:3 + N] = bi
    view = wide[3:3 + N]
    assert view.data_ptr() % 16 and G._aligned_bias(view).data_ptr() % 16 == 0
    o1buf, o1 = guarded((M, N), "cuda")
    o2buf, o2 = guarded((M, N), "cuda")
    G.matmul4(pa, pb, bias=bi, act="gelu_tanh", out=o1)
    G.matmul4(pa, pb, bias=view, act="gelu_tanh", out=o2)
    assert_guard_intact(o1buf, (M, N), "aligned bias")
    assert_guard_intact(o2buf, (M, N), "bias view")
    assert bits_equal(o1.contiguous(), o2.contiguous())
    check_product(o2, a, b, bias=bi, act="gelu_tanh", group="gemm4 epilogue", what="gemm4 bias view at offset 3")
    # the linear rule copies it too
    G.last_gemm_backend_counts(reset=True)
    o3 = G.linear(pa, pb.t(), view, None, "gelu_tanh")
    assert G.last_gemm_backend_counts(reset=True) == {"gemm4": 1}
    assert bits_equal(o1.contiguous(), o3)


# ------------------------------------------------------------------------------------------------
# 3. split-K at hand-built slice counts
# ------------------------------------------------------------------------------------------------
def _splitk_record(G, pa, pb, bias, M, N, s):
    lay = G.gemm4_layout(pa, pb)
    nwg = -(-M // 256) * -(-N // 256)
    return G._gemm4_launch(pa, lay, bias, None, None, 1, None, (M, N))._replace(
        entry=G.GEMM4_SPLITK, ksplit=s, tail=0, ws=s * nwg * 256 * 256)


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("P,s", [(5, 2), (5, 3), (7, 3), (4, 4), (2, 2)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gemm4_splitk(layout, P, s, exact):
    G = _gemm()
    M, N, K = 328, 264, 128 * P
    a, b, _, _ = _inputs(M, N, K, 6, exact, "cuda")
    pa, pb = _place(a, b, layout)
    d = _splitk_record(G, pa, pb, None, M, N, s)
    assert (d.at, d.bt) == (int(layout[0] == "t"), int(layout[1] != "t"))
    what = f"splitk {layout} P={P} s={s}"
    G.last_gemm_backend_counts(reset=True)
    out = _run_guarded(G, d, pa, pb, None, None, 1.0, M, N, what)
    assert G.last_gemm_backend_counts(reset=True) == {"gemm4": 2}
    check_product(out, a, b, exact=exact, group="gemm4 splitk", what=what)


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("P,s", [(5, 2), (5, 3), (7, 3), (4, 4), (2, 2)])
def test_gemm4_splitk_bias_alpha(P, s, exact):
    G = _gemm()
    M, N, K = 328, 264, 128 * P
    a, b, bi, _ = _inputs(M, N, K, 7, exact, "cuda", bias=True)
    pa, pb = _place(a, b, "nt")
    d = _splitk_record(G, pa, pb, bi, M, N, s)
    what = f"splitk bias alpha=0.5 P={P} s={s}"
    out = _run_guarded(G, d, pa, pb, bi, None, 0.5, M, N, what)
    check_product(out, a, b, bias=bi, alpha=0.5, exact=exact, group="gemm4 splitk", what=what)


@gpu
@pytest.mark.parametrize("P,s", [(2, 3), (5, 6), (5, 1)])
def test_gemm4_splitk_rejects_bad_split(P, s):
    """More slices than K pairs, or a single slice: -2 and nothing is launched."""
    from lightning_thunder_amd.ops._lib import require, stream_ptr

    G = _gemm()
    M, N, K = 328, 264, 128 * P
    a, b, _, _ = _inputs(M, N, K, 8, False, "cuda")
    pa, pb = _place(a, b, "nt")
    _, _, lda, ldb = G.gemm4_layout(pa, pb)
    obuf, out = guarded((M, N), "cuda")
    ws = poison(G._workspace(max(s, 2) * 4 * 256 * 256, pa.device))
    rc = require().lta_gemm4_bf16_splitk(pa.data_ptr(), pb.data_ptr(), out.data_ptr(), None, M, N, K, lda, ldb,
                                         out.stride(0), 1.0, 0, 0, s, ws.data_ptr(), ws.numel() * 4,
                                         stream_ptr(pa.device))
    torch.cuda.synchronize()
    assert rc == -2
    assert_guard_intact(obuf, (0, 0), "rejected split")  # not one word of the output was written
    assert torch.isnan(ws).all()


# ------------------------------------------------------------------------------------------------
# 4. wave-tail split
# ------------------------------------------------------------------------------------------------
def _tail_shape(nTm, cus):
    """The narrowest grid of nTm tile rows with more than one wave of tiles and a last wave at most half full."""
    for nTn in range(1, 4 * cus):
        nwg = nTm * nTn
        if nwg > cus and 1 <= nwg % cus <= cus // 2:
            return 256 * nTm - 56, 256 * nTn - 248, nwg % cus
    raise AssertionError(f"no tail-split grid with {nTm} tile rows for {cus} compute units")


def test_tail_shape_cpu():
    assert _tail_shape(8, 256) == (1992, 8200, 8) and _tail_shape(9, 256) == (2248, 7176, 5)
    for cus in (64, 80, 104, 120, 228, 256, 304):
        for nTm in (8, 9):
            M, N, tail = _tail_shape(nTm, cus)
            assert -(-M // 256) == nTm and N % 8 == 0 and M % 8 == 0 and 1 <= tail <= cus // 2


@gpu
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("nTm", [8, 9])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gemm4_tail_split(layout, nTm, K):
    G = _gemm()
    cus = G._device_cus(torch.device("cuda", torch.cuda.current_device()))
    M, N, tail = _tail_shape(nTm, cus)
    for exact in (True, False):
        a, b, _, _ = _inputs(M, N, K, 9, exact, "cuda")
        pa, pb = _place(a, b, layout)
        d = G._decide(pa, pb, None, None, None, "auto", linear=False)
        assert d.entry == G.GEMM4_TAIL and d.tail == tail and d.ws == 2 * tail * 256 * 256, d
        what = f"tail split {layout} {nTm} tile rows K={K} {'exact' if exact else 'random'}"
        out = _run_guarded(G, d, pa, pb, None, None, 1.0, M, N, what)
        check_product(out, a, b, exact=exact, group="gemm4 tail", what=what)


# ------------------------------------------------------------------------------------------------
# 5. grouped GEMMs
# ------------------------------------------------------------------------------------------------
def _offsets(sizes, device):
    return torch.tensor(sizes).cumsum(0).to(torch.int32).to(device)


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("sizes", list(SIZE_LISTS), ids=str)
@pytest.mark.parametrize("N", [8, 264])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("bt", [0, 1], ids=["forward", "dgrad"])
def test_gemm4_grouped_rows(bt, K, N, sizes, exact):
    """Mode 1: rows of group g times b[g], stored [N][K] (forward, bt = 0) or [K][N] (dgrad, bt = 1)."""
    from lightning_thunder_amd.ops._lib import require, stream_ptr

    G = _gemm()
    sizes = SIZE_LISTS[sizes]
    M, ng = sum(sizes), len(sizes)
    gen = torch.Generator().manual_seed(10)
    a = _values((M, K), gen, exact).cuda()
    b = _values((ng, K, N), gen, exact, K ** -0.5).cuda()
    offs = _offsets(sizes, "cuda")
    pa = nan_padded(a)
    pb = nan_padded(b) if bt else nan_padded(b.transpose(1, 2)).transpose(1, 2)
    assert G.grouped_rows_supported(pa, pb, offs) and G._grouped_b_layout(pb)[0] == bt
    ldb = G._grouped_b_layout(pb)[1]
    obuf, out = guarded((M, N), "cuda")
    rc = require().lta_gemm4_grouped(1, pa.data_ptr(), pb.data_ptr(), out.data_ptr(), offs.data_ptr(), ng, M, N, K,
                                     pa.stride(0), ldb, out.stride(0), pb.stride(0), 0, bt, stream_ptr(pa.device))
    assert rc == 0
    what = f"grouped {'dgrad' if bt else 'forward'} K={K} N={N} sizes={sizes}"
    assert_guard_intact(obuf, (M, N), what)
    ref64 = ref_grouped_rows(a, b, sizes, torch.float64)
    if exact:
        assert_bits(out, ref64, what)
    else:
        assert_within(out, ref64, ref_grouped_rows(a, b, sizes, torch.float32), BF16, "gemm4 grouped", what)
    # the wrapper passes the same arguments (its own contiguous output)
    G.last_gemm_backend_counts(reset=True)
    y = G.grouped_mm(pa, pb, offs)
    assert G.last_gemm_backend_counts(reset=True) == {"gemm4": 1}
    assert bits_equal(y, out.contiguous())


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("sizes", list(SIZE_LISTS), ids=str)
@pytest.mark.parametrize("K,N", [(128, 8), (264, 264), (8, 520)])
def test_gemm4_grouped_wgrad(K, N, sizes, exact):
    """Mode 2: [G, N, K] = per group dy_g^T x_g, the group's rows as the (zero-filled) reduction."""
    from lightning_thunder_amd.ops._lib import require, stream_ptr

    G = _gemm()
    sizes = SIZE_LISTS[sizes]
    M, ng = sum(sizes), len(sizes)
    gen = torch.Generator().manual_seed(11)
    x = _values((M, K), gen, exact).cuda()
    dy = _values((M, N), gen, exact).cuda()
    offs = _offsets(sizes, "cuda")
    px, pdy = nan_padded(x), nan_padded(dy)
    assert G.grouped_wgrad_supported(px.t(), pdy, offs)
    obuf, out = guarded((ng, N, K), "cuda")
    rc = require().lta_gemm4_grouped(2, pdy.data_ptr(), px.data_ptr(), out.data_ptr(), offs.data_ptr(), ng, N, K, M,
                                     pdy.stride(0), px.stride(0), out.stride(1), 0, out.stride(0), 1,
                                     stream_ptr(px.device))
    assert rc == 0
    what = f"grouped wgrad K={K} N={N} sizes={sizes}"
    assert_guard_intact(obuf, (ng, N, K), what)
    ref64 = ref_grouped_wgrad(x, dy, sizes, torch.float64)
    ref32 = ref_grouped_wgrad(x, dy, sizes, torch.float32)
    for g, n in enumerate(sizes):
        if n == 0:
            assert not out[g].contiguous().view(torch.int16).any(), f"{what}: empty group {g} is not exact zeros"
        elif exact:
            assert_bits(out[g], ref64[g], f"{what} group {g}")
        else:
            assert_within(out[g], ref64[g], ref32[g], BF16, "gemm4 grouped", f"{what} group {g} ({n} rows)")
    G.last_gemm_backend_counts(reset=True)
    y = G.grouped_mm(px.t(), pdy, offs)  # [G, K, N], the transposed view of its [G, N, K] result
    assert G.last_gemm_backend_counts(reset=True) == {"gemm4": 1}
    assert bits_equal(y.transpose(1, 2).contiguous(), out.contiguous())


# ------------------------------------------------------------------------------------------------
# 6. fused SwiGLU epilogues
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("Nh", [128, 384])
@pytest.mark.parametrize("M", [64, 328, 520])
def test_gemm4_gate_up_swiglu(M, Nh, K, exact, monkeypatch):
    """EPI 1: a = x W1^T, b = x W2^T, y = silu(a) b in one launch, on edge row tiles."""
    from lightning_thunder_amd.ops._lib import require, stream_ptr

    monkeypatch.setenv("LTA_FUSED_SWIGLU", "1")
    G = _gemm()
    gen = torch.Generator().manual_seed(12)
    x = _values((M, K), gen, exact).cuda()
    w1 = _values((Nh, K), gen, exact, K ** -0.5).cuda()
    w2 = _values((Nh, K), gen, exact, K ** -0.5).cuda()
    px, p1, p2 = nan_padded(x), nan_padded(w1), nan_padded(w2)
    assert G.gate_up_supported(px, p1, p2)
    what = f"gate-up M={M} Nh={Nh} K={K}"

    def launch(need_ab):
        bufs = [guarded((M, Nh), "cuda") for _ in range(3)]
        (_, a), (_, b), (_, y) = bufs
        rc = require().lta_gemm4_swiglu(px.data_ptr(), p1.data_ptr(), p2.data_ptr(), a.data_ptr() if need_ab else None,
                                        b.data_ptr() if need_ab else None, y.data_ptr(), None, None, M, Nh, K,
                                        px.stride(0), p1.stride(0), y.stride(0), 1, stream_ptr(px.device))
        assert rc == 0
        for (buf, _), name in zip(bufs, "aby"):
            # without need_ab not one word of a, b may be written
            assert_guard_intact(buf, (M, Nh) if need_ab or name == "y" else (0, 0), f"{what} {name} need_ab={need_ab}")
        return a, b, y

    a, b, y = launch(True)
    _, _, y2 = launch(False)
    assert bits_equal(y.contiguous(), y2.contiguous())
    for got, w, name in ((a, w1, "a"), (b, w2, "b")):
        if exact:
            assert_bits(got, x.double() @ w.double().t(), f"{what} {name}")
        else:
            assert_within(got, x.double() @ w.double().t(), x.float() @ w.float().t(), BF16, "swiglu EPI 1",
                          f"{what} {name}")
    assert_within(y, ref_swiglu(a, b, torch.float64), ref_swiglu(a, b, torch.float32), BF16, "swiglu EPI 1",
                  f"{what} y from the stored a, b")
    G.last_gemm_backend_counts(reset=True)
    wa, wb, wy = G.gate_up_swiglu(px, p1, p2)
    assert G.last_gemm_backend_counts(reset=True) == {"gemm4": 1}
    assert bits_equal(wa, a.contiguous()) and bits_equal(wb, b.contiguous()) and bits_equal(wy, y.contiguous())


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [64, 328])
def test_gemm4_swiglu_backward(M, N, K, exact, monkeypatch):
    """EPI 2: g = dY W stays on chip; da = g b silu'(a), db = g silu(a) from the bf16-rounded g."""
    from lightning_thunder_amd.ops._lib import require, stream_ptr

    monkeypatch.setenv("LTA_FUSED_SWIGLU", "1")
    G = _gemm()
    gen = torch.Generator().manual_seed(13)
    dy = _values((M, K), gen, exact).cuda()
    w = _values((K, N), gen, exact, K ** -0.5).cuda()  # the down-projection weight [out, in] read as [K][N]
    a = _values((M, N), gen, False).cuda()
    b = _values((M, N), gen, False).cuda()
    pdy, pw = nan_padded(dy), nan_padded(w)
    assert G.gemm4_layout(pdy, pw)[:2] == (0, 1)
    (abuf, ga), (bbuf, gb) = _guarded_copy(a), _guarded_copy(b)
    (dabuf, da), (dbbuf, db) = guarded((M, N), "cuda"), guarded((M, N), "cuda")
    rc = require().lta_gemm4_swiglu(pdy.data_ptr(), pw.data_ptr(), None, da.data_ptr(), db.data_ptr(), None,
                                    ga.data_ptr(), gb.data_ptr(), M, N, K, pdy.stride(0), pw.stride(0), da.stride(0), 2,
                                    stream_ptr(pdy.device))
    assert rc == 0
    what = f"swiglu bwd M={M} N={N} K={K}"
    for buf, name in ((abuf, "a"), (bbuf, "b"), (dabuf, "da"), (dbbuf, "db")):
        assert_guard_intact(buf, (M, N), f"{what} {name}")
    assert bits_equal(ga.contiguous(), a) and bits_equal(gb.contiguous(), b)
    g64 = dy.double() @ w.double()
    if exact:  # g is exact in fp32: the kernel's bf16 g is the rounded g64, nothing propagates
        refs = ref_swiglu_bwd(round_bf16(g64), a, b, torch.float64)
        refs32 = ref_swiglu_bwd(round_bf16(g64), a, b, torch.float32)
    else:
        refs = ref_swiglu_bwd(g64, a, b, torch.float64)
        refs32 = ref_swiglu_bwd(dy.float() @ w.float(), a, b, torch.float32)
    for got, r64, r32, name in ((da, refs[0], refs32[0], "da"), (db, refs[1], refs32[1], "db")):
        assert_within(got, r64, r32, BF16, "swiglu EPI 2", f"{what} {name}",
                      extra=None if exact else ULP[BF16] * r64.abs())
    G.last_gemm_backend_counts(reset=True)
    wda, wdb = G.matmul_swiglu_bwd(pdy, pw, a, b)
    assert G.last_gemm_backend_counts(reset=True) == {"gemm4": 1}
    assert bits_equal(wda, da.contiguous()) and bits_equal(wdb, db.contiguous())


# ------------------------------------------------------------------------------------------------
# 7. qkv projection + RoPE
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("nh,ng", [(2, 1), (2, 2), (4, 1)])
@pytest.mark.parametrize("B,T", [(2, 200), (3, 100), (1, 64)])
def test_gemm4_qkv_rope(B, T, nh, ng, K, exact):
    """EPI 3: q, k rotated from the bf16-rounded projection and stored as [B, H, T, 128]; tiles that span two
    batches ((2, 200), (3, 100)), edge row tiles (all three), k and v heads in one tile ((2, 1), (4, 1))."""
    from lightning_thunder_amd.ops._lib import require, stream_ptr
    from lightning_thunder_amd.ops.fused import qkv_rope_fwd

    G = _gemm()
    M, nq = B * T, nh + 2 * ng
    gen = torch.Generator().manual_seed(14)
    x = _values((M, K), gen, exact).cuda()
    w = _values((nq * 128, K), gen, exact, K ** -0.5).cuda()
    cos = (torch.rand(T + 16, 64, generator=gen) * 2 - 1).repeat(1, 2).cuda()
    sin = (torch.rand(T + 16, 64, generator=gen) * 2 - 1).repeat(1, 2).cuda()
    px, pw = nan_padded(x), nan_padded(w)
    c, s = cos[:T].contiguous(), sin[:T].contiguous()
    lead = (1, 0, 0, 0)  # one more batch of sentinels behind each output
    (qbuf, q), (kbuf, k), (vbuf, v) = (guarded((B, h, T, 128), "cuda", pads=lead) for h in (nh, ng, ng))
    rc = require().lta_gemm4_qkv_rope(px.data_ptr(), pw.data_ptr(), c.data_ptr(), s.data_ptr(), q.data_ptr(),
                                      k.data_ptr(), v.data_ptr(), M, K, px.stride(0), pw.stride(0), T, nh, ng,
                                      stream_ptr(px.device))
    assert rc == 0
    what = f"qkv rope B={B} T={T} nh={nh} ng={ng} K={K}"
    for buf, h, name in ((qbuf, nh, "q"), (kbuf, ng, "k"), (vbuf, ng, "v")):
        assert_guard_intact(buf, (B, h, T, 128), f"{what} {name}")
    p64 = x.double() @ w.double().t()
    if exact:  # the projection is exact in fp32: its bf16 rounding is the rounded p64, nothing propagates
        rq, rk, rv, _, _ = ref_rope_split(round_bf16(p64), cos.double(), sin.double(), B, T, nh, ng)
        sq, sk, _, _, _ = ref_rope_split(round_bf16(p64).float(), cos, sin, B, T, nh, ng)
        assert_bits(v, rv, f"{what} v")
        assert_within(q, rq, sq, BF16, "qkv rope EPI 3", f"{what} q")
        assert_within(k, rk, sk, BF16, "qkv rope EPI 3", f"{what} k")
    else:
        rq, rk, rv, qm, km = ref_rope_split(p64, cos.double(), sin.double(), B, T, nh, ng)
        sq, sk, sv, _, _ = ref_rope_split(x.float() @ w.float().t(), cos, sin, B, T, nh, ng)
        assert_within(q, rq, sq, BF16, "qkv rope EPI 3", f"{what} q", extra=ULP[BF16] * qm)
        assert_within(k, rk, sk, BF16, "qkv rope EPI 3", f"{what} k", extra=ULP[BF16] * km)
        assert_within(v, rv, sv, BF16, "qkv rope EPI 3", f"{what} v")
    # the wrapper passes the same arguments; the unfused pair computes the same v bit for bit
    G.last_gemm_backend_counts(reset=True)
    wq, wk, wv = G.linear_qkv_rope(px.view(B, T, K), pw, cos, sin, nh, ng, 128, 128)
    assert G.last_gemm_backend_counts(reset=True) == {"gemm4": 1}
    assert bits_equal(wq, q) and bits_equal(wk, k) and bits_equal(wv, v)
    d = G._decide(px, pw, None, None, None, "auto", linear=True)
    assert d.entry in (G.GEMM4, G.GEMM4_SPLITK)
    d = d._replace(entry=G.GEMM4, ksplit=0, ws=0)  # the unsplit product: the fused kernel's summation order
    uq, uk, uv = qkv_rope_fwd(G._run(d, px, pw, None, None).view(B, T, -1), cos, sin, nh, ng, 128, 128)
    assert bits_equal(uv, v)
    def rel(t, u):
        return ((t.float() - u.float()).norm() / (u.float().norm() + 1e-12)).item()

    assert rel(q, uq) < 1e-3 and rel(k, uk) < 1e-3


# ------------------------------------------------------------------------------------------------
# 8. the 8-wave kernel (csrc/gemm.hip)
# ------------------------------------------------------------------------------------------------
def _gemm_nt_call(G, a, b, bi, r, act, alpha, variant, what):
    M, N = a.shape[0], b.shape[1]
    pa, pb = _place(a, b, "nt")
    rbuf, res = (None, None) if r is None else _guarded_copy(r)
    assert G.gemm_nt_supported(pa, pb.t(), bi, res)
    obuf, out = guarded((M, N), "cuda")
    G.gemm_nt(pa, pb.t(), bias=bi, residual=res, act=act, alpha=alpha, out=out, variant=variant)
    assert_guard_intact(obuf, (M, N), what)
    if r is not None:
        assert_guard_intact(rbuf, (M, N), what + " residual")
    return out


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("variant,shape", [(0, (256, 256, 64)), (0, (256, 512, 192)), (0, (512, 256, 384)),
                                           (1, (512, 256, 384))], ids=str)
def test_gemm_nt_plain(variant, shape, residual, exact):
    G = _gemm()
    M, N, K = shape
    a, b, _, r = _inputs(M, N, K, 15, exact, "cuda", residual=residual)
    what = f"gemm_nt v{variant} {shape} res={residual}"
    out = _gemm_nt_call(G, a, b, None, r, None, 1.0, variant, what)
    check_product(out, a, b, residual=r, exact=exact, group="gemm 8-wave", what=what)


@gpu
@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("act", ACTS, ids=str)
def test_gemm_nt_epilogues(act, bias, residual):
    G = _gemm()
    M, N, K = 256, 512, 192
    a, b, bi, r = _inputs(M, N, K, 16, False, "cuda", bias=bias, residual=residual)
    what = f"gemm_nt epilogue act={act} bias={bias} res={residual}"
    out = _gemm_nt_call(G, a, b, bi, r, act, 1.0, 0, what)
    check_product(out, a, b, bias=bi, act=act, residual=r, group="gemm 8-wave", what=what)


@gpu
def test_gemm_nt_alpha_bias_exact_and_act():
    G = _gemm()
    M, N, K = 256, 512, 192
    a, b, bi, _ = _inputs(M, N, K, 17, True, "cuda", bias=True)
    out = _gemm_nt_call(G, a, b, bi, None, None, 0.5, 0, "gemm_nt exact alpha bias")
    check_product(out, a, b, bias=bi, alpha=0.5, exact=True, group="gemm 8-wave", what="gemm_nt exact alpha bias")
    a, b, bi, _ = _inputs(M, N, K, 17, False, "cuda", bias=True)
    out = _gemm_nt_call(G, a, b, bi, None, "gelu_tanh", 0.5, 0, "gemm_nt alpha bias gelu_tanh")
    check_product(out, a, b, bias=bi, act="gelu_tanh", alpha=0.5, group="gemm 8-wave",
                  what="gemm_nt alpha bias gelu_tanh")


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_matmul_hip_layouts(layout, residual, exact):
    G = _gemm()
    M, N, K = 256, 512, 192
    a, b, _, r = _inputs(M, N, K, 18, exact, "cuda", residual=residual)
    pa, pb = _place(a, b, layout)
    assert G.matmul_layout(pa, pb)[:2] == (int(layout[0] == "t"), int(layout[1] != "t"))
    rbuf, res = _guarded_copy(r) if residual else (None, None)
    obuf, out = guarded((M, N), "cuda")
    G.matmul_hip(pa, pb, residual=res, out=out)
    what = f"matmul_hip {layout} res={residual}"
    assert_guard_intact(obuf, (M, N), what)
    if residual:
        assert_guard_intact(rbuf, (M, N), what + " residual")
    check_product(out, a, b, residual=r, exact=exact, group="gemm 8-wave", what=what)


@gpu
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("sizes", list(SIZE_LISTS), ids=str)
def test_grouped_mm_8wave(sizes, exact):
    """K = 192 is no multiple of 128: the grouped NT kernel of csrc/gemm.hip serves the call."""
    G = _gemm()
    sizes = SIZE_LISTS[sizes]
    M, ng, K, N = sum(sizes), len(sizes), 192, 256
    gen = torch.Generator().manual_seed(19)
    a = _values((M, K), gen, exact).cuda()
    w = _values((ng, N, K), gen, exact, K ** -0.5).cuda()
    offs = _offsets(sizes, "cuda")
    b = w.transpose(1, 2)
    assert not G.grouped_rows_supported(a, b, offs) and G.grouped_nt_supported(a, b, offs)
    G.last_gemm_backend_counts(reset=True)
    out = G.grouped_mm(a, b, offs)
    assert G.last_gemm_backend_counts(reset=True) == {"gemm": 1}
    what = f"grouped 8-wave sizes={sizes}"
    ref64 = ref_grouped_rows(a, b, sizes, torch.float64)
    if exact:
        assert_bits(out, ref64, what)
    else:
        assert_within(out, ref64, ref_grouped_rows(a, b, sizes, torch.float32), BF16, "gemm 8-wave", what)
