"""``ops.sampling.sample_last`` (csrc/sampling.hip ``lta_sample_rows``): temperature / top-k / top-p
sampling from the project's Philox stream, against an fp64 reference of the definition written here.

The definition (``ops/sampling.py`` docstring): kept set by top-k (ties at the k-th logit all kept), then
by top-p (largest value whose at-least-as-large kept logits hold ``top_p`` of the mass; tie groups whole),
then Gumbel-max over the kept set with ``u = (2 (w >> 9) + 1) 2^-24`` from Philox word ``e % 4`` of block
``e // 4``, ``e = r * V4 + i``.  Sampling has one right token per row, so the comparison is exact, except
where the inputs themselves leave the answer to rounding.  A row is *ambiguous* (decided on the reference
alone, before any result is looked at) when

(a) the fp64 gap between the best and the second-best kept score is at most ``2 (8 e32 + 2^-23 |best|)``,
    ``e32`` the largest difference over the row's finite scores between a torch fp32 evaluation of the
    same formula and the fp64 one (the ``8 e32`` convention of kernel_checks), or
(b) the winner changes when ``top_p`` is replaced by ``top_p +- 1e-5`` (fp32 masses over at most 2^18
    terms plus the error of expf stay near 1e-6 relative: a 10x margin).

An unambiguous row must match the reference exactly; an ambiguous one may return the runner-up (a) or the
other winner (b).  No row may be ambiguous in a case of R <= 3 rows and at most one in a case of 64.
"""
import math

import pytest
import torch

from kernel_checks import BF16, F16, F32, _dt_id

from lightning_thunder_amd.core import rng

gpu = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
M32 = 0xFFFFFFFF
# (temperature, top_k, top_p)
PARAMS = [(0.8, None, None), (1.0, 50, None), (0.7, None, 0.9), (1.3, 40, 0.95)]
SCALES = [0.02, 2.0, 8.0]


def _pid(p):
    return f"T{p[0]}-k{p[1]}-p{p[2]}"


def _clamp_k(k, V):
    """A top_k that does not filter says nothing: k >= V becomes max(1, V // 2)."""
    return k if k is None or k < V else max(1, V // 2)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


# ------------------------------------------------------------------------------------------------
# the fp64 reference
# ------------------------------------------------------------------------------------------------
class Reference:
    """The definition in fp64 on the exactly upcast rows ``x`` [R, V] (CPU) for one (seed, offset); the
    sort and the uniforms are shared by every parameter set asked of it."""

    def __init__(self, x, seed, offset):
        assert x.device.type == "cpu" and x.dim() == 2
        self.R, self.V = R, V = x.shape
        self.x32 = x.float()
        self.xd = x.double()
        V4 = (V + 3) // 4 * 4
        blk = torch.arange(R * V4 // 4, dtype=torch.int64)
        w = rng.philox4x32(blk & M32, blk >> 32, torch.full_like(blk, offset & M32),
                           torch.full_like(blk, (offset >> 32) & M32), seed & M32, 0)
        w = torch.stack(w, dim=1).reshape(R, V4)[:, :V]
        n = 2 * (w >> 9) + 1  # < 2^24: exact in fp32
        self.g64 = -torch.log(-torch.log(n.double() * 2.0 ** -24))
        self.g32 = -torch.log(-torch.log(n.float() * 2.0 ** -24))
        self.xs, _ = torch.sort(self.xd, dim=-1, descending=True)
        xd = self.xd
        self.nan, self.pinf = xd.isnan(), xd == INF
        self.special = self.nan.any(-1) | self.pinf.any(-1) | (xd == -INF).all(-1)
        sp = torch.where(self.pinf.any(-1), self.pinf.int().argmax(-1), torch.zeros(R, dtype=torch.int64))
        self.special_index = torch.where(self.nan.any(-1), self.nan.int().argmax(-1), sp)

    def kept(self, T, top_k, top_p):
        """bool [R, V]: the kept set (rows of point 4 aside), without the -inf entries."""
        xd, xs, V = self.xd, self.xs, self.V
        keep = torch.ones_like(xd, dtype=torch.bool)
        ks = torch.ones_like(keep)  # the kept set in sorted order: a prefix
        if top_k is not None and top_k < V:
            tk = xs[:, top_k - 1:top_k]
            keep, ks = xd >= tk, xs >= tk
        if top_p is not None and top_p < 1:
            ms = torch.exp(xs / T - xs[:, :1] / T) * ks
            cs = ms.cumsum(-1)
            j = torch.arange(V).expand_as(xs)
            last = torch.ones_like(keep)
            last[:, :-1] = xs[:, :-1] != xs[:, 1:]
            end = torch.cummin(torch.where(last, j, torch.full_like(j, V - 1)).flip(-1), dim=-1).values.flip(-1)
            at_least = cs.gather(-1, end)  # mass of the kept logits >= this value
            qualifies = (at_least >= top_p * cs[:, -1:]) & ks
            tp = xs.gather(-1, qualifies.int().argmax(-1, keepdim=True))  # first in descending order: the largest
            keep = keep & (xd >= tp)
        return keep & (xd != -INF)

    def winners(self, T, top_k, top_p):
        """(winner [R], runner-up [R], gap [R], e32 [R], best score [R]) of the Gumbel-max draw."""
        keep = self.kept(T, top_k, top_p)
        s = (self.xd / T + self.g64).masked_fill(~keep, -INF)
        s32 = (self.x32 / torch.tensor(T, dtype=torch.float32) + self.g32).masked_fill(~keep, -INF)
        fin = torch.isfinite(s)
        e32 = torch.where(fin, (s32.double() - s).abs(), torch.zeros_like(s)).max(-1).values
        best, win = s.max(-1)
        win = s.argmax(-1)  # the first index on ties
        s2 = s.scatter(-1, win[:, None], -INF)
        second, run = s2.max(-1)
        return win, run, best - second, e32, best

    def expect(self, T, top_k, top_p):
        """(winner, ambiguous, alternatives): alternatives [R, 3] hold, per row, the tokens an ambiguous
        row may return instead of the winner (the winner itself where there is none)."""
        T = _f32(T)
        top_p = None if top_p is None else _f32(top_p)
        win, run, gap, e32, best = self.winners(T, top_k, top_p)
        amb_a = gap <= 2 * (8 * e32 + 2.0 ** -23 * best.abs())
        alts = [torch.where(amb_a, run, win)]
        amb = amb_a
        if top_p is not None and top_p < 1:
            for p in (top_p - 1e-5, top_p + 1e-5):
                other = self.winners(T, top_k, p)[0]
                amb = amb | (other != win)
                alts.append(other)
        else:
            alts += [win, win]
        amb = amb & ~self.special
        win = torch.where(self.special, self.special_index, win)
        alts = torch.stack([torch.where(self.special, win, a) for a in alts], dim=1)
        return win, amb, alts


def check_tokens(got, ref, params, what):
    """``got`` (a callable giving the tokens [R]) against the reference; the cap on ambiguous rows is
    asserted before ``got`` runs."""
    T, k, p = params
    win, amb, alts = ref.expect(T, k, p)
    n_amb = int(amb.sum())
    assert n_amb <= (0 if ref.R <= 3 else 1), f"{what}: {n_amb} ambiguous rows of {ref.R}: choose another seed"
    tok = got().cpu()
    assert tok.dtype == torch.int64 and tok.shape == (ref.R,), (tok.dtype, tok.shape)
    ok = (tok == win) | (amb & (tok[:, None] == alts).any(-1))
    bad = (~ok).nonzero().flatten().tolist()
    assert not bad, (f"{what}: rows {bad[:8]} gave {tok[bad[:8]].tolist()}, reference {win[bad[:8]].tolist()}"
                     f" ({len(bad)} of {ref.R} rows, {n_amb} ambiguous)")
    return n_amb


def _logits(R, V, scale, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, V, generator=g) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------
# CPU: the torch fallback
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_dt_id)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("R", [3, 64])
@pytest.mark.parametrize("V", [1, 7, 9, 37, 8195, 32003, 65544, 128259])
def test_fallback_matches_reference(V, R, scale, dtype):
    from lightning_thunder_amd.ops.sampling import sample_last

    seed, offset = 1234 + V, 7 * R
    x = _logits(R, V, scale, dtype, V * 64 + R)
    ref = Reference(x, seed, offset)
    for T, k, p in PARAMS:
        k = _clamp_k(k, V)
        check_tokens(lambda: sample_last(x, T, k, p, seed=seed, offset=offset), ref, (T, k, p),
                     f"V={V} R={R} scale={scale} {_pid((T, k, p))}")


@pytest.mark.parametrize("params", PARAMS, ids=_pid)
def test_distribution_chi_square(params):
    """16384 draws from one row in one call against the fp64 softmax over the kept set: Pearson's chi-square
    below the Laurent-Massart bound at 1e-6, and never a token outside the kept set."""
    from lightning_thunder_amd.ops.sampling import sample_last

    T, k, p = params
    V, R = 37, 16384
    k = _clamp_k(k, V)
    row = _logits(1, V, 2.0, F32, 99)
    tok = sample_last(row.repeat(R, 1), T, k, p, seed=2024, offset=4096)
    ref = Reference(row, 0, 0)
    keep = ref.kept(_f32(T), k, None if p is None else _f32(p))[0]
    prob = torch.softmax((row[0].double() / _f32(T)).masked_fill(~keep, -INF), -1)
    counts = torch.bincount(tok, minlength=V).double()
    assert not counts[~keep].any(), f"drew {counts[~keep].nonzero().flatten().tolist()} outside the kept set"
    exp = prob[keep] * R
    obs = counts[keep]
    order = torch.argsort(exp)
    exp, obs = exp[order].tolist(), obs[order].tolist()
    while len(exp) > 1 and exp[0] < 5:  # merge the smallest cells until every expectation reaches 5
        exp[1] += exp[0]
        obs[1] += obs[0]
        exp, obs = exp[1:], obs[1:]
        pairs = sorted(zip(exp, obs))
        exp, obs = [a for a, _ in pairs], [b for _, b in pairs]
    d = len(exp) - 1
    chi2 = sum((o - e) ** 2 / e for o, e in zip(obs, exp))
    x = math.log(1e6)
    bound = d + 2 * math.sqrt(d * x) + 2 * x
    print(f"[sampling chi2 {_pid(params)}] cells={d + 1} chi2={chi2:.2f} bound={bound:.2f}")
    assert chi2 <= bound, f"chi-square {chi2:.2f} > {bound:.2f} with {d} degrees of freedom"


def _drawn(sample, row, R, T, k, p, seed=11):
    """The set of tokens drawn from R copies of ``row`` in one call."""
    return set(sample(row[None].repeat(R, 1), T, k, p, seed=seed, offset=0).cpu().tolist())


def _planted_rows(V, nv):
    """(name, {index: value}, T, top_k, top_p, the exact set of drawable tokens) for a row of V >= 37 random
    values in [-4, 4] read as vectors of ``nv``.  The planted values hold all the mass that matters, and the
    threshold or a tie sits at each of: a vector-body / scalar-tail boundary, two waves, two loads of one lane
    (the index choices of test_decode_kernels._argmax_scenarios)."""
    nvec = V // nv
    body = nvec * nv
    triples = [("neighbours", (V - 3, V - 2, V - 1), 0)]
    if body < V and nvec >= 1:
        triples.append(("body_tail", (body - 2, body - 1, body), 1))
    if nvec > 1024 + 5:
        triples.append(("two_waves", (70 * nv + 1, (1024 + 5) * nv, 3), 0))
        triples.append(("same_lane", (5 * nv + 2, (1024 + 5) * nv + 2, 9), 1))
    out = []
    for name, (a, b, c), top in triples:
        hi = 20 + top  # an index outside every triple
        # 10 > 9 > 8 = 8 = 8: the tie straddles rank 3, all five stay drawable
        out.append((f"tie_at_rank_k/{name}", {hi: 10.0, hi + 2: 9.0, a: 8.0, b: 8.0, c: 8.0}, 1.0, 3, None,
                    {hi, hi + 2, a, b, c}))
        # 2 > +0 = -0 and everything else negative: rank 2 is a zero, both zeros stay
        out.append((f"signed_zeros/{name}", {a: 2.0, b: 0.0, c: -0.0, "negative": True}, 1.0, 2, None, {a, b, c}))
        # masses e^2 : 1 : 1 : 1 (the rest below e^-44): 0.8 of the mass is reached inside the tie, kept whole
        out.append((f"tie_at_top_p/{name}", {hi: 52.0, a: 50.0, b: 50.0, c: 50.0}, 1.0, None, 0.8, {hi, a, b, c}))
        out.append((f"top_k_1/{name}", {b: 9.0}, 0.8, 1, None, {b}))
        out.append((f"tiny_top_p/{name}", {c: 9.0}, 1.5, None, 1e-6, {c}))
        out.append((f"minus_inf_never_drawn/{name}", {a: 1.0, b: 1.5, c: 0.5, "fill": -INF}, 1.0, None, None, {a, b, c}))
        out.append((f"first_nan/{name}", {b: NAN, c: NAN, hi: INF}, 1.0, 5, 0.9, {min(b, c)}))
        out.append((f"first_pos_inf/{name}", {b: INF, c: INF, hi: 100.0}, 1.0, 5, 0.9, {min(b, c)}))
    out.append(("all_minus_inf", {"fill": -INF}, 1.0, 5, 0.9, {0}))
    return out


def _plant(base, plant, dtype):
    row = base.clone()
    if plant.get("negative"):
        row = -row.abs() - 1
    if "fill" in plant:
        row[:] = plant["fill"]
    for j, val in plant.items():
        if not isinstance(j, str):
            row[j] = val
    return row.to(dtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_dt_id)
def test_planted_cases_fallback(dtype):
    from lightning_thunder_amd.ops.sampling import sample_last

    V = 37
    base = _logits(1, V, 1.0, F32, 5)[0].clamp_(-4, 4)
    for name, plant, T, k, p, want in _planted_rows(V, 16 // torch.empty(0, dtype=dtype).element_size()):
        got = _drawn(sample_last, _plant(base, plant, dtype), 512, T, k, p)
        assert got == want, f"{name}: drew {sorted(got)}, drawable {sorted(want)}"
    one = torch.randn(5, 1).to(dtype)
    assert sample_last(one, 0.7, 3, 0.5, seed=1, offset=0).tolist() == [0] * 5  # V = 1


def test_stream_handling():
    from lightning_thunder_amd.ops.sampling import sample_last

    R, V = 32, 37
    x = _logits(1, V, 1.0, F32, 3).repeat(R, 1)
    a = sample_last(x, 1.0, seed=5, offset=100)
    assert torch.equal(a, sample_last(x, 1.0, seed=5, offset=100))
    assert not torch.equal(a, sample_last(x, 1.0, seed=5, offset=101))
    assert not torch.equal(a, sample_last(x, 1.0, seed=6, offset=100))
    assert len(set(a.tolist())) > 1, "identical rows of one call must not share their uniforms"
    # without a seed: the project's counter stream, which follows torch.manual_seed
    torch.manual_seed(77)
    seed, off0 = rng.peek_seed_offset()
    b1, b2 = sample_last(x, 1.0, 5, 0.9), sample_last(x, 1.0, 5, 0.9)
    assert rng.peek_seed_offset() == (seed, off0 + 2 * R * 40)  # V4 = 40 counters per row
    assert torch.equal(b1, sample_last(x, 1.0, 5, 0.9, seed=seed, offset=off0))
    assert torch.equal(b2, sample_last(x, 1.0, 5, 0.9, seed=seed, offset=off0 + R * 40))
    torch.manual_seed(77)
    assert torch.equal(b1, sample_last(x, 1.0, 5, 0.9)) and torch.equal(b2, sample_last(x, 1.0, 5, 0.9))
    # shapes: leading dimensions are kept, keepdim adds the last one back
    x3 = x.reshape(4, 8, V)
    assert sample_last(x3, 1.0, seed=5, offset=100).shape == (4, 8)
    assert torch.equal(sample_last(x3, 1.0, seed=5, offset=100, keepdim=True), a.reshape(4, 8, 1))


def test_argument_validation():
    from lightning_thunder_amd.ops.sampling import argmax_last, sample_last

    x = _logits(3, 37, 2.0, F32, 1)
    for bad in (dict(temperature=-0.5), dict(temperature=INF), dict(temperature=NAN),
                dict(temperature=1.0, top_k=0), dict(temperature=1.0, top_k=-3),
                dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=1.5), dict(temperature=1.0, top_p=-0.1),
                dict(temperature=1.0, top_p=NAN)):
        with pytest.raises(ValueError):
            sample_last(x, **bad)
    assert torch.equal(sample_last(x, 0.0, 5, 0.5), argmax_last(x))
    assert torch.equal(sample_last(x, 0, keepdim=True), argmax_last(x, keepdim=True))
    sample_last(x, 1.0, top_k=1000, top_p=1.0)  # a top_k beyond V and top_p = 1 filter nothing


def _tiny_gpt(device="cpu", dtype=torch.float32):
    from lightning_thunder_amd.models.litgpt import GPT, init_weights

    torch.manual_seed(0)
    m = GPT.from_name("llama3-like").to(device=device, dtype=dtype)
    init_weights(m, std=0.2)
    return m.requires_grad_(False)


def test_generate_samples_from_the_kept_set():
    from lightning_thunder_amd.models.litgpt import generate

    m = _tiny_gpt()
    B, T0, n = 2, 8, 10
    prompt = torch.randint(0, 300, (B, T0), generator=torch.Generator().manual_seed(1))
    outs = []
    for _ in range(2):
        m.set_kv_cache(B, 64)
        torch.manual_seed(123)
        outs.append(generate(m, prompt, n, temperature=0.8, top_k=5, top_p=0.9))
    out = outs[0]
    assert out.shape == (B, T0 + n) and out.dtype == torch.int64 and torch.equal(out[:, :T0], prompt)
    assert torch.equal(outs[0], outs[1]), "torch.manual_seed must reproduce the sampled tokens"
    torch.manual_seed(124)
    m.set_kv_cache(B, 64)
    assert not torch.equal(out, generate(m, prompt, n, temperature=0.8, top_k=5, top_p=0.9))
    # every token lies in its step's kept set, recomputed from a full forward over the generated prefix
    logits = m(out[:, :-1])  # [B, T0 + n - 1, V]
    for i in range(n):
        keep = Reference(logits[:, T0 + i - 1], 0, 0).kept(_f32(0.8), 5, _f32(0.9))
        tok = out[:, T0 + i]
        assert keep.gather(-1, tok[:, None]).all(), f"step {i}: token {tok.tolist()} outside the kept set"
        assert keep.sum(-1).max() <= 5


# ------------------------------------------------------------------------------------------------
# GPU: the kernel
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def sample_spy(monkeypatch):
    import lightning_thunder_amd.ops.sampling  # noqa: F401  (registers the signature on the real entry first)
    from lightning_thunder_amd.ops import require

    lib = require()
    real = lib.lta_sample_rows
    calls = []

    def spy(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "lta_sample_rows", spy)
    return calls


def _strided_cuda(rows, dtype):
    """rows [R, V] -> the same values on the GPU with row stride (V + 8) // 8 * 8; the slack columns hold
    1000.0, which would win every draw if it were read."""
    R, V = rows.shape
    ld = (V + 8) // 8 * 8
    buf = torch.full((R, ld), 1000.0, dtype=dtype)
    buf[:, :V] = rows.to(dtype)
    x = buf.cuda()[:, :V]
    assert x.stride(0) == ld and x.data_ptr() % 16 == 0
    return x


def _kernel_case(V, R, dtype, sample_spy, seed0):
    from lightning_thunder_amd.ops.sampling import sample_last

    inputs = [(f"randn*{s}", _logits(R, V, s, dtype, seed0 + i)) for i, s in enumerate(SCALES)]
    inputs.append(("negative only", (-_logits(R, V, 2.0, F32, seed0 + 9).abs() - 1).to(dtype)))
    seed, offset = 4321 + V, (1 << 33) + 12 * R  # an offset beyond 32 bits: both counter words are used
    for name, rows in inputs:
        ref = Reference(rows, seed, offset)
        x = _strided_cuda(rows, dtype)
        for T, k, p in PARAMS:
            k = _clamp_k(k, V)

            def got():
                n = len(sample_spy)
                tok = sample_last(x, T, k, p, seed=seed, offset=offset)
                assert len(sample_spy) == n + 1, "the kernel was not launched"
                return tok

            check_tokens(got, ref, (T, k, p), f"V={V} R={R} {_dt_id(dtype)} {name} {_pid((T, k, p))}")


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_dt_id)
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("V", [1, 7, 8, 9, 37, 8195, 32003, 65544, 128259])
def test_kernel_matches_reference(V, R, dtype, sample_spy):
    _kernel_case(V, R, dtype, sample_spy, V * 16 + R)


@gpu
def test_kernel_matches_reference_64_rows(sample_spy):
    _kernel_case(32003, 64, BF16, sample_spy, 640)


@gpu
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=_dt_id)
@pytest.mark.parametrize("V", [37, 8251])
def test_planted_cases_kernel(V, dtype, sample_spy):
    from lightning_thunder_amd.ops.sampling import sample_last

    base = _logits(1, V, 1.0, F32, 5)[0].clamp_(-4, 4)
    R = 512

    def sample(rows, T, k, p, **kw):
        n = len(sample_spy)
        tok = sample_last(_strided_cuda(rows, dtype), T, k, p, **kw)
        assert len(sample_spy) == n + 1, "the kernel was not launched"
        return tok

    for name, plant, T, k, p, want in _planted_rows(V, 16 // torch.empty(0, dtype=dtype).element_size()):
        got = _drawn(sample, _plant(base, plant, dtype), R, T, k, p)
        assert got == want, f"{name}: drew {sorted(got)}, drawable {sorted(want)}"
    assert sample(torch.randn(5, 1), 0.7, 3, 0.5, seed=1, offset=0).tolist() == [0] * 5  # V = 1


@gpu
@pytest.mark.parametrize("params", PARAMS, ids=_pid)
def test_kernel_is_deterministic(params, sample_spy):
    from lightning_thunder_amd.ops.sampling import sample_last

    T, k, p = params
    x = _strided_cuda(_logits(3, 128259, 2.0, BF16, 17), BF16)
    a = sample_last(x, T, k, p, seed=9, offset=1 << 20)
    for _ in range(3):
        assert torch.equal(a, sample_last(x, T, k, p, seed=9, offset=1 << 20))
    assert len(sample_spy) == 4


@gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_dt_id)
def test_misaligned_rows_take_the_fallback(dtype, sample_spy):
    from lightning_thunder_amd.ops.sampling import sample_last

    rows = _logits(3, 32003, 2.0, dtype, 23)
    x = rows.cuda()  # row stride 32003: rows are not 16-byte aligned
    ref = Reference(rows, 31, 64)
    for T, k, p in PARAMS:
        check_tokens(lambda: sample_last(x, T, k, p, seed=31, offset=64), ref, (T, k, p), f"misaligned {_pid((T, k, p))}")
    assert len(sample_spy) == 0, "rows that are not 16-byte aligned must not reach the kernel"


@gpu
def test_generate_gpu_samples_with_the_kernel(sample_spy):
    import lightning_thunder_amd as thunder
    from lightning_thunder_amd.models.litgpt import generate
    from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

    m = _tiny_gpt("cuda", BF16)
    prompt = torch.randint(0, 300, (1, 8), device="cuda")
    m.set_kv_cache(1, 64)
    jm = thunder.jit(m, transforms=[HipGraphTransform()])
    n = 12
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        calls = len(sample_spy)
        outs.append(generate(m, prompt, n, forward=jm, temperature=0.8, top_k=50, top_p=0.9))
        assert len(sample_spy) == calls + n, "one sampling kernel per new token"
    torch.cuda.synchronize()
    assert outs[0].shape == (1, 8 + n) and torch.equal(outs[0][:, :8], prompt)
    assert torch.equal(outs[0], outs[1]), "torch.manual_seed must reproduce the sampled tokens"
