"""Prefill attention at head dim 256 (csrc/prefill_attention_d256.hip, reached through the twelve
``lta_prefill_attn*`` entries): every cache format, static and paged, global and windowed, against fp64 with
``test_prefill_pos_kernels._check_fp64``'s tolerance; the wrappers' admission; a head-dim-256 model's prefill under
the compiler; and the compiler's rewrite on a hand-built trace (no GPU).

Every key row outside what a workgroup may stage is NaN / 0x7F and the caches and pools sit in guarded buffers, so a
finite result within tolerance shows that nothing dead was read.  The kernel defers the rescale of O, so it is held to
fp64 and not to the masked v1 forward's bits; what holds bit for bit whatever the order of the sums: each e4m3 form =
the 16-bit form over the dequantised cache, each paged form = the static form over ``gather_pages``, and a window that
covers the cache = no window.  Shapes are the smallest that reach every branch of a 32-key-tile, 128-row kernel."""
import copy

import pytest
import torch

import lightning_thunder_amd as thunder
from kernel_checks import BF16, F16, _dt_id, assert_guard_intact, bits_equal
from test_hipex_passes import Program, unchanged
from test_prefill_pos_kernels import CASES, _check_fp64, _positions as _plain_positions
from test_ragged_generate import FORMATS as CACHE_FORMATS, _model
from test_window_kernels import (FORMATS, PAGE, _entry, _holes, _launch, _Operands, _prefill_positions, _span,
                                 _static_16bit, _words, _wrapper, spy)  # noqa: F401

from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.ops import attention as A
from lightning_thunder_amd.ops.kv_pages import gather_pages, paged_mask, paged_window_mask
from lightning_thunder_amd.ops.kv_rows import kv_position_mask, position_mask, window_mask
from lightning_thunder_amd.torch.custom_op import custom_op_symbol, opdef_of

gpu = pytest.mark.gpu
I64 = torch.int64
D = 256
RUNS = [(name, (2, 4, 2), dtype) for name in CASES for dtype in (BF16, F16)] + [("mixed", (1, 4, 1), BF16)]


def _positions(name, B, T, S):
    """``test_prefill_pos_kernels._positions`` with the 32-key tile edges in the non-monotone set."""
    if name != "mixed":
        return _plain_positions(name, B, T, S)
    g = torch.Generator().manual_seed(T + S)
    special = torch.tensor([0, 31, 32, 63, 64, 127, 128, S - 1, -1, S + 5])  # tile edges, dead, clamped
    return torch.stack([torch.cat([special, torch.randint(0, S, (T - len(special),), generator=g)])
                        [torch.randperm(T, generator=g)] for _ in range(B)]).to(I64)


def _checked(ops, pos, live, mask, what, window=None, table=None):
    """One launch over the cache poisoned outside ``live`` [B, S]: the entry, finiteness, fp64 under ``mask``, the
    buffers untouched.  Returns (the output, the views it read, the dequantised cache with zeros at the dead keys)."""
    views, bufs, (k, v) = ops.poisoned(live)
    before = [b.clone() for b in bufs]
    out = _launch("prefill", ops.fmt, ops, views, pos, window, table=table)
    assert out.dtype == ops.dtype and out.shape == ops.q.shape and out.transpose(1, 2).is_contiguous()
    assert torch.isfinite(out).all(), f"{what}: a dead key was consumed"
    n_dead = _check_fp64(out, ops.q, k, v, mask, ops.dtype, what)
    for buf, old, view in zip(bufs, before, views):
        assert torch.equal(_words(buf), _words(old)), f"{what}: a cache buffer was written"
        if buf.dtype == torch.int16:
            assert_guard_intact(buf, view.shape, what)
    return out, views, ops.dequantised((k, v)), n_dead


def _fp64_and_other_forms(name, heads, dtype, fmt, paged, spy):  # noqa: F811
    (B, Hq, Hkv), (T, S) = heads, CASES[name]
    del spy[:]
    what = f"{name} {fmt} paged={paged} {_dt_id(dtype)}"
    ops = _Operands(B, Hq, Hkv, T, S, D, dtype, fmt, T + S, paged)
    pos = _positions(name, B, T, S).cuda()
    mask = position_mask(pos, S)
    out, views, (kd, vd), n_dead = _checked(ops, pos, mask.any(dim=2)[:, 0], mask, what)
    assert spy == [(_entry("prefill", fmt, paged, win=False),)], spy
    assert n_dead == int((pos < 0).sum()) and (n_dead > 0) == (name == "mixed")
    # the 16-bit static form over the dequantised (gathered) cache, zeros in place of the poison: the same LDS tiles
    ref16 = _static_16bit("prefill", ops.q, kd, vd, pos)
    assert bits_equal(out, ref16), f"{what}: {(out != ref16).sum().item()} elements differ from the 16-bit static form"
    # a window over the cache and over the clamped position past it (lo = p + 1 - window counts from the position)
    covered = _launch("prefill", fmt, ops, views, pos, max(S, int(pos.max()) + 1))
    assert spy[-1] == (_entry("prefill", fmt, paged),)
    assert bits_equal(out, covered), f"{what}: a window that covers the cache differs from none"
    if paged:
        static = _wrapper("prefill", fmt, False)(ops.q, *[gather_pages(p, ops.table, PAGE) for p in views], pos, None)
        assert bits_equal(out, static), f"{what}: differs from the static form over gather_pages"
        # table entries that are no page: a dropped one in the middle of sequence 0, one past the pool at the start
        holed = ops.table.clone()
        holed[0, holed.shape[1] // 2], holed[B - 1, 0] = -1, ops.num_pages
        mask = paged_mask(pos, holed, PAGE, ops.num_pages)
        _, _, _, more_dead = _checked(ops, pos, mask.any(dim=2)[:, 0], mask, what + " holes", table=holed)
        assert more_dead >= n_dead + int(((pos[B - 1] >= 0) & (pos[B - 1] < PAGE)).sum())
        assert mask[0, 0, :, (holed.shape[1] // 2 + 1) * PAGE:].any(), "keys behind the dropped page stay live"


@gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_d256_fp64(fmt, spy):  # noqa: F811
    """Every run of RUNS, static and paged (one test per format: the runs are a twentieth of a second each)."""
    for paged in (False, True):
        for name, heads, dtype in RUNS:
            _fp64_and_other_forms(name, heads, dtype, fmt, paged, spy)


def _window_run(W, fmt, paged, spy):  # noqa: F811
    """T = 160 (two workgroups) over S = 320: chunks at base 0 and 100 and a shuffled set, each with one dead row; every
    key outside the span of its sequence's windows is poisoned, and on a paged cache every table entry below it is -1
    or an id outside the pool in the run that is checked."""
    (B, Hq, Hkv), T, S = (2, 4, 2), 160, 320
    ops = _Operands(B, Hq, Hkv, T, S, D, BF16, fmt, T + W, paged)
    holes = 0
    for n_set, pos in enumerate(_prefill_positions(T)):
        what = f"W{W} {fmt} paged={paged} set {n_set}"
        pos, table, mask = pos.cuda(), None, window_mask(pos.cuda(), S, W)
        if paged:
            table, outside, n_holes = _holes(ops.table, pos, S, W, ops.num_pages)
            table = outside if n_set == 1 else table
            holes += n_holes
            assert torch.equal(mask, paged_window_mask(pos, table, PAGE, ops.num_pages, W))
        del spy[:]
        out, views, (kd, vd), n_dead = _checked(ops, pos, _span(pos, S, W), mask, what, W, table)
        assert spy == [(_entry("prefill", fmt, paged),)] and n_dead == 1
        ref16 = _static_16bit("prefill", ops.q, kd, vd, pos, W)
        assert bits_equal(out, ref16), f"{what}: {(out != ref16).sum().item()} elements differ from the 16-bit static form"
    assert holes > 0 or not paged


@gpu
@pytest.mark.parametrize("W", [1, 40])
def test_d256_window(W, spy):  # noqa: F811
    for fmt in FORMATS:
        for paged in (False, True):
            _window_run(W, fmt, paged, spy)


def _admission_operands(T):
    """{wrapper name: its operands} at head dim 256 and ``T`` rows for the six prefill wrappers."""
    z = lambda *shape, dtype=BF16: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    q, pos, table = z(2, 4, T, D), z(2, T, dtype=I64), torch.arange(8, device="cuda").view(2, 4)
    k, k8, s = z(2, 2, 64, D), z(2, 2, 64, D, dtype=torch.uint8), z(2, 2, 64, 1, dtype=torch.uint8)
    kp, k8p, sp = z(2, 129, D), z(2, 129, D, dtype=torch.uint8), z(2, 129, 1, dtype=torch.uint8)
    ops = {}
    for name, static, pools in (("prefill_attn", (k, k), (kp, kp)), ("prefill_attn_kv8", (k8, k8), (k8p, k8p)),
                                ("prefill_attn_kv8s", (k8, k8, s, s), (k8p, k8p, sp, sp))):
        ops[name + "_pos"] = (q, *static, pos)
        ops[name + "_paged"] = (q, *pools, pos, table, PAGE, 8)
    return ops


@gpu
def test_d256_admission(spy, monkeypatch):  # noqa: F811
    """17 rows are the prefill kernel's, 16 the decode kernels'; every wrapper launches its own entry, and the native
    ``*_win`` entry refuses ``window = 0`` at this head dim as at the others."""
    for name, operands in _admission_operands(17).items():
        assert getattr(A, name + "_supported")(*operands), name
        for window in (None, 5):
            del spy[:]
            assert not getattr(A, name)(*operands, window=window).any()  # zero values: zero output
            assert spy == [("lta_" + name + ("_win" if window else ""),)], spy
    for name, operands in _admission_operands(16).items():
        assert not getattr(A, name + "_supported")(*operands), name
        with pytest.raises(ValueError):
            getattr(A, name)(*operands)
    monkeypatch.setattr(A, "_window_arg", lambda fn, window: (window,))
    for name, operands in _admission_operands(17).items():
        with pytest.raises(RuntimeError, match=f"lta_{name}_win failed with HIP error code 1"):
            getattr(A, name)(*operands, window=0)


E2E_LENGTHS, E2E_CACHE, E2E_WINDOW, E2E_CHUNK = (40, 9), 128, 24, 24
_MASK_OPS = ("kv_position_mask", "kv_window_mask", "kv_paged_mask", "kv_paged_window_mask", "kv_paged_gather")


def _gemma_run(route, fmt, window, monkeypatch):
    """The prompt's logits (40 / 9 tokens, padded) of bf16 ``gemma-like``: the paged route in one forward, the static
    ragged route in chunks of 24 and 16 rows (the second is the decode kernel's).  Measured on an MI355X (worst |logit
    - fp64|, new kernel / LTA_PREFILL_D256=0): see the README's "Prefill at head dim 256"; both figures are printed."""
    kw = dict(sliding_window_size=E2E_WINDOW, sliding_window_indices=[1, 0]) if window else {}
    m = _model("gemma-like", device="cuda", **kw).to(BF16)
    m64 = copy.deepcopy(m).to(device="cpu", dtype=torch.float64)
    B, T = len(E2E_LENGTHS), max(E2E_LENGTHS)
    prompt = torch.randint(1, 300, (B, T), generator=torch.Generator().manual_seed(8))
    m64.set_kv_cache(B, E2E_CACHE)
    ref = m64(prompt, torch.arange(T))
    pos = torch.arange(T, device="cuda").expand(B, T).contiguous()

    def compiled():
        paging = dict(page_size=PAGE) if route == "paged" else {}
        m.set_kv_cache(B, E2E_CACHE, device=torch.device("cuda"), **paging, **CACHE_FORMATS[fmt])
        jm = thunder.jit(m)
        if route == "paged":
            m.kv_pages.reset()
            m.kv_pages.reserve(list(E2E_LENGTHS))
        chunk = T if route == "paged" else E2E_CHUNK
        first = jm(prompt[:, :chunk].cuda(), pos[:, :chunk])
        names = [b.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols]
        rest = [jm(prompt[:, chunk:].cuda(), pos[:, chunk:])] if chunk < T else []
        return (torch.cat([first, *rest], dim=1).double().cpu() - ref).abs().max().item(), names

    err, names = compiled()
    attn = [n for n in names if n.startswith("hip_prefill_attn")]
    assert len(attn) == 2 and [n.endswith("_win") for n in attn] == [window, False], names
    assert not any(w in n for n in names for w in _MASK_OPS), names
    monkeypatch.setenv("LTA_PREFILL_D256", "0")
    err_chain, names_chain = compiled()
    assert not any(n.startswith("hip_prefill_attn") for n in names_chain), names_chain
    print(f"[prefill D256 {route} {fmt} window={window}] max |logits - fp64|: kernel {err:.4e}, masked chain {err_chain:.4e}")
    # both are bf16 programs that differ in the order of the fp32 sums inside one attention: reordering, nothing larger
    assert err <= 2 * err_chain, (err, err_chain)


@gpu
@pytest.mark.parametrize("route,fmt", [("ragged", "16bit"), ("paged", "e4m3_row")])
def test_d256_gemma_like(route, fmt):
    """``_gemma_run`` plain and with a window of 24 on layer 0."""
    for window in (False, True):
        with pytest.MonkeyPatch.context() as mp:
            _gemma_run(route, fmt, window, mp)


def _trace_program(rows):
    """One layer at head dim 256 over a static 16-bit cache under ``kv_position_mask``, as ``_sdpa_exec`` claims it."""
    B, Hq, H, S = 2, 8, 1, 64
    p = Program()
    pos, mask = p.t("pos", B, rows, dtype=I64), p.t("mask", B, 1, rows, S, dtype=torch.bool)
    p(custom_op_symbol(opdef_of(kv_position_mask)), pos, S, out=mask)
    q, o = p.ts("q o", B, Hq, rows, D)
    k, v = p.ts("kc vc", B, H, S, D)
    if rows <= A.DECODE_MAX_QUERIES:
        p(hipex.hip_decode_attn, q, k, v, mask, False, 0.0625, out=o)
    else:
        p(hipex.hip_attn_fwd_ex, q, k, v, mask, False, 0.0625, 0.0, 0, 0, out=(o, p.t("lse", B, Hq, rows, dtype=torch.float32)))
    return p.run(o)


def test_d256_rewrite_cpu(monkeypatch):
    assert _trace_program(17)[0] == ["o = hip_prefill_attn_pos(q, kc, vc, pos, 0.0625)"]
    assert _trace_program(16)[0] == ["o = hip_decode_attn_pos(q, kc, vc, pos, 0.0625)"]
    monkeypatch.setenv("LTA_PREFILL_D256", "0")
    unchanged(_trace_program(17))
    assert _trace_program(16)[0] == ["o = hip_decode_attn_pos(q, kc, vc, pos, 0.0625)"]
