"""Decode attention at head dim 256 (csrc/decode_attention_wide.h): every cache format and key selector against fp64
at all four launch shapes, the wrappers' admission, and a head-dim-256 model's decode steps under the compiler.

Keys outside a row's live range are NaN / 0x7F and dead table entries point outside the pool, so a finite result
within tolerance shows that nothing dead was read.  Two equalities hold bit for bit by construction (one kernel, other
addresses): paged = positions over ``gather_pages``, and a window that covers the cache = no window."""
import copy

import pytest
import torch

import lightning_thunder_amd as thunder
from kernel_checks import BF16, F16, F32, _dt_id, assert_within, bits_equal, nan_padded
from test_decode_kernels import ref_attention
from test_decode_pos_kernels import LAUNCH_SHAPES, _kv_case, _poisoned, _position_sets
from test_ragged_generate import FORMATS as CACHE_FORMATS, _model

from lightning_thunder_amd.ops import attention as A
from lightning_thunder_amd.ops.kv_pages import gather_pages, write_slots
from lightning_thunder_amd.ops.kv_rows import position_mask, window_mask

gpu = pytest.mark.gpu
U8, I64 = torch.uint8, torch.int64
D, PAGE, WINDOW = 256, 16, 24
WRAPPER = {"16bit": "decode_attn", "kv8": "decode_attn_kv8", "kv8s": "decode_attn_kv8s"}
SELECTORS = ["mask", "pos", "paged", "pos_win", "paged_win"]
CASES = [(s, BF16) for s in LAUNCH_SHAPES] + [("wsplit_split_t3", F16)]


def _tables(B, S, live):
    """A shuffled block table [B, S / 16] over ``B * S / 16 + 3`` pages, the same with the entry of every page that
    holds no ``live`` [B, S] key replaced by -1 or the page count, and that count."""
    P = S // PAGE
    num_pages = B * P + 3
    table = torch.randperm(num_pages, generator=torch.Generator().manual_seed(S))[:B * P].view(B, P).cuda()
    holes = torch.where(torch.arange(P, device="cuda") % 2 == 0, -1, num_pages).expand(B, P)
    return table, torch.where(live.view(B, P, PAGE).any(dim=2), table, holes), num_pages


@gpu
@pytest.mark.parametrize("sel", SELECTORS)
@pytest.mark.parametrize("fmt", list(WRAPPER))
@pytest.mark.parametrize("shape,dtype", CASES, ids=[f"{s}-{_dt_id(t)}" for s, t in CASES])
def test_decode_attn_d256_against_fp64(shape, dtype, fmt, sel):
    (B, Hq, Hkv, T, S), launch = LAUNCH_SHAPES[shape]
    assert A.decode_launch_shape(B * Hq * T, S)[:2] == launch and S % PAGE == 0
    kind, W = sel.split("_")[0], WINDOW if sel.endswith("_win") else None
    q, caches, exact = _kv_case(B, Hq, Hkv, T, S, D, dtype, fmt, seed=S)
    q = nan_padded(q.cuda())
    by_pos, paged = getattr(A, WRAPPER[fmt] + "_pos"), getattr(A, WRAPPER[fmt] + "_paged")
    for n, pos in enumerate(_position_sets(B, T, S)):
        what = f"{shape} {fmt} {sel} set {n}"
        posg = pos.cuda()
        mask = position_mask(posg, S) if W is None else window_mask(posg, S, W)
        live = mask.any(dim=2)[:, 0]  # [B, S]: the keys some row of the sequence attends
        dead = ~live[:, None, :, None]
        cg, (k, v) = _poisoned(caches, exact, pos, fmt)
        for c in cg:  # the keys below every window as well; scale bytes stay valid exponents
            if c.shape[-1] > 1:
                c.masked_fill_(dead, 0x7F if c.dtype == U8 else float("nan"))
        k, v = k.masked_fill(dead, 0.0), v.masked_fill(dead, 0.0)
        if kind == "mask":
            out = getattr(A, WRAPPER[fmt])(q, *cg, mask)
        elif kind == "pos":
            run = lambda window: by_pos(q, *cg, posg, None, window=window)  # noqa: E731
        else:
            table, holed, num_pages = _tables(B, S, live)
            j = torch.arange(S, device="cuda")
            slots = table[:, j // PAGE] * PAGE + j % PAGE
            pools = [write_slots(torch.full((Hkv, num_pages * PAGE + 1, c.shape[3]),
                                            float("nan") if c.is_floating_point() else 0x7F if c.shape[3] > 1 else 127,
                                            dtype=c.dtype, device="cuda"), slots, c) for c in cg]
            run = lambda window: paged(q, *pools, posg, holed, PAGE, num_pages, None, window=window)  # noqa: E731
        if kind != "mask":
            out = run(W)
            if W is None:
                assert bits_equal(out, run(S)), f"{what}: a window that covers the cache differs from none"
        if kind == "paged":
            static = by_pos(q, *[gather_pages(p, table, PAGE) for p in pools], posg, None, window=W)
            assert bits_equal(out, static), f"{what}: differs from the position kernel over gather_pages"
        assert out.dtype == dtype and out.shape == q.shape and out.is_contiguous()
        assert torch.isfinite(out).all(), f"{what}: a dead key was consumed"
        ref64 = ref_attention(q, k, v, mask, False, D ** -0.5)
        ref32 = ref_attention(q, k, v, mask, False, D ** -0.5, F32)
        assert_within(out, ref64, ref32, dtype, f"decode attention D256 {fmt} {sel}", what)


def _admission_operands(hd):
    """{wrapper name: its operands} at head dim ``hd`` for the nine decode wrappers (2 sequences, 4 heads on 2)."""
    z = lambda *shape, dtype=BF16: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    q, pos, table = z(2, 4, 1, hd), z(2, 1, dtype=I64), torch.arange(8, device="cuda").view(2, 4)
    k, k8, s = z(2, 2, 64, hd), z(2, 2, 64, hd, dtype=U8), z(2, 2, 64, 1, dtype=U8)
    kp, k8p, sp = z(2, 129, hd), z(2, 129, hd, dtype=U8), z(2, 129, 1, dtype=U8)
    ops = {}
    for name, static, pools in (("decode_attn", (k, k), (kp, kp)), ("decode_attn_kv8", (k8, k8), (k8p, k8p)),
                                ("decode_attn_kv8s", (k8, k8, s, s), (k8p, k8p, sp, sp))):
        ops[name] = (q, *static)
        ops[name + "_pos"] = (q, *static, pos)
        ops[name + "_paged"] = (q, *pools, pos, table, PAGE, 8)
    return ops


@gpu
def test_d256_admission():
    for name, operands in _admission_operands(D).items():
        if name != "decode_attn":  # the plain mask wrapper has no predicate: the entry decides
            assert getattr(A, name + "_supported")(*operands), name
        if name.endswith(("_pos", "_paged")):
            assert not getattr(A, name.replace("decode", "prefill") + "_supported")(*operands), name
    for name, operands in _admission_operands(192).items():
        with pytest.raises((ValueError, RuntimeError)):
            getattr(A, name)(*operands)


E2E_LENGTHS, E2E_STEPS, E2E_CACHE = (40, 9), 20, 128
_MASK_OPS = ("kv_position_mask", "kv_window_mask", "kv_paged_mask", "kv_paged_window_mask", "kv_paged_gather")


def _teacher_forced(m, forward, prompt, steps):
    """fp64 logits [B, E2E_STEPS, V] of the decode steps that feed ``steps`` [B, E2E_STEPS] after the padded prompt."""
    dev = prompt.device
    pages = getattr(m, "kv_pages", None)
    held = list(E2E_LENGTHS)
    T = prompt.shape[1]
    if pages is None:
        forward(prompt, torch.arange(T, device=dev))
    else:
        pages.reset()
        pages.reserve(held)
        forward(prompt, torch.arange(T, device=dev).expand(len(held), T).contiguous())
    pos = torch.tensor(E2E_LENGTHS, device=dev).view(-1, 1)
    logits = []
    for i in range(E2E_STEPS):
        if pages is not None:
            held = [n + 1 for n in held]
            pages.reserve(held)
        logits.append(forward(steps[:, i:i + 1], pos)[:, -1].double().cpu())
        pos.add_(1)
    return torch.stack(logits, dim=1)


@gpu
@pytest.mark.parametrize("window", [False, True], ids=["global", "window24"])
@pytest.mark.parametrize("route,fmt", [("ragged", "16bit"), ("paged", "e4m3_row")])
def test_gemma_like_decode_steps_against_fp64(route, fmt, window, monkeypatch):
    """Measured on an MI355X (worst |logit - fp64| over the 20 steps, new kernel / ATen path): see the README's
    "Decode at head dim 256" section; both figures are printed."""
    from lightning_thunder_amd.transforms.hipgraph import HipGraphTransform

    kw = dict(sliding_window_size=WINDOW, sliding_window_indices=[1, 0]) if window else {}
    m = _model("gemma-like", device="cuda", **kw).to(BF16)
    m64 = copy.deepcopy(m).to(device="cpu", dtype=torch.float64)
    g = torch.Generator().manual_seed(8)
    prompt = torch.randint(1, 300, (len(E2E_LENGTHS), max(E2E_LENGTHS)), generator=g)
    steps = torch.randint(1, 300, (len(E2E_LENGTHS), E2E_STEPS), generator=g)
    m64.set_kv_cache(len(E2E_LENGTHS), E2E_CACHE)
    ref = _teacher_forced(m64, m64, prompt, steps)

    def compiled():
        paging = dict(page_size=PAGE) if route == "paged" else {}
        m.set_kv_cache(len(E2E_LENGTHS), E2E_CACHE, device=torch.device("cuda"), **paging, **CACHE_FORMATS[fmt])
        jm = thunder.jit(m, transforms=[HipGraphTransform()])
        out = _teacher_forced(m, jm, prompt.cuda(), steps.cuda())
        names = [s.sym.name for b in thunder.last_traces(jm)[-1].bound_symbols
                 for s in (b.subsymbols if b.sym.name.startswith("HipGraph") else [b])]
        return (out - ref).abs().max().item(), names

    err, names = compiled()
    attn = [n for n in names if n.startswith("hip_decode_attn")]
    assert len(attn) == 2 and [n.endswith("_win") for n in attn] == [window, False], names
    assert not any(w in n for n in names for w in _MASK_OPS), names
    monkeypatch.setenv("LTA_DECODE_D256", "0")
    err_aten, names_aten = compiled()
    assert not any(n.startswith("hip_decode_attn") for n in names_aten), names_aten
    print(f"[decode D256 {route} {fmt} window={window}] max |logits - fp64|: kernel {err:.4e}, ATen path {err_aten:.4e}")
    # both are bf16 programs that differ in the order of the fp32 sums inside one attention: reordering, nothing larger
    assert err <= 2 * err_aten, (err, err_aten)
