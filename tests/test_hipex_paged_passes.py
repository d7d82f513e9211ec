"""The rewrites of a paged KV cache's decode step in ``hipex._post_claim``, on hand-built traces (the shape of
``test_hipex_pos_passes.py``): slot writes into the RoPE (``hip_qkv_rope_cache_slots`` / ``_slots_s8``) and the page
gathers and paged mask into the decode attention (``hip_decode_attn_paged`` and its two e4m3 forms), for the three
cache formats, with their refusals and the ``LTA_KV_PAGED_FUSION=0`` switch."""
import pytest
import torch

from lightning_thunder_amd import torch as lt
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.ops.kv8 import kv8_dequantise_rows, kv8_quantise_rows
from lightning_thunder_amd.ops.kv_pages import kv_page_slots, kv_paged_gather, kv_paged_mask
from lightning_thunder_amd.torch.custom_op import custom_op_symbol, opdef_of
from lightning_thunder_amd.transforms.inplace_index_copy import index_copy_inplace
from test_hipex_passes import Program, unchanged

BF16, U8, I64, F8 = torch.bfloat16, torch.uint8, torch.int64, torch.float8_e4m3fn
QUANTISE, DEQUANTISE = custom_op_symbol(opdef_of(kv8_quantise_rows)), custom_op_symbol(opdef_of(kv8_dequantise_rows))
GATHER, MASK = custom_op_symbol(opdef_of(kv_paged_gather)), custom_op_symbol(opdef_of(kv_paged_mask))
SLOTS = custom_op_symbol(opdef_of(kv_page_slots))
B, T, H, D = 3, 1, 4, 64
PAGE, PAGES, MAXP = 16, 5, 2
R, S = PAGE * PAGES, PAGE * MAXP
FORMATS = ["16bit", "e4m3", "e4m3_row"]
_KV = "hipex: 1 KV-cache write pair(s) fused into RoPE"
_READ = "hipex: 2 decode attention(s) read their paged KV cache through the block table"


def test_the_symbols_are_the_ones_the_passes_match():
    assert GATHER.id in hipex._KV_PAGED_GATHER_IDS and MASK.id in hipex._KV_PAGED_MASK_IDS


def _e4m3_chain(p, t, tag):
    c, f, u = p.t(tag + "_c", B, H, T, D), p.t(tag + "_f", B, H, T, D, dtype=F8), p.t(tag + "_u", B, H, T, D, dtype=U8)
    p(lt.clamp, t, -448.0, 448.0, out=c)
    p(lt.to, c, F8, out=f)
    p(lt.view, f, U8, out=u)
    return u


def _relayout(p, t, tag, case=None):
    d, dt = t.shape[-1], t.dtype
    r = p.t(tag + "_r", H, B * T, d, dtype=dt)
    if case == "other_permute" and tag == "k":
        a = p(lt.permute, t, 1, 0, 3, 2, out=p.t(tag + "_p", H, B, d, T, dtype=dt))
    else:
        a = p(lt.permute, t, 1, 0, 2, 3, out=p.t(tag + "_p", H, B, T, d, dtype=dt))
    p(lt.reshape, a, H, B * T, d, out=r)
    return r


def _write_program(fmt, case=None):
    p = Program()
    slots, slots2 = p.ts("slots slots2", B, T, dtype=I64)
    flat, flat2 = p.ts("flat flat2", B * T, dtype=I64)
    qkv = p.t("qkv", B, T, 3 * H * D)
    cos, sin = p.ts("cos sin", B, T, D)
    q, k, v = p.ts("q k v", B, H, T, D)
    cdt = BF16 if fmt == "16bit" else U8
    kp, vp, kp2, vp2 = p.ts("kp vp kp2 vp2", H, R + 1, D, dtype=cdt)
    p(lt.reshape, slots, -1, out=flat)
    if case == "other_slots":
        p(lt.reshape, slots2, -1, out=flat2)
    p(hipex.hip_qkv_rope, qkv, cos, sin, H, H, D, D, out=(q, k, v))
    extra, outs = [], [kp2, vp2]
    if case == "k_read_twice":
        extra.append(p(lt.neg, k, out=p.t("s", B, H, T, D)))
    if fmt == "16bit":
        ksrc, vsrc, scales = k, v, ()
    elif fmt == "e4m3":
        ksrc, vsrc, scales = _e4m3_chain(p, k, "k"), _e4m3_chain(p, v, "v"), ()
    else:
        k8, v8 = p.ts("k8 v8", B, H, T, D, dtype=U8)
        ks, vs = p.ts("ks vs", B, H, T, 1, dtype=U8)
        p(QUANTISE, k, out=(k8, ks))
        p(QUANTISE, v, out=(v8, vs))
        ksrc, vsrc, scales = k8, v8, (ks, vs)
    p(index_copy_inplace, kp, 2 if case == "other_dim" else 1, flat, _relayout(p, ksrc, "k", case), out=kp2)
    p(index_copy_inplace, vp, 1, flat2 if case == "other_slots" else flat, _relayout(p, vsrc, "v", case), out=vp2)
    if scales:
        ksp, vsp, ksp2, vsp2 = p.ts("ksp vsp ksp2 vsp2", H, R + 1, 1, dtype=U8)
        p(index_copy_inplace, ksp, 1, flat, _relayout(p, scales[0], "ks"), out=ksp2)
        p(index_copy_inplace, vsp, 1, flat, _relayout(p, scales[1], "vs"), out=vsp2)
        outs += [ksp2, vsp2]
    return p.run(q, *outs, *extra)


@pytest.mark.parametrize("fmt", FORMATS)
def test_slot_writes_fused_into_the_rope(fmt):
    """The relayouts, the writes and ``reshape(slots, -1)`` (its last reader gone) leave; one operator stays."""
    want = {"16bit": "q, kp2, vp2 = hip_qkv_rope_cache_slots(qkv, cos, sin, 4, 4, 64, 64, kp, vp, slots)",
            "e4m3": "q, kp2, vp2 = hip_qkv_rope_cache_slots(qkv, cos, sin, 4, 4, 64, 64, kp, vp, slots)",
            "e4m3_row": "q, kp2, vp2, ksp2, vsp2 = hip_qkv_rope_cache_slots_s8(qkv, cos, sin, 4, 4, 64, 64, kp, vp, ksp, "
                        "vsp, slots)"}[fmt]
    assert _write_program(fmt) == ([want], _KV)


@pytest.mark.parametrize("case", ["k_read_twice", "other_slots", "other_dim", "other_permute"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_slot_writes_refused(fmt, case):
    """k read twice, slots differing between k and v, a write along another dim, another relayout."""
    unchanged(_write_program(fmt, case))


@pytest.mark.parametrize("fmt", FORMATS)
def test_slot_write_fusion_switch(fmt, monkeypatch):
    monkeypatch.setenv("LTA_KV_PAGED_FUSION", "0")
    unchanged(_write_program(fmt))


def test_written_args_of_the_slot_writes_are_the_pools():
    assert hipex.hip_qkv_rope_cache_slots.written_args == (7, 8)
    assert hipex.hip_qkv_rope_cache_slots_s8.written_args == (7, 8, 9, 10)
    for op in (hipex.hip_qkv_rope_cache_slots, hipex.hip_qkv_rope_cache_slots_s8):
        assert hipex.OpTags.DONT_DCE in op.tags and hipex.OpTags.IN_PLACE in op.tags


def _pool_reads(p, fmt, layer, table, case):
    """The k / v operands of a layer's attention as the model spells them over its pools, the fused names, and the
    extra outputs of the case."""
    n = str(layer)
    hit = layer == 1  # the refusal cases change the second layer only
    table_v = p.t("table2", B, MAXP, dtype=I64) if case == "other_table" and hit else table
    extra = []

    def gather(name, d, dtype, tab=table, written=False):
        pool, g = p.t(name, H, R + 1, d, dtype=dtype), p.t("g" + name, B, H, S, d, dtype=dtype)
        p(GATHER, pool, tab, PAGE, out=g)
        if written:  # the pool is written in place between its gather and the attention
            extra.append(p(index_copy_inplace, pool, 1, p.t("idx", B * T, dtype=I64), p.t("src", H, B * T, d, dtype=dtype),
                           out=p.t("w" + name, H, R + 1, d, dtype=dtype)))
        return g

    cdt = BF16 if fmt == "16bit" else U8
    gk = gather(f"kp{n}", D, cdt, written=case == "pool_written" and hit)
    gv = gather(f"vp{n}", D, cdt, table_v)
    if case == "gather_read_twice" and hit:
        extra.append(p(lt.neg, gk, out=p.t("s", B, H, S, D, dtype=cdt)))
    if fmt == "16bit":
        return gk, gv, f"kp{n}, vp{n}", extra
    kd, vd = p.ts(f"kd{n} vd{n}", B, H, S, D)
    if fmt == "e4m3":
        kf, vf = p.ts(f"kf{n} vf{n}", B, H, S, D, dtype=F8)
        p(lt.view, gk, F8, out=kf)
        p(lt.to, kf, BF16, out=kd)
        p(lt.view, gv, F8, out=vf)
        p(lt.to, vf, BF16, out=vd)
        return kd, vd, f"kp{n}, vp{n}", extra
    gks, gvs = gather(f"ksp{n}", 1, U8), gather(f"vsp{n}", 1, U8)
    p(DEQUANTISE, gk, gks, BF16, out=kd)
    p(DEQUANTISE, gv, gvs, BF16, out=vd)
    return kd, vd, f"kp{n}, vp{n}, ksp{n}, vsp{n}", extra


def _read_program(fmt, case=None):
    p = Program()
    pos = p.t("pos", B, T, dtype=I64)
    table = p.t("table", B, MAXP, dtype=I64)
    mask = p.t("mask", B, 1, T, S, dtype=torch.bool)
    p(MASK, pos, table, PAGE, PAGES, out=mask)
    outs, names = [], []
    for layer in range(2):
        q, o = p.ts(f"q{layer} o{layer}", B, 8, T, D)
        k, v, fused, extra = _pool_reads(p, fmt, layer, table, case)
        p(hipex.hip_decode_attn, q, k, v, mask, case == "causal" and layer == 1, 0.125, out=o)
        outs += [o, *extra]
        names.append(fused)
    if case == "mask_returned":
        outs.append(mask)
    return p.run(*outs), names


PAGED_OP = {"16bit": "hip_decode_attn_paged", "e4m3": "hip_decode_attn_kv8_paged", "e4m3_row": "hip_decode_attn_kv8s_paged"}


@pytest.mark.parametrize("fmt", FORMATS)
def test_paged_reads_fused_and_gathers_and_mask_dropped(fmt):
    (lines, msg), names = _read_program(fmt)
    assert lines == [f"o{n} = {PAGED_OP[fmt]}(q{n}, {names[n]}, pos, table, 16, 5, 0.125)" for n in range(2)], lines
    assert msg == _READ


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_mask_stays_for_another_reader(fmt):
    (lines, msg), names = _read_program(fmt, "mask_returned")
    assert lines[0].startswith("mask = ") and msg == _READ
    assert lines[1:] == [f"o{n} = {PAGED_OP[fmt]}(q{n}, {names[n]}, pos, table, 16, 5, 0.125)" for n in range(2)]


@pytest.mark.parametrize("case", ["other_table", "gather_read_twice", "pool_written", "causal"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_paged_reads_refused(fmt, case):
    """k and v at different tables, a gather read twice, a pool written in between, causal true: that layer keeps its
    gathers and the mask form (for the e4m3 caches with their own read fusion); the other layer is still folded."""
    (lines, msg), names = _read_program(fmt, case)
    text = "\n".join(lines)
    assert lines[0].startswith("mask = "), "the mask keeps a reader"
    assert f"o0 = {PAGED_OP[fmt]}(q0, {names[0]}, pos, table, 16, 5, 0.125)" in lines
    assert text.count("_paged(") == 1 and msg == _READ.replace("2 decode", "1 decode")
    plain = {"16bit": "hip_decode_attn", "e4m3": "hip_decode_attn_kv8", "e4m3_row": "hip_decode_attn_kv8s"}[fmt]
    (o1,) = [ln for ln in lines if ln.startswith("o1 = ")]
    assert o1.startswith(f"o1 = {plain}(q1, gkp1, gvp1, ") and o1.endswith(f"mask, {case == 'causal'}, 0.125)")
    assert "gkp1 = " in text and "gvp1 = " in text, "the refused layer's gathers stay"


@pytest.mark.parametrize("fmt", FORMATS)
def test_paged_read_fusion_switch(fmt, monkeypatch):
    monkeypatch.setenv("LTA_KV_PAGED_FUSION", "0")
    (lines, msg), _ = _read_program(fmt)
    if fmt == "16bit":
        assert (lines, msg) == (None, None)
    else:
        assert "_paged(" not in "\n".join(lines) and lines[0].startswith("mask = ")
        assert sum("kv_paged_gather" in ln for ln in lines) == (4 if fmt == "e4m3" else 8)
