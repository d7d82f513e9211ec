"""The rewrites of a ragged batch's decode step in ``hipex._post_claim``, on hand-built traces (the way
``test_hipex_passes.py`` pins the other passes): per-row cache writes into the RoPE (``hip_qkv_rope_cache_rows`` /
``hip_qkv_rope_cache_rows_s8``) and the position mask into the decode attention (``hip_decode_attn_pos`` and its
two e4m3 forms), for the three cache formats, with their refusals and the ``LTA_KV_POS_FUSION=0`` switch."""
import pytest
import torch

from lightning_thunder_amd import torch as lt
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.ops.kv8 import kv8_dequantise_rows, kv8_quantise_rows
from lightning_thunder_amd.ops.kv_rows import kv_position_mask
from lightning_thunder_amd.torch.custom_op import custom_op_symbol, opdef_of
from lightning_thunder_amd.transforms.inplace_index_copy import index_copy_inplace, scatter_rows_inplace
from test_hipex_passes import Program, unchanged

BF16, U8, I64, F8 = torch.bfloat16, torch.uint8, torch.int64, torch.float8_e4m3fn
QUANTISE, DEQUANTISE = custom_op_symbol(opdef_of(kv8_quantise_rows)), custom_op_symbol(opdef_of(kv8_dequantise_rows))
MASK = custom_op_symbol(opdef_of(kv_position_mask))
B, T, S = 3, 1, 32
FORMATS = ["16bit", "e4m3", "e4m3_row"]
_KV = "hipex: 1 KV-cache write pair(s) fused into RoPE"


def test_the_mask_symbol_is_the_one_the_pass_matches():
    assert MASK.id in hipex._KV_POSITION_MASK_IDS


def _e4m3_chain(p, t, tag):
    c, f, u = p.t(tag + "_c", B, 4, T, 64), p.t(tag + "_f", B, 4, T, 64, dtype=F8), p.t(tag + "_u", B, 4, T, 64, dtype=U8)
    p(lt.clamp, t, -448.0, 448.0, out=c)
    p(lt.to, c, F8, out=f)
    p(lt.view, f, U8, out=u)
    return u


def _write_program(fmt, case=None):
    p = Program()
    pos, pos2 = p.ts("pos pos2", B, T, dtype=I64)
    qkv = p.t("qkv", B, T, 3 * 4 * 64)
    cos, sin = (p.ts("cos sin", T, 64) if case == "shared_cos" else p.ts("cos sin", B, T, 64))
    q, k, v = p.ts("q k v", B, 4, T, 64)
    cdt = BF16 if fmt == "16bit" else U8
    kc, vc, kc2, vc2 = p.ts("kc vc kc2 vc2", B, 4, S, 64, dtype=cdt)
    p(hipex.hip_qkv_rope, qkv, cos, sin, 4, 4, 64, 64, out=(q, k, v))
    extra, outs = [], [kc2, vc2]
    if case == "k_read_twice":
        extra.append(p(lt.neg, k, out=p.t("s", B, 4, T, 64)))
    if fmt == "16bit":
        ksrc, vsrc, scales = k, v, ()
    elif fmt == "e4m3":
        ksrc, vsrc, scales = _e4m3_chain(p, k, "k"), _e4m3_chain(p, v, "v"), ()
    else:
        k8, v8 = p.ts("k8 v8", B, 4, T, 64, dtype=U8)
        ks, vs = p.ts("ks vs", B, 4, T, 1, dtype=U8)
        p(QUANTISE, k, out=(k8, ks))
        p(QUANTISE, v, out=(v8, vs))
        ksrc, vsrc, scales = k8, v8, (ks, vs)
    if case == "index_copy_write":  # the shared-position write under per-token rotations
        p(index_copy_inplace, kc, 2, pos, ksrc, out=kc2)
    else:
        p(scatter_rows_inplace, kc, pos, ksrc, out=kc2)
    p(scatter_rows_inplace, vc, pos2 if case == "other_positions" else pos, vsrc, out=vc2)
    if scales:
        ksc, vsc, ksc2, vsc2 = p.ts("ksc vsc ksc2 vsc2", B, 4, S, 1, dtype=U8)
        p(scatter_rows_inplace, ksc, pos, scales[0], out=ksc2)
        p(scatter_rows_inplace, vsc, pos, scales[1], out=vsc2)
        outs += [ksc2, vsc2]
    return p.run(q, *outs, *extra)


@pytest.mark.parametrize("fmt", FORMATS)
def test_row_writes_fused_into_the_rope(fmt):
    want = {"16bit": "q, kc2, vc2 = hip_qkv_rope_cache_rows(qkv, cos, sin, 4, 4, 64, 64, kc, vc, pos)",
            "e4m3": "q, kc2, vc2 = hip_qkv_rope_cache_rows(qkv, cos, sin, 4, 4, 64, 64, kc, vc, pos)",
            "e4m3_row": "q, kc2, vc2, ksc2, vsc2 = hip_qkv_rope_cache_rows_s8(qkv, cos, sin, 4, 4, 64, 64, kc, vc, ksc, "
                        "vsc, pos)"}[fmt]
    assert _write_program(fmt) == ([want], _KV)


@pytest.mark.parametrize("case", ["k_read_twice", "other_positions", "shared_cos", "index_copy_write"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_row_writes_refused(fmt, case):
    unchanged(_write_program(fmt, case))


@pytest.mark.parametrize("fmt", FORMATS)
def test_row_write_fusion_switch(fmt, monkeypatch):
    monkeypatch.setenv("LTA_KV_POS_FUSION", "0")
    unchanged(_write_program(fmt))


def test_row_writes_of_the_written_args_are_the_caches():
    assert hipex.hip_qkv_rope_cache_rows.written_args == (7, 8)
    assert hipex.hip_qkv_rope_cache_rows_s8.written_args == (7, 8, 9, 10)
    for op in (hipex.hip_qkv_rope_cache_rows, hipex.hip_qkv_rope_cache_rows_s8):
        assert hipex.OpTags.DONT_DCE in op.tags and hipex.OpTags.IN_PLACE in op.tags


def _cache_reads(p, fmt, layer):
    """The k / v operands of a layer's attention as the model spells them, and how the fused form names them."""
    n = str(layer)
    if fmt == "16bit":
        kc, vc = p.ts(f"kc{n} vc{n}", B, 4, S, 64)
        return kc, vc, f"kc{n}, vc{n}"
    kc, vc = p.ts(f"kc{n} vc{n}", B, 4, S, 64, dtype=U8)
    kd, vd = p.ts(f"kd{n} vd{n}", B, 4, S, 64)
    if fmt == "e4m3":
        kf, vf = p.ts(f"kf{n} vf{n}", B, 4, S, 64, dtype=F8)
        p(lt.view, kc, F8, out=kf)
        p(lt.to, kf, BF16, out=kd)
        p(lt.view, vc, F8, out=vf)
        p(lt.to, vf, BF16, out=vd)
        return kd, vd, f"kc{n}, vc{n}"
    ksc, vsc = p.ts(f"ksc{n} vsc{n}", B, 4, S, 1, dtype=U8)
    p(DEQUANTISE, kc, ksc, BF16, out=kd)
    p(DEQUANTISE, vc, vsc, BF16, out=vd)
    return kd, vd, f"kc{n}, vc{n}, ksc{n}, vsc{n}"


def _read_program(fmt, case=None):
    p = Program()
    pos = p.t("pos", B, T, dtype=I64)
    mask = p.t("mask", B, 1, T, 16 if case == "other_capacity" else S, dtype=torch.bool)
    p(MASK, pos, 16 if case == "other_capacity" else S, out=mask)
    outs, names = [], []
    for layer in range(2):
        q, o = p.ts(f"q{layer} o{layer}", B, 8, T, 64)
        k, v, fused = _cache_reads(p, fmt, layer)
        p(hipex.hip_decode_attn, q, k, v, mask, case == "causal" and layer == 1, 0.125, out=o)
        outs.append(o)
        names.append(fused)
    if case == "mask_read_elsewhere":
        outs.append(p(lt.neg, mask, out=p.t("s", B, 1, T, S, dtype=torch.bool)))
    if case == "mask_returned":
        outs.append(mask)
    return p.run(*outs), names


@pytest.mark.parametrize("fmt", FORMATS)
def test_position_reads_fused_and_the_mask_dropped(fmt):
    (lines, msg), names = _read_program(fmt)
    op = {"16bit": "hip_decode_attn_pos", "e4m3": "hip_decode_attn_kv8_pos", "e4m3_row": "hip_decode_attn_kv8s_pos"}[fmt]
    assert lines == [f"o{n} = {op}(q{n}, {names[n]}, pos, 0.125)" for n in range(2)], lines
    assert msg == ("hipex: 2 decode attention(s) take their key counts from the positions" if fmt == "16bit"
                   else "hipex: 2 decode attention(s) read their e4m3 KV cache directly")


@pytest.mark.parametrize("case", ["mask_read_elsewhere", "mask_returned", "other_capacity", "causal"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_position_reads_refused(fmt, case):
    """Nothing takes the positions while the mask has another reader (or one attention cannot take them): the mask
    forms stay, for the e4m3 caches with their own read fusion."""
    (lines, msg), names = _read_program(fmt, case)
    if fmt == "16bit":
        assert (lines, msg) == (None, None)
        return
    op = {"e4m3": "hip_decode_attn_kv8", "e4m3_row": "hip_decode_attn_kv8s"}[fmt]
    assert msg == "hipex: 2 decode attention(s) read their e4m3 KV cache directly"
    assert lines[0].startswith("mask = ") and "_pos(" not in "".join(lines)
    attn = [ln for ln in lines if ln.startswith("o")]
    assert attn == [f"o{n} = {op}(q{n}, {names[n]}, mask, {case == 'causal' and n == 1}, 0.125)" for n in range(2)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_position_read_fusion_switch(fmt, monkeypatch):
    monkeypatch.setenv("LTA_KV_POS_FUSION", "0")
    (lines, msg), _ = _read_program(fmt)
    assert lines is None or ("_pos(" not in "".join(lines) and lines[0].startswith("mask = "))
    assert (lines is None) == (fmt == "16bit")
