"""The rewrite of a prefill against the KV cache in ``hipex._post_claim`` (``_fuse_kv_prefill_reads``), on hand-built
traces (the shape of ``test_hipex_pos_passes.py`` / ``test_hipex_paged_passes.py``): the masked flash attention over
the raw, dequantised or gathered cache becomes ``hip_prefill_attn_pos`` / ``hip_prefill_attn_paged`` or one of their
e4m3 forms, the dequantise links, the gathers and the shared mask leave, and every operand shape the pass declines
leaves the trace as it is."""
import pytest
import torch

from lightning_thunder_amd import torch as lt
from lightning_thunder_amd.executors import hipex
from lightning_thunder_amd.ops.kv8 import kv8_dequantise_rows
from lightning_thunder_amd.ops.kv_pages import kv_paged_gather, kv_paged_mask
from lightning_thunder_amd.ops.kv_rows import kv_position_mask
from lightning_thunder_amd.torch.custom_op import custom_op_symbol, opdef_of
from lightning_thunder_amd.transforms.inplace_index_copy import index_copy_inplace
from test_hipex_passes import Program, unchanged

BF16, U8, I64, F8, F32 = torch.bfloat16, torch.uint8, torch.int64, torch.float8_e4m3fn, torch.float32
DEQUANTISE = custom_op_symbol(opdef_of(kv8_dequantise_rows))
GATHER, PAGED_MASK = custom_op_symbol(opdef_of(kv_paged_gather)), custom_op_symbol(opdef_of(kv_paged_mask))
POS_MASK = custom_op_symbol(opdef_of(kv_position_mask))
B, T, HQ, H, D = 3, 40, 8, 4, 64
PAGE, PAGES, MAXP = 16, 20, 4
R, S = PAGE * PAGES, PAGE * MAXP
FORMATS = ["16bit", "e4m3", "e4m3_row"]
OP = {"16bit": "hip_prefill_attn", "e4m3": "hip_prefill_attn_kv8", "e4m3_row": "hip_prefill_attn_kv8s"}
_MSG = "hipex: 2 prefill attention(s) read their KV cache by positions"


def _reads(p, fmt, layer, paged, table, case):
    """The k / v operands of a layer's attention as the model spells them over its caches (``KVCache.forward``) or
    pools (``PagedKVCache.forward``: the gather of a pool is dequantised), the fused names, the case's extra outputs."""
    n = str(layer)
    hit = layer == 1  # the refusal cases change the second layer only
    d = 96 if case == "d96" and hit else D
    extra = []
    cdt = BF16 if fmt == "16bit" else U8

    def stored(name, width, dtype, tab=table, raw=False, written=False):
        if not paged or raw:
            return p.t(name, B, H, S, width, dtype=dtype)
        pool, g = p.t(name, H, R + 1, width, dtype=dtype), p.t("g" + name, B, H, S, width, dtype=dtype)
        p(GATHER, pool, tab, PAGE, out=g)
        if written:  # the pool is written in place between its gather and the attention
            extra.append(p(index_copy_inplace, pool, 1, p.t("idx", B * T, dtype=I64),
                           p.t("src", H, B * T, width, dtype=dtype), out=p.t("w" + name, H, R + 1, width, dtype=dtype)))
        return g

    table_v = p.t("table2", B, MAXP, dtype=I64) if case == "other_table" and hit else table
    ck = stored(f"kc{n}", d, cdt, written=case == "written" and hit and paged)
    cv = stored(f"vc{n}", d, cdt, table_v, raw=case == "v_raw" and hit)
    if fmt == "16bit":
        return ck, cv, f"kc{n}, vc{n}", extra
    kd, vd = p.ts(f"kd{n} vd{n}", B, H, S, d)
    if case == "mixed_kinds" and hit:  # k through the e4m3 dequantise, v a 16-bit cache
        kf = p.t(f"kf{n}", B, H, S, d, dtype=F8)
        p(lt.view, ck, F8, out=kf)
        p(lt.to, kf, BF16, out=kd)
        return kd, p.t(f"vraw{n}", B, H, S, d), "", extra
    if fmt == "e4m3":
        kf, vf = p.ts(f"kf{n} vf{n}", B, H, S, d, dtype=F8)
        p(lt.view, ck, F8, out=kf)
        p(lt.to, kf, BF16, out=kd)
        if case == "written" and hit and not paged:  # the cache is written in place between its view and the attention
            extra.append(p(index_copy_inplace, ck, 2, p.t("idx", T, dtype=I64), p.t("src", B, H, T, d, dtype=U8),
                           out=p.t("wkc", B, H, S, d, dtype=U8)))
        p(lt.view, cv, F8, out=vf)
        p(lt.to, vf, BF16, out=vd)
        return kd, vd, f"kc{n}, vc{n}", extra
    ks, vs = stored(f"ksc{n}", 1, U8), stored(f"vsc{n}", 1, U8)
    p(DEQUANTISE, ck, ks, BF16, out=kd)
    if case == "written" and hit and not paged:
        extra.append(p(index_copy_inplace, ck, 2, p.t("idx", T, dtype=I64), p.t("src", B, H, T, d, dtype=U8),
                       out=p.t("wkc", B, H, S, d, dtype=U8)))
    p(DEQUANTISE, cv, vs, BF16, out=vd)
    return kd, vd, f"kc{n}, vc{n}, ksc{n}, vsc{n}", extra


def _program(fmt, paged, case=None, t=T):
    p = Program()
    pos = p.t("pos", B, t + 1 if case == "pos_shape" else t, dtype=I64)
    table = p.t("table", B, MAXP, dtype=I64)
    mask = p.t("mask", B, 1, t, S, dtype=F32 if case == "float_mask" else torch.bool)
    if case == "float_mask":
        pass  # a program input: an additive mask of unknown content
    elif paged:
        p(PAGED_MASK, pos, table, PAGE, PAGES, out=mask)
    else:
        p(POS_MASK, pos, 2 * S if case == "other_capacity" else S, out=mask)
    outs, names = [], []
    for layer in range(2):
        hit = layer == 1
        d = 96 if case == "d96" and hit else D
        q, o = p.ts(f"q{layer} o{layer}", B, HQ, t, d)
        lse = p.t(f"lse{layer}", B, HQ, t, dtype=F32)
        k, v, fused, extra = _reads(p, fmt, layer, paged, table, case)
        p(hipex.hip_attn_fwd_ex, q, k, v, mask, case == "causal" and hit, 0.125, 0.1 if case == "dropout" and hit else 0.0,
          0, 0, out=(o, lse))
        outs += [o, *extra]
        if case == "lse_read" and hit:
            outs.append(lse)
        names.append(fused)
    if case == "mask_returned":
        outs.append(mask)
    return p.run(*outs), names


def _fused(fmt, paged, n, names):
    tail = "pos, table, 16, 20, 0.125" if paged else "pos, 0.125"
    return f"o{n} = {OP[fmt]}_{'paged' if paged else 'pos'}(q{n}, {names[n]}, {tail})"


def test_the_symbols_are_the_ones_the_pass_matches():
    assert POS_MASK.id in hipex._KV_POSITION_MASK_IDS and PAGED_MASK.id in hipex._KV_PAGED_MASK_IDS
    assert GATHER.id in hipex._KV_PAGED_GATHER_IDS and DEQUANTISE.id in hipex._KV8_DEQUANTISE_IDS
    assert hipex._fuse_kv_prefill_reads in hipex._PASSES


@pytest.mark.parametrize("paged", [False, True], ids=["position_mask", "paged_mask"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_prefill_reads_fused_and_links_and_mask_dropped(fmt, paged):
    """Two layers, one mask: only the two operators stay (no gather, no dequantise link, no mask)."""
    (lines, msg), names = _program(fmt, paged)
    assert lines == [_fused(fmt, paged, n, names) for n in range(2)], lines
    assert msg == _MSG


@pytest.mark.parametrize("paged", [False, True], ids=["position_mask", "paged_mask"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_mask_stays_for_another_reader(fmt, paged):
    (lines, msg), names = _program(fmt, paged, "mask_returned")
    assert lines[0].startswith("mask = ") and msg == _MSG
    assert lines[1:] == [_fused(fmt, paged, n, names) for n in range(2)]


DECLINES = ["lse_read", "causal", "dropout", "d96", "pos_shape"]


@pytest.mark.parametrize("case", DECLINES)
@pytest.mark.parametrize("paged", [False, True], ids=["position_mask", "paged_mask"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_prefill_reads_declined_in_one_layer(fmt, paged, case):
    """A read LSE, ``causal=True``, dropout, head dim 96 in the second layer: that layer keeps the masked attention
    over its gathers and dequantise links, the mask keeps a reader, the first layer is still folded.  ``pos`` of
    another shape than ``[B, T]`` declines both."""
    (lines, msg), names = _program(fmt, paged, case)
    if case == "pos_shape":
        assert (lines, msg) == (None, None)
        return
    text = "\n".join(lines)
    assert lines[0].startswith("mask = "), "the mask keeps a reader"
    assert _fused(fmt, paged, 0, names) in lines and msg == _MSG.replace("2 prefill", "1 prefill")
    assert text.count("hip_prefill_attn") == 1
    (o1,) = [ln for ln in lines if ln.startswith("o1, lse1 = ")]
    assert o1.startswith("o1, lse1 = hip_flash_attn_fwd_ex(q1, ") and ", mask, " in o1
    if fmt != "16bit":
        assert "kd1 = " in text and "vd1 = " in text, "the declined layer's dequantise links stay"
    if paged:
        assert "gkc1 = " in text and "gvc1 = " in text, "the declined layer's gathers stay"


@pytest.mark.parametrize("paged", [False, True], ids=["position_mask", "paged_mask"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_float_mask_is_declined(fmt, paged):
    unchanged(_program(fmt, paged, "float_mask")[0])


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_position_mask_of_another_capacity_is_declined(fmt):
    unchanged(_program(fmt, False, "other_capacity")[0])


@pytest.mark.parametrize("case", ["v_raw", "other_table", "written"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_paged_reads_declined(fmt, case):
    """k from a gather and v raw, gathers at two tables, a pool written in place between its gather and the
    attention: that layer stays as it is."""
    (lines, msg), names = _program(fmt, True, case)
    text = "\n".join(lines)
    assert lines[0].startswith("mask = ") and msg == _MSG.replace("2 prefill", "1 prefill")
    assert _fused(fmt, True, 0, names) in lines and text.count("hip_prefill_attn") == 1
    assert "o1, lse1 = hip_flash_attn_fwd_ex(q1, " in text and "gkc1 = " in text


@pytest.mark.parametrize("fmt", ["e4m3", "e4m3_row"])
def test_static_e4m3_reads_declined(fmt):
    """A cache written in place between its dequantise and the attention, and k / v of different kinds."""
    for case in ("written", "mixed_kinds"):
        (lines, msg), names = _program(fmt, False, case)
        text = "\n".join(lines)
        assert _fused(fmt, False, 0, names) in lines and text.count("hip_prefill_attn") == 1, case
        assert "o1, lse1 = hip_flash_attn_fwd_ex(q1, kd1, " in text and lines[0].startswith("mask = "), case


@pytest.mark.parametrize("switch", ["LTA_KV_PREFILL_FUSION", "LTA_KV_POS_FUSION", "LTA_KV_PAGED_FUSION", "LTA_KV8_FUSION"])
@pytest.mark.parametrize("paged", [False, True], ids=["position_mask", "paged_mask"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fusion_switches(fmt, paged, switch, monkeypatch):
    """LTA_KV_PREFILL_FUSION=0 leaves the trace unchanged; so does the switch of the cache kind a prefill reads."""
    monkeypatch.setenv(switch, "0")
    result, names = _program(fmt, paged)
    applies = (switch == "LTA_KV_PREFILL_FUSION" or (switch == "LTA_KV_POS_FUSION" and not paged)
               or (switch == "LTA_KV_PAGED_FUSION" and paged) or (switch == "LTA_KV8_FUSION" and fmt != "16bit"))
    if applies:
        unchanged(result)
    else:
        assert result[0] == [_fused(fmt, paged, n, names) for n in range(2)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_sixteen_rows_still_become_the_decode_operator(fmt):
    """T = 16 is claimed as ``hip_decode_attn`` (``_sdpa_exec``), and the decode passes, not this one, rewrite it."""
    from lightning_thunder_amd.ops.attention import DECODE_MAX_QUERIES

    assert DECODE_MAX_QUERIES == 16
    p = Program()
    pos = p.t("pos", B, 16, dtype=I64)
    mask = p.t("mask", B, 1, 16, S, dtype=torch.bool)
    p(POS_MASK, pos, S, out=mask)
    q, o = p.ts("q0 o0", B, HQ, 16, D)
    k, v, names, _ = _reads(p, fmt, 0, False, None, None)
    p(hipex.hip_decode_attn, q, k, v, mask, False, 0.125, out=o)
    lines, _ = p.run(o)
    op = {"16bit": "hip_decode_attn_pos", "e4m3": "hip_decode_attn_kv8_pos", "e4m3_row": "hip_decode_attn_kv8s_pos"}[fmt]
    assert lines == [f"o0 = {op}(q0, {names}, pos, 0.125)"]


def test_sdpa_claims_sixteen_rows_as_decode_and_seventeen_as_flash():
    """Where the operators come from: ``_sdpa_exec`` emits ``hip_decode_attn`` up to 16 rows and
    ``hip_flash_attn_fwd_ex`` beyond, so the prefill pass never sees a decode step."""
    for t, want in ((16, "hip_decode_attn"), (17, "hip_flash_attn_fwd_ex")):
        p = Program()
        q = p.t("q", B, HQ, t, D)
        k, v = p.ts("k v", B, H, S, D)
        mask = p.t("mask", B, 1, t, S, dtype=torch.bool)
        from lightning_thunder_amd.core.trace import tracectx

        with tracectx(p.trace):
            hipex._sdpa_exec(q, k, v, mask, 0.0, False, scale=None, enable_gqa=True)
        assert [b.sym.name for b in p.trace.bound_symbols] == [want]
