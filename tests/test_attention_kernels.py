"""The flash-attention forward and backward kernels, branch by branch, against an fp64 reference written here:

* ``attn_fwd``: the generic v1 kernel (csrc/attention_fwd.hip: D 64 / 96, masks, dropout, and D = 128 / 256
  behind ``lta_attn_fwd_set_impl(0)`` / ``lta_attn_fwd_set_ring(0)``), the v4 kernel (attention_fwd4.hip,
  ``impl`` 10 deferred rescale and 9 exact) and the D = 256 ring kernel (attention_fwd_d256.hip), at the
  lengths around every tile and ring edge, causal with T != S, GQA / MQA, both output layouts, strided views,
  misaligned pointers, padded head dims, explicit scales and row maxima that rise across the rescale threshold;
* ``attn_bwd``: the v1 dK/dV and dQ kernels, the v4 ones (D = 128), the GQA head split and its reduce, the
  masked / dropout builds and the mask gradient (csrc/attention_bwd.hip);
* ``attn_bwd_rope``: the fused rotate-half epilogues, with dQ from the stored dS and without;
* bitwise identities under permutations of (batch, head) and under slicing.

Tolerance, per element:  R_T(ref) + extra + 8 e32 + 1e-6 max |ref|  (kernel_checks.assert_within with
``extra``).  R_T(x) = max(ulp(T) |x|, half the subnormal spacing of T) is the rounding of the output, ``e32``
the error of the same formula evaluated by plain torch in fp32.  ``extra`` is a first-order model of the
roundings to T the kernels perform on intermediates before the second MFMA, every one entering once, all
formed from the fp64 reference (P: after mask, causal, dropout and keep scale):

    O       R_T(P) @ |V|                          P is packed to T for O^T += V^T P^T
    dV      R_T(P)^T @ |dO|                       ... and for dV += P^T dO
    dQ      scale (R_T(dS) + P ddelta) @ |K|      dS is packed to T; delta = rowsum(dO o O) is taken from
    dK      scale (R_T(dS) + P ddelta)^T @ |Q|    the stored (rounded) O: ddelta_i = sum_d |dO_id| R_T(O_id)
    dmask   P ddelta                              the unrounded fp32 dS
    lse     -                                     fp32, plain formula

(the P multiplying ddelta is the probability before dropout: dS = P (dP - delta), and a dropped entry still
carries delta).  The fused-RoPE outputs rotate dQ / dK in fp32 before the one rounding, so their extra term is
the rotated one: extra |cos| + rotate(extra |sin|).  The dQ-from-dS path stores dS in T once; that rounding is
the R_T(dS) already in the model.

A fully masked query row is O = 0, lse = -inf and contributes nothing to any gradient (the forward's
convention); the reference says so and the outputs of such rows must be exact zeros.

Every case also runs on the CPU through an fp32 emulation that applies exactly the modelled roundings
(test_emulation_within_tolerance_cpu): inputs and tolerance are consistent without the kernel.

Not covered: LTA_ATTN_BWD_V1 (read once per process in C) and ``attn_fwd_v4_q8`` (bf16 only; it keeps its
test in test_hip_kernels.py).
"""
import ctypes
import functools
import math
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import BF16, F16, F32, HALF_SUBNORMAL, ULP, _WORST, _dt_id, assert_within, bits_equal, keep_mask

gpu = pytest.mark.gpu
F64 = torch.float64
DTYPES = [BF16, F16]
SEED, OFFSET = 1234567890123, 4099  # dropout generator state: a seed above 2^32, a nonzero offset
NEG_INF = float("-inf")

# Largest err / tol measured on MI355X per group, bf16 / fp16 (test_zz_report_worst_ratios prints them with -s):
#   fwd O             0.87 / 0.45    dQ                0.47 / 0.25    dmask (fp32)  0.38
#   lse (fp32)        0.14           dK                0.77 / 0.40
#   fused-RoPE dqkv   0.83 / 0.37    dV                0.95 / 0.46
# The emulation on the CPU reaches 0.95 (dV, T = 1: one query row, so no averaging over rows).  Every term of
# the model has factor 1; no group needed a further term.  The whole file takes 14 s on MI355X (851 tests, the
# slowest 0.8 s, both on the CPU: the SDPA comparison and the emulation of a whole tag), the GPU cases 10 ms each.


# ------------------------------------------------------------------------------------------------
# reference: one formula, three uses (fp64 reference; plain fp32 = e32; fp32 with the modelled roundings)
# ------------------------------------------------------------------------------------------------
def _mask4(mask):
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    return mask


def _reduce_to(x, shape):
    """Sum ``x`` [B, Hq, T, S] over the dims a mask of ``shape`` broadcasts over."""
    lead = x.dim() - len(shape)
    if lead:
        x = x.sum(tuple(range(lead)))
    dims = tuple(i for i, n in enumerate(shape) if n == 1 and x.shape[i] != 1)
    return x.sum(dims, keepdim=True) if dims else x


def _group_sum(x, Hkv):
    B, Hq, S, D = x.shape
    return x.view(B, Hkv, Hq // Hkv, S, D).sum(2)


def _R(x, T):
    return (ULP[T] * x.abs()).clamp(min=HALF_SUBNORMAL[T])


def rope_bwd(g, cos, sin):
    """Backward of y = x cos + cat(-x[64:], x[:64]) sin over the last dim: g [B, H, T, D], cos / sin [T, D]."""
    h = g.shape[-1] // 2
    gs = g * sin
    return g * cos + torch.cat((gs[..., h:], -gs[..., :h]), -1)


def _rope_abs(e, cos, sin):
    h = e.shape[-1] // 2
    es = e * sin.abs()
    return e * cos.abs() + torch.cat((es[..., h:], es[..., :h]), -1)


def ref_attention(q, k, v, do, mask=None, causal=False, keep=None, p=0.0, scale=None, dt=F64, round_to=None,
                  model=None, want_dmask=False):
    """Forward and backward of softmax(q k^T scale + mask) (dropout) v in ``dt``.

    q, do [B, Hq, T, D]; k, v [B, Hkv, S, D]; mask boolean (True = attend) or additive, broadcastable to
    [B, Hq, T, S] from the right; causal is top-left aligned (query t sees keys 0..t); keep [B, Hq, T, S]
    boolean.  A fully masked row has P = 0, O = 0, lse = -inf and no gradient.  ``round_to`` = T applies the
    kernels' intermediate roundings (P, O under delta, dS); ``model`` = T adds the tolerance terms ``x_*``.
    Returns a dict: o, lse, dq, dk, dv, dmask (unrounded)."""
    q, k, v, do = (t.to(dt) for t in (q, k, v, do))
    B, Hq, T, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    sc = D ** -0.5 if scale is None else scale
    rt = (lambda x: x.to(round_to).to(dt)) if round_to is not None else (lambda x: x)
    kk, vv = k.repeat_interleave(Hq // Hkv, 1), v.repeat_interleave(Hq // Hkv, 1)
    s = torch.matmul(q, kk.transpose(-1, -2)) * sc
    if mask is not None:
        m4 = _mask4(mask)
        if m4.dtype == torch.bool:
            m4 = torch.where(m4, torch.zeros((), dtype=dt), torch.full((), NEG_INF, dtype=dt))
        s = s + m4.to(dt)
    if causal:
        s = s.masked_fill(~torch.ones(T, S, dtype=torch.bool).tril(), NEG_INF)
    mx = s.amax(-1, keepdim=True)
    dead = mx == NEG_INF
    mx = mx.masked_fill(dead, 0.0)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    P = (e / l.masked_fill(dead, 1.0)).masked_fill(dead, 0.0)
    lse = (mx + torch.log(l.masked_fill(dead, 1.0))).masked_fill(dead, NEG_INF).squeeze(-1)
    ks = 1.0 / (1.0 - p) if keep is not None else 1.0
    Pd = P * keep.to(dt) * ks if keep is not None else P
    Pr = rt(Pd)
    o = torch.matmul(Pr, vv)
    dP = torch.matmul(do, vv.transpose(-1, -2))
    if keep is not None:
        dP = dP * keep.to(dt) * ks
    delta = (do * rt(o)).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dSr = rt(dS)
    out = {"o": o, "lse": lse,
           "dq": sc * torch.matmul(dSr, kk),
           "dk": sc * _group_sum(torch.matmul(dSr.transpose(-1, -2), q), Hkv),
           "dv": _group_sum(torch.matmul(Pr.transpose(-1, -2), do), Hkv)}
    if want_dmask:
        out["dmask"] = _reduce_to(dS, tuple(mask.shape))
    if model is not None:
        RP = _R(Pd, model)
        ddelta = (do.abs() * _R(o, model)).sum(-1, keepdim=True)
        E = _R(dS, model) + P * ddelta
        out["x_o"] = torch.matmul(RP, vv.abs())
        out["x_dv"] = _group_sum(torch.matmul(RP.transpose(-1, -2), do.abs()), Hkv)
        out["x_dq"] = sc * torch.matmul(E, kk.abs())
        out["x_dk"] = sc * _group_sum(torch.matmul(E.transpose(-1, -2), q.abs()), Hkv)
        if want_dmask:
            out["x_dmask"] = _reduce_to(P * ddelta, tuple(mask.shape))
    return out


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    tag: str
    B: int
    Hq: int
    Hkv: int
    T: int
    S: int
    D: int
    causal: bool = False
    mask: str = ""           # "<bool|float>_<11|b1|1h|bh|2d|3d|pad>[+inf][+dead_mid|+dead_wave|+dead_last]"
    p: float = 0.0
    scale: float = 0.0       # 0: the default D^-0.5
    qmul: float = 1.0
    rising: int = 0          # key block of the rising-score construction (0: random normal inputs)
    layout: str = "plain"    # plain | views (one fused projection; T == S) | tmajor | misaligned
    out_layout: str = "bshd"
    do_layout: str = "bhtd"
    hook: str = ""           # impl0 | impl9 | ring0
    path: str = ""           # forward kernel the case must reach: v4 | d256 | "" (v1)
    mask_grad: bool = False
    split: str = ""          # LTA_ATTN_GQA_SPLIT ("" = unset)
    rope: str = ""           # "" | "ds0" | "ds1": attn_bwd_rope with LTA_ATTN_DQ_FROM_DS = 0 / 1

    @property
    def id(self):
        s = f"{self.tag}-B{self.B}H{self.Hq}k{self.Hkv}-T{self.T}S{self.S}D{self.D}"
        for name, dflt in (("causal", False), ("mask", ""), ("p", 0.0), ("scale", 0.0), ("qmul", 1.0), ("rising", 0),
                           ("layout", "plain"), ("out_layout", "bshd"), ("do_layout", "bhtd"), ("hook", ""),
                           ("mask_grad", False), ("split", ""), ("rope", "")):
            val = getattr(self, name)
            if val != dflt:
                s += f"-{name}" if val is True else f"-{name}={val}"
        return s

    @property
    def sc(self):
        return self.scale if self.scale else None


def _fwd_path(D, hook="", mask="", p=0.0):
    Dp = next(d for d in (64, 96, 128, 256) if d >= D)
    if mask or p:
        return ""
    if Dp == 128 and hook != "impl0":
        return "v4"
    if Dp == 256 and hook != "ring0":
        return "d256"
    return ""


def C(tag, B, Hq, Hkv, T, S, D, **kw):
    kw.setdefault("path", _fwd_path(D, kw.get("hook", ""), kw.get("mask", ""), kw.get("p", 0.0)))
    return Case(tag, B, Hq, Hkv, T, S, D, **kw)


def _edge_cases():
    out = []
    # v1 forward and backward: 128 queries per workgroup, 32 per wave, 64-key tiles (32 at D = 256); the
    # backward's 128-key workgroups, 32-query double-buffered tiles (dK/dV) and 64-key tiles (dQ)
    v1 = [(64, ""), (96, ""), (128, "impl0"), (256, "ring0")]
    for D, hook in v1:
        for causal in (False, True):
            for T, S in [(1, 1), (33, 63), (127, 64), (128, 65), (129, 129), (1, 129), (129, 1), (33, 129), (128, 64),
                         (31, 127), (65, 257), (129, 127), (33, 257)]:
                out.append(C("v1", 1, 2, 2, T, S, D, hook=hook, causal=causal))
        for S in (31, 33) if D == 256 else ():
            out.append(C("v1", 1, 2, 1, 33, S, D, hook=hook))
    # v4 forward (impl 10 deferred, 9 exact): 256 queries per workgroup, 64 per wave, 4-slot ring with two
    # tiles in flight (S = 321 wraps it, 577 wraps it twice); v4 backward: 256 keys / 256 queries per workgroup,
    # 32-key streamed tiles
    for hook in ("", "impl9"):
        for causal in (False, True):
            for T, S in [(1, 1), (63, 64), (65, 65), (255, 257), (256, 321), (257, 577), (1, 577), (257, 1), (33, 33),
                         (255, 255), (513, 33), (33, 513), (513, 513)]:
                if hook == "impl9" and max(T, S) == 513:
                    continue  # the backward lengths: one forward flavour is enough
                out.append(C("v4", 1, 2, 2, T, S, 128, hook=hook, causal=causal))
    # D = 256 ring forward: 32-key tiles, 4 stages, three in flight; causal T = S: wave 0 runs the up to three
    # fully masked tiles past its diagonal
    for S in (1, 31, 32, 33, 97, 129, 161):
        out.append(C("d256", 1, 2, 1, 70, S, 256))
    for T in (128, 129, 200):
        out.append(C("d256", 1, 2, 1, T, T, 256, causal=True))
    for T, S in ((129, 257), (257, 129), (1, 161), (161, 1)):
        out.append(C("d256", 1, 2, 2, T, S, 256, causal=True))
        out.append(C("d256", 1, 2, 2, T, S, 256))
    return out


def _variation_cases():
    out = []
    paths = [(64, ""), (128, "impl0"), (128, ""), (128, "impl9"), (256, ""), (256, "ring0")]
    for D, hook in paths:
        # causal with T < S and T > S, more than one workgroup per head, two batches
        out.append(C("var", 2, 4, 2, 70, 300, D, hook=hook, causal=True))
        out.append(C("var", 2, 4, 2, 300, 70, D, hook=hook, causal=True))
        # GQA groups 1 / 2 / MQA, both output layouts
        out.append(C("var", 2, 4, 4, 130, 200, D, hook=hook, out_layout="bhsd"))
        out.append(C("var", 2, 4, 2, 130, 200, D, hook=hook, causal=True, out_layout="bhsd"))
        out.append(C("var", 2, 4, 1, 130, 200, D, hook=hook))
        # q / k / v views into one projection, token-major buffers, misaligned data pointers
        out.append(C("var", 2, 4, 2, 200, 200, D, hook=hook, causal=True, layout="views", do_layout="bthd"))
        out.append(C("var", 2, 4, 2, 130, 333, D, hook=hook, layout="tmajor", do_layout="bthd"))
        out.append(C("var", 1, 4, 2, 130, 200, D, hook=hook, causal=True, layout="misaligned"))
        # an explicit scale, larger scores
        out.append(C("var", 1, 2, 2, 130, 200, D, hook=hook, scale=0.05))
        out.append(C("var", 1, 2, 1, 130, 130, D, hook=hook, causal=True, qmul=4.0))
    # padded head dims: 32 -> 64, 80 -> 96, 112 -> 128 (v4), 192 -> 256 (ring)
    for D in (32, 80, 112, 192):
        out.append(C("pad", 2, 4, 2, 130, 200, D, causal=True))
        out.append(C("pad", 1, 2, 2, 65, 129, D, scale=0.11, out_layout="bhsd"))
    # the GQA head split of the dK/dV pass and its reduce, on (default) and off, groups 2 / 4 / 8
    for D in (64, 128, 256):
        for group in (2, 4, 8):
            for split in ("", "1"):
                out.append(C("gqa", 2, 8, 8 // group, 130, 300, D, causal=group == 4, split=split,
                             do_layout="bthd" if group == 2 else "bhtd"))
        out.append(C("gqa", 1, 8, 2, 200, 200, D, split="2", layout="views", causal=True))
    return out


def _rising_cases():
    # row maxima that rise per key tile by just under, then just over 8 log2 units (the deferred-rescale
    # threshold), some rows of every wave flat: 64-key tiles on v4 (impl 10 / 9) and v1, 32-key on D = 256
    out = []
    for D, hook, blk in ((128, "", 64), (128, "impl9", 64), (128, "impl0", 64), (64, "", 64), (256, "", 32), (256, "ring0", 32)):
        for T, S in ((70, 5 * blk + 1), (257, 9 * blk + 1)):
            out.append(C("rising", 1, 2, 1, T, S, D, hook=hook, rising=blk))
    return out


def _mask_cases():
    out = []
    for D in (64, 128, 256):
        for typ in ("bool", "float"):
            for shp in ("11", "b1", "1h", "bh", "2d", "3d", "pad"):
                out.append(C("mask", 2, 4, 2, 70, 200, D, mask=f"{typ}_{shp}", causal=shp == "b1"))
        out.append(C("mask", 1, 2, 2, 129, 65, D, mask="float_bh+inf"))
        out.append(C("mask", 2, 2, 1, 33, 64, D, mask="bool_bh"))  # no -inf padding of the image
        for dead in ("dead_mid", "dead_wave", "dead_last"):
            out.append(C("dead", 2, 4, 2, 100, 200, D, mask=f"bool_bh+{dead}"))
            out.append(C("dead", 1, 2, 2, 70, 130, D, mask=f"float_1h+inf+{dead}", mask_grad=True))
        out.append(C("dead", 2, 4, 2, 100, 200, D, mask="bool_b1+dead_mid", p=0.1, causal=True))
        for p in (0.1, 0.5):
            out.append(C("drop", 2, 4, 2, 130, 200, D, p=p, causal=p == 0.5))
        out.append(C("drop", 1, 4, 4, 129, 65, D, p=0.5, layout="tmajor", do_layout="bthd"))
        out.append(C("drop", 2, 4, 2, 70, 200, D, p=0.1, mask="bool_pad"))
        out.append(C("drop", 2, 4, 1, 70, 200, D, p=0.5, mask="float_1h+inf", mask_grad=True))
        # the mask gradient at broadcast mask shapes, after its reduction
        for shp in ("1h", "b1", "2d", "11", "bh"):
            out.append(C("mgrad", 2, 4, 2, 70, 130, D, mask=f"float_{shp}", mask_grad=True, causal=shp == "2d"))
    out.append(C("mask", 2, 4, 2, 70, 200, 80, mask="bool_b1", p=0.1))
    out.append(C("mgrad", 2, 4, 2, 70, 130, 192, mask="float_1h", mask_grad=True))
    return out


def _rope_cases():
    out = []
    for T in (64, 256, 320, 200):  # 200: T % 64 != 0, the dQ-from-dS entry declines and the recompute entry runs
        for ds in ("ds0", "ds1"):
            out.append(C("rope", 1, 4, 4, T, T, 128, causal=True, rope=ds))
            out.append(C("rope", 2, 4, 2, T, T, 128, causal=T != 256, rope=ds, do_layout="bthd"))
            out.append(C("rope", 1, 8, 2, T, T, 128, causal=True, rope=ds, split="1"))
    return out


CASES = _edge_cases() + _variation_cases() + _rising_cases() + _mask_cases() + _rope_cases()
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"
FUSED = [c for c in CASES if c.rope]
PLAIN = [c for c in CASES if not c.rope]


def _ids(cases):
    return [c.id for c in cases]


def _dead_rows(kind, T):
    if "dead_mid" in kind:
        return [48] if T > 48 else [T // 2]
    if "dead_wave" in kind:
        return list(range(32, 64))
    if "dead_last" in kind:
        return [T - 1]
    return []


def make_mask(kind, B, Hq, T, S, g):
    base, *mods = kind.split("+")
    typ, shp = base.split("_")
    shape = {"11": (1, 1, T, S), "b1": (B, 1, T, S), "1h": (1, Hq, T, S), "bh": (B, Hq, T, S), "2d": (T, S),
             "3d": (Hq, T, S), "pad": (B, 1, 1, S)}[shp]
    if shp == "pad":  # left padding: another pad length per batch
        pad = (17 + 70 * torch.arange(B)) % S
        keep = (torch.arange(S).view(1, 1, 1, S) >= pad.view(B, 1, 1, 1)) | (torch.arange(S) == 0).view(1, 1, 1, S)
        return keep if typ == "bool" else torch.where(keep, torch.randn(shape, generator=g), torch.tensor(NEG_INF))
    if typ == "bool":
        m = torch.rand(shape, generator=g) > 0.3
        m[..., 0] = True  # key 0 is visible to every row, causal or not: only the rows below are fully masked
        m[..., _dead_rows(kind, T), :] = False
    else:
        m = torch.randn(shape, generator=g) * 2.0
        if "inf" in mods:
            hole = torch.rand(shape, generator=g) > 0.7
            hole[..., 0] = False
            m = m.masked_fill(hole, NEG_INF)
        m[..., _dead_rows(kind, T), :] = NEG_INF
    return m


def rising_inputs(B, Hq, Hkv, T, S, D, blk, g):
    """The rising-score construction of test_decode_kernels._rising_inputs with a key block of ``blk`` and
    steps that alternate: k[j] = base + c[j // blk] ln 2 qhat with c rising by 0.9, 1.1, 0.9, ..., q = 8
    (sqrt(D) a qhat + noise): with scale D^-0.5 the scores of a row with a = 1 rise from one key block to the
    next by 7.2, then 8.8 log2 units (cumulative 16 from the last rescale); every third row has a = 0 (flat)."""
    qhat = F.normalize(torch.randn(B, Hkv, 1, D, generator=g), dim=-1)
    a = (torch.arange(T) % 3 != 1).float().view(1, 1, T, 1)
    q = 8.0 * (math.sqrt(D) * a * qhat.repeat_interleave(Hq // Hkv, 1) + 0.1 * torch.randn(B, Hq, T, D, generator=g))
    j = torch.arange(S) // blk
    steps = torch.where(torch.arange(int(j.max()) + 1) % 2 == 0, 0.9, 1.1)
    c = torch.cat((torch.zeros(1), steps.cumsum(0)))[j].view(1, 1, S, 1)
    k = 0.02 * torch.randn(B, Hkv, S, D, generator=g) + c * math.log(2.0) * qhat
    return q, k


def check_rising(q, k, scale, blk):
    """The construction does what it says, on the exactly upcast inputs in fp64 (log2 units)."""
    g = q.shape[1] // k.shape[1]
    s = torch.matmul(q.double(), k.double().repeat_interleave(g, 1).transpose(-1, -2)) * scale / math.log(2.0)
    S = s.shape[-1]
    nblk = (S + blk - 1) // blk
    pad = torch.full(s.shape[:-1] + (nblk * blk - S,), NEG_INF, dtype=s.dtype)
    bmax = torch.cat((s, pad), -1).view(*s.shape[:-1], nblk, blk).max(-1).values
    rise = bmax[..., 1:] - bmax[..., :-1]
    up = torch.arange(s.shape[-2]) % 3 != 1
    r = rise[..., up, :]
    if S % blk:  # the last block is partial: the maximum over its few keys lacks the noise of a full block's
        assert (r[..., -1] > 5.6).all() and (r[..., -1] < 9.6).all()
        r = r[..., :-1]
    assert ((r[..., 0::2] > 6.4) & (r[..., 0::2] < 8.0)).all(), "even steps must rise by just under 8 log2 units"
    assert ((r[..., 1::2] > 8.0) & (r[..., 1::2] < 9.6)).all(), "odd steps must rise by just over 8 log2 units"
    assert rise[..., ~up, :].abs().max() < 2.0, "the flat rows must stay flat"


@functools.lru_cache(maxsize=None)
def inputs(c, dtype):
    g = torch.Generator().manual_seed(1 + len(c.id) + 131 * c.T + 17 * c.S + c.D)
    q = torch.randn(c.B, c.Hq, c.T, c.D, generator=g) * c.qmul
    k = torch.randn(c.B, c.Hkv, c.S, c.D, generator=g)
    v = torch.randn(c.B, c.Hkv, c.S, c.D, generator=g)
    do = torch.randn(c.B, c.Hq, c.T, c.D, generator=g)
    if c.rising:
        q, k = rising_inputs(c.B, c.Hq, c.Hkv, c.T, c.S, c.D, c.rising, g)
    d = {"q": q.to(dtype), "k": k.to(dtype), "v": v.to(dtype), "do": do.to(dtype), "mask": None, "keep": None}
    if c.rising:
        check_rising(d["q"], d["k"], c.D ** -0.5, c.rising)
    if c.mask:
        d["mask"] = make_mask(c.mask, c.B, c.Hq, c.T, c.S, g)
    if c.p:
        d["keep"] = keep_mask(SEED, OFFSET, c.B, c.Hq, c.T, c.S, c.p, "cpu")
    if c.rope:  # random tables with two different halves: a kernel that mixes the halves up shows
        d["cos"] = torch.rand(c.T, c.D, generator=g) * 2 - 1
        d["sin"] = torch.rand(c.T, c.D, generator=g) * 2 - 1
    return d


def _evaluate(c, dtype, dt, round_to=None, model=None):
    i = inputs(c, dtype)
    r = ref_attention(i["q"], i["k"], i["v"], i["do"], i["mask"], c.causal, i["keep"], c.p, c.sc, dt, round_to, model,
                      c.mask_grad)
    if c.rope:
        cos, sin = i["cos"].to(dt), i["sin"].to(dt)
        r["dq"], r["dk"] = rope_bwd(r["dq"], cos, sin), rope_bwd(r["dk"], cos, sin)
        if model is not None:
            r["x_dq"], r["x_dk"] = _rope_abs(r["x_dq"], cos, sin), _rope_abs(r["x_dk"], cos, sin)
        cat = lambda a, b, d: torch.cat([t.transpose(1, 2).flatten(2) for t in (a, b, d)], -1)  # noqa: E731
        r["dqkv"] = cat(r["dq"], r["dk"], r["dv"])
        if model is not None:
            r["x_dqkv"] = cat(r["x_dq"], r["x_dk"], r["x_dv"])
    return r


@functools.lru_cache(maxsize=None)
def reference(c, dtype):
    """(fp64 reference with the model terms, plain fp32 evaluation) of a case, computed once."""
    return _evaluate(c, dtype, F64, model=dtype), _evaluate(c, dtype, F32)


GROUP = {"o": "fwd O", "lse": "lse", "dq": "dQ", "dk": "dK", "dv": "dV", "dmask": "dmask", "dqkv": "fused-RoPE dqkv"}


def check(c, dtype, name, out, emulated=False):
    """One output of a case against the reference, with the model's extra term; lse and dmask are fp32.
    ``emulated`` files the ratio under its own group, so the printed worst figures are the kernels' alone."""
    r64, r32 = reference(c, dtype)
    what = f"{c.id} {name}"
    out = out.detach().cpu()
    ref, ref32 = r64[name], r32[name]
    T = F32 if name in ("lse", "dmask") else dtype
    assert out.dtype == T and out.shape == ref.shape, (what, out.dtype, tuple(out.shape), tuple(ref.shape))
    rows = _dead_rows(c.mask, c.T)
    if name == "lse":
        dead = torch.isneginf(ref)
        assert dead[..., rows].all() and dead.sum().item() == len(rows) * c.B * c.Hq
        assert torch.equal(torch.isneginf(out), dead), f"{what}: lse must be -inf on exactly the fully masked rows"
        out, ref, ref32 = (t.masked_fill(dead, 0.0) for t in (out, ref, ref32))
    elif rows and name in ("o", "dq", "dmask"):
        assert not ref[..., rows, :].any()
        assert not torch.isnan(out).any(), f"{what}: NaN in the kernel output"
        assert not out[..., rows, :].any(), f"{what}: a fully masked row must be exactly zero"
    group = ("emulated " if emulated else "") + GROUP[name]
    assert_within(out, ref, ref32, T, group, what, rel_floor=True, extra=r64.get("x_" + name))


# ------------------------------------------------------------------------------------------------
# CPU: the reference against torch, the emulation against the tolerance
# ------------------------------------------------------------------------------------------------
def _sdpa_inputs(B, Hq, Hkv, T, S, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(s, dtype=F64, generator=g) for s in ((B, Hq, T, D), (B, Hkv, S, D), (B, Hkv, S, D), (B, Hq, T, D)))


@pytest.mark.parametrize("T,S", [(5, 11), (11, 5), (7, 7)])
@pytest.mark.parametrize("Hkv", [4, 2, 1])
def test_reference_matches_sdpa_cpu(Hkv, T, S):
    B, Hq, D = 2, 4, 8
    q, k, v, do = _sdpa_inputs(B, Hq, Hkv, T, S, D)
    g = torch.Generator().manual_seed(1)
    tril = torch.ones(T, S, dtype=torch.bool).tril()
    masks = [None] + [make_mask(f"{typ}_{shp}", B, Hq, T, S, g) for typ in ("bool", "float")
                      for shp in ("11", "b1", "1h", "bh", "2d", "3d", "pad")] + [make_mask("float_bh+inf", B, Hq, T, S, g)]
    for mask in masks:
        for causal in (False, True):
            for scale in (None, 0.3):
                isf = mask is not None and mask.dtype != torch.bool
                qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
                ma = mask.to(F64).requires_grad_(True) if isf else mask
                am = ma
                if causal:  # top-left aligned, as torch's is_causal
                    am = tril if mask is None else (ma & tril if not isf else ma + torch.zeros(T, S, dtype=F64).masked_fill(~tril, NEG_INF))
                exp = F.scaled_dot_product_attention(qa, ka.repeat_interleave(Hq // Hkv, 1), va.repeat_interleave(Hq // Hkv, 1),
                                                     attn_mask=am, scale=scale)
                exp.backward(do)
                r = ref_attention(q, k, v, do, mask, causal, None, 0.0, scale, want_dmask=isf)
                pairs = [(r["o"], exp), (r["dq"], qa.grad), (r["dk"], ka.grad), (r["dv"], va.grad)]
                if isf:
                    pairs.append((r["dmask"], ma.grad))
                for a, b in pairs:
                    torch.testing.assert_close(a, b.detach(), atol=1e-12, rtol=1e-11)
                if mask is None and causal:
                    exp2 = F.scaled_dot_product_attention(q, k.repeat_interleave(Hq // Hkv, 1), v.repeat_interleave(Hq // Hkv, 1),
                                                          is_causal=True, scale=scale)
                    torch.testing.assert_close(r["o"], exp2, atol=1e-12, rtol=1e-11)
                    kk = k.repeat_interleave(Hq // Hkv, 1)
                    s = (q @ kk.transpose(-1, -2) * (scale or D ** -0.5)).masked_fill(~tril, NEG_INF)
                    torch.testing.assert_close(r["lse"], torch.logsumexp(s, -1), atol=1e-12, rtol=1e-12)


def test_reference_dropout_and_rope_match_autograd_cpu():
    B, Hq, Hkv, T, S, D, p = 2, 4, 2, 9, 13, 8, 0.5
    q, k, v, do = _sdpa_inputs(B, Hq, Hkv, T, S, D, seed=2)
    keep = keep_mask(SEED, OFFSET, B, Hq, T, S, p, "cpu")
    assert 0.3 < keep.float().mean().item() < 0.7
    g = torch.Generator().manual_seed(3)
    mask = make_mask("float_1h+inf", B, Hq, T, S, g).to(F64)
    qa, ka, va, ma = (t.clone().requires_grad_(True) for t in (q, k, v, mask))
    s = qa @ ka.repeat_interleave(2, 1).transpose(-1, -2) * D ** -0.5 + ma
    o = (torch.softmax(s, -1) * keep / (1 - p)) @ va.repeat_interleave(2, 1)
    o.backward(do)
    r = ref_attention(q, k, v, do, mask, False, keep, p, want_dmask=True)
    for a, b in ((r["o"], o), (r["dq"], qa.grad), (r["dk"], ka.grad), (r["dv"], va.grad), (r["dmask"], ma.grad)):
        torch.testing.assert_close(a, b.detach(), atol=1e-12, rtol=1e-11)
    # rotate-half backward against autograd of the forward rotation
    x = torch.randn(B, Hq, T, D, dtype=F64, generator=g).requires_grad_(True)
    cos, sin = torch.rand(T, D, dtype=F64, generator=g) * 2 - 1, torch.rand(T, D, dtype=F64, generator=g) * 2 - 1
    y = x * cos + torch.cat((-x[..., D // 2:], x[..., :D // 2]), -1) * sin
    y.backward(do)
    torch.testing.assert_close(rope_bwd(do, cos, sin), x.grad, atol=1e-13, rtol=1e-12)


@pytest.mark.parametrize("kind", ["bool_bh+dead_mid", "float_1h+inf+dead_last", "bool_11+dead_wave"])
def test_reference_fully_masked_rows_cpu(kind):
    """The convention torch has no answer for (its softmax of an all -inf row is NaN): a fully masked row is
    O = 0, lse = -inf, dQ = 0, dmask = 0, and every other output is what the batch without those query rows
    gives."""
    B, Hq, Hkv, T, S, D = 2, 4, 2, 70, 21, 8
    q, k, v, do = _sdpa_inputs(B, Hq, Hkv, T, S, D, seed=4)
    mask = make_mask(kind, B, Hq, T, S, torch.Generator().manual_seed(5))
    isf = mask.dtype != torch.bool
    rows = _dead_rows(kind, T)
    live = [t for t in range(T) if t not in rows]
    r = ref_attention(q, k, v, do, mask, False, None, 0.0, None, want_dmask=isf)
    assert all(torch.isfinite(r[n]).all() for n in ("o", "dq", "dk", "dv"))
    assert torch.isneginf(r["lse"][..., rows]).all() and torch.isfinite(r["lse"][..., live]).all()
    assert not r["o"][..., rows, :].any() and not r["dq"][..., rows, :].any()
    sub = ref_attention(q[:, :, live], k, v, do[:, :, live], _mask4(mask)[..., live, :], False, None, 0.0, None, want_dmask=isf)
    for n in ("o", "dq"):
        torch.testing.assert_close(r[n][..., live, :], sub[n], atol=1e-13, rtol=1e-12)
    torch.testing.assert_close(r["lse"][..., live], sub["lse"], atol=1e-13, rtol=1e-12)
    for n in ("dk", "dv"):
        torch.testing.assert_close(r[n], sub[n], atol=1e-13, rtol=1e-12)
    if isf:
        assert not r["dmask"][..., rows, :].any()
        torch.testing.assert_close(r["dmask"][..., live, :], sub["dmask"], atol=1e-13, rtol=1e-12)


def test_case_list_reaches_every_path_cpu():
    """The lists above name what the issue names; a shape dropped by mistake fails here, not silently."""
    def has(**kw):
        return any(all(getattr(c, a) == b for a, b in kw.items()) for c in CASES)

    for T in (1, 33, 127, 128, 129):
        assert has(tag="v1", T=T, D=64) and has(tag="v1", T=T, D=256, hook="ring0") and has(tag="v1", T=T, D=128, hook="impl0")
    for S in (1, 63, 64, 65, 129, 127, 257):
        assert has(tag="v1", S=S, D=64) and has(tag="v1", S=S, D=96)
    assert has(tag="v1", S=31, D=256) and has(tag="v1", S=33, D=256)
    for T in (1, 63, 65, 255, 256, 257, 33, 513):
        assert has(tag="v4", T=T, hook="") and (T in (33, 513) or has(tag="v4", T=T, hook="impl9"))
    for S in (1, 64, 65, 257, 321, 577, 33, 255, 513):
        assert has(tag="v4", S=S, hook="")
    for S in (1, 31, 32, 33, 97, 129, 161):
        assert has(tag="d256", S=S, causal=False)
    for T in (128, 129, 200):
        assert has(tag="d256", T=T, S=T, causal=True)
    for T in (1, 31, 33, 65, 129):
        assert has(tag="v1", T=T, D=64)
    for D in (32, 80, 112, 192):
        assert has(tag="pad", D=D)
    for T in (64, 256, 320, 200):
        assert has(rope="ds0", T=T) and has(rope="ds1", T=T) and has(rope="ds1", T=T, split="1")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("tag", sorted({c.tag for c in CASES}))
def test_emulation_within_tolerance_cpu(tag, dtype):
    """Every case with the fp32 evaluation that applies exactly the modelled roundings (P, the O under delta,
    dS, the outputs) in place of the kernel: none may exceed 1.0 of its tolerance."""
    for c in (c for c in CASES if c.tag == tag):
        emu = _evaluate(c, dtype, F32, round_to=dtype)
        for name in (("dqkv",) if c.rope else ("o", "lse", "dq", "dk", "dv") + (("dmask",) if c.mask_grad else ())):
            out = emu[name] if name in ("lse", "dmask") else emu[name].to(dtype)
            check(c, dtype, name, out, emulated=True)


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
_FWD_SIG = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p,
                                                                          ctypes.c_void_p]


@pytest.fixture
def lib():
    import lightning_thunder_amd.ops.attention  # noqa: F401  (registers the signatures on the real entries first)
    from lightning_thunder_amd.ops import _lib

    _lib.register_signature("lta_attn_fwd_v4", _FWD_SIG + [ctypes.c_int, ctypes.c_void_p])
    _lib.register_signature("lta_attn_fwd_d256", _FWD_SIG + [ctypes.c_void_p])
    return _lib.require()


@pytest.fixture
def spy(lib, monkeypatch):
    """Records the arguments of every native attention launch, by entry."""
    calls = {}
    for name in ("lta_attn_fwd_ex2", "lta_attn_bwd_ex3", "lta_attn_set_gqa_workspace", "lta_attn_bwd_rope",
                 "lta_attn_bwd_rope_ds"):
        real = getattr(lib, name)
        calls[name] = []

        def wrap(*a, _real=real, _log=calls[name]):
            _log.append(a)
            return _real(*a)

        monkeypatch.setattr(lib, name, wrap)
    return calls


def off1(t):
    """A copy of ``t`` that starts one element into a larger buffer: rows not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0
    return out


def tmajor(t):
    """``t`` [B, H, T, D] as the head-split view of a token-major [B, T, H, D] buffer."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def place(c, dtype):
    """The case's inputs on the device in the storage the case names."""
    i = inputs(c, dtype)
    q, k, v, do = (i[n].cuda() for n in ("q", "k", "v", "do"))
    if c.layout == "views":
        assert c.T == c.S
        proj = torch.cat([t.transpose(1, 2).flatten(2) for t in (q, k, v)], -1)  # [B, T, (Hq + 2 Hkv) D]
        heads = proj.view(c.B, c.T, c.Hq + 2 * c.Hkv, c.D).transpose(1, 2)
        q, k, v = heads[:, :c.Hq], heads[:, c.Hq:c.Hq + c.Hkv], heads[:, c.Hq + c.Hkv:]
        assert q.data_ptr() == proj.data_ptr() and not k.is_contiguous()
    elif c.layout == "tmajor":
        q, k, v = tmajor(q), tmajor(k), tmajor(v)
    elif c.layout == "misaligned":
        q, k, v, do = off1(q), off1(k), off1(v), off1(do)
    if c.do_layout == "bthd":
        do = tmajor(do)
    mask = None if i["mask"] is None else i["mask"].cuda()
    return q, k, v, do, mask


class Hooks:
    """The forward's A/B hooks for one case; restores what the setters returned."""

    def __init__(self, lib, hook):
        self.lib, self.hook = lib, hook

    def __enter__(self):
        self.old_impl = self.old_ring = None
        if self.hook in ("impl0", "impl9"):
            self.old_impl = self.lib.lta_attn_fwd_set_impl(int(self.hook[4:]))
        elif self.hook == "ring0":
            self.old_ring = self.lib.lta_attn_fwd_set_ring(0)
        return self

    def __exit__(self, *exc):
        if self.old_impl is not None:
            was = self.lib.lta_attn_fwd_set_impl(self.old_impl)
            assert was == int(self.hook[4:]), "the impl hook did not hold during the call"
        if self.old_ring is not None:
            was = self.lib.lta_attn_fwd_set_ring(self.old_ring)
            assert was == 0, "the ring hook did not hold during the call"
        return False


def run_forward(c, dtype, lib, spy, q, k, v, mask):
    from lightning_thunder_amd.ops.attention import attn_fwd, padded_head_dim

    spy["lta_attn_fwd_ex2"].clear()
    with Hooks(lib, c.hook):
        o, lse = attn_fwd(q, k, v, c.causal, c.sc, c.out_layout, mask, c.p, SEED, OFFSET)
        assert len(spy["lta_attn_fwd_ex2"]) == 1
        a = spy["lta_attn_fwd_ex2"][0]
        if c.path and padded_head_dim(c.D) == c.D:
            # the path taken: the exported kernel entry accepts the very same arguments (0, not -1) and gives
            # the same bits
            o2, lse2 = torch.empty_like(o), torch.empty_like(lse)
            assert o2.stride() == o.stride()
            head = a[:4] + (o2.data_ptr(), lse2.data_ptr()) + a[6:15] + (a[21],)
            if c.path == "v4":
                rc = lib.lta_attn_fwd_v4(*head, 0 if c.hook == "impl9" else 1, a[22])
            else:
                rc = lib.lta_attn_fwd_d256(*head, a[22])
            assert rc == 0, f"{c.id}: the {c.path} entry returned {rc}"
            assert bits_equal(o2, o) and bits_equal(lse2, lse), f"{c.id}: attn_fwd did not run the {c.path} kernel"
    if padded_head_dim(c.D) == c.D:
        if c.layout in ("views", "tmajor"):  # read in place
            assert (a[1], a[2], a[3]) == (q.data_ptr(), k.data_ptr(), v.data_ptr())
        elif c.layout == "misaligned":  # the copy fallback of _rows_ok
            assert a[1] != q.data_ptr() and a[2] != k.data_ptr() and a[3] != v.data_ptr()
        assert (o.transpose(1, 2) if c.out_layout == "bshd" else o).is_contiguous()
    assert o.shape == q.shape and lse.shape == q.shape[:3]
    return o, lse


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("c", PLAIN, ids=_ids(PLAIN))
def test_attention_fwd_bwd(c, dtype, lib, spy, monkeypatch):
    from lightning_thunder_amd.ops.attention import attn_bwd, padded_head_dim

    q, k, v, do, mask = place(c, dtype)
    o, lse = run_forward(c, dtype, lib, spy, q, k, v, mask)
    check(c, dtype, "o", o)
    check(c, dtype, "lse", lse)
    if c.split:
        monkeypatch.setenv("LTA_ATTN_GQA_SPLIT", c.split)
    else:
        monkeypatch.delenv("LTA_ATTN_GQA_SPLIT", raising=False)
    res = attn_bwd(do, q, k, v, o, lse, c.causal, c.sc, mask, c.p, SEED, OFFSET, c.mask_grad)
    assert len(spy["lta_attn_bwd_ex3"]) == 1
    group = c.Hq // c.Hkv
    splits = [a[2] for a in spy["lta_attn_set_gqa_workspace"]]
    if group > 1 and not c.mask and not c.p:  # small grids: the largest divisor of the group up to the cap
        want = max(d for d in range(1, group + 1) if group % d == 0 and d <= int(c.split or 8))
        assert splits == ([want] if want > 1 else []), (c.id, splits)
    else:
        assert splits == []
    if padded_head_dim(c.D) == c.D and c.layout in ("views", "tmajor") and c.T > 1:
        # gradients of head-split views take their operand's order: the transposed branch of _grad_like
        assert all(g.transpose(1, 2).is_contiguous() for g in res[:3])
    for name, g in zip(("dq", "dk", "dv", "dmask"), res):
        check(c, dtype, name, g)
    if c.mask_grad:
        assert res[3].shape == inputs(c, dtype)["mask"].shape


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("c", FUSED, ids=_ids(FUSED))
def test_attention_bwd_fused_rope(c, dtype, lib, spy, monkeypatch):
    from lightning_thunder_amd.ops.attention import attn_bwd_rope

    q, k, v, do, _ = place(c, dtype)
    i = inputs(c, dtype)
    o, lse = run_forward(c, dtype, lib, spy, q, k, v, None)
    monkeypatch.setenv("LTA_ATTN_DQ_FROM_DS", c.rope[2])
    if c.split:
        monkeypatch.setenv("LTA_ATTN_GQA_SPLIT", c.split)
    else:
        monkeypatch.delenv("LTA_ATTN_GQA_SPLIT", raising=False)
    dqkv = attn_bwd_rope(do, q, k, v, o, lse, c.causal, c.sc, i["cos"].cuda(), i["sin"].cuda(), c.Hq, c.Hkv)
    ds, plain = spy["lta_attn_bwd_rope_ds"], spy["lta_attn_bwd_rope"]
    if c.rope == "ds1" and c.T % 64 == 0:
        assert (len(ds), len(plain)) == (1, 0), "the dQ-from-dS entry must have run"
        hsplit = ds[0][-2]
    else:  # switched off, or T % 64 != 0: the recompute entry, and no two-pass fallback
        assert (len(ds), len(plain)) == (0, 1) and not spy["lta_attn_bwd_ex3"]
        hsplit = plain[0][-2]
    group = c.Hq // c.Hkv
    assert hsplit == (1 if c.split == "1" or group == 1 else group), (c.id, hsplit)
    check(c, dtype, "dqkv", dqkv)


IDENTITY = [(64, ""), (128, ""), (128, "impl9"), (256, ""), (96, "")]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,hook", IDENTITY)
def test_batch_head_order_is_bitwise_irrelevant(D, hook, causal, dtype, lib):
    """O, lse, dQ, dK, dV of a batch with permuted (batch, head) order are the permutation of the original, and
    O / lse of the [B, H] run are those of the B = 1, H = 1 run of each slice: no workgroup depends on its
    place in the grid."""
    from lightning_thunder_amd.ops.attention import attn_bwd, attn_fwd

    c = C("ident", 2, 3, 3, 130, 200, D, causal=causal, hook=hook)
    q, k, v, do, _ = place(c, dtype)
    pb, ph = torch.tensor([1, 0], device="cuda"), torch.tensor([2, 0, 1], device="cuda")
    perm = lambda t: t[pb][:, ph].contiguous()  # noqa: E731
    with Hooks(lib, hook):
        o, lse = attn_fwd(q, k, v, causal, out_layout="bhsd")
        o2, lse2 = attn_fwd(perm(q), perm(k), perm(v), causal, out_layout="bhsd")
        assert bits_equal(o2, perm(o)) and bits_equal(lse2, perm(lse))
        for b in range(c.B):
            for h in range(c.Hq):
                o1, lse1 = attn_fwd(q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1], causal, out_layout="bhsd")
                assert bits_equal(o1[0, 0], o[b, h]) and bits_equal(lse1[0, 0], lse[b, h]), (b, h)
    g = attn_bwd(do, q, k, v, o, lse, causal)
    g2 = attn_bwd(perm(do), perm(q), perm(k), perm(v), o2, lse2, causal)
    for name, a, b in zip(("dq", "dk", "dv"), g, g2):
        assert bits_equal(b, perm(a)), name


@gpu
def test_zz_report_worst_ratios():
    """Prints the table of the header (run the file with -s); every entry was already asserted <= 1."""
    for (group, dt), ratio in sorted(_WORST.items()):
        if group in GROUP.values():
            print(f"worst err/tol  {group:16s} {dt:9s} {ratio:.3f}")
            assert ratio <= 1.0
