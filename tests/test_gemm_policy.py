"""Static GEMM dispatch rules (ops/gemm.py): the K-split choice for under-filled tile grids, and the
launch decided for a call's operands (driven on the CPU: stand-in tensors, no native library)."""
import pytest
import torch

from lightning_thunder_amd.ops import gemm as G
from lightning_thunder_amd.ops.gemm import splitk_factor


@pytest.mark.parametrize("M,N,K", [(4096, 4096, 4096), (8192, 4096, 1024), (4096, 12288, 4096)])
def test_splitk_off_for_full_waves(M, N, K):
    assert splitk_factor(M, N, K, 256) == 0


def test_splitk_off_for_short_k():
    # 128 tiles x K=1024: the partial traffic costs more than the idle half of the chip
    assert splitk_factor(8192, 1024, 1024, 256) == 0
    assert splitk_factor(8192, 1024, 1000, 256) == 0  # K % 128: not a gemm4 shape


@pytest.mark.parametrize("M,N,K", [(1024, 1024, 8192), (3072, 1024, 8192), (4096, 1024, 8192), (8192, 1024, 4096),
                                   (8192, 1024, 50304), (1000, 1000, 4096)])
def test_splitk_fills_at_most_one_wave(M, N, K):
    nwg = -(-M // 256) * -(-N // 256)
    s = splitk_factor(M, N, K, 256)
    assert s >= 2
    assert nwg * s <= 256
    assert K // 128 >= s  # every slice gets at least one 128-deep K pair
    # fewer CUs: fewer slices
    assert splitk_factor(M, N, K, 128) <= s


class _OnGpu(torch.Tensor):
    """A tensor that says it is on the GPU: the decision reads shapes, strides, dtypes and pointer alignment only."""
    is_cuda = True


def _t(*shape, dtype=torch.bfloat16, device="meta"):
    """No storage by default (a meta tensor's data_ptr is its byte offset, so views keep their alignment)."""
    return torch.empty(shape, dtype=dtype, device=device).as_subclass(_OnGpu)


def _lin(M, N, K, bias=False, res=False, act=None, dtype=torch.bfloat16, x=None, w=None, r=None):
    """The arguments linear hands to the decision: x [M,K], the weight [N,K], bias, residual, act."""
    x = _t(M, K, dtype=dtype) if x is None else x
    w = _t(N, K, dtype=dtype) if w is None else w
    r = (_t(M, N, dtype=dtype) if res else None) if r is None else r
    return dict(a=x, b=w, bias=_t(N, dtype=dtype) if bias else None, residual=r, act=act, linear=True)


def _mm(a, b, r=None):
    return dict(a=a, b=b, bias=None, residual=r, act=None, linear=False)


T = 65536  # fp32 workspace elements of one 256 x 256 tile
# (operands, LTA_GEMM mode, CUs, the entry point and scalars the parent of this table's commit launched)
_CASES = {
    # Llama-2-7B step, M = 4096
    "llama qkv fwd": (lambda: _lin(4096, 12288, 4096), "auto", 256, dict(entry=G.GEMM4, at=0, bt=0, variant=1)),
    "llama gate/up fwd: tail split": (lambda: _lin(4096, 22016, 4096), "auto", 256,
                                      dict(entry=G.GEMM4_TAIL, at=0, bt=0, tail=96, ws=2 * 96 * T, lda=4096, ldb=4096)),
    "llama gate/up fwd, 128 CUs: whole waves": (lambda: _lin(4096, 22016, 4096), "auto", 128, dict(entry=G.GEMM4)),
    "llama gate/up wgrad: tail split": (lambda: _mm(_t(4096, 22016).t(), _t(4096, 4096)), "auto", 256,
                                        dict(entry=G.GEMM4_TAIL, at=1, bt=1, tail=96, lda=22016, ldb=4096)),
    "llama down dgrad + residual": (lambda: _mm(_t(4096, 4096), _t(4096, 11008), _t(4096, 11008)), "auto", 256,
                                    dict(entry=G.GEMM4, at=0, bt=1, ldr=11008, ksplit=0, tail=0)),
    "llama head + residual": (lambda: _lin(4096, 32000, 4096, res=True), "auto", 256,
                              dict(entry=G.GEMM4, ldr=32000, M=4096, N=32000, K=4096)),
    # GPT-2-medium, M = 8192
    "gpt2 proj bias": (lambda: _lin(8192, 1024, 1024, bias=True), "auto", 256, dict(entry=G.GEMM4, act=None)),
    "gpt2 proj bias gelu": (lambda: _lin(8192, 1024, 1024, bias=True, act="gelu_tanh"), "auto", 256,
                            dict(entry=G.GEMM4, act="gelu_tanh")),
    "gpt2 mlp down bias: split-K carries the bias": (lambda: _lin(8192, 1024, 4096, bias=True), "auto", 256,
                                                     dict(entry=G.GEMM4_SPLITK, ksplit=2, ws=2 * 128 * T)),
    "gpt2 mlp down bias, 128 CUs": (lambda: _lin(8192, 1024, 4096, bias=True), "auto", 128, dict(entry=G.GEMM4)),
    "gpt2 mlp down wgrad": (lambda: _mm(_t(8192, 1024).t(), _t(8192, 4096)), "auto", 256,
                            dict(entry=G.GEMM4_SPLITK, at=1, bt=1, ksplit=4, ws=4 * 64 * T)),
    "gpt2 mlp down wgrad, 128 CUs": (lambda: _mm(_t(8192, 1024).t(), _t(8192, 4096)), "auto", 128,
                                     dict(entry=G.GEMM4_SPLITK, ksplit=2)),
    "gpt2 mlp up dgrad": (lambda: _mm(_t(8192, 3072), _t(3072, 1024)), "auto", 256,
                          dict(entry=G.GEMM4_SPLITK, at=0, bt=1, ksplit=2)),
    "gpt2 mlp up plain: tail of 128": (lambda: _lin(8192, 3072, 1024), "auto", 256, dict(entry=G.GEMM4_TAIL, tail=128)),
    "gpt2 head bias gelu": (lambda: _lin(8192, 50304, 1024, bias=True, act="gelu_tanh"), "auto", 256,
                            dict(entry=G.GEMM4)),
    # decode rows
    "4 rows": (lambda: _lin(4, 512, 512), "auto", 256, dict(entry=G.GEMV)),
    "8 rows fp16": (lambda: _lin(8, 512, 512, dtype=torch.float16), "auto", 256, dict(entry=G.GEMV)),
    "9 rows": (lambda: _lin(9, 512, 512), "auto", 256, dict(entry=G.TORCH_LINEAR)),
    "63 rows: below GEMM4_MIN_M": (lambda: _lin(63, 512, 512), "auto", 256, dict(entry=G.TORCH_LINEAR)),
    "64 rows": (lambda: _lin(64, 512, 512), "auto", 256, dict(entry=G.GEMM4_SPLITK, ksplit=4)),
    "512 rows fp16": (lambda: _lin(512, 512, 512, dtype=torch.float16), "auto", 256, dict(entry=G.TORCH_LINEAR)),
    # edge tiles, the 8-wave kernel, odd K, tail split, split-K
    "edge 1000 x 16032": (lambda: _lin(1000, 16032, 256), "auto", 256, dict(entry=G.GEMM4, lda=256, ldb=256)),
    "edge 300 x 50304": (lambda: _lin(300, 50304, 128), "auto", 256, dict(entry=G.GEMM4)),
    "edge 777 x 1000": (lambda: _lin(777, 1000, 384), "auto", 256, dict(entry=G.GEMM4)),
    "K % 128: 8-wave NT": (lambda: _lin(512, 512, 192), "auto", 256, dict(entry=G.GEMM_NT)),
    "K % 128: 8-wave layout": (lambda: _mm(_t(512, 192), _t(512, 192).t()), "auto", 256, dict(entry=G.GEMM_LAYOUT)),
    "K % 64": (lambda: _lin(512, 512, 100), "auto", 256, dict(entry=G.TORCH_LINEAR)),
    "N % 8": (lambda: _mm(_t(512, 1024), _t(1004, 1024).t()), "auto", 256, dict(entry=G.TORCH_MM)),
    "tail of 2": (lambda: _lin(512, 33024, 256), "auto", 256, dict(entry=G.GEMM4_TAIL, tail=2, ws=2 * 2 * T)),
    "tail of 2, 128 CUs": (lambda: _lin(512, 33024, 256), "auto", 128, dict(entry=G.GEMM4_TAIL, tail=2)),
    "a bias ends the tail split": (lambda: _lin(512, 33024, 256, bias=True), "auto", 256, dict(entry=G.GEMM4)),
    "split-K": (lambda: _lin(1024, 1024, 1024), "auto", 256, dict(entry=G.GEMM4_SPLITK, ksplit=4, ws=4 * 16 * T)),
    "a residual ends the K split": (lambda: _lin(1024, 1024, 1024, res=True), "auto", 256,
                                    dict(entry=G.GEMM4, ldr=1024)),
    "split-K tt": (lambda: _mm(_t(8192, 1024).t(), _t(1024, 8192).t()), "auto", 256,
                   dict(entry=G.GEMM4_SPLITK, at=1, bt=0, ksplit=11, lda=1024, ldb=8192)),
    "split-K tt, 128 CUs": (lambda: _mm(_t(8192, 1024).t(), _t(1024, 8192).t()), "auto", 128,
                            dict(entry=G.GEMM4_SPLITK, ksplit=8)),
    # operand layouts the hand kernels refuse or take
    "x column slice": (lambda: _lin(2048, 4608, 1536, x=_t(2048, 3080)[:, :1536]), "auto", 256,
                       dict(entry=G.GEMM4, lda=3080)),
    "x at an odd element": (lambda: _lin(2048, 4608, 1536, x=_t(2048, 3080)[:, 1:1537]), "auto", 256,
                            dict(entry=G.TORCH_LINEAR)),
    "w stored transposed": (lambda: _lin(2048, 4608, 1536, w=_t(1536, 4608).t()), "auto", 256,
                            dict(entry=G.TORCH_LINEAR)),
    "residual pitch % 8, linear": (lambda: _lin(2048, 4608, 1536, r=_t(2048, 4612)[:, :4608]), "auto", 256,
                                   dict(entry=G.TORCH_LINEAR)),
    "residual pitch % 8, matmul": (lambda: _mm(_t(2048, 1536), _t(4608, 1536).t(), _t(2048, 4612)[:, :4608]),
                                   "auto", 256, dict(entry=G.TORCH_MM)),
    "MN-major a with M % 8": (lambda: _mm(_t(512, 1004).t(), _t(512, 1024)), "auto", 256, dict(entry=G.TORCH_MM)),
    "MN-major a with M % 8 == 0": (lambda: _mm(_t(512, 1008).t(), _t(512, 1024)), "auto", 256,
                                   dict(entry=G.GEMM4, at=1, bt=1, lda=1008)),
    "a past 32-bit offsets": (lambda: _lin(4096, 512, 512, x=_t(4096, 262144)[:, :512]), "auto", 256,
                              dict(entry=G.GEMM_NT)),
    "a within 32-bit offsets": (lambda: _lin(4088, 512, 512, x=_t(4096, 262144)[:4088, :512]), "auto", 256,
                                dict(entry=G.GEMM4, lda=262144)),
    "fp32 linear": (lambda: _lin(512, 512, 512, dtype=torch.float32), "auto", 256, dict(entry=G.TORCH_LINEAR)),
    "fp32 matmul": (lambda: _mm(_t(512, 512, dtype=torch.float32), _t(512, 512, dtype=torch.float32)), "auto", 256,
                    dict(entry=G.TORCH_MM)),
    # LTA_GEMM=torch
    "mode torch, linear": (lambda: _lin(4096, 12288, 4096), "torch", 256, dict(entry=G.TORCH_LINEAR)),
    "mode torch, rows": (lambda: _lin(4, 512, 512), "torch", 256, dict(entry=G.TORCH_LINEAR)),
    "mode torch, matmul": (lambda: _mm(_t(8192, 1024).t(), _t(8192, 4096)), "torch", 256, dict(entry=G.TORCH_MM)),
}


@pytest.mark.parametrize("name", list(_CASES))
def test_decision_table(name):
    """The decision function gives the entry point and scalars that the dispatch launched before the
    rule chain, the plans and matmul4's split conditions became this one function."""
    build, mode, cus, want = _CASES[name]
    d = G._decide(**build(), mode=mode, cus=cus)
    got = {k: getattr(d, k) for k in want}
    assert got == want, d
    if d.entry not in (G.GEMM4_SPLITK, G.GEMM4_TAIL):
        assert (d.ksplit, d.tail, d.ws) == (0, 0, 0), d
    if d.entry in (G.GEMM4, G.GEMM4_SPLITK, G.GEMM4_TAIL):
        assert d.variant == 1, d


class _Recorder:
    """Stands for the native library: records (entry name, arguments) and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.fixture
def cpu_dispatch(monkeypatch):
    lib = _Recorder()
    decided = []
    decide = G._decide
    monkeypatch.setattr(G, "require", lambda: lib)
    monkeypatch.setattr(G, "stream_ptr", lambda device=None: 0)
    monkeypatch.setattr(G, "_device_cus", lambda device: 256)
    monkeypatch.setattr(G, "_PLANS", {})
    monkeypatch.setattr(G, "_WS", {})
    monkeypatch.setattr(G, "_decide", lambda *a, **kw: decided.append(decide(*a, **kw)) or decided[-1])
    monkeypatch.setattr(G, "_torch_linear", lambda x, w, b, r, act: lib.calls.append(("torch", ())) or
                        torch.empty(x.shape[0], w.shape[0]))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 0}))
    monkeypatch.delenv("LTA_GEMM", raising=False)
    return lib, decided


def test_repeated_site_reuses_the_record(cpu_dispatch, monkeypatch):
    lib, decided = cpu_dispatch
    G.last_gemm_backend_counts(reset=True)
    x, w = _t(8, 128, 1024, device="cpu"), _t(1024, 1024, device="cpu")
    bias = _t(1032, device="cpu")[3:1027]  # a bias slice at an odd element
    outs = [G.linear(x, w, bias) for _ in range(3)]
    assert len(decided) == 1 and decided[0].entry == G.GEMM4_SPLITK and list(G._PLANS.values()) == decided
    assert [o.shape for o in outs] == [(8, 128, 1024)] * 3
    names, args = zip(*lib.calls)
    assert names == ("lta_gemm4_bf16_splitk",) * 3
    for a in args:  # the replays launch what the first call launched, on an aligned copy of the bias
        assert a[:3] == (x.data_ptr(), w.data_ptr(), a[2]) and a[3] % 16 == 0 and a[3] != bias.data_ptr()
        assert a[4:14] == args[0][4:14] == (1024, 1024, 1024, 1024, 1024, 1024, 1.0, 0, 0, 4)
    # a reshape that copied is decided on every call and never recorded
    xc = _t(128, 8, 1024, device="cpu").transpose(0, 1)
    for _ in range(2):
        G.linear(xc, w)
    assert len(decided) == 3 and len(G._PLANS) == 1
    # LTA_GEMM is part of the site: torch mode does not hit the record made under auto, nor the reverse
    monkeypatch.setenv("LTA_GEMM", "torch")
    G.linear(x, w, bias)
    assert len(decided) == 4 and decided[-1].entry == G.TORCH_LINEAR and lib.calls[-1][0] == "torch"
    G.linear(x, w, bias)
    assert len(decided) == 4 and lib.calls[-1][0] == "torch" and len(G._PLANS) == 2
    monkeypatch.delenv("LTA_GEMM")
    G.linear(x, w, bias)
    assert len(decided) == 4 and lib.calls[-1][0] == "lta_gemm4_bf16_splitk"
    assert G.last_gemm_backend_counts(reset=True).get("torch") == 2


def test_matmul4_takes_gemm4_or_raises(cpu_dispatch):
    """matmul4 launches gemm4 with the caller's variant, splits K only where the rule allows (variant 1,
    no residual or activation, a bias only in the forward layout), and raises on other operands."""
    lib, _ = cpu_dispatch
    x, w, g = _t(1024, 1024, device="cpu"), _t(1024, 1024, device="cpu"), _t(1024, 1024, device="cpu")
    bias = _t(1024, device="cpu")

    def launch(*args, **kw):
        del lib.calls[:]
        G.matmul4(*args, **kw)
        (name, a), = lib.calls
        return name, a

    assert launch(x, w.t())[0] == "lta_gemm4_bf16_splitk"
    assert launch(x, w.t(), bias=bias)[0] == "lta_gemm4_bf16_splitk"  # forward layout: the fixup adds the bias
    name, a = launch(g.t(), x, bias=bias)  # a bias on a transposed layout ends the K split
    assert name == "lta_gemm4_bf16" and a[3] == bias.data_ptr() and a[14:17] == (1, 1, 1)
    name, a = launch(x, w.t(), variant=0)  # only variant 1 splits
    assert name == "lta_gemm4_bf16" and a[14:17] == (0, 0, 0)
    assert launch(x, w.t(), bias=bias, act="silu")[0] == "lta_gemm4_bf16"
    name, a = launch(x, w.t(), residual=_t(1024, 1028, device="cpu")[:, :1024])  # any row pitch when called directly
    assert name == "lta_gemm4_bf16" and a[11] == 1028
    with pytest.raises(ValueError):
        G.matmul4(_t(8, 1024, device="cpu"), w.t())
    with pytest.raises(AssertionError):  # a residual of another shape never reaches the kernel
        G.matmul4(x, w.t(), residual=_t(1024, 2048, device="cpu"))
    with pytest.raises(AssertionError):
        G.matmul(x, w.t(), _t(1024, 2048, device="cpu"))
    with pytest.raises(AssertionError):
        G.matmul4(x, w.t(), bias=_t(1024, dtype=torch.float32, device="cpu"))
