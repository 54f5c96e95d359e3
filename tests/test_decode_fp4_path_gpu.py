"""The W4A8 decode path (`args.fp4_decode_weights`) at layer level, following tests/test_decode_fp8_path_gpu.py: where the fp8 decode
path would run (a call that needs no backward, at most decode_rows() routed rows, `args.fp8_experts` and `args.fp8_weight_cache`), the
T token rows are quantised to MXFP8 where they lie and both expert GEMMs run on csmoe_grouped_gemm_skinny_mxfp4w over MXFP4 weight
tables of a cache of their own; every other call does what it does with the flag off, bit for bit.  Which path ran is read from
ops.profile_start/stop.

Outputs are held to MX_OUT = 3e-3 relative L2 (the project's bound for the fp8 paths) against oracle/mxfp8.py fed the DEQUANTISED
MXFP4 masters: the oracle's own MXFP8 quantiser gives such a table back unchanged (tests/test_mxfp4_cpu.py), so that is an exact
emulation of W4A8 -- the quality cost of 4-bit weights is not in this number.  The routing is that of the flag-off run.
Measured on MI355X (relative L2 against that oracle):
  smoe relu: T=1 0.00e+00  T=3 0.00e+00  T=16 1.20e-04  T=17 2.50e-04
  smoe gelu: T=1 2.99e-04  T=3 1.29e-03  T=16 1.98e-04  T=17 3.55e-04
  deepseekv2, T=5: 1.99e-03
(the fp8 decode path against its own oracle on the same inputs: relu 0 / 6.68e-05 / 2.26e-04 / 4.77e-04, gelu 0 / 1.76e-04 /
5.82e-04 / 6.47e-04; the two oracles are 0.17 - 0.20 apart: that is the 4-bit weights, not the kernel)"""
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import competesmoe_amd
    from competesmoe_amd import ops
    from competesmoe_amd import functional as Fn

from oracle import mxfp8 as MX
from oracle import moe_oracle as O
from tests import mxfp4_ref as R4
from tests.golden_util import rel_l2

DEV = "cuda"
BF = torch.bfloat16
MX_OUT = 3e-3                                                   # tests/test_fp8_gpu.py
D, FH, E, K = 128, 256, 8, 2
PRETRAIN_ARGS = dict(stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
                     balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False,
                     tribrid=False, balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False,
                     scale_weight=1.0, test_only=False, n_shared_experts=2)
DISPATCH = ("dispatch_tokens_mxfp8", "dispatch_rows_mxfp8", "dispatch_tokens", "dispatch_rows")


def _layer(name, act, bias, seed, cache=True, fp4=True, fp8=True):
    from competesmoe_amd.pretrain import get_moe
    torch.manual_seed(seed)
    args = types.SimpleNamespace(**PRETRAIN_ARGS, fp8_experts=fp8, fp8_weight_cache=cache, fp4_decode_weights=fp4)
    layer = get_moe(name)(D, E, FH, n_heads=K, activation=act, bias=bias, log_interval=None, args=args).to(DEV).to(BF).eval()
    if bias:
        with torch.no_grad():
            layer.bias.copy_(torch.randn(layer.bias.shape) * 0.1)
    return layer


def _run(layer, x, rows, monkeypatch=None):
    """layer(x) with decode_rows(rows) in force (undone afterwards); returns (output, profile, routing indices seen by bin_tokens)."""
    seen = []
    if monkeypatch is not None:
        orig = ops.bin_tokens

        def spy(idx, n_experts, hist=None):
            seen.append(idx.detach().clone())
            return orig(idx, n_experts, hist)
        monkeypatch.setattr(ops, "bin_tokens", spy)
    try:
        competesmoe_amd.decode_rows(rows)
        ops.profile_start()
        try:
            out = layer(x)
        finally:
            prof = ops.profile_stop()
    finally:
        competesmoe_amd.decode_rows(0)
        if monkeypatch is not None:
            monkeypatch.undo()
    return out, prof, seen


def _calls(prof, name):
    return prof.get(name, {}).get("calls", 0)


def _assert_fp4_decode(prof, launches):
    assert _calls(prof, "grouped_gemm_skinny_mxfp4w") == launches, prof.keys()
    assert _calls(prof, "grouped_gemm_skinny_mxfp8") == 0, prof.keys()
    assert _calls(prof, "grouped_gemm_mxfp8") == 0 and _calls(prof, "dense_gemm_mxfp8") == 0, prof.keys()
    assert all(_calls(prof, n) == 0 for n in DISPATCH), prof.keys()
    assert _calls(prof, "quantize_mxfp8") == launches // 2, prof.keys()       # x once per FFN; never the hidden activations
    assert _calls(prof, "quantize_mxfp8_both") == 0 and _calls(prof, "quantize_mxfp8_t") == 0, prof.keys()


def _assert_fp8_decode(prof, launches):
    assert _calls(prof, "grouped_gemm_skinny_mxfp8") == launches, prof.keys()
    assert _calls(prof, "grouped_gemm_skinny_mxfp4w") == 0 and _calls(prof, "quantize_mxfp4_t") == 0, prof.keys()


def _assert_tiled(prof, shared=False):
    assert _calls(prof, "grouped_gemm_skinny_mxfp4w") == 0 and _calls(prof, "quantize_mxfp4_t") == 0, prof.keys()
    assert _calls(prof, "grouped_gemm_skinny_mxfp8") == 0, prof.keys()
    assert _calls(prof, "grouped_gemm_mxfp8") == 2, prof.keys()
    assert _calls(prof, "dense_gemm_mxfp8") == (2 if shared else 0), prof.keys()
    assert _calls(prof, "dispatch_tokens_mxfp8") == 1, prof.keys()


def _spy_ffn(layer):
    """Records (selected experts, weights) the layer hands to its routed FFN."""
    rec = {}
    ffn0 = layer.ffn

    def ffn(xx, sel, ww, *a, **k):
        rec["idx"], rec["w"] = sel.detach().cpu().long(), ww.detach().float().cpu()
        return ffn0(xx, sel, ww, *a, **k)
    layer.ffn = ffn
    return rec


def _w4(master):
    """The values an MXFP4 forward table of a master [.., R, C] holds (blocks along R), back in the master's layout, fp32."""
    q, s = R4.quantize(master.detach().cpu().float().transpose(-1, -2).contiguous())
    return R4.dequantize(q, s).transpose(-1, -2).contiguous().float()


def _clear():
    Fn.fp8_weight_cache_clear()
    Fn.fp4_weight_cache_clear()


@pytest.mark.parametrize("actname", ["relu", "gelu"])
def test_pretrain_smoe(actname, monkeypatch):
    layer = _layer("smoe", F.relu if actname == "relu" else F.gelu, True, 71)
    rec = _spy_ffn(layer)
    g = torch.Generator().manual_seed(72)
    _clear()
    k4, v4 = _w4(layer.keys), _w4(layer.values)
    for T in (1, 3, 16, 17):
        x = torch.randn(1, T, D, generator=g).to(BF)
        xd = x.to(DEV)
        with torch.no_grad():
            layer.fp4_decode_weights = False
            off, p_off, i_off = _run(layer, xd, 64, monkeypatch=monkeypatch)     # the fp8 decode path on the same inputs
            layer.fp4_decode_weights = True
            on, p_on, i_on = _run(layer, xd, 64, monkeypatch=monkeypatch)
        _assert_fp8_decode(p_off, 2)
        _assert_fp4_decode(p_on, 2)
        assert len(i_on) == len(i_off) == 1 and torch.equal(i_on[0], i_off[0])
        idx, w = rec["idx"].reshape(T, K), rec["w"].reshape(T, K)
        zero, b = torch.zeros(T, D).bfloat16(), layer.bias.detach().cpu()
        ref4 = MX.ffn_forward_backward(x.reshape(T, D), idx, w, k4, v4, actname, zero, bias=b)["out"]
        ref8 = MX.ffn_forward_backward(x.reshape(T, D), idx, w, layer.keys.detach().cpu(), layer.values.detach().cpu(), actname, zero,
                                       bias=b)["out"]
        e4, e8 = rel_l2(on.cpu().reshape(T, D), ref4), rel_l2(off.cpu().reshape(T, D), ref8)
        print(f"smoe {actname} T={T}: rel_l2 fp4 path against the W4A8 oracle {e4:.2e}; fp8 decode path against the MX oracle {e8:.2e}; "
              f"W4A8 oracle against the MX oracle {rel_l2(ref4, ref8):.2e}")
        assert e4 <= MX_OUT, (T, e4, e8)
    assert len(Fn._FP8_WCACHE) == 2 and len(Fn._FP4_WCACHE) == 2
    _clear()


def test_pretrain_deepseekv2_shared_expert(monkeypatch):
    T = 5
    layer = _layer("deepseekv2", F.relu, False, 73)
    rec = _spy_ffn(layer)
    x = torch.randn(1, T, D, generator=torch.Generator().manual_seed(74)).to(BF)
    xd = x.to(DEV)
    _clear()
    with torch.no_grad():
        layer.fp4_decode_weights = False
        off, p_off, i_off = _run(layer, xd, 0, monkeypatch=monkeypatch)
        layer.fp4_decode_weights = True
        on, p_on, i_on = _run(layer, xd, 64, monkeypatch=monkeypatch)
    _assert_tiled(p_off, shared=True)
    _assert_fp4_decode(p_on, 4)                                 # routed experts + the always-on shared expert, two launches each
    assert _calls(p_on, "quantize_mxfp4_t") == 4                # cold: the four tables
    assert len(i_on) == len(i_off) == 1 and torch.equal(i_on[0], i_off[0])
    ps = {k: v.detach().cpu() for k, v in layer.state_dict().items() if v.is_floating_point()}
    del MX.RECORDED[:]
    ref, _ = O.pretrain_deepseek_forward(x, ps["w_gate"], _w4(ps["keys"]), _w4(ps["values"]), _w4(ps["keys_shared"]),
                                         _w4(ps["values_shared"]), K, "deepseekv2", BF, x.dtype, forced_idx=rec["idx"].view(1, T, K),
                                         ffn=MX.pretrain_ffn)
    del MX.RECORDED[:]
    e_on = rel_l2(on.float().cpu(), ref.float())
    print(f"deepseekv2 T={T}: rel_l2 fp4 path against the W4A8 oracle layer {e_on:.2e}")
    assert e_on <= MX_OUT, e_on
    _clear()


# ------------------------------------------------------------------------------------------------ the guard's other side
def _fwd_bwd(layer, x, rows):
    layer.zero_grad(set_to_none=True)
    xi = x.detach().clone().requires_grad_(True)
    out, prof, _ = _run(layer, xi, rows)
    out.float().pow(2).mean().backward()
    grads = {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}
    return out.detach().clone(), prof, xi.grad.clone(), grads


def test_guard_input_requires_grad():
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(76)).to(BF).to(DEV)
    o0, p0, gx0, g0 = _fwd_bwd(_layer("smoe", F.gelu, True, 75, fp4=False).train(), x, 64)
    _clear()
    o1, p1, gx1, g1 = _fwd_bwd(_layer("smoe", F.gelu, True, 75).train(), x, 64)
    _assert_tiled(p1)
    assert torch.equal(o1, o0) and torch.equal(gx1, gx0)
    assert set(g1) == set(g0) and len(g0) > 0 and all(torch.equal(g1[k], g0[k]) for k in g0)
    assert len(Fn._FP4_WCACHE) == 0
    _clear()


def test_guard_rows_above_the_limit_and_at_it():
    off_layer, layer = _layer("smoe", F.relu, True, 77, fp4=False), _layer("smoe", F.relu, True, 77)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(78)).to(BF).to(DEV)
    _clear()
    with torch.no_grad():
        off, p_off, _ = _run(off_layer, x, 9)                   # T * K = 10 routed rows
        on, p_on, _ = _run(layer, x, 9)
        at, p_at, _ = _run(layer, x, 10)
    _assert_tiled(p_off)
    _assert_tiled(p_on)
    assert torch.equal(on, off)
    _assert_fp4_decode(p_at, 2)                                 # ... and exactly at the limit the path is taken
    _clear()


def test_guard_without_the_weight_cache():
    off_layer, layer = _layer("smoe", F.relu, True, 79, cache=False, fp4=False), _layer("smoe", F.relu, True, 79, cache=False)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(80)).to(BF).to(DEV)
    _clear()
    with torch.no_grad():
        off, _, _ = _run(off_layer, x, 64)
        on, p_on, _ = _run(layer, x, 64)
    _assert_tiled(p_on)
    assert torch.equal(on, off)
    assert len(Fn._FP4_WCACHE) == 0 and len(Fn._FP8_WCACHE) == 0


def test_guard_flag_off():
    """The default: the fp8 decode path, bit-equal to a layer built without the attribute at all."""
    layer = _layer("smoe", F.gelu, True, 83, fp4=False)
    from competesmoe_amd.pretrain import get_moe
    torch.manual_seed(83)
    args = types.SimpleNamespace(**PRETRAIN_ARGS, fp8_experts=True, fp8_weight_cache=True)
    plain = get_moe("smoe")(D, E, FH, n_heads=K, activation=F.gelu, bias=True, log_interval=None, args=args).to(DEV).to(BF).eval()
    plain.load_state_dict(layer.state_dict())
    assert plain.fp4_decode_weights is False
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(84)).to(BF).to(DEV)
    _clear()
    with torch.no_grad():
        a, pa, _ = _run(plain, x, 64)
        b, pb, _ = _run(layer, x, 64)
    _assert_fp8_decode(pa, 2)
    _assert_fp8_decode(pb, 2)
    assert torch.equal(a, b) and len(Fn._FP4_WCACHE) == 0
    _clear()


def test_flag_without_fp8_experts_is_refused():
    with pytest.raises(ValueError, match="fp4_decode_weights"):
        _layer("smoe", F.relu, True, 85, fp8=False)


# ------------------------------------------------------------------------------------------------ the MXFP4 weight cache
def test_fp4_weight_cache():
    layer = _layer("smoe", F.gelu, True, 81)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(82)).to(BF).to(DEV)
    _clear()
    with torch.no_grad():
        o1, p1, _ = _run(layer, x, 64)
        o2, p2, _ = _run(layer, x, 64)
    _assert_fp4_decode(p1, 2)
    _assert_fp4_decode(p2, 2)
    assert _calls(p1, "quantize_mxfp4_t") == 2 and _calls(p2, "quantize_mxfp4_t") == 0      # cold: the two tables; warm: nothing
    assert torch.equal(o1, o2)
    assert len(Fn._FP4_WCACHE) == 2 and len(Fn._FP8_WCACHE) == 0
    q4, s4 = Fn._FP4_WCACHE[(layer.keys.data_ptr(), tuple(layer.keys.shape), layer.keys.dtype)][1]
    assert q4.shape == (E, FH, D // 2) and s4.shape == (E, FH, D // 32)
    # an in-place update of keys: keys alone is quantised again and the output follows the new weights
    with torch.no_grad():
        layer.keys.mul_(1.5)
        o3, p3, _ = _run(layer, x, 64)
    _assert_fp4_decode(p3, 2)
    assert _calls(p3, "quantize_mxfp4_t") == 1
    assert not torch.equal(o3, o1)
    fresh = _layer("smoe", F.gelu, True, 81)
    fresh.load_state_dict(layer.state_dict())
    with torch.no_grad():
        of, _, _ = _run(fresh, x, 64)
    assert torch.equal(o3, of)
    assert len(Fn._FP8_WCACHE) == 0                             # a decode-only session never builds an fp8 entry
    # a training call afterwards is the fp8 step as today: it builds the fp8 entries (both orientations) and equals a fresh layer's
    layer.train()
    fresh2 = _layer("smoe", F.gelu, True, 81, fp4=False).train()
    fresh2.load_state_dict(layer.state_dict())
    ot, pt, gxt, gt = _fwd_bwd(layer, x, 64)
    _assert_tiled(pt)
    assert _calls(pt, "quantize_mxfp8_both") == 2, pt.keys()
    keys_ent = Fn._FP8_WCACHE[(layer.keys.data_ptr(), tuple(layer.keys.shape), layer.keys.dtype)]
    assert keys_ent[1][0] is not None and keys_ent[0] == layer.keys._version
    orf, _, gxf, gf = _fwd_bwd(fresh2, x, 64)
    assert torch.equal(ot, orf) and torch.equal(gxt, gxf)
    assert set(gt) == set(gf) and len(gf) > 0 and all(torch.equal(gt[k], gf[k]) for k in gf)
    # ... and the next decode call is served by the MXFP4 tables it already has
    layer.eval()
    with torch.no_grad():
        o4, p4, _ = _run(layer, x, 64)
    _assert_fp4_decode(p4, 2)
    assert _calls(p4, "quantize_mxfp4_t") == 0 and torch.equal(o4, o3)
    _clear()
