"""The forward-only decode path of the fp8 layers (`args.fp8_experts`) at layer level, both sides of its guard: with
`decode_rows(n)` on, a call that needs no backward, has at most n routed rows and runs with `args.fp8_weight_cache` quantises its T
token rows where they lie and runs both expert GEMMs on csmoe_grouped_gemm_skinny_mxfp8 -- no dispatch copy, no quantiser launch
for the hidden activations, no backward orientation of the weight tables; every other call does what it does with the switch off.
Which path ran is read from ops.profile_start/stop.

Outputs are held to the bound tests/test_fp8_gpu.py holds the tiled path to (MX_OUT = 3e-3 relative L2 against oracle/mxfp8.py, the
emulation of the same quantised operands), the switch-off path on the same inputs first.  Bit-equality on against off is not
demanded: the matrix pipe does not carry fp32 through its 128-term sums (oracle/mxfp8.py), so the order of K-steps may show.
Measured on MI355X (relative L2 against the oracle; off and on gave the same value to the three digits printed):
  smoe relu: T=1 0.00e+00  T=3 6.68e-05  T=16 2.26e-04  T=17 4.77e-04
  smoe gelu: T=1 0.00e+00  T=3 1.76e-04  T=16 5.82e-04  T=17 6.47e-04
  deepseekv2, T=5: 8.73e-04"""
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
from tests.golden_util import rel_l2

DEV = "cuda"
BF = torch.bfloat16
MX_OUT = 3e-3                                                   # tests/test_fp8_gpu.py:183
D, FH, E, K = 128, 256, 8, 2
PRETRAIN_ARGS = dict(stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
                     balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False,
                     tribrid=False, balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False,
                     scale_weight=1.0, test_only=False, n_shared_experts=2)


def _layer(name, act, bias, seed, cache=True):
    from competesmoe_amd.pretrain import get_moe
    torch.manual_seed(seed)
    args = types.SimpleNamespace(**PRETRAIN_ARGS, fp8_experts=True, fp8_weight_cache=cache)
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


def _assert_decode(prof, launches):
    assert _calls(prof, "grouped_gemm_skinny_mxfp8") == launches, prof.keys()
    assert _calls(prof, "grouped_gemm_mxfp8") == 0 and _calls(prof, "dense_gemm_mxfp8") == 0, prof.keys()
    assert all(_calls(prof, n) == 0 for n in ("dispatch_tokens_mxfp8", "dispatch_rows_mxfp8", "dispatch_tokens", "dispatch_rows")), prof.keys()
    assert _calls(prof, "quantize_mxfp8") == launches // 2, prof.keys()       # x once per FFN; never the hidden activations
    assert _calls(prof, "quantize_mxfp8_both") == 0, prof.keys()


def _assert_tiled(prof, shared=False):
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


@pytest.mark.parametrize("actname", ["relu", "gelu"])
def test_pretrain_smoe(actname, monkeypatch):
    layer = _layer("smoe", F.relu if actname == "relu" else F.gelu, True, 71)
    rec = _spy_ffn(layer)
    g = torch.Generator().manual_seed(72)
    Fn.fp8_weight_cache_clear()
    for T in (1, 3, 16, 17):
        x = torch.randn(1, T, D, generator=g).to(BF)
        xd = x.to(DEV)
        with torch.no_grad():
            off, p_off, i_off = _run(layer, xd, 0, monkeypatch=monkeypatch)
            on, p_on, i_on = _run(layer, xd, 64, monkeypatch=monkeypatch)
        _assert_tiled(p_off)
        _assert_decode(p_on, 2)
        assert len(i_on) == len(i_off) == 1 and torch.equal(i_on[0], i_off[0])
        ref = MX.ffn_forward_backward(x.reshape(T, D), rec["idx"].reshape(T, K), rec["w"].reshape(T, K), layer.keys.detach().cpu(),
                                      layer.values.detach().cpu(), actname, torch.zeros(T, D).bfloat16(),
                                      bias=layer.bias.detach().cpu())["out"]
        e_off, e_on = rel_l2(off.cpu().reshape(T, D), ref), rel_l2(on.cpu().reshape(T, D), ref)
        print(f"smoe {actname} T={T}: rel_l2 against the MX oracle off {e_off:.2e} on {e_on:.2e}")
        assert e_off <= MX_OUT, (T, e_off)
        assert e_on <= MX_OUT, (T, e_on)
    Fn.fp8_weight_cache_clear()


def test_pretrain_deepseekv2_shared_expert(monkeypatch):
    T = 5
    layer = _layer("deepseekv2", F.relu, False, 73)
    rec = _spy_ffn(layer)
    x = torch.randn(1, T, D, generator=torch.Generator().manual_seed(74)).to(BF)
    xd = x.to(DEV)
    Fn.fp8_weight_cache_clear()
    with torch.no_grad():
        off, p_off, i_off = _run(layer, xd, 0, monkeypatch=monkeypatch)
        on, p_on, i_on = _run(layer, xd, 64, monkeypatch=monkeypatch)
    _assert_tiled(p_off, shared=True)
    _assert_decode(p_on, 4)                                     # routed experts + the always-on shared expert, two launches each
    assert len(i_on) == len(i_off) == 1 and torch.equal(i_on[0], i_off[0])
    ps = {k: v.detach().cpu() for k, v in layer.state_dict().items() if v.is_floating_point()}
    del MX.RECORDED[:]
    ref, _ = O.pretrain_deepseek_forward(x, ps["w_gate"], ps["keys"], ps["values"], ps["keys_shared"], ps["values_shared"], K,
                                         "deepseekv2", BF, x.dtype, forced_idx=rec["idx"].view(1, T, K), ffn=MX.pretrain_ffn)
    del MX.RECORDED[:]
    e_off, e_on = rel_l2(off.float().cpu(), ref.float()), rel_l2(on.float().cpu(), ref.float())
    print(f"deepseekv2 T={T}: rel_l2 against the oracle layer off {e_off:.2e} on {e_on:.2e}")
    assert e_off <= MX_OUT, e_off
    assert e_on <= MX_OUT, e_on
    Fn.fp8_weight_cache_clear()


# ------------------------------------------------------------------------------------------------ the guard's other side
def _fwd_bwd(layer, x, rows):
    layer.zero_grad(set_to_none=True)
    xi = x.detach().clone().requires_grad_(True)
    out, prof, _ = _run(layer, xi, rows)
    out.float().pow(2).mean().backward()
    grads = {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}
    return out.detach().clone(), prof, xi.grad.clone(), grads


def test_guard_input_requires_grad():
    layer = _layer("smoe", F.gelu, True, 75).train()
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(76)).to(BF).to(DEV)
    o0, p0, gx0, g0 = _fwd_bwd(layer, x, 0)
    o1, p1, gx1, g1 = _fwd_bwd(layer, x, 64)
    _assert_tiled(p1)
    assert torch.equal(o1, o0) and torch.equal(gx1, gx0)
    assert set(g1) == set(g0) and len(g0) > 0 and all(torch.equal(g1[k], g0[k]) for k in g0)
    Fn.fp8_weight_cache_clear()


def test_guard_rows_above_the_limit():
    layer = _layer("smoe", F.relu, True, 77)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(78)).to(BF).to(DEV)
    with torch.no_grad():
        off, _, _ = _run(layer, x, 0)
        on, p_on, _ = _run(layer, x, 9)                         # T * K = 10 routed rows
        at, p_at, _ = _run(layer, x, 10)
    _assert_tiled(p_on)
    assert torch.equal(on, off)
    _assert_decode(p_at, 2)                                     # ... and exactly at the limit the path is taken
    Fn.fp8_weight_cache_clear()


def test_guard_without_the_weight_cache():
    """Without `args.fp8_weight_cache` the call would quantise whole tables first: the path does not save what that costs."""
    layer = _layer("smoe", F.relu, True, 79, cache=False)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(80)).to(BF).to(DEV)
    with torch.no_grad():
        off, _, _ = _run(layer, x, 0)
        on, p_on, _ = _run(layer, x, 64)
    _assert_tiled(p_on)
    assert torch.equal(on, off)


# ------------------------------------------------------------------------------------------------ forward-only weight tables
def test_forward_only_weight_cache():
    layer = _layer("smoe", F.gelu, True, 81)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(82)).to(BF).to(DEV)
    Fn.fp8_weight_cache_clear()
    with torch.no_grad():
        o1, p1, _ = _run(layer, x, 64)
        o2, p2, _ = _run(layer, x, 64)
    _assert_decode(p1, 2)
    _assert_decode(p2, 2)
    # cold cache: the forward orientation of the two tables, never both orientations; warm: nothing
    assert _calls(p1, "quantize_mxfp8_t") == 2 and _calls(p1, "quantize_mxfp8_both") == 0, p1.keys()
    assert _calls(p2, "quantize_mxfp8_t") == 0 and _calls(p2, "quantize_mxfp8_both") == 0, p2.keys()
    assert torch.equal(o1, o2)
    assert all(ent[1][0] is None for ent in Fn._FP8_WCACHE.values()) and len(Fn._FP8_WCACHE) == 2
    # an in-place update of keys: keys alone is quantised again and the output follows the new weights
    with torch.no_grad():
        layer.keys.mul_(1.5)
        o3, p3, _ = _run(layer, x, 64)
    _assert_decode(p3, 2)
    assert _calls(p3, "quantize_mxfp8_t") == 1 and _calls(p3, "quantize_mxfp8_both") == 0, p3.keys()
    assert not torch.equal(o3, o1)
    fresh = _layer("smoe", F.gelu, True, 81)
    fresh.load_state_dict(layer.state_dict())
    with torch.no_grad():
        of, _, _ = _run(fresh, x, 64)
    assert torch.equal(o3, of)
    # a training call afterwards needs both orientations: it quantises both, replaces the entries, and equals a fresh layer's
    layer.train()
    fresh2 = _layer("smoe", F.gelu, True, 81).train()
    fresh2.load_state_dict(layer.state_dict())
    ot, pt, gxt, gt = _fwd_bwd(layer, x, 64)
    _assert_tiled(pt)
    assert _calls(pt, "quantize_mxfp8_both") == 2 and _calls(pt, "quantize_mxfp8_t") == 0, pt.keys()
    orf, _, gxf, gf = _fwd_bwd(fresh2, x, 64)
    assert torch.equal(ot, orf) and torch.equal(gxt, gxf)
    assert set(gt) == set(gf) and len(gf) > 0 and all(torch.equal(gt[k], gf[k]) for k in gf)
    keys_ent = Fn._FP8_WCACHE[(layer.keys.data_ptr(), tuple(layer.keys.shape), layer.keys.dtype)]
    assert keys_ent[1][0] is not None and keys_ent[0] == layer.keys._version
    # ... whose forward half then serves the next decode call without a launch
    layer.eval()
    with torch.no_grad():
        o4, p4, _ = _run(layer, x, 64)
    _assert_decode(p4, 2)
    assert _calls(p4, "quantize_mxfp8_t") == 0 and torch.equal(o4, o3)
    Fn.fp8_weight_cache_clear()
