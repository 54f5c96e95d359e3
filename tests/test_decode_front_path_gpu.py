"""The decode front end (competesmoe_amd.decode_front) at layer level, both sides of every guard.  With the switch on, a call in
no-grad mode with at most decode_rows() routed rows, on a layer whose gate is the plain bf16 linear map, routes, bins and -- in the
fp8 layers with `args.fp8_weight_cache` -- quantises its tokens in ONE launch (csmoe_decode_route); every other call does what it
does with the switch off.  Which path ran is read from ops.profile_start/stop and from a spy on ops.bin_tokens.

Inputs make the gate product exact: x entries from {-2..2} / 2, gate entries from {-2..2} / 8, D <= 256, so every partial sum is a
multiple of 2^-4 below 2^7 and exact in fp32 in any order: the logits of all routers agree bit for bit (and hold many exact ties,
which go to the lowest index in all of them).  The expert launches of the two arms are then the same launches on the same idx, w,
bins and quantised rows, so switch on against switch off is torch.equal on the layer output."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import competesmoe_amd
    from competesmoe_amd import ops
    from competesmoe_amd import functional as Fn

DEV = "cuda"
BF = torch.bfloat16
PRETRAIN_ARGS = dict(stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
                     balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False,
                     tribrid=False, balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False,
                     scale_weight=1.0, test_only=False, n_shared_experts=2)
LLAVA_ARGS = types.SimpleNamespace(balance_loss_coef=0.01, router_z_loss_coef=0.001)


def _out(r):
    return r[0] if isinstance(r, tuple) else r


def _calls(prof, name):
    return prof.get(name, {}).get("calls", 0)


def _exact_gate(p, seed):
    with torch.no_grad():
        p.copy_((torch.randint(-2, 3, tuple(p.shape), generator=torch.Generator().manual_seed(seed)).float() / 8).to(p.dtype))


def _exact_x(T, D, seed):
    return (torch.randint(-2, 3, (1, T, D), generator=torch.Generator().manual_seed(seed)).float() / 2).to(BF).to(DEV)


def _run(layer, x, front, rows=64, monkeypatch=None):
    """layer(x) under decode_rows(rows) and decode_front(front), both undone afterwards.  Returns (output, profile, what the spy on
    ops.bin_tokens saw: for each call, whether the route plan answered for its idx at call time)."""
    seen = []
    if monkeypatch is not None:
        orig = ops.bin_tokens

        def spy(idx, E, hist=None):
            seen.append(ops._route_plan_for(idx.contiguous(), E) is not None)
            return orig(idx, E, hist)
        monkeypatch.setattr(ops, "bin_tokens", spy)
    try:
        competesmoe_amd.decode_rows(rows)
        competesmoe_amd.decode_front(front)
        ops.profile_start()
        try:
            out = _out(layer(x))
        finally:
            prof = ops.profile_stop()
    finally:
        competesmoe_amd.decode_rows(0)
        competesmoe_amd.decode_front(False)
        if monkeypatch is not None:
            monkeypatch.undo()
    return out, prof, seen


def _on_off(layer, x, monkeypatch, rows=64):
    with torch.no_grad():
        off, p_off, s_off = _run(layer, x, False, rows, monkeypatch)
        on, p_on, s_on = _run(layer, x, True, rows, monkeypatch)
    assert _calls(p_off, "decode_route") == 0 and s_off == [False], (p_off.keys(), s_off)
    assert _calls(p_on, "decode_route") == 1 and _calls(p_on, "gate_select") == 0 and _calls(p_on, "gate_logits") == 0, p_on.keys()
    assert s_on == [True], s_on                                 # the one bin_tokens call of the layer met the plan
    assert torch.equal(on, off)
    return p_off, p_on


def _same_counts(p_off, p_on, names):
    for n in names:
        assert _calls(p_on, n) == _calls(p_off, n), (n, p_off.keys(), p_on.keys())


# ------------------------------------------------------------------------------------------------ pretrain stack
def _pretrain_layer(name, D, E, FH, K, act, bias, seed, **extra):
    from competesmoe_amd.pretrain import get_moe
    torch.manual_seed(seed)
    args = types.SimpleNamespace(**PRETRAIN_ARGS, **extra)
    layer = get_moe(name)(D, E, FH, n_heads=K, activation=act, bias=bias, log_interval=None, args=args).to(DEV).to(BF).eval()
    if bias:
        with torch.no_grad():
            layer.bias.copy_(torch.randn(layer.bias.shape) * 0.1)
    if hasattr(layer, "w_gate"):
        _exact_gate(layer.w_gate, seed + 1000)
    return layer


@pytest.mark.parametrize("T", [1, 3, 16, 17])
def test_pretrain_smoe_bf16(T, monkeypatch):
    layer = _pretrain_layer("smoe", 128, 8, 256, 2, F.relu, True, 11)
    p_off, p_on = _on_off(layer, _exact_x(T, 128, 12 + T), monkeypatch)
    assert _calls(p_on, "grouped_gemm_skinny") == 2
    _same_counts(p_off, p_on, ("grouped_gemm_skinny", "grouped_gemm_nt", "grouped_gemm_nn", "dispatch_rows", "combine"))


@pytest.mark.parametrize("T", [1, 5])
def test_pretrain_smoe_fp8(T, monkeypatch):
    layer = _pretrain_layer("smoe", 128, 8, 256, 2, F.relu, True, 21, fp8_experts=True, fp8_weight_cache=True)
    Fn.fp8_weight_cache_clear()
    p_off, p_on = _on_off(layer, _exact_x(T, 128, 22 + T), monkeypatch)
    assert _calls(p_off, "quantize_mxfp8") == 1 and _calls(p_off, "grouped_gemm_skinny_mxfp8") == 2, p_off.keys()
    assert _calls(p_on, "quantize_mxfp8") == 0 and _calls(p_on, "grouped_gemm_skinny_mxfp8") == 2, p_on.keys()
    Fn.fp8_weight_cache_clear()


@pytest.mark.parametrize("fp4", [False, True])
def test_pretrain_deepseekv2_fp8_more_than_64_experts(fp4, monkeypatch):
    """E = 80: the layer the one-pass router refuses (gate_logits + router_select with the switch off); the shared expert reuses the
    quantised rows of the routed experts, so no quantiser launch remains."""
    extra = dict(fp8_experts=True, fp8_weight_cache=True)
    if fp4:
        extra["fp4_decode_weights"] = True
    layer = _pretrain_layer("deepseekv2", 128, 80, 128, 2, F.relu, False, 31, **extra)
    Fn.fp8_weight_cache_clear()
    Fn.fp4_weight_cache_clear()
    p_off, p_on = _on_off(layer, _exact_x(5, 128, 32), monkeypatch)
    gemm = "grouped_gemm_skinny_mxfp4w" if fp4 else "grouped_gemm_skinny_mxfp8"
    assert _calls(p_off, "gate_logits") == 1 and _calls(p_off, "gate_select") == 0, p_off.keys()
    assert _calls(p_off, "quantize_mxfp8") == 2 and _calls(p_off, gemm) == 4, p_off.keys()
    assert _calls(p_on, "quantize_mxfp8") == 0 and _calls(p_on, gemm) == 4, p_on.keys()
    Fn.fp8_weight_cache_clear()
    Fn.fp4_weight_cache_clear()


# ------------------------------------------------------------------------------------------------ LLaVA stack
def _llava_smoe(D, FH, E, K, seed):
    from competesmoe_amd.moe import get_moe
    torch.manual_seed(seed)
    experts = nn.ModuleList([nn.Sequential(nn.Linear(D, FH), nn.GELU(), nn.Linear(FH, D)) for _ in range(E)])
    layer = get_moe("smoe")(D, D, E, K, experts, LLAVA_ARGS)
    _exact_gate(layer.gate.weight, seed + 1000)
    return layer.to(DEV).to(BF).eval()


def test_llava_smoe(monkeypatch):
    layer = _llava_smoe(256, 512, 8, 2, 41)
    p_off, p_on = _on_off(layer, _exact_x(5, 256, 42), monkeypatch)
    assert _calls(p_on, "grouped_gemm_skinny") == 2
    _same_counts(p_off, p_on, ("grouped_gemm_skinny", "grouped_gemm_nt", "grouped_gemm_nn", "dispatch_rows", "combine"))


# ------------------------------------------------------------------------------------------------ guards
def test_guard_rows_above_the_limit(monkeypatch):
    layer = _pretrain_layer("smoe", 128, 8, 256, 2, F.relu, True, 51)
    x = _exact_x(5, 128, 52)                                    # T * K = 10 routed rows
    with torch.no_grad():
        off, _, _ = _run(layer, x, False, 9)
        above, p_above, _ = _run(layer, x, True, 9)
        at, p_at, s_at = _run(layer, x, True, 10, monkeypatch)
        at_off, _, _ = _run(layer, x, False, 10)
    assert _calls(p_above, "decode_route") == 0 and _calls(p_above, "gate_select") == 1 and torch.equal(above, off)
    assert _calls(p_at, "decode_route") == 1 and s_at == [True] and torch.equal(at, at_off)      # exactly at the limit: taken


def _fwd_bwd(layer, x, front):
    layer.zero_grad(set_to_none=True)
    xi = x.detach().clone().requires_grad_(True)
    out, prof, _ = _run(layer, xi, front)
    out.float().pow(2).mean().backward()
    grads = {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}
    return out.detach().clone(), prof, xi.grad.clone(), grads


@pytest.mark.parametrize("stack", ["pretrain", "llava"])
def test_guard_grad_mode_on(stack):
    layer = (_pretrain_layer("smoe", 128, 8, 256, 2, F.relu, True, 61) if stack == "pretrain" else _llava_smoe(256, 512, 8, 2, 63)).train()
    x = _exact_x(5, 128 if stack == "pretrain" else 256, 62)
    o0, p0, gx0, g0 = _fwd_bwd(layer, x, False)
    o1, p1, gx1, g1 = _fwd_bwd(layer, x, True)
    assert _calls(p1, "decode_route") == 0 and _calls(p1, "gate_select") == _calls(p0, "gate_select") == 1, p1.keys()
    assert torch.equal(o1, o0) and torch.equal(gx1, gx0)
    assert set(g1) == set(g0) and len(g0) > 0 and all(torch.equal(g1[k], g0[k]) for k in g0)


def test_guard_cosine_router_is_left_alone():
    layer = _pretrain_layer("xmoe", 128, 8, 256, 2, F.relu, False, 71)
    x = _exact_x(5, 128, 72)
    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    with torch.no_grad():
        off, p_off, _ = _run(layer, x, False)
        layer.load_state_dict(state)                            # a forward rescales `expert_embeddings` in place (xmoe.py:145-149)
        on, p_on, _ = _run(layer, x, True)
    assert _calls(p_on, "decode_route") == 0 and set(p_on) == set(p_off), (p_on.keys(), p_off.keys())
    assert torch.equal(on, off)


def test_switch_off_launches_nothing_new(monkeypatch):
    layer = _pretrain_layer("smoe", 128, 8, 256, 2, F.relu, True, 81)
    with torch.no_grad():
        _, prof, seen = _run(layer, _exact_x(5, 128, 82), False, 64, monkeypatch)
    assert _calls(prof, "decode_route") == 0 and _calls(prof, "gate_select") == 1 and seen == [False]
    assert ops._ROUTE_PLAN is None
