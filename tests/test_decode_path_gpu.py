"""The forward-only decode path at layer level, both sides of its guard: with `decode_rows(n)` on, a call that needs no backward
and has at most n routed rows runs its expert GEMMs on csmoe_grouped_gemm_skinny without a dispatch copy; every other call does
what it does with the switch off.  Which path ran is read from ops.profile_start/stop.

Pretrain `smoe` on exact data (x integers in [-2, 2], keys / values integers in [-1, 1] * 2^-3, bias multiples of 2^-5 in [-2, 2]):
both GEMMs' fp32 accumulators are exact in any summation order -- the test checks that on the CPU for its own data before it
trusts it -- so on and off must agree bit for bit.  The LLaVA layers run random bf16 weights: on against off under the bound
tests/test_gemm_fuzz_gpu.py holds the bf16 kernels to (rtol 2^-7, atol 2e-2), same routing both ways.
"""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import competesmoe_amd
    from competesmoe_amd import ops

DEV = "cuda"
BF = torch.bfloat16
RTOL, ATOL = 2.0 ** -7, 2e-2
D, FH = 64, 136
PRETRAIN_ARGS = dict(stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
                     balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False,
                     tribrid=False, balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False,
                     scale_weight=1.0, test_only=False)
LLAVA_ARGS = types.SimpleNamespace(balance_loss_coef=0.01, router_z_loss_coef=0.001)


def _out(r):
    return r[0] if isinstance(r, tuple) else r


def _run(layer, x, rows, monkeypatch=None):
    """layer(x) with decode_rows(rows) in force (undone afterwards); returns (output, profile, routing indices seen by bin_tokens)."""
    seen = []
    if monkeypatch is not None:
        orig = ops.bin_tokens

        def spy(idx, E, hist=None):
            seen.append(idx.detach().clone())
            return orig(idx, E, hist)
        monkeypatch.setattr(ops, "bin_tokens", spy)
    try:
        competesmoe_amd.decode_rows(rows)
        ops.profile_start()
        try:
            out = _out(layer(x))
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
    assert _calls(prof, "grouped_gemm_skinny") == launches, prof.keys()
    assert _calls(prof, "dispatch_rows") == 0, prof.keys()
    assert _calls(prof, "grouped_gemm_nt") == 0 and _calls(prof, "grouped_gemm_nn") == 0, prof.keys()


def _assert_tiled(prof):
    assert _calls(prof, "grouped_gemm_skinny") == 0, prof.keys()
    assert _calls(prof, "dispatch_rows") == 1, prof.keys()
    assert _calls(prof, "grouped_gemm_nt") + _calls(prof, "grouped_gemm_nn") == 2, prof.keys()


# ------------------------------------------------------------------------------------------------ pretrain stack
def _pretrain_layer(name, E, K, bias, dtype, seed):
    from competesmoe_amd.pretrain import get_moe
    torch.manual_seed(seed)
    layer = get_moe(name)(D, E, FH, n_heads=K, activation=F.relu, bias=bias, log_interval=None,
                          args=types.SimpleNamespace(**PRETRAIN_ARGS)).to(DEV).to(dtype).eval()
    return layer


def _exact_fill(layer, seed):
    """keys / values integers in [-1, 1] * 2^-3, bias multiples of 2^-5 in [-2, 2] (all bf16-exact)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in (layer.keys, layer.values):
            p.copy_((torch.randint(-1, 2, tuple(p.shape), generator=g).float() * 2.0 ** -3).to(p.dtype))
        if layer.bias is not None:
            layer.bias.copy_((torch.randint(-64, 65, tuple(layer.bias.shape), generator=g).float() * 2.0 ** -5).to(layer.bias.dtype))


def _sum_orders(a, b):
    """(fp32 sum over k in ascending order, in descending order, fp64 sum) of a[t, k] * b[k, n]."""
    prod32 = a.float()[:, :, None] * b.float()[None]
    fwd = prod32.cumsum(1)[:, -1]
    rev = prod32.flip(1).cumsum(1)[:, -1]
    return fwd, rev, a.double() @ b.double()


def _assert_exact_on_cpu(layer, x):
    """Both GEMMs' accumulators of every (token, expert) pair are exact in fp32 in two summation orders."""
    x2 = x.reshape(-1, D).cpu()
    keys, values = layer.keys.detach().cpu(), layer.values.detach().cpu()
    bias = None if layer.bias is None else layer.bias.detach().cpu()
    for e in range(keys.shape[0]):
        f, r, d = _sum_orders(x2, keys[e])
        assert torch.equal(f.double(), d) and torch.equal(r.double(), d)
        pre = d.float() + (0 if bias is None else bias[e].float())
        h = torch.relu(pre.to(BF))
        f, r, d2 = _sum_orders(h, values[e])
        assert torch.equal(f.double(), d2) and torch.equal(r.double(), d2)
        assert float(d.abs().max()) <= 16 and float(d2.abs().max()) <= 128


@pytest.mark.parametrize("bias", [False, True])
def test_pretrain_smoe_exact(bias):
    E, K = 8, 2
    layer = _pretrain_layer("smoe", E, K, bias, BF, 21)
    _exact_fill(layer, 22)
    g = torch.Generator().manual_seed(23)
    for T in (1, 3, 16, 17):
        x = torch.randint(-2, 3, (1, T, D), generator=g).to(BF)
        _assert_exact_on_cpu(layer, x)
        xd = x.to(DEV)
        with torch.no_grad():
            off, p_off, _ = _run(layer, xd, 0)
            on, p_on, _ = _run(layer, xd, 64)
        _assert_tiled(p_off)
        _assert_decode(p_on, 2)
        assert torch.equal(on, off), f"T={T} bias={bias}"


def test_pretrain_deepseekv2_shared_expert(monkeypatch):
    E, K, T = 8, 2, 5
    layer = _pretrain_layer("deepseekv2", E, K, True, BF, 31)
    x = torch.randn(1, T, D, generator=torch.Generator().manual_seed(32)).to(BF).to(DEV)
    with torch.no_grad():
        off, p_off, i_off = _run(layer, x, 0, monkeypatch=monkeypatch)
        on, p_on, i_on = _run(layer, x, 64, monkeypatch=monkeypatch)
    _assert_tiled(p_off)
    _assert_decode(p_on, 4)                                     # routed experts + the always-on shared expert, two launches each
    assert len(i_on) == len(i_off) == 1 and torch.equal(i_on[0], i_off[0])
    torch.testing.assert_close(on.float(), off.float(), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------------ LLaVA stack
def _llava_layer(name, hidden, E, K, seed):
    from competesmoe_amd.moe import get_moe
    torch.manual_seed(seed)
    if name == "smoe":
        experts = nn.ModuleList([nn.Sequential(nn.Linear(hidden, FH), nn.GELU(), nn.Linear(FH, hidden)) for _ in range(E)])
        layer = get_moe(name)(hidden, hidden, E, K, experts, LLAVA_ARGS)
    else:
        layer = get_moe(name)(hidden, hidden, E, K, nn.Sequential(nn.Linear(hidden, FH), nn.GELU(), nn.Linear(FH, hidden)), LLAVA_ARGS)
    with torch.no_grad():
        for p in layer.parameters():                            # the copies of one expert module get weights of their own
            p.copy_(torch.randn(p.shape) * (p.shape[-1] ** -0.5 if p.dim() > 1 else 0.1))
    return layer.to(DEV).to(BF).eval()


@pytest.mark.parametrize("T", [1, 5, 17])
def test_llava_smoe(T, monkeypatch):
    layer = _llava_layer("smoe", D, 4, 2, 41)
    x = torch.randn(1, T, D, generator=torch.Generator().manual_seed(42 + T)).to(BF).to(DEV)
    with torch.no_grad():
        off, p_off, i_off = _run(layer, x, 0, monkeypatch=monkeypatch)
        on, p_on, i_on = _run(layer, x, 64, monkeypatch=monkeypatch)
    _assert_tiled(p_off)
    _assert_decode(p_on, 2)
    assert len(i_on) == len(i_off) == 1 and torch.equal(i_on[0], i_off[0])
    torch.testing.assert_close(on.float(), off.float(), rtol=RTOL, atol=ATOL)


def test_llava_smoe_share(monkeypatch):
    layer = _llava_layer("smoe_share", D, 4, 2, 51)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(52)).to(BF).to(DEV)
    with torch.no_grad():
        off, p_off, i_off = _run(layer, x, 0, monkeypatch=monkeypatch)
        on, p_on, i_on = _run(layer, x, 64, monkeypatch=monkeypatch)
    _assert_tiled(p_off)
    _assert_decode(p_on, 4)                                     # 3 routed experts (top 1) + the always-on last expert
    assert len(i_on) == len(i_off) == 1 and torch.equal(i_on[0], i_off[0])
    torch.testing.assert_close(on.float(), off.float(), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------------ the guard's other side
def _fwd_bwd(layer, x, rows):
    layer.zero_grad(set_to_none=True)
    xi = x.detach().clone().requires_grad_(True)
    out, prof, _ = _run(layer, xi, rows)
    out.float().pow(2).mean().backward()
    grads = [p.grad.clone() for p in layer.parameters() if p.grad is not None]
    return out.detach().clone(), prof, xi.grad.clone(), grads


def test_guard_input_requires_grad():
    layer = _llava_layer("smoe", D, 4, 2, 61).train()
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(62)).to(BF).to(DEV)
    o0, p0, gx0, g0 = _fwd_bwd(layer, x, 0)
    o1, p1, gx1, g1 = _fwd_bwd(layer, x, 64)
    _assert_tiled(p1)
    assert torch.equal(o1, o0) and torch.equal(gx1, gx0)
    assert len(g1) == len(g0) > 0 and all(torch.equal(a, b) for a, b in zip(g1, g0))


def test_guard_rows_above_the_limit():
    layer = _llava_layer("smoe", D, 4, 2, 63)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(64)).to(BF).to(DEV)
    with torch.no_grad():
        off, _, _ = _run(layer, x, 0)
        on, p_on, _ = _run(layer, x, 9)                         # T * K = 10 routed rows
        at, p_at, _ = _run(layer, x, 10)
    _assert_tiled(p_on)
    assert torch.equal(on, off)
    _assert_decode(p_at, 2)                                     # ... and exactly at the limit the path is taken


def test_guard_fp32_masters_without_weight_cache():
    layer = _pretrain_layer("smoe", 8, 2, True, torch.float32, 65)
    x = torch.randn(1, 5, D, generator=torch.Generator().manual_seed(66)).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        off, _, _ = _run(layer, x, 0)
        on, p_on, _ = _run(layer, x, 64)
    _assert_tiled(p_on)
    assert torch.equal(on, off)


def test_guard_unaligned_model_dim():
    hidden = 68                                                 # not a multiple of 8: the shape rule rejects both GEMMs
    layer = _llava_layer("smoe", hidden, 4, 2, 67)
    x = torch.randn(1, 5, hidden, generator=torch.Generator().manual_seed(68)).to(BF).to(DEV)
    with torch.no_grad():
        off, _, _ = _run(layer, x, 0)
        on, p_on, _ = _run(layer, x, 64)
    _assert_tiled(p_on)
    assert torch.equal(on, off)
